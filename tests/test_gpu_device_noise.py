"""GPU tests (-m gpu) of the opt-in device noise (noise="device"): the generator against its NumPy restatement (tests/noise_ref.py),
the placement-independence contract, and every consumer (reverse step eager / graph, padding, confidence score, sharded entry) against
the same call on the tape that fdipt_noise_fill writes for the same keys — the path every parity fixture already covers."""
import functools
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest
import torch

import noise_ref
from conftest import ROOT, kabsch_free_rmsd, load_golden
from test_gpu_parity import _feats, _net, dev

pytestmark = pytest.mark.gpu


def time_limit(seconds):
    """An individual wall-clock limit per test (SIGALRM): a test that hangs fails instead of holding the GPU."""
    def deco(fn):
        @functools.wraps(fn)
        def run(*a, **kw):
            def on_alarm(signum, frame):
                raise TimeoutError(f"{fn.__name__} exceeded its time limit of {seconds} s")
            old = signal.signal(signal.SIGALRM, on_alarm)
            signal.alarm(seconds)
            try:
                return fn(*a, **kw)
            finally:
                signal.alarm(0)
                signal.signal(signal.SIGALRM, old)
        return run
    return deco


def _host(v):
    return v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _assert_same(ref, got, what=""):
    assert sorted(ref) == sorted(got)
    for k in ref:
        np.testing.assert_array_equal(_host(ref[k]), _host(got[k]), err_msg=f"{what}: {k}")


def _fill(keys, purpose, n_steps, N, k_begin=0):
    from framedipt_amd import noise
    return noise.fill(noise.keys_tensor(noise.as_keys(keys, len(keys)), "cuda"), purpose, n_steps, N, "cuda", k_begin=k_begin)


BIT_A = 0x0123456789ABCDEF
KEYS = [0, 2 ** 63 - 1, BIT_A, BIT_A ^ (1 << 17), BIT_A ^ (1 << 49), 2 ** 64 - 1]


@time_limit(120)
def test_fill_equals_the_numpy_restatement():
    """fdipt_noise_fill against tests/noise_ref.py: four purposes, keys 0, 2^63 - 1, 2^64 - 1 and keys that differ in one bit (low and
    high word), k_begin = 7, N = 61 (no multiple of 64).  Both sides run the same float64 formula on the same 53-bit uniforms and
    differ by the last-place accuracy of log / sin / cos only: |z| < 8.7 (u0 >= 2^-54), sqrt is correctly rounded, log / sin / cos are
    each within a few ulp on either side (HIP's math accuracy table is recalled as 1 / 2 / 2 ulp for float64; the table is not among the
    documents installed with the toolchain, so the figure is not confirmed here; NumPy's are within 1 ulp), so two values of a draw
    differ by well under 32 ulp of 8.7 = 5.7e-14; the bound is 1e-13.  A wrong constant, word order or counter gives differences of order 1.
    Measured on an MI355X: maximum 4.44e-16 for every purpose (one ulp of a value in [2, 4)), 95 - 96 % of the values bit-equal."""
    worst = 0.0
    for purpose in range(4):
        got = _fill(KEYS, purpose, 5, 61, k_begin=7).cpu().numpy()
        ref = noise_ref.normals(KEYS, purpose, 7, 5, 61)
        assert got.shape == ref.shape == (5, len(KEYS), 61, 3)
        d = float(np.abs(got - ref).max())
        print(f"purpose {purpose}: max |device - restatement| = {d:.3e}, bit-equal values {np.mean(got == ref):.4f}")
        worst = max(worst, d)
        assert d < 1e-13, (purpose, d)
    print(f"max over purposes: {worst:.3e}")
    from framedipt_amd import _lib
    with pytest.raises(_lib.FdiptError):
        _fill([1], 4, 1, 8)  # no such purpose


@time_limit(120)
def test_a_draw_does_not_depend_on_where_it_is_computed():
    """The contract of include/fdipt.h, bit for bit: one key at B = 1, N = 61 against the rows [:, b, :61] of a fill at B = 4, N = 64
    where sample b carries that key; and steps 3:5 of a fill from step 0 against a fill that begins at step 3."""
    key = BIT_A
    for purpose in range(4):
        one = _fill([key], purpose, 8, 61)
        for b in range(4):
            keys = [11, 12, 13, 14]
            keys[b] = key
            many = _fill(keys, purpose, 8, 64)
            assert torch.equal(one[:, 0], many[:, b, :61]), (purpose, b)
        assert torch.equal(one[3:5], _fill([key], purpose, 2, 61, k_begin=3)), purpose
        assert not torch.equal(one, _fill([key], purpose ^ 1, 8, 61))  # separate purposes, separate values


def _denovo(N, B, precision, seed=5, diffuse_rot=True):
    from framedipt_amd import config, sharding
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import UnconditionalSampler
    conf = config.base_config()
    d = SE3Diffuser(conf.diffuser, device="cuda")
    net = ScoreNetwork(conf.model, d, precision=precision).load_synthetic(7).to("cuda")
    ds = UnconditionalSampler(config.to_conf({"min_length": N, "max_length": N, "length_step": 1, "samples_per_length": B}), d, "cuda")
    items = [sharding.seeded_item(ds, i, seed, d, 4, 0.01, noise="device") for i in range(B)]
    feats, keys = sharding.stack_items(items)
    if not diffuse_rot:  # (x_T needs a diffuser that diffuses rotations; the steps run without)
        conf.diffuser.diffuse_rot = False
        d = SE3Diffuser(conf.diffuser, device="cuda")
        assert not d._diffuse_rot
    return net, d, feats, keys


def _device_vs_filled_tape(net, d, feats, keys, T, **kw):
    """inference_fn(noise="device") against the same call on the filled tape: every returned array, graph and eager, with and without the
    auxiliary trajectories."""
    from framedipt_amd import noise
    from framedipt_amd.inference import inference_fn
    B, N = feats["rigids_t"].shape[:2]
    tape = noise.filled_tape(keys, T - 1, N, "cuda")
    assert tape[0].shape == (T - 1, B, N, 3) and np.abs(tape[0]).max() > 1 and not np.array_equal(tape[0], tape[1])
    base = dict(num_t=T, min_t=0.01, noise_scale=0.1, **kw)
    ref = None
    for graph in (True, False):
        for aux in (True, False):
            got = inference_fn(net, d, feats, graph=graph, aux_traj=aux, noise="device", noise_keys=keys, **base)
            want = inference_fn(net, d, feats, graph=graph, aux_traj=aux, noise_tape=tape, **base)
            _assert_same(want, got, f"graph={graph} aux_traj={aux}")
            if aux and ref is None:
                ref = got
    return ref


@time_limit(420)
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_step_kernel_draws_what_the_fill_says(precision):
    """N = 64 full-size network, synthetic weights, 11 noisy steps, two samples."""
    net, d, feats, keys = _denovo(64, 2, precision)
    assert list(keys) == [5, 6]
    res = _device_vs_filled_tape(net, d, feats, keys, 12)
    # another key, another trajectory; the same key in another batch position, the same trajectory
    from framedipt_amd.inference import inference_fn
    kw = dict(num_t=12, min_t=0.01, noise_scale=0.1, aux_traj=True, noise="device")
    f0 = {k: v[:1] for k, v in feats.items()}
    alone = inference_fn(net, d, f0, noise_keys=[5], **kw)
    np.testing.assert_array_equal(alone["prot_traj"][:, 0], res["prot_traj"][:, 0])
    other = inference_fn(net, d, f0, noise_keys=[6], **kw)
    assert np.abs(other["prot_traj"][0] - alone["prot_traj"][0]).max() > 1e-3


@time_limit(300)
def test_translation_draws_do_not_move_without_rotation_noise():
    """diffuse_rot = False on the diffuser: the translations still take the draws of purpose 1."""
    net, d, feats, keys = _denovo(64, 2, "fp16", diffuse_rot=False)
    _device_vs_filled_tape(net, d, feats, keys, 12)


@time_limit(300)
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_inpainting_with_masked_residues(precision):
    """The inpainting N = 40 fixture's features (fixed residues: diffuse_mask = 0 rows inside the sample)."""
    G = load_golden("traj_full_inpaint_n40_T4_aatype.npz")
    net, d, _ = _net("full_inpaint_n40_T4_aatype", G, precision)
    feats = _feats(G)
    assert 0 < float(feats["fixed_mask"].sum()) < 40
    _device_vs_filled_tape(net, d, feats, [77], 12, inpainting=True, input_aatype=True)


@time_limit(300)
def test_padded_sample_keeps_its_draws():
    """N = 62 alone through inference_fn's pad_to_four path (fp16: padded to 64): the real rows' draws do not depend on the padded length."""
    from framedipt_amd import _lib, noise
    from framedipt_amd.inference import inference_fn
    net, d, feats, keys = _denovo(62, 1, "fp16")
    assert net.precision != _lib.PREC_F32 and feats["rigids_t"].shape[1] == 62
    tape = noise.filled_tape(keys, 11, 62, "cuda")
    kw = dict(num_t=12, min_t=0.01, noise_scale=0.1, aux_traj=True)
    got = inference_fn(net, d, feats, noise="device", noise_keys=keys, **kw)
    want = inference_fn(net, d, feats, noise_tape=tape, **kw)
    assert got["prot_traj"].shape == (12, 1, 62, 37, 3)
    _assert_same(want, got, "pad_to_four")


@time_limit(300)
def test_free_running_small_against_the_oracle(tables):
    """The network and features of test_free_running_small_fp32 with noise="device", against oracle/inference.py on the filled tape of
    the same key; the two bounds of that test (5e-2 A on prot_traj[0], 1e-3 A on the last rigid_0_traj row)."""
    from framedipt_amd import inference as inf
    from framedipt_amd import noise
    import test_oracle_forward as tof
    from oracle import inference as oi
    G = load_golden("traj_small_denovo_n16_T10.npz")
    net, d, _ = _net("small_denovo_n16_T10", G, "fp32")
    T, key = int(G["num_t"]), [2024]
    res = inf.inference_fn(net, d, _feats(G), T, float(G["min_t"]), aux_traj=True, noise_scale=float(G["noise_scale"]),
                           noise="device", noise_keys=key)
    z_rot, z_trans = noise.filled_tape(key, T - 1, 16, "cuda")
    model, diff = tof._model("small_denovo_n16_T10", G, tables)
    ref = oi.inference_fn(model, diff, tof._feats(G), T, float(G["min_t"]), noise_scale=float(G["noise_scale"]),
                          noise_tape=[(z_rot[i], z_trans[i]) for i in range(T - 1)], orthogonalize=True)
    for k in ("prot_traj", "rigid_0_traj", "trans_traj"):
        assert res[k].shape == ref[k].shape, k
    a, b = kabsch_free_rmsd(res["prot_traj"][0], ref["prot_traj"][0]), kabsch_free_rmsd(res["rigid_0_traj"][-1], ref["rigid_0_traj"][-1])
    print(f"prot_traj[0] {a:.3e} A, rigid_0_traj[-1] {b:.3e} A")
    assert a < 5e-2
    assert b < 1e-3


@time_limit(420)
def test_distribution_on_the_device():
    """One fill of T = 500, B = 8, N = 300 per purpose (3.6e6 values each) under the bounds of noise_ref.distribution_report: KS distance
    under the Dvoretzky-Kiefer-Wolfowitz bound, mean, variance, and the sample correlations between rotation / translation draws,
    neighbouring steps, residues, components, samples (consecutive keys) and two keys that differ in one bit; alpha = 1e-9 each."""
    T, N = noise_ref.DIST_T, noise_ref.DIST_N
    z = {p: _fill(list(noise_ref.DIST_KEYS), p, T, N).cpu().numpy() for p in range(4)}
    for p in range(4):
        bit = _fill(list(noise_ref.DIST_BIT_KEYS), p, T, N).cpu().numpy()
        for name, value, bound in noise_ref.distribution_report(z[p], z[p ^ 1], bit):
            print(f"purpose {p} {name}: {value:.3e} (bound {bound:.3e})")
            assert value < bound, (p, name, value, bound)


@time_limit(300)
def test_confidence_score_draws_what_the_fill_says():
    """logp_confidence_score(noise="device") against the call on the filled tape of purposes 2 and 3 (conf_small_denovo_n24_T6 inputs)."""
    from framedipt_amd import noise
    from framedipt_amd.confidence import logp_confidence_score
    from framedipt_amd.rigid import Rigid
    G = load_golden("conf_small_denovo_n24_T6.npz")
    net, d, _ = _net("small_denovo_n24_T6", G, "fp32")
    feats = {k[3:]: torch.as_tensor(G[k]) for k in G if k.startswith("in_")}
    T, key = int(G["num_t"]), [31337]
    args = (net, d, Rigid.from_tensor_7(dev(G["x0"])), feats, G["diffuse_mask"], T, float(G["min_t"]), "cuda", True)
    tape = noise.filled_tape(key, T - 1, 24, "cuda", forward=True)
    lp, lps = logp_confidence_score(*args, noise="device", noise_keys=key)
    lp_t, lps_t = logp_confidence_score(*args, noise_tape=tape)
    assert isinstance(lp, float) and len(lps) == T and np.isfinite(lp)
    assert lp == lp_t and lps == lps_t
    rev = noise.filled_tape(key, T - 1, 24, "cuda")  # the reverse purposes are other values
    assert logp_confidence_score(*args, noise_tape=rev)[0] != lp
    with pytest.raises(ValueError):
        logp_confidence_score(*args, noise="device", noise_keys=key, noise_tape=tape)


@time_limit(300)
def test_diffuser_reverse_takes_a_key_and_a_step():
    """SE3Diffuser.reverse(noise_key=, step=) for callers who step by hand: the same frames as reverse_device on the filled rows, and
    the global np.random stream is not touched."""
    from framedipt_amd import config, noise
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.rigid import Rigid
    d = SE3Diffuser(config.base_config().diffuser, device="cuda")
    g = torch.Generator().manual_seed(3)
    q = torch.nn.functional.normalize(torch.randn(2, 21, 4, generator=g), dim=-1)
    t7 = torch.cat([q, torch.randn(2, 21, 3, generator=g) * 5], -1).cuda()
    rs, ts = torch.randn(2, 21, 3, generator=g, dtype=torch.float64), torch.randn(2, 21, 3, generator=g)
    np.random.seed(9)
    state = np.random.get_state()[1].copy()
    out = d.reverse(Rigid.from_tensor_7(t7), rs, ts, 0.5, 0.01, noise_key=40, step=6, noise_scale=0.5)
    assert np.array_equal(np.random.get_state()[1], state)
    z = [noise.fill([40, 41], p, 1, 21, "cuda", k_begin=6)[0] for p in (noise.REVERSE_ROT, noise.REVERSE_TRANS)]
    want = d.reverse_device(t7, rs.cuda(), ts.cuda(), None, z[0], z[1], 0.5, 0.01, True, 0.5)
    assert torch.equal(out.get_trans(), want[..., 4:])
    with pytest.raises(ValueError):
        d.reverse(Rigid.from_tensor_7(t7), rs, ts, 0.5, 0.01, noise_key=40)


@time_limit(1500)
def test_run_sharded_device_noise_two_ranks(tmp_path):
    """run_sharded --noise device on two ranks sharing this GPU (fresh child processes, one after the other launch; FDIPT_ONE_GPU=1
    serialises their batches) writes the same files as one rank does, and other files than --noise host."""
    outs = {}
    for tag, world, port, noise in (("w2", 2, "29651", "device"), ("w1", 1, "29652", "device"), ("host", 1, "29653", "host")):
        out_dir = str(tmp_path / tag)
        env = dict(os.environ, FDIPT_ONE_GPU="1", MASTER_ADDR="127.0.0.1")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", port, "-m", "framedipt_amd.run_sharded", "--out-dir", out_dir, "--min-length", "24", "--max-length", "28",
               "--length-step", "2", "--samples-per-length", "2", "--num-t", "5", "--max-batch", "3", "--precision", "fp32",
               "--noise", noise]
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=450)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(os.path.join(out_dir, "manifest.json")) as f:
            man = json.load(f)
        assert man["noise"] == noise and man["n_items"] == 6 and man["world_size"] == world
        if world == 2:
            assert {s["rank"] for s in man["samples"]} == {0, 1}
        outs[tag] = {s["item"]: np.load(os.path.join(out_dir, s["file"]))["prot_traj"] for s in man["samples"]}
    for item in range(6):
        np.testing.assert_array_equal(outs["w1"][item], outs["w2"][item], err_msg=f"item {item}")
        assert np.abs(outs["w1"][item] - outs["host"][item]).max() > 1e-3
