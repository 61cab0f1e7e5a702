"""GPU tests (-m gpu) of kept-frame trajectories (``keep=``) and reusable sampling sessions (``ReverseLoop.reset``, ``inference.Session``).

Everything here is an equality of bits: a kept frame is the frame the ``keep="all"`` run of the same inputs holds at that step, and a
session call returns what a fresh call returns.  The shapes are the smallest that reach each addressing path (full-size network,
synthetic weights): num_t = 20 runs one-step replays, the 8-step chunk graph and the eager last step, num_t = 5 the one-step graph only;
N = 16 the edge_transition4 + pair_z path, N = 12 fewer than 16 keys, N = 45 the pad_to_four path (padded to 48); fp16, once fp32."""
import functools
import json
import os
import subprocess
import sys
import zipfile

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from test_gpu_parity import _feats, _net

pytestmark = pytest.mark.gpu

KEEPS = (1, 3, 7, "last")


def _host(v):
    return v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


@functools.lru_cache(maxsize=None)
def _model(precision, inpainting=False):
    from framedipt_amd import config
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    conf = config.base_config(inpainting=inpainting)
    d = SE3Diffuser(conf.diffuser, device="cuda")
    return ScoreNetwork(conf.model, d, inpainting=inpainting, precision=precision).load_synthetic(7).to("cuda"), d


def _batch(d, N, B, seed, T, gap=None):
    """B de novo samples of N residues (x_T and features from the sampler under ``seed``), a host noise tape and noise keys.
    ``gap=(b, i)``: sample b's residue numbering jumps by 200 at residue i (a chain break)."""
    from framedipt_amd import config, inference
    from framedipt_amd.sampler import UnconditionalSampler
    ds = UnconditionalSampler(config.to_conf({"min_length": N, "max_length": N, "length_step": 1, "samples_per_length": B}), d, "cuda")
    np.random.seed(seed)
    feats = {k: torch.cat([ds[i][2][k] for i in range(B)], 0) for k in ds[0][2]}
    if gap is not None:
        b, i = gap
        feats["seq_idx"] = feats["seq_idx"].clone()
        feats["seq_idx"][b, i:] += 200
    tape = inference.draw_noise_tape(d, T - 1, B, N)
    return feats, tape, [1000 * seed + b for b in range(B)]


def _check_contract(full, kept, keep, num_t, what):
    """The issue's contract between the keep="all" result and a kept one of the same call."""
    from framedipt_amd.inference import kept_steps
    s = num_t if keep == "last" else keep  # ("last" is row 0 of each: a stride no smaller than num_t)
    steps = kept_steps(num_t, keep)[::-1]
    np.testing.assert_array_equal(kept["kept_steps"], steps, err_msg=what)
    assert sorted(kept) == sorted(list(full) + ["kept_steps"]), what
    for k in full:
        a, b = _host(full[k]), _host(kept[k])
        if k == "psi_pred":
            want = a
        elif k == "rigid_traj":
            want = a[:num_t:s]
        else:
            want = a[::s]
        assert b.shape == want.shape and b.shape[0] == (1 if k == "psi_pred" else len(steps)), (what, k, b.shape, want.shape)
        np.testing.assert_array_equal(b, want, err_msg=f"{what}: {k}")


@pytest.mark.parametrize("N,num_t,precision", [(16, 20, "fp16"), (12, 20, "fp16"), (45, 20, "fp16"), (16, 5, "fp16"), (16, 20, "fp32")])
def test_kept_frames_equal_the_full_trajectory(N, num_t, precision):
    """keep in {1, 3, 7, "last"} against keep="all" for graph replays and eager launches, with and without the auxiliary trajectories, on
    the host tape and with device noise: every returned array bit for bit (B = 2)."""
    from framedipt_amd.inference import inference_fn
    net, d = _model(precision)
    feats, tape, keys = _batch(d, N, 2, 3, num_t)
    for noise in (dict(noise_tape=tape), dict(noise="device", noise_keys=keys)):
        first = None
        for graph in (True, False):
            for aux in (True, False):
                kw = dict(num_t=num_t, min_t=0.01, noise_scale=0.1, graph=graph, aux_traj=aux, **noise)
                full = inference_fn(net, d, feats, **kw)
                assert "kept_steps" not in full and full["prot_traj"].shape == (num_t, 2, N, 37, 3)
                if aux:  # (graph and eager agree with each other, as before)
                    first = first or full
                    for k in full:
                        np.testing.assert_array_equal(_host(full[k]), _host(first[k]), err_msg=f"graph={graph}: {k}")  # (psi_pred stays a device tensor)
                for keep in KEEPS:
                    kept = inference_fn(net, d, feats, keep=keep, **kw)
                    _check_contract(full, kept, keep, num_t, f"N={N} T={num_t} {precision} graph={graph} aux={aux} {sorted(noise)} keep={keep}")


def test_inpainting_with_a_separate_backbone_launch():
    """inference input_aatype=True on a model with input_aatype=False: the network sees 20 = unknown on the diffused residues, so the
    rigid_0_traj rows come from the separate cursor-addressed backbone launch (bb0_from_forward False) — the kept entry of it.
    Features: 48 residues of the four-chain inpainting golden around the first fixed / diffused boundary."""
    from framedipt_amd.inference import ReverseLoop, inference_fn
    G = load_golden("fwd_full_inpaint_n724_4chain.npz")
    fixed = G["in_fixed_mask"][0]
    edge = int(np.flatnonzero(np.diff(fixed) != 0)[0])
    lo = min(max(edge - 23, 0), fixed.shape[0] - 48)
    feats = {k: v[:, lo:lo + 48].contiguous() for k, v in _feats(G).items() if k != "t"}
    assert 0 < float(feats["fixed_mask"].sum()) < 48
    net, d = _model("fp16", inpainting=True)
    assert not net._model_conf.input_aatype
    num_t = 20
    np.random.seed(5)
    from framedipt_amd import inference
    tape = inference.draw_noise_tape(d, num_t - 1, 1, 48)
    base = dict(num_t=num_t, min_t=0.01, noise_scale=0.1, aux_traj=True, inpainting=True, input_aatype=True, noise_tape=tape)
    assert not ReverseLoop(net, d, feats, keep=3, **base).bb0_from_forward
    for graph in (True, False):
        full = inference_fn(net, d, feats, graph=graph, **base)
        for keep in (3, "last"):
            _check_contract(full, inference_fn(net, d, feats, graph=graph, keep=keep, **base), keep, num_t, f"inpainting graph={graph} keep={keep}")


def test_verified_steps_keep_the_same_frames():
    """verify=4 (every fourth step runs eagerly with its forward twice) with keep=3 equals the unverified run."""
    from framedipt_amd.inference import inference_fn
    net, d = _model("fp16")
    feats, tape, _ = _batch(d, 16, 2, 3, 20)
    kw = dict(num_t=20, min_t=0.01, noise_scale=0.1, aux_traj=True, noise_tape=tape, keep=3)
    plain, verified = inference_fn(net, d, feats, **kw), inference_fn(net, d, feats, verify=4, **kw)
    assert sorted(plain) == sorted(verified)
    for k in plain:
        np.testing.assert_array_equal(_host(plain[k]), _host(verified[k]), err_msg=k)


def test_buffers_are_sized_to_the_kept_frames():
    """keep="last": one frame per kept array plus the two-row state; a stride: n_kept rows; keep="all": the shapes it always had."""
    from framedipt_amd.inference import ReverseLoop, kept_steps
    net, d = _model("fp16")
    feats, tape, _ = _batch(d, 16, 2, 3, 20)
    kw = dict(num_t=20, min_t=0.01, aux_traj=True, noise_tape=tape)
    for keep in ("last", 3, 1):
        n = len(kept_steps(20, keep))
        lp = ReverseLoop(net, d, feats, keep=keep, **kw)
        assert lp.rigid_traj.shape == (2, 2, 16, 7) and lp.kept_rigids.shape == (n, 2, 16, 7)
        assert lp.prot_traj.shape == lp.bb0_traj.shape == (n, 2, 16, 37, 3) and lp.trans_traj.shape == (n, 2, 16, 3)
        assert lp.frame_rows.dtype == torch.int32 and lp.frame_rows.shape == (20,)
        rows = lp.frame_rows.cpu().numpy()
        np.testing.assert_array_equal(np.flatnonzero(rows >= 0), kept_steps(20, keep))
        np.testing.assert_array_equal(rows[rows >= 0], np.arange(n))
    assert ReverseLoop(net, d, feats, keep="last", **dict(kw, aux_traj=False)).kept_rigids is None
    lp = ReverseLoop(net, d, feats, **kw)
    assert lp.rigid_traj.shape == (21, 2, 16, 7) and lp.prot_traj.shape == lp.bb0_traj.shape == (20, 2, 16, 37, 3)
    assert lp.trans_traj.shape == (20, 2, 16, 3) and lp.frame_rows is None and lp.kept_rigids is None
    with pytest.raises(ValueError):
        ReverseLoop(net, d, feats, keep=0, **kw)


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        np.testing.assert_array_equal(_host(a[k]), _host(b[k]), err_msg=f"{what}: {k}")


@pytest.mark.parametrize("keep,noise", [("all", "host"), (3, "host"), ("last", "device")])
def test_session_reuses_buffers_and_graphs(keep, noise):
    """Two different batches (x_T, masks, seq_idx with a chain gap in another sample, noise) through one Session: each result equals
    a fresh call without a session, and the second call captures no graph.  A third call with another N makes a second loop; a batch
    whose residue-number range differs is exact too (that one captures again: the range is a launch scalar).  Device results of call
    1 are unchanged after the later calls.  session= with streams=2 raises."""
    from framedipt_amd.inference import Session, inference_fn
    net, d = _model("fp16")
    T = 20
    kw = dict(num_t=T, min_t=0.01, noise_scale=0.1, aux_traj=True, keep=keep)

    def how(tape, keys):
        return dict(noise="device", noise_keys=keys) if noise == "device" else dict(noise_tape=tape)

    fa, ta, ka = _batch(d, 16, 2, 3, T, gap=(0, 5))
    fb, tb, kb = _batch(d, 16, 2, 4, T, gap=(1, 8))
    fb["res_mask"] = fb["res_mask"].clone()
    fb["res_mask"][1, -2:] = 0  # (another mask: two masked residues at the end of sample 1)
    assert not torch.equal(fa["rigids_t"], fb["rigids_t"]) and not torch.equal(fa["seq_idx"], fb["seq_idx"])
    fresh_a, fresh_b = inference_fn(net, d, fa, **kw, **how(ta, ka)), inference_fn(net, d, fb, **kw, **how(tb, kb))
    assert np.abs(fresh_a["prot_traj"][0] - fresh_b["prot_traj"][0]).max() > 1e-3
    with Session() as sess:
        r1 = inference_fn(net, d, fa, session=sess, return_device=True, **kw, **how(ta, ka))
        r1_then = {k: _host(v).copy() for k, v in r1.items()}
        (loop,) = sess.loops.values()
        captures = loop.captures
        assert captures > 0 and loop.capture_seconds > 0 and (sess.hits, sess.misses) == (0, 1)
        _same(fresh_a, r1_then, "session call 1")
        r2 = inference_fn(net, d, fb, session=sess, **kw, **how(tb, kb))
        _same(fresh_b, r2, "session call 2 (reset loop)")
        assert list(sess.loops.values()) == [loop] and loop.captures == captures and (sess.hits, sess.misses) == (1, 1)
        _same(r1_then, r1, "device results of call 1 after call 2")
        # another N: a second loop
        fc, tc, kc = _batch(d, 12, 2, 5, T)
        r3 = inference_fn(net, d, fc, session=sess, **kw, **how(tc, kc))
        _same(inference_fn(net, d, fc, **kw, **how(tc, kc)), r3, "session call 3 (another N)")
        assert len(sess.loops) == 2 and sess.misses == 2
        # back to the first shape, with another residue-number range (no gap): still exact
        fd_, td, kd = _batch(d, 16, 2, 6, T)
        r4 = inference_fn(net, d, fd_, session=sess, **kw, **how(td, kd))
        _same(inference_fn(net, d, fd_, **kw, **how(td, kd)), r4, "session call 4 (another index range)")
        assert sess.hits == 2 and len(sess.loops) == 2
        _same(r1_then, r1, "device results of call 1 after call 4")
        with pytest.raises(ValueError):
            inference_fn(net, d, fa, session=sess, streams=2, experimental_streams=True, **kw, **how(ta, ka))
    assert len(sess.loops) == 0


def test_reset_refuses_what_changes_the_launch_sequence():
    """Another shape, another noise mode, or a batch that switches who builds the rigid_0_traj rows raise instead of replaying stale graphs."""
    from framedipt_amd.inference import ReverseLoop
    net, d = _model("fp16")
    fa, ta, ka = _batch(d, 16, 2, 3, 20)
    lp = ReverseLoop(net, d, fa, 20, 0.01, aux_traj=True, noise_tape=ta, state=net.new_batch_state(fa["seq_idx"]))
    fc, tc, _ = _batch(d, 12, 2, 5, 20)
    with pytest.raises(ValueError):
        lp.reset(fc, noise_tape=tc)
    with pytest.raises(ValueError):
        lp.reset(fa, noise_keys=ka)
    with pytest.raises(ValueError):
        lp.reset(fa, noise_tape=(ta[0][:5], ta[1][:5]))
    lp.reset(fa, noise_tape=ta)  # (and the loop is still usable)


def test_reset_of_a_default_constructed_loop_leaves_the_model_cache_right():
    """A loop built without state= shares the model's cached BatchState; reset() to a batch with other residue numbers must not leave
    that cache answering for the first batch: a fresh call on the first batch afterwards equals its earlier result, the reset loop
    equals a fresh call on the second batch, and a failed reset leaves a session's loop cached."""
    from framedipt_amd.inference import ReverseLoop, Session, inference_fn
    net, d = _model("fp16")
    fa, ta, _ = _batch(d, 16, 2, 3, 20)
    fb, tb, _ = _batch(d, 16, 2, 4, 20, gap=(1, 8))
    kw = dict(num_t=20, min_t=0.01, noise_scale=0.1, aux_traj=True, keep=3)
    before_a = inference_fn(net, d, fa, noise_tape=ta, **kw)
    fresh_b = inference_fn(net, d, fb, noise_tape=tb, **kw)
    lp = ReverseLoop(net, d, fa, noise_tape=ta, **kw)
    assert lp.st is net.batch_state(fa["seq_idx"])
    _same(before_a, lp.run().results(), "default-constructed loop")
    _same(fresh_b, lp.reset(fb, noise_tape=tb).run().results(), "the same loop after reset")
    _same(before_a, inference_fn(net, d, fa, noise_tape=ta, **kw), "fresh call on the first batch after the reset")
    assert net.batch_state(fa["seq_idx"]) is not lp.st
    with Session() as sess:
        inference_fn(net, d, fa, noise_tape=ta, session=sess, **kw)
        (loop,) = sess.loops.values()
        with pytest.raises(ValueError):
            inference_fn(net, d, fb, noise_tape=(tb[0][:5], tb[1][:5]), session=sess, pad_to_four=False, **kw)
        assert list(sess.loops.values()) == [loop]
        _same(fresh_b, inference_fn(net, d, fb, noise_tape=tb, session=sess, **kw), "the session loop after a refused reset")
        assert loop.captures > 0 and sess.hits == 1


@pytest.mark.parametrize("cached_score", [False, True])
def test_kept_rows_with_the_launch_folds_off(cached_score):
    """FDIPT_KF_UNFOLDED: the forward builds the rigid_0_traj row by its own backbone launch (no fold into the score tail) — keep=3 and
    "last" against keep="all", graph and eager.  With so3.use_cached_score the score launch also reads its table row at the cursor (the
    one row offset that only rot_score_kernel applies)."""
    from framedipt_amd import _lib, config
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.inference import inference_fn
    from framedipt_amd.model import ScoreNetwork
    conf = config.base_config()
    conf.diffuser.so3.use_cached_score = cached_score
    d = SE3Diffuser(conf.diffuser, device="cuda")
    net = ScoreNetwork(conf.model, d, precision="fp16", kernel_flags=_lib.KF_UNFOLDED).load_synthetic(7).to("cuda")
    feats, tape, _ = _batch(d, 16, 2, 3, 20)
    for graph in (True, False):
        kw = dict(num_t=20, min_t=0.01, noise_scale=0.1, aux_traj=True, noise_tape=tape, graph=graph)
        full = inference_fn(net, d, feats, **kw)
        for keep in (3, "last"):
            _check_contract(full, inference_fn(net, d, feats, keep=keep, **kw), keep, 20, f"unfolded graph={graph} keep={keep}")


def test_session_drops_the_least_recently_used_loop():
    from framedipt_amd.inference import Session, inference_fn
    net, d = _model("fp16")
    sess = Session(max_loops=1)
    for N in (16, 12):
        f, t, _ = _batch(d, N, 1, 3, 5)
        inference_fn(net, d, f, num_t=5, min_t=0.01, noise_tape=t, keep="last", session=sess)
        assert len(sess.loops) == 1 and next(iter(sess.loops.values())).N == N
    with pytest.raises(ValueError):
        Session(max_loops=0)


def test_run_sharded_keep_last_two_ranks(tmp_path):
    """run_sharded on two ranks sharing this GPU (FDIPT_ONE_GPU=1), as test_run_sharded_torchrun_entry_two_ranks launches it: --keep last
    writes the final structures --keep all writes.  The per-sample files are .npz archives, whose zip headers carry the time of
    writing; every member (the .npy files inside) is compared byte for byte."""
    members = {}
    for keep, port in (("last", "29661"), ("all", "29662")):
        out_dir = str(tmp_path / keep)
        env = dict(os.environ, FDIPT_ONE_GPU="1", MASTER_ADDR="127.0.0.1")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", port, "-m", "framedipt_amd.run_sharded", "--out-dir", out_dir, "--min-length", "24", "--max-length", "28",
               "--length-step", "4", "--samples-per-length", "4", "--num-t", "5", "--max-batch", "2", "--precision", "fp16", "--keep", keep]
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(os.path.join(out_dir, "manifest.json")) as f:
            man = json.load(f)
        assert man["n_items"] == 8 and {s["rank"] for s in man["samples"]} == {0, 1} and man.get("keep", "all") == keep
        members[keep] = {}
        for s in man["samples"]:
            with zipfile.ZipFile(os.path.join(out_dir, s["file"])) as z:
                members[keep][s["file"]] = {n: z.read(n) for n in z.namelist()}
            assert np.load(os.path.join(out_dir, s["file"]))["prot_traj"].shape == (s["n_res"], 37, 3)
    assert sorted(members["last"]) == sorted(members["all"]) and len(members["all"]) == 8
    for f in members["all"]:
        assert members["last"][f] == members["all"][f], f
