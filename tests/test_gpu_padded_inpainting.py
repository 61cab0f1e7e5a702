"""GPU parity tests (-m gpu) of the padded inpainting path against the reference: inference_fn's default pad_to_four on two-chain
inpainting inputs whose length is no multiple of four, and mixed-length batches of different complexes (sharding.stack_items_padded),
against trajectories recorded from the reference (tests/golden/make_goldens_padded.py: N = 45, 42, 126, 122, T = 4, the reference's
default inpainting configuration).  Every run is free-running on the fixture's noise tape.

Bars (per sample, worst step): backbone RMSD of prot_traj and rigid_0_traj below 1e-3 A in fp16 / fp16x and 1e-4 A in fp32 — the bars of
test_gpu_round3.py::test_inpainting_trajectory_with_inference_side_aatype.  The translations of rigid_traj and trans_traj and the psi
prediction take the per-forward bounds of tests/test_gpu_sizes.py, which a T = 4 trajectory with a 0.1 noise scale has to keep: largest
CA coordinate error 3e-4 A (fp32, test_forward_fp32_at_size) / 5e-4 A (half precision, FP16_BOUND["ca"]), psi angle 3e-4 rad at worst
(fp32) / 5e-4 rad RMS over the diffused residues (half precision, FP16_BOUND["psi_rms"]).  Motif rows of rigid_traj stay on the input
frames: translations to 1e-4 A (test_baseline_config_shapes_run, test_inpainting_on_real_complex_keeps_the_motif), quaternions to 1e-5
up to sign (the forward tests' bound).  `-s` prints every figure next to its bound.

The inpainting model embeds aatype, so the edge embedder's row table never serves it (tests/test_padded_inpainting_host.py); the table
path runs on the same mixed, padded features in test_row_table_on_a_mixed_padded_batch_equals_the_pair_kernel, on a network without
aatype features, against the per-pair kernel these reference runs pin."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import kabsch_free_rmsd, load_golden
from padded_inpainting_cases import FIXTURES, PAIRS, SAMPLER_KEYS, hand_item, tape_of
from test_gpu_parity import _feats, _net

pytestmark = pytest.mark.gpu

HALF = ("fp16", "fp16x")
BAR = {"fp32": 1e-4, "fp16": 1e-3, "fp16x": 1e-3}      # worst step backbone RMSD, A
CA = {"fp32": 3e-4, "fp16": 5e-4, "fp16x": 5e-4}       # largest translation coordinate error, A
PSI = {"fp32": 3e-4, "fp16": 5e-4, "fp16x": 5e-4}      # rad: fp32 the worst residue, half precision RMS over the diffused residues
TRAJ = ("prot_traj", "rigid_traj", "trans_traj", "psi_pred", "rigid_0_traj")
N45, N126 = "full_inpaint_n45_T4_aatype", "full_inpaint_n126_T4_aatype"

_GOLDEN, _NETS, _RUNS = {}, {}, {}


def _golden(name):
    if name not in _GOLDEN:
        _GOLDEN[name] = load_golden(f"traj_{name}.npz")
    return _GOLDEN[name]


def _network(prec):
    """One inpainting network per precision mode: the fixtures share weights (weight seed, bb_gain) and configuration."""
    if prec not in _NETS:
        G = _golden(N45)
        assert all(int(_golden(n)["weight_seed"]) == int(G["weight_seed"]) and float(_golden(n)["bb_gain"]) == float(G["bb_gain"]) for n in FIXTURES)
        net, d, conf = _net(N45, G, prec)
        assert not conf.model.input_aatype and net.inpainting
        _NETS[prec] = (net, d)
    return _NETS[prec]


def _kw(G, **over):
    kw = dict(num_t=int(G["num_t"]), min_t=float(G["min_t"]), aux_traj=True, noise_scale=float(G["noise_scale"]), inpainting=True,
              input_aatype=True)
    kw.update(over)
    return kw


def _host(res):
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in res.items()}


def _run(name, prec, how="auto"):
    """One fixture alone through inference_fn, computed once per (fixture, precision, route): "auto" the default pad_to_four,
    "plain" pad_to_four=False, an integer: padded by hand to that length (sharding.pad_item) and returned uncut."""
    key = (name, prec, how)
    if key not in _RUNS:
        from framedipt_amd import inference, sharding
        G = _golden(name)
        net, d = _network(prec)
        feats, tape = _feats(G), tape_of(G)
        if isinstance(how, int):
            feats, tape = sharding.pad_item(feats, tape, how)
        _RUNS[key] = _host(inference.inference_fn(net, d, feats, noise_tape=tape, pad_to_four=how != "plain", **_kw(G)))
        st = net._state  # (the loop of that call ran on the network's cached batch state)
        _RUNS[("shape",) + key] = (st.B, st.N, st.n_rel)
    return _RUNS[key]


def _psi_err(a, b):
    ang = lambda p: np.arctan2(p[..., 0], p[..., 1])  # noqa: E731
    return np.abs(np.angle(np.exp(1j * (ang(a) - ang(b)))))


def _against_the_reference(tag, res, G, prec, rmsd_bar=None):
    """``res``: one sample's returned arrays cut to its own N residues ([T, 1, N, ...]).  Shapes, the zero pattern of the atoms, the motif
    rows, and every figure against its bound; returns the figures."""
    n, T = G["in_rigids_t"].shape[1], int(G["num_t"])
    fixed = G["in_fixed_mask"][0] == 1
    for k in TRAJ:
        assert tuple(res[k].shape) == tuple(G["res_" + k].shape), (tag, k, res[k].shape)
        assert res[k].shape[2] == n and np.isfinite(res[k]).all(), (tag, k)
    figs = {}
    for k in ("prot_traj", "rigid_0_traj"):
        ref = G["res_" + k]
        # atoms the reference leaves at zero (GLY CB, every side-chain slot) are zero here too
        np.testing.assert_array_equal(res[k] == 0, ref == 0, err_msg=f"{tag} {k}")
        figs[k] = (max(kabsch_free_rmsd(res[k][s], ref[s]) for s in range(T)), rmsd_bar or BAR[prec])
    figs["rigid_traj trans"] = (float(np.abs(res["rigid_traj"][..., 4:] - G["res_rigid_traj"][..., 4:]).max()), CA[prec])
    figs["trans_traj"] = (float(np.abs(res["trans_traj"] - G["res_trans_traj"]).max()), CA[prec])
    pe = _psi_err(res["psi_pred"][0, 0], G["res_psi_pred"][0, 0])
    figs["psi_pred"] = (float(pe.max()) if prec == "fp32" else float(np.sqrt((pe[~fixed] ** 2).mean())), PSI[prec])
    # motif rows never move: every row of rigid_traj (x_T first, the x_0 prediction last) holds the input frames there
    x_in = G["in_rigids_t"][0]
    figs["motif trans"] = (float(np.abs(res["rigid_traj"][:, 0, fixed, 4:] - x_in[fixed, 4:]).max()), 1e-4)
    figs["motif quat"] = (float(np.abs(np.abs(res["rigid_traj"][:, 0, fixed, :4]) - np.abs(x_in[fixed, :4])).max()), 1e-5)
    print(f"{tag}: " + ", ".join(f"{k} {v:.2e} (< {b:.0e})" for k, (v, b) in figs.items()))
    for k, (v, b) in figs.items():
        assert v < b, (tag, k, v, b)
    return figs


def _same_bits(tag, a, b, keys=TRAJ):
    for k in keys:
        assert a[k].shape == b[k].shape, (tag, k, a[k].shape, b[k].shape)
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{tag}: {k}")


def _cut(res, b, n):
    """Sample ``b`` of a batch's arrays ([T, B, N_pad, ...]) cut to its own length: what a B = 1 run of it returns."""
    return {k: v[:, b:b + 1, :n] for k, v in res.items() if k != "kept_steps"}


# ------------------------------------------------------------------ 1. one padded sample against the reference
@pytest.mark.parametrize("prec", HALF)
@pytest.mark.parametrize("name", [N45, N126])
def test_padded_sample_against_the_reference(name, prec):
    """The default path: N = 45 runs at 48 and N = 126 at 128 (masked rows behind the sample), cut back to N."""
    n, gap, n_pad, n_rel = FIXTURES[name]
    res = _run(name, prec)
    net, _ = _network(prec)
    _against_the_reference(f"{prec} N={n} padded to {n_pad}", res, _golden(name), prec)
    assert _RUNS["shape", name, prec, "auto"] == (1, n_pad, n_rel)  # it ran padded, and pad rows did not widen the relative positions
    # the inpainting model embeds aatype: the row table declines, every pair is evaluated (tests/test_padded_inpainting_host.py)
    from framedipt_amd import _lib
    assert int(_lib.load().fdipt_embed_table_rows(C.byref(net.dims), 1, n_pad, n_rel)) == 0 and net.dims.use_aatype == 1


@pytest.mark.parametrize("name", [N45, N126])
def test_unpadded_fall_back_kernels_against_the_reference(name):
    """pad_to_four=False in fp16: the kernels of lengths that are no multiple of four, as shipped before padding was the default.
    (fp16x has none: it refuses such a length.)"""
    res = _run(name, "fp16", "plain")
    _against_the_reference(f"fp16 N={FIXTURES[name][0]} unpadded", res, _golden(name), "fp16")
    assert not np.array_equal(res["prot_traj"], _run(name, "fp16")["prot_traj"])  # (other kernels than the padded run's)


@pytest.mark.parametrize("name", [N45, N126])
def test_fp32_ragged_inpainting_length_against_the_reference(name):
    """fp32 never pads: a two-chain inpainting input at a ragged length on the fp32 kernels, at the fp32 bars."""
    from framedipt_amd import inference
    res = _run(name, "fp32")
    _against_the_reference(f"fp32 N={FIXTURES[name][0]}", res, _golden(name), "fp32")
    G = _golden(name)
    net, d = _network("fp32")
    again = _host(inference.inference_fn(net, d, _feats(G), noise_tape=tape_of(G), pad_to_four=False, **_kw(G)))
    _same_bits("fp32: pad_to_four has no say", res, again)


# ------------------------------------------------------------------ 2. padded by the default = padded by hand
@pytest.mark.parametrize("prec", HALF)
@pytest.mark.parametrize("name", [N45, N126])
def test_default_padding_equals_padding_by_hand(name, prec):
    """The automatic run against sharding.pad_item to the same length followed by a cut, and against eight rows more (56 / 136: the same
    kernel-selection class): bit-identical on every returned key."""
    from framedipt_amd import sharding
    n, _, n_pad, _ = FIXTURES[name]
    auto = _run(name, prec)
    assert sharding.kernel_class(n_pad) == sharding.kernel_class(n_pad + 8)
    for to in (n_pad, n_pad + 8):
        hand = _run(name, prec, to)
        assert set(hand) == set(auto) and all(hand[k].shape[2] == to for k in TRAJ)
        _same_bits(f"{prec} N={n}: by hand to {to}", auto, _cut(hand, 0, n))
        assert all(np.isfinite(hand[k]).all() for k in TRAJ)  # (the pad rows too)


# ------------------------------------------------------------------ 3. mixed-length batches of different complexes
def _batch(pair, prec, order):
    key = ("batch", pair, prec, order)
    if key not in _RUNS:
        from framedipt_amd import inference, sharding
        names = [PAIRS[pair][i] for i in order]
        items = [(nm, 0, _feats(_golden(nm)), tape_of(_golden(nm))) for nm in names]
        feats, tape, lengths = sharding.stack_items_padded(items)
        assert lengths == [FIXTURES[nm][0] for nm in names] and feats["rigids_t"].shape[:2] == (2, PAIRS[pair][2])
        net, d = _network(prec)
        res = inference.inference_fn(net, d, feats, noise_tape=tape, return_device=True, **_kw(_golden(names[0])))
        assert all(torch.is_tensor(res[k]) and res[k].is_cuda for k in TRAJ)
        _RUNS[key] = _host(res)
    return _RUNS[key]


@pytest.mark.parametrize("prec", HALF)
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_mixed_length_batch_against_the_reference(pair, prec):
    """Two different complexes (own seq_idx, chain split, diffused windows, aatype) in one padded batch: each within the bars of its own
    fixture, bit-identical to its own default B = 1 run (44 / 48 and 124 / 128 rows: one kernel-selection class), pad rows finite before
    any cut, and the batch order does not matter."""
    from framedipt_amd import sharding
    a, b, n_pad = PAIRS[pair]
    both = _batch(pair, prec, (0, 1))
    for k in TRAJ:
        assert both[k].shape[1:3] == (2, n_pad) and np.isfinite(both[k]).all(), k  # (pad rows of the shorter sample included)
    for i, name in enumerate((a, b)):
        n = FIXTURES[name][0]
        assert sharding.kernel_class(n) == sharding.kernel_class(n_pad)
        one = _cut(both, i, n)
        _against_the_reference(f"{prec} N={n} in a batch of {n_pad} rows", one, _golden(name), prec)
        _same_bits(f"{prec} N={n}: batch of {n_pad} rows against its own run", one, _run(name, prec))
    swapped = _batch(pair, prec, (1, 0))
    _same_bits(f"{prec} {pair}: order swapped", {k: both[k][:, ::-1] for k in TRAJ}, swapped)


# ------------------------------------------------------------------ 4. the un-pad step
@pytest.mark.parametrize("prec", HALF)
def test_every_returned_key_is_cut_back_to_the_real_length(prec):
    """Every key inference_fn returns for an inpainting call — aux_traj on and off, keep="all" / "last" / a stride, host and device
    arrays — carries the N = 45 real residues on axis 2, kept_steps passes through, and the kept rows are the full run's."""
    from framedipt_amd import inference
    G = _golden(N45)
    n, T = 45, int(G["num_t"])
    net, d = _network(prec)
    full = _run(N45, prec)
    assert sorted(full) == sorted(TRAJ)
    assert full["prot_traj"].shape == (T, 1, n, 37, 3) and full["rigid_0_traj"].shape == (T, 1, n, 37, 3)
    assert full["rigid_traj"].shape == (T + 1, 1, n, 7) and full["trans_traj"].shape == (T, 1, n, 3) and full["psi_pred"].shape == (1, 1, n, 2)
    call = lambda **over: inference.inference_fn(net, d, _feats(G), noise_tape=tape_of(G), **_kw(G, **over))  # noqa: E731
    for keep in ("last", 2):
        steps = inference.kept_steps(T, keep)[::-1]
        got = call(keep=keep)
        assert sorted(got) == sorted(TRAJ + ("kept_steps",))
        np.testing.assert_array_equal(got["kept_steps"], steps)
        got = _host(got)
        rows = [T - 1 - int(k) for k in steps]  # (flipped arrays: row 0 = the final step)
        for k in TRAJ:
            assert got[k].shape[2] == n and got[k].shape[0] == (1 if k == "psi_pred" else len(steps)), (keep, k, got[k].shape)
            want = full[k] if k == "psi_pred" else full[k][rows]  # (rigid_traj: x_{t-1} of the kept steps = the same rows, no x_T row)
            np.testing.assert_array_equal(got[k], want, err_msg=f"keep={keep}: {k}")
    lean = call(aux_traj=False)
    assert sorted(lean) == ["prot_traj"] and lean["prot_traj"].shape == (T, 1, n, 37, 3)
    np.testing.assert_array_equal(lean["prot_traj"], full["prot_traj"])
    on_dev = call(return_device=True, keep="last")
    assert all(torch.is_tensor(on_dev[k]) and on_dev[k].shape[2] == n for k in TRAJ) and not torch.is_tensor(on_dev["kept_steps"])
    np.testing.assert_array_equal(on_dev["prot_traj"].cpu().numpy(), full["prot_traj"][:1])


def test_the_samplers_own_dict_goes_through_the_padded_path():
    """ConditionalSampler's item (its complete key set: rigids_0 and t ride along) at N = 45: the keys and shapes the host test's hand-made
    dict stands for, and the fp16 default run (padded to 48) beside the fp32 run of the same item (ragged, never padded).  No reference
    run exists for this item; two runs that each keep their bar against it differ by less than the sum of the bars, 1.1e-3 A."""
    import bench
    from framedipt_amd import inference
    from framedipt_amd.sampler import ConditionalSampler
    n, T = 45, 4
    (net, d), (net32, _) = _network("fp16"), _network("fp32")
    ds = ConditionalSampler.from_features([("synthetic", bench.synthetic_complex((22, 23), ((3, 8), (38, 42)), seed=4))], d, "cuda", samples=1)
    np.random.seed(11)
    _, _, feats = ds[0]
    want, _ = hand_item(n, seed=0)
    assert sorted(feats) == sorted(SAMPLER_KEYS)
    for k in SAMPLER_KEYS:
        assert tuple(feats[k].shape) == tuple(want[k].shape), (k, feats[k].shape)
    tape = inference.draw_noise_tape(d, T - 1, 1, n)
    kw = dict(num_t=T, min_t=0.01, aux_traj=True, noise_scale=0.1, inpainting=True, input_aatype=True, noise_tape=tape)
    half, full = _host(inference.inference_fn(net, d, feats, **kw)), _host(inference.inference_fn(net32, d, feats, **kw))
    fixed = feats["fixed_mask"][0].bool().cpu().numpy()
    for k in TRAJ:
        assert half[k].shape == full[k].shape and half[k].shape[2] == n, k
    for k in ("prot_traj", "rigid_0_traj"):
        np.testing.assert_array_equal(half[k] == 0, full[k] == 0, err_msg=k)
        worst = max(kabsch_free_rmsd(half[k][s], full[k][s]) for s in range(T))
        print(f"sampler item N=45: fp16 (padded to 48) against fp32 (unpadded), {k}: worst step {worst:.2e} A (< 1.1e-03)")
        assert worst < 1.1e-3, (k, worst)
    x0 = feats["rigids_0"][0].cpu().numpy()
    np.testing.assert_allclose(half["rigid_traj"][:, 0, fixed, 4:], np.broadcast_to(x0[fixed, 4:], (T + 1,) + x0[fixed, 4:].shape), atol=1e-4)


# ------------------------------------------------------------------ 5. the row table on the same mixed, padded features
@pytest.mark.parametrize("prec", HALF)
def test_row_table_on_a_mixed_padded_batch_equals_the_pair_kernel(prec):
    """The edge embedder's row table (a network without aatype features takes it at N = 128, n_rel = 291) on the stacked N = 126 / 122
    fixtures: every sample its own seq_idx, chain split and fixed-mask classes, pad rows with fixed_mask = 0, res_mask = 0 and the last
    real index.  One forward through the table against the same forward with every pair evaluated (FdiptForwardArgs.pair_embed = 1: the
    kernel the inpainting runs above pin to the reference), bit for bit; and each sample alone (128 / 124 rows, n_rel 291 / 283: its own
    table) against its rows of the batch, bit for bit."""
    from framedipt_amd import config, sharding
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from test_gpu_embed_table import OUT, _compare, _forward
    conf = config.base_config()
    net = ScoreNetwork(conf.model, SE3Diffuser(conf.diffuser, device="cuda"), precision=prec).load_synthetic(7).to("cuda")
    assert net.dims.use_aatype == 0
    a, b, n_pad = PAIRS["n126_n122"]

    def inputs(items, t):
        feats, _, lengths = sharding.stack_items_padded(items)
        f = {k: v.cpu().numpy() for k, v in feats.items()}
        rigids = f["rigids_t"].astype(np.float32)
        mask = f["res_mask"].astype(np.float32)
        return dict(seq=f["seq_idx"].astype(np.int64), fixed=f["fixed_mask"].astype(np.float32), mask=mask, rigids=rigids,
                    sc=(rigids[..., 4:] + 0.5) * mask[..., None], psi=f["torsion_angles_sin_cos"][..., 2, :].astype(np.float32),
                    t=np.full(len(lengths), t)), lengths

    items = [(nm, 0, _feats(_golden(nm)), tape_of(_golden(nm))) for nm in (a, b)]
    x, lengths = inputs(items, 0.37)
    assert x["seq"].shape == (2, n_pad) and (x["mask"][1, lengths[1]:] == 0).all() and (x["fixed"][1, lengths[1]:] == 0).all()
    assert not np.array_equal(x["seq"][0], x["seq"][1]) and not np.array_equal(x["fixed"][0], x["fixed"][1])
    (table, rows), (pairs, _) = _forward(net, x, 0), _forward(net, x, 1)
    assert rows == 291 * 23, "the predicate declined the batch"
    assert _compare(f"{prec} mixed batch N=126/122 at {n_pad} rows", table, pairs), "not bit-identical"
    for i, it in enumerate(items):
        x1, (n,) = inputs([it], 0.37)
        alone, rows1 = _forward(net, x1, 0)
        assert rows1 == (FIXTURES[it[0]][3]) * 23 and x1["seq"].shape[1] == FIXTURES[it[0]][2]
        for k in OUT:
            got, want = (table[k][:, i, :n], alone[k][:, 0, :n]) if k == "trace_node" else (table[k][i, :n], alone[k][0, :n])
            np.testing.assert_array_equal(got, want, err_msg=f"{prec} sample {i} alone: {k}")
