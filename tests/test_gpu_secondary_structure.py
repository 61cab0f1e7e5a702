"""GPU tests (-m gpu) of the secondary structure (framedipt_amd/secondary_structure.py -> fdipt_sample_dssp, csrc/dssp.hip) against the
NumPy restatement tests/dssp_ref.py on the fixture tests/golden/dssp_cases.npz.  Every integer output, the fractions (ratios of
integers) and the rounded energies are compared exactly."""
import functools

import numpy as np
import pytest
import torch

import dssp_ref as dr
from conftest import load_golden

pytestmark = pytest.mark.gpu

PRO = 14
ARRAYS = ("ss", "acceptor", "acceptor_energy")
SCALARS = ("n_rows", "n_hbonds", "n_bridges", "n_ladders", "status") + dr.FRACTIONS


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("dssp_cases.npz")


def _atom37(bb):
    """[..., 4, 3] (N, CA, C, O) -> [..., 37, 3] float32 with CB and the other columns zero."""
    out = np.zeros(bb.shape[:-2] + (37, 3), dtype=np.float32)
    out[..., [0, 1, 2, 4], :] = bb
    return out


def _call(bb, res_mask=None, chain_idx=None, is_proline=None, atoms=37, device=False):
    """One launch for bb [B,n,4,3]; the proline flag travels as aatype (14: proline, 0 otherwise)."""
    from framedipt_amd import secondary_structure as sec
    prot = _atom37(np.asarray(bb, dtype=np.float32))
    if atoms == 5:
        prot = np.ascontiguousarray(prot[:, :, :5])
    aatype = None if is_proline is None else np.where(np.asarray(is_proline) != 0, PRO, 0).astype(np.int64)
    if device:
        prot = torch.from_numpy(prot).cuda()
    return sec.secondary_structure(prot, res_mask, chain_idx, aatype)


@functools.lru_cache(maxsize=None)
def _stated(name):
    return dr.dssp(**dr.case_inputs(_fix(), name))


@functools.lru_cache(maxsize=None)
def _single(name):
    inp = dr.case_inputs(_fix(), name)
    return _call(inp["bb"][None], None, inp["chain_idx"][None], inp["is_proline"][None])


def _check(got, b, want, what=""):
    """Sample b of a device result against one restatement result, exactly."""
    n = len(want["ss"])
    for k in ARRAYS:
        x = np.asarray(got[k][b])
        assert np.array_equal(x[:n], want[k]), (what, k, np.flatnonzero((x[:n] != want[k]).reshape(n, -1).any(1))[:10])
        assert (x[n:] == (dr.ABSENT if k == "ss" else -1 if k == "acceptor" else 0)).all(), (what, k)
    for k in SCALARS:
        assert np.array_equal(got[k][b], want[k], equal_nan=True), (what, k, got[k][b], want[k])
    assert got["ss_string"][b] == dr.ss_string(want["ss"]), what


def _same_sample(a, i, b, j, n):
    for k in ARRAYS:
        x, y = np.asarray(a[k][i]), np.asarray(b[k][j])
        assert x.dtype == y.dtype and np.array_equal(x[:n], y[:n]), k
    for k in SCALARS:
        assert np.array_equal(a[k][i], b[k][j], equal_nan=True), k
    assert a["ss_string"][i] == b["ss_string"][j]


def test_ideal_backbones_in_one_launch():
    bb = np.stack([dr.ideal_backbone(20, phi, psi) for phi, psi, _ in dr.IDEAL.values()])
    got = _call(bb)
    assert got["ss_string"] == [want for _, _, want in dr.IDEAL.values()]
    for b in range(len(bb)):
        _check(got, b, dr.dssp(bb[b]), list(dr.IDEAL)[b])
    assert got["helix_percent"].tolist() == [0.9, 0.9, 0.9, 0.0, 0.0] and got["coil_percent"][3] == 1.0


@pytest.mark.parametrize("n", [1, 2, 4, 5, 6])
def test_shortest_chains(n):
    """The bounds of the i +- 1 and i + n loops.  An extended chain is all coil at every length.  A chain with alpha torsions is all coil
    up to five rows and ``CHHHHC`` at six, the shortest helix the definitions allow: two consecutive 4-turns need HB(4, 0) and HB(5, 1)."""
    bb = np.stack([dr.ideal_backbone(n, *dr.IDEAL[kind][:2]) for kind in ("extended", "alpha", "three_ten", "pi")])
    got = _call(bb)
    assert got["ss_string"][0] == "C" * n and got["coil_percent"][0] == 1.0 and got["n_bridges"][0] == 0
    assert got["ss_string"][1] == ("C" * n if n < 6 else "CHHHHC") and (got["n_rows"] == n).all()
    for b in range(len(bb)):
        _check(got, b, dr.dssp(bb[b]), f"n = {n}, sample {b}")


@pytest.mark.parametrize("name", ["anti", "bulge", "parallel", "helix", "boundary"])
def test_excerpt_matches_the_restatement(name):
    if name not in dr.case_names(_fix()):
        assert name == "parallel"  # (kept only if a complex holds a parallel ladder)
        return
    _check(_single(name), 0, _stated(name), name)


@pytest.mark.parametrize("name", dr.COMPLEXES)
def test_whole_complex_matches_the_restatement(name):
    """N = 801 .. 820: the shapes past one block's stride in every per-row loop."""
    got, want = _single(name), _stated(name)
    assert want["n_rows"] > 3 * 256 and want["n_bridges"] > 200 and want["n_ladders"] > 40
    _check(got, 0, want, name)


def test_excerpts_in_one_padded_launch_equal_their_own_launches():
    """The excerpts and three short chains as one launch padded to the largest N with masked tail rows that hold garbage: each sample
    equals its own launch bit for bit."""
    fix = _fix()
    names = [c for c in dr.case_names(fix) if c not in dr.COMPLEXES]
    n_max = max(len(fix[f"{c}.bb"]) for c in names) + 3
    rng = np.random.default_rng(3)
    bb = (rng.normal(size=(len(names), n_max, 4, 3)) * 20).astype(np.float32)
    mask, chain = np.zeros((len(names), n_max), dtype=np.float32), rng.integers(0, 3, size=(len(names), n_max)).astype(np.int32)
    pro = np.ones((len(names), n_max), dtype=np.uint8)
    for b, c in enumerate(names):
        n = len(fix[f"{c}.bb"])
        bb[b, :n], mask[b, :n], chain[b, :n], pro[b, :n] = fix[f"{c}.bb"], 1, fix[f"{c}.chain_idx"], fix[f"{c}.is_proline"]
    got = _call(bb, mask, chain, pro)
    for b, c in enumerate(names):
        n = len(fix[f"{c}.bb"])
        _same_sample(got, b, _single(c), 0, n)
        assert (got["ss"][b, n:] == dr.ABSENT).all() and (got["acceptor"][b, n:] == -1).all() and not got["acceptor_energy"][b, n:].any()


def test_complexes_in_one_padded_launch_equal_their_own_launches():
    fix = _fix()
    n_max = max(len(fix[f"{c}.bb"]) for c in dr.COMPLEXES)
    bb = np.full((3, n_max, 4, 3), 7.0, dtype=np.float32)
    mask, chain, pro = np.zeros((3, n_max), dtype=np.float32), np.zeros((3, n_max), dtype=np.int32), np.zeros((3, n_max), dtype=np.uint8)
    for b, c in enumerate(dr.COMPLEXES):
        n = len(fix[f"{c}.bb"])
        bb[b, :n], mask[b, :n], chain[b, :n], pro[b, :n] = fix[f"{c}.bb"], 1, fix[f"{c}.chain_idx"], fix[f"{c}.is_proline"]
    got = _call(bb, mask, chain, pro)
    for b, c in enumerate(dr.COMPLEXES):
        _same_sample(got, b, _single(c), 0, len(fix[f"{c}.bb"]))


def test_chains_break_by_distance_as_by_index():
    """Two helices 10 Angstrom apart: under one chain_idx they break at the C - N distance exactly as under two."""
    phi, psi, _ = dr.IDEAL["alpha"]
    first = dr.ideal_backbone(12, phi, psi)
    second = dr.ideal_backbone(12, phi, psi, origin=np.array([12.0, -7.0, 30.0]) + (first[-1, 2] - first[0, 0]) + np.array([0.0, 10.0, 0.0]))
    bb = np.concatenate([first, second])
    assert np.linalg.norm(second[0, 0].astype(np.float64) - first[-1, 2]) > 9.9
    one, two = _call(bb[None]), _call(bb[None], chain_idx=np.repeat([0, 1], 12)[None])
    _same_sample(one, 0, two, 0, 24)
    assert one["ss_string"] == ["C" + "H" * 10 + "CC" + "H" * 10 + "C"]
    _check(one, 0, dr.dssp(bb), "one chain index")
    # the same 24 rows as one unbroken helix: no coil inside
    whole = _call(dr.ideal_backbone(24, phi, psi)[None])
    assert whole["ss_string"] == ["C" + "H" * 22 + "C"]


def test_proline_in_a_helix():
    phi, psi, _ = dr.IDEAL["alpha"]
    bb = dr.ideal_backbone(20, phi, psi)
    pro = np.zeros(20, dtype=np.uint8)
    pro[9:13] = 1
    got, want = _call(bb[None], is_proline=pro[None]), dr.dssp(bb, is_proline=pro)
    _check(got, 0, want, "proline")
    assert (got["acceptor"][0, 9:13] == -1).all() and got["n_hbonds"][0] == _call(bb[None])["n_hbonds"][0] - 4
    # turn_4(5 .. 8) are gone: the last helix start before them is row 4 (rows 4 .. 7), the first after them row 10
    assert got["ss_string"][0] == "C" + "H" * 7 + "CC" + "H" * 9 + "C"


def test_third_acceptor_does_not_bond():
    bb, chain = dr.three_acceptor_case()
    got = _call(bb[None], chain_idx=chain[None])
    _check(got, 0, dr.dssp(bb, None, chain), "three acceptors")
    assert got["acceptor"][0, 1].tolist() == [2, 3] and got["n_hbonds"][0] == 2


def test_masked_and_origin_rows_inside_a_chain():
    inp = dr.case_inputs(_fix(), "anti")
    n = len(inp["bb"])
    keep = np.sort(np.random.default_rng(5).choice(n + 6, size=n, replace=False))
    bb = np.random.default_rng(6).normal(size=(n + 6, 4, 3)).astype(np.float32) * 30
    chain, pro, mask = np.full(n + 6, 9, dtype=np.int32), np.ones(n + 6, dtype=np.uint8), np.ones(n + 6, dtype=np.float32)
    bb[keep], chain[keep], pro[keep] = inp["bb"], inp["chain_idx"], inp["is_proline"]
    holes = np.setdiff1d(np.arange(n + 6), keep)
    mask[holes[:3]] = 0
    bb[holes[3:5]] = 0
    bb[holes[5], 2] = 0
    got = _call(bb[None], mask[None], chain[None], pro[None])
    _check(got, 0, dr.dssp(bb, mask, chain, pro), "holes")
    one = _single("anti")
    assert np.array_equal(got["ss"][0, keep], one["ss"][0]) and (got["ss"][0, holes] == dr.ABSENT).all()
    assert np.array_equal(got["acceptor_energy"][0, keep], one["acceptor_energy"][0])
    for k in SCALARS:
        assert got[k][0] == one[k][0], k


def test_no_row_gives_nan():
    got = _call(np.zeros((2, 7, 4, 3), dtype=np.float32))
    assert (got["n_rows"] == 0).all() and (got["ss"] == dr.ABSENT).all() and all(np.isnan(got[k]).all() for k in dr.FRACTIONS)
    assert got["ss_string"] == ["", ""] and (got["status"] == 0).all()


def test_input_routes_agree():
    """A device tensor against a NumPy array, [B,N,5,3] against [B,N,37,3], and garbage in the atoms that are not read."""
    from framedipt_amd import secondary_structure as sec
    inp = dr.case_inputs(_fix(), "helix")
    one = _single("helix")
    n = len(inp["bb"])
    args = (None, inp["chain_idx"][None], inp["is_proline"][None])
    noisy = _atom37(inp["bb"][None])
    noisy[:, :, [3] + list(range(5, 37))] = np.random.default_rng(1).normal(size=(1, n, 33, 3)) * 50
    aatype = np.where(inp["is_proline"] != 0, PRO, 0)[None]
    for other in (_call(inp["bb"][None], *args, device=True), _call(inp["bb"][None], *args, atoms=5), _call(inp["bb"][None], *args, atoms=5, device=True),
                  sec.secondary_structure(noisy, None, inp["chain_idx"][None], aatype),
                  sec.secondary_structure(torch.from_numpy(noisy).cuda(), None, torch.from_numpy(inp["chain_idx"][None]).cuda(), torch.from_numpy(aatype).cuda())):
        _same_sample(other, 0, one, 0, n)


def test_workspace_and_argument_errors():
    """The workspace covers the ladder list's capacity (FDIPT_DSSP_BRIDGES_PER_ROW x N ladders of five ints) - the status path itself
    is not provoked - and the entry refuses what the header says it refuses."""
    import ctypes as C

    from framedipt_amd import _lib
    lib = _lib.load()
    for b, n in ((1, 1), (5, 820), (64, 300)):
        assert lib.fdipt_sample_dssp_workspace(b, n) >= b * n * (17 * 8 + (5 + 6 * _lib.DSSP_BRIDGES_PER_ROW) * 4 + 3)
        assert lib.fdipt_sample_dssp_workspace(b, n) % 8 == 0
    assert lib.fdipt_sample_dssp_workspace(0, 5) == 0 and lib.fdipt_sample_dssp_workspace(5, 0) == 0
    assert lib.fdipt_sample_dssp(None, None) == _lib.EINVAL
    x = torch.ones(1, 4, 37, 3, device="cuda")
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = _lib.ptr(buf)
    fields = {name: p for name, t in _lib.DsspArgs._fields_ if t is C.c_void_p}
    good = dict(fields, B=1, N=4, atoms=37, prot=_lib.ptr(x), workspace_bytes=lib.fdipt_sample_dssp_workspace(1, 4))
    assert good["workspace_bytes"] <= 4096
    for bad, code in ((dict(atoms=14), _lib.EINVAL), (dict(B=0), _lib.EINVAL), (dict(N=0), _lib.EINVAL), (dict(status=None), _lib.EINVAL),
                      (dict(workspace_bytes=good["workspace_bytes"] - 1), _lib.ESIZE)):
        args = _lib.DsspArgs(**dict(good, **bad))
        assert lib.fdipt_sample_dssp(C.byref(args), _lib.stream_ptr()) == code, bad


def test_end_to_end_inpainting_small_config():
    """Three inpainting samples of one two-chain structure (small config, N = 24, T = 3), the result left on the device: the call runs
    on the device tensor with the run's own res_mask, chain_idx and aatype and equals the restatement on the downloaded coordinates, the
    fractions sum to 1, region_counts sums to the region lengths."""
    from framedipt_amd import config, inference
    from framedipt_amd import secondary_structure as sec
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import ConditionalSampler
    n, b = 24, 3
    conf = config.small_config(True)
    d = SE3Diffuser(conf.diffuser)
    net = ScoreNetwork(conf.model, d, inpainting=True, precision="fp32").load_synthetic(5).to("cuda")
    rng = np.random.default_rng(n)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    tr = np.cumsum(rng.standard_normal((n, 3)) * 2.0, 0) + 30.0
    dm = np.zeros(n)
    dm[5:11], dm[16:20] = 1, 1
    aatype = rng.integers(0, 20, n)
    aatype[[7, 18]] = PRO
    feats_np = {"rigids_0": np.concatenate([q, tr], -1).astype(np.float32), "diffuse_mask": dm, "aatype": aatype,
                "seq_idx": np.concatenate([np.arange(12), np.arange(12) + 212]), "chain_idx": np.repeat([0.0, 1.0], 12),
                "torsion_angles_sin_cos": np.tile(np.array([0.0, 1.0]), (n, 7, 1))}
    ds = ConditionalSampler.from_features([("synthetic", feats_np)], d, "cuda", samples=b)
    np.random.seed(3)
    items = [ds[i][2] for i in range(b)]
    feats = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    res = inference.inference_fn(net, d, feats, num_t=3, min_t=0.01, aux_traj=True, noise_scale=0.1, inpainting=True, return_device=True)
    prot = res["prot_traj"][0]
    assert prot.is_cuda and tuple(prot.shape) == (b, n, 37, 3)
    got = sec.secondary_structure(prot, feats["res_mask"], feats["chain_idx"], feats["aatype"])
    host, chain = prot.cpu().numpy(), feats["chain_idx"].cpu().numpy()
    pro = feats["aatype"].cpu().numpy() == PRO
    assert pro[:, [7, 18]].all()
    regions = [(5, 10), (16, 19)]
    for s in range(b):
        _check(got, s, dr.dssp(host[s], feats["res_mask"][s].cpu().numpy(), chain[s], pro[s]), f"sample {s}")
        metrics = sec.shape_metrics(got, s)
        assert abs(metrics["coil_percent"] + metrics["helix_percent"] + metrics["strand_percent"] - 1.0) <= 1e-15
        assert metrics["non_coil_percent"] == got["helix_percent"][s] + got["strand_percent"][s]
        assert got["n_rows"][s] == n and len(got["ss_string"][s]) == n
        assert sum(sec.region_counts(got, s, regions)) == 6 + 4 and sum(sec.region_counts(got, s, [(0, n - 1)])) == n


def test_run_sharded_secondary_structure_on_two_ranks(tmp_path):
    """``run_sharded --secondary-structure`` on two ranks with the small configuration writes ``secondary_structure.json`` and
    ``secondary_structure.csv`` with the numbers of a direct call on every written sample."""
    import csv
    import json
    import os
    import subprocess
    import sys

    from conftest import ROOT
    from framedipt_amd import secondary_structure as sec

    out_dir = tmp_path / "run"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29671",
           "-m", "framedipt_amd.run_sharded", "--out-dir", str(out_dir), "--min-length", "9", "--max-length", "14", "--length-step", "5",
           "--samples-per-length", "2", "--num-t", "2", "--max-batch", "4", "--precision", "fp32", "--keep", "last", "--secondary-structure"]
    env = dict(os.environ, FDIPT_ONE_GPU="1", FDIPT_SHARED_GPU="allow", MASTER_ADDR="127.0.0.1")  # two ranks on this box's one GPU
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out_dir))
    assert "secondary_structure.json" in files and "secondary_structure.csv" in files
    with open(out_dir / "secondary_structure.json") as f:
        summary = json.load(f)
    with open(out_dir / "secondary_structure.csv", newline="") as f:
        table = list(csv.DictReader(f))
    with open(out_dir / "manifest.json") as f:
        records = {(r["name"], r["sample_i"]): r for r in json.load(f)["samples"]}
    assert len(summary["samples"]) == len(table) == 4 and sorted(e["n_res"] for e in summary["samples"]) == [9, 9, 14, 14]
    for entry, row in zip(summary["samples"], table):
        prot = np.load(out_dir / records[(entry["pdb_name"], entry["sample"])]["file"])["prot_traj"]
        direct = sec.secondary_structure(prot[None])
        assert entry["ss"] == row["ss"] == direct["ss_string"][0] and len(entry["ss"]) == entry["n_res"]
        for k in sec.FRACTIONS:
            assert entry[k] == direct[k][0].item() and float(row[k]) == direct[k][0].item(), k
        assert row["pdb_name"] == str(entry["pdb_name"]) and row["sample"] == str(entry["sample"])
