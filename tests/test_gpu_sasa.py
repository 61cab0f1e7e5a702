"""GPU tests (-m gpu) of the solvent accessibility (framedipt_amd/sasa.py -> fdipt_sample_sasa, csrc/sasa.hip) against the NumPy
restatement tests/sasa_ref.py on the fixture tests/golden/sasa_cases.npz.  The counts, n_atoms and every float64 output are compared
exactly."""
import functools

import numpy as np
import pytest
import torch

import sasa_ref as sr
from conftest import load_golden

pytestmark = pytest.mark.gpu

EXCERPTS = list(sr.BACKBONE_EXCERPTS) + ["fullatom"]


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("sasa_cases.npz")


@functools.lru_cache(maxsize=None)
def _case(name, atoms=37):
    return sr.case_prot(_fix(), name, atoms)


@functools.lru_cache(maxsize=None)
def _stated(name):
    prot, mask, aatype = _case(name)
    return sr.sasa(prot, mask, None, aatype)


@functools.lru_cache(maxsize=None)
def _single(name):
    from framedipt_amd import sasa
    prot, mask, aatype = _case(name)
    return sasa.solvent_accessibility(prot[None], mask[None], None, aatype[None])


def _call(prot, *args, **kw):
    from framedipt_amd import sasa
    return sasa.solvent_accessibility(prot, *args, **kw)


def _check(got, b, want, what=""):
    """Sample b of a device result against one restatement result, exactly; rows behind the restatement's are empty."""
    n = len(want["residue_sasa"])
    for k in ("accessible", "atom_sasa", "residue_sasa", "rsa"):
        x = np.asarray(got[k][b])
        assert x.dtype == np.asarray(want[k]).dtype, (what, k, x.dtype)
        assert np.array_equal(x[:n], want[k], equal_nan=True), (what, k, np.flatnonzero((x[:n] != want[k]).reshape(n, -1).any(1))[:10])
        if k != "rsa":
            assert not x[n:].any(), (what, k)
    assert got["n_atoms"][b] == want["n_atoms"], (what, got["n_atoms"][b], want["n_atoms"])
    assert np.array_equal(got["total_sasa"], got["residue_sasa"].sum(1))


def _same_sample(a, i, b, j, n):
    for k in ("accessible", "atom_sasa", "residue_sasa", "rsa"):
        x, y = np.asarray(a[k][i]), np.asarray(b[k][j])
        assert x.dtype == y.dtype and np.array_equal(x[:n], y[:n], equal_nan=True), k
    assert a["n_atoms"][i] == b["n_atoms"][j]


def _first_atoms(name, count):
    """The first ``count`` atoms of a case in (row, column) order -> (prot, atom_mask, aatype) cut to the rows they touch."""
    prot, mask, aatype = _case(name)
    rows, cols = np.nonzero(mask)
    keep = np.zeros_like(mask)
    keep[rows[:count], cols[:count]] = 1
    n = int(rows[count - 1]) + 1
    return prot[:n], keep[:n], aatype[:n]


def test_one_atom():
    prot = np.zeros((1, 1, 37, 3), dtype=np.float32)
    prot[0, 0, 1] = [3.0, -1.0, 2.5]
    got = _call(prot)
    _check(got, 0, sr.sasa(prot[0]), "one atom")
    assert got["accessible"][0, 0].tolist() == [0, 100] + [0] * 35 and got["n_atoms"].tolist() == [1]
    assert got["residue_sasa"][0, 0] == 100 * ((1.70 + 1.40) ** 2 * (4.0 * np.pi / 100)) and got["rsa"][0, 0] == got["residue_sasa"][0, 0] / 121.0


def test_two_and_three_atoms_and_a_swallowed_one():
    """Two overlapping atoms, three atoms, and an atom wholly inside another: every point of it is buried by its first neighbour, so
    the walk leaves at the first tile."""
    prot = np.zeros((3, 1, 5, 3), dtype=np.float32)
    prot[0, 0, :2] = [[1.0, 1.0, 1.0], [2.2, 1.5, 0.7]]
    prot[1, 0, [0, 2, 4]] = [[1.0, 1.0, 1.0], [2.2, 1.5, 0.7], [0.1, 2.9, 1.6]]
    prot[2, 0, [0, 1, 4]] = [[0.3, 0.1, 0.2], [0.1, 0.1, 0.1], [3.5, 0.1, 0.1]]
    got = _call(prot)
    for b in range(2):
        _check(got, b, sr.sasa(prot[b]), f"sample {b}")
        assert 0 < got["accessible"][b, 0, 0] < 100
    radii = np.array([0.2, 3.0, 1.0, 1.0, 1.5])
    got = _call(prot, probe_radius=0.0, radii=radii)
    for b in range(3):
        _check(got, b, sr.sasa(prot[b], probe_radius=0.0, atom_radii=radii), f"sample {b}, custom radii")
    assert got["accessible"][2, 0].tolist()[0] == 0 and got["accessible"][2, 0, 1] > 0 and got["n_atoms"].tolist() == [2, 3, 3]


@pytest.mark.parametrize("count", [63, 64, 65, 129])
def test_tile_edges_of_the_atom_walk(count):
    prot, mask, aatype = _first_atoms("fullatom", count)
    got = _call(prot[None], mask[None], None, aatype[None])
    assert got["n_atoms"].tolist() == [count]
    _check(got, 0, sr.sasa(prot, mask, None, aatype), f"{count} atoms")


@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 100, 128, 1000])
def test_lane_ownership_edges(n_points):
    prot, mask, aatype = _case("anti")
    got = _call(prot[None], mask[None], None, aatype[None], n_points=n_points)
    _check(got, 0, sr.sasa(prot, mask, None, aatype, n_points=n_points), f"{n_points} points")
    assert got["accessible"].max() <= n_points


@pytest.mark.parametrize("name", EXCERPTS)
def test_excerpt_matches_the_restatement(name):
    got, want = _single(name), _stated(name)
    _check(got, 0, want, name)
    rows, cols = np.nonzero(_case(name)[1])
    assert np.array_equal(got["accessible"][0][rows, cols], _fix()[f"{name}.accessible"])


@pytest.mark.parametrize("name", sr.COMPLEXES)
def test_whole_complex_matches_the_restatement(name):
    """About 6 500 atoms: the only shapes with more than a hundred tiles in the walk."""
    got, want = _single(name), _stated(name)
    assert want["n_atoms"] > 100 * 64
    _check(got, 0, want, name)
    rows, cols = np.nonzero(_case(name)[1])
    assert np.array_equal(got["accessible"][0][rows, cols], _fix()[f"{name}.accessible"])


@pytest.mark.parametrize("name", sr.BACKBONE_EXCERPTS)
def test_five_atom_layout_equals_atom37(name):
    prot5, mask5, aatype = _case(name, 5)
    got5, got37 = _call(prot5[None], mask5[None], None, aatype[None]), _single(name)
    for k in ("accessible", "atom_sasa"):
        assert np.array_equal(got5[k][0], got37[k][0][:, :5]) and not got37[k][0][:, 5:].any()
    for k in ("residue_sasa", "rsa", "n_atoms", "total_sasa"):
        assert np.array_equal(got5[k], got37[k])
    _check(got5, 0, sr.sasa(prot5, mask5, None, aatype), name)


def test_masked_rows_and_atoms():
    prot, mask, aatype = _case("fullatom")
    rng = np.random.default_rng(11)
    res_mask = (rng.random(len(prot)) > 0.2).astype(np.float32)
    atom_mask = mask * (rng.random(mask.shape) > 0.15)
    garbage = prot.copy()
    garbage[atom_mask == 0] = rng.normal(size=(int((atom_mask == 0).sum()), 3)) * 5 + prot[mask != 0].mean(0)  # (absent atoms hold coordinates)
    got = _call(garbage[None], atom_mask[None], res_mask[None], aatype[None])
    _check(got, 0, sr.sasa(prot, atom_mask, res_mask, aatype), "masks")
    assert not got["accessible"][0][res_mask == 0].any() and not got["residue_sasa"][0][res_mask == 0].any()
    assert got["n_atoms"][0] == (atom_mask * res_mask[:, None]).sum() < mask.sum()


def test_origin_atoms_under_the_default_mask():
    """Without atom_mask the atoms at the origin are absent: rows the sampler left there and the columns a backbone does not fill."""
    prot, mask, aatype = _case("helix")
    holes = prot.copy()
    holes[[3, 9]] = 0
    holes[5, 3] = 0
    got = _call(holes[None], None, None, aatype[None])
    explicit = mask.copy()
    explicit[[3, 9]] = 0
    explicit[5, 3] = 0
    _check(got, 0, sr.sasa(holes, None, None, aatype), "default mask")
    _same_sample(got, 0, _call(prot[None], explicit[None], None, aatype[None]), 0, len(prot))
    assert got["n_atoms"][0] == explicit.sum()


def test_padded_batch_equals_each_samples_own_launch():
    """The excerpts and two small atom sets as one launch padded to the largest N, the tail rows masked and holding garbage: each
    sample equals its own launch bit for bit."""
    members = [_case(name) for name in EXCERPTS] + [_first_atoms("fullatom", 65), _first_atoms("fullatom", 7)]
    n_max = max(len(m[0]) for m in members) + 3
    rng = np.random.default_rng(3)
    prot = (rng.normal(size=(len(members), n_max, 37, 3)) * 8).astype(np.float32)
    atom_mask = np.ones((len(members), n_max, 37), dtype=np.uint8)
    res_mask, aatype = np.zeros((len(members), n_max), dtype=np.float32), rng.integers(0, 20, size=(len(members), n_max))
    for b, (p, m, a) in enumerate(members):
        prot[b, :len(p)], atom_mask[b, :len(p)], res_mask[b, :len(p)], aatype[b, :len(p)] = p, m, 1, a
    got = _call(prot, atom_mask, res_mask, aatype)
    for b, (p, m, a) in enumerate(members):
        own = _call(p[None], m[None], None, a[None])
        _same_sample(got, b, own, 0, len(p))
        _check(got, b, sr.sasa(p, m, None, a), f"member {b}")
        assert not got["accessible"][b, len(p):].any() and not got["residue_sasa"][b, len(p):].any()


def test_custom_radii_and_probe():
    prot, mask, aatype = _case("boundary")
    radii = np.linspace(1.2, 2.1, 37)
    got = _call(prot[None], mask[None], None, aatype[None], probe_radius=1.1, n_points=96, radii=radii)
    _check(got, 0, sr.sasa(prot, mask, None, aatype, probe_radius=1.1, n_points=96, atom_radii=radii), "custom radii")
    assert not np.array_equal(got["accessible"], _single("boundary")["accessible"])


def test_unknown_residue_types_give_nan():
    prot, mask, _ = _case("anti")
    aatype = np.arange(len(prot)) % 23
    got = _call(prot[None], mask[None], None, aatype[None])
    _check(got, 0, sr.sasa(prot, mask, None, aatype), "aatype >= 20")
    assert np.array_equal(np.isnan(got["rsa"][0]), aatype >= 20) and np.array_equal(got["residue_sasa"], _single("anti")["residue_sasa"])


def test_input_routes_agree():
    """A device tensor against a NumPy array, with every other argument on the device as well."""
    prot, mask, aatype = _case("helix")
    one = _single("helix")
    on = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    ones = np.ones(len(prot), dtype=np.float32)
    for other in (_call(on(prot[None]), mask[None], None, aatype[None]), _call(on(prot[None]), on(mask[None]), on(ones[None]), on(aatype[None])),
                  _call(prot[None], on(mask[None]), ones[None], on(aatype[None].astype(np.float32)))):
        _same_sample(other, 0, one, 0, len(prot))
        assert np.array_equal(other["total_sasa"], one["total_sasa"])


def test_python_argument_errors():
    from framedipt_amd import _lib
    prot = np.ones((2, 4, 37, 3), dtype=np.float32)
    for bad in (dict(prot=prot[0]), dict(prot=np.ones((2, 4, 14, 3), dtype=np.float32)), dict(prot=prot[:0]), dict(atom_mask=np.ones((2, 4, 5))),
                dict(res_mask=np.ones((2, 5))), dict(aatype=np.zeros((1, 4))), dict(n_points=0), dict(n_points=1025), dict(radii=np.ones(5)),
                dict(radii=np.full(37, -2.0)), dict(prot=torch.ones(2, 4, 37, 3, dtype=torch.float64, device="cuda"))):
        with pytest.raises(ValueError):
            _call(**dict(dict(prot=prot), **bad))
    with pytest.raises(_lib.FdiptError):
        _call(torch.ones(2, 4, 37, 3))


def test_workspace_and_entry_errors():
    """The workspace holds five doubles and an int per possible atom and a count per sample, and the entry refuses what the header
    says it refuses."""
    import ctypes as C

    from framedipt_amd import _lib
    lib = _lib.load()
    for b, n, atoms in ((1, 1, 37), (5, 820, 37), (64, 300, 5)):
        assert lib.fdipt_sample_sasa_workspace(b, n, atoms) >= b * (n * atoms * 44 + 4)
        assert lib.fdipt_sample_sasa_workspace(b, n, atoms) % 8 == 0
    assert lib.fdipt_sample_sasa_workspace(0, 5, 37) == 0 and lib.fdipt_sample_sasa_workspace(5, 0, 37) == 0 and lib.fdipt_sample_sasa_workspace(5, 5, 14) == 0
    assert lib.fdipt_sample_sasa(None, None) == _lib.EINVAL
    x = torch.ones(1, 4, 37, 3, device="cuda")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = _lib.ptr(buf)
    fields = {name: p for name, t in _lib.SasaArgs._fields_ if t is C.c_void_p}
    good = dict(fields, B=1, N=4, atoms=37, n_points=100, prot=_lib.ptr(x), workspace_bytes=lib.fdipt_sample_sasa_workspace(1, 4, 37))
    assert good["workspace_bytes"] <= 1 << 16
    for bad, code in ((dict(atoms=14), _lib.EINVAL), (dict(B=0), _lib.EINVAL), (dict(N=0), _lib.EINVAL), (dict(n_points=0), _lib.EINVAL),
                      (dict(n_points=1025), _lib.EINVAL), (dict(n_atoms=None), _lib.EINVAL), (dict(sphere=None), _lib.EINVAL),
                      (dict(workspace=None), _lib.EINVAL), (dict(workspace_bytes=good["workspace_bytes"] - 1), _lib.ESIZE),
                      (dict(B=65536, workspace_bytes=1 << 62), _lib.ESIZE), (dict(B=60000, N=1000, workspace_bytes=1 << 62), _lib.ESIZE)):
        args = _lib.SasaArgs(**dict(good, **bad))
        assert lib.fdipt_sample_sasa(C.byref(args), _lib.stream_ptr()) == code, bad


def test_end_to_end_inpainting_small_config():
    """Three inpainting samples of one two-chain structure (small config, N = 24, T = 3), the result left on the device: the call runs
    on the device tensor with the run's res_mask and aatype, equals the restatement on the downloaded coordinates, and sasa_metrics of
    a sample against itself has no error."""
    from framedipt_amd import config, inference, sasa
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
    got = sasa.solvent_accessibility(prot, None, feats["res_mask"], feats["aatype"])
    host, kinds = prot.cpu().numpy(), feats["aatype"].cpu().numpy()
    regions = [(5, 10), (16, 19)]
    for s in range(b):
        _check(got, s, sr.sasa(host[s], None, feats["res_mask"][s].cpu().numpy(), kinds[s]), f"sample {s}")
        assert got["n_atoms"][s] == (host[s] != 0).any(-1).sum() >= 4 * n
        metrics = sasa.sasa_metrics(got, s, got, s, regions)
        assert all(len(v) == 10 for v in metrics.values()) and not metrics["asa_abs_error"].any() and not metrics["rsa_square_error"].any()
        assert np.array_equal(metrics["sample_rsa"], metrics["sample_asa"] / sasa.MAX_SASA[kinds[s][sasa.region_rows(regions)]])


def test_run_sasa_scores_the_ground_truth_of_an_inpainting_run(tmp_path):
    """``run_sharded.run_sasa`` (what ``--sasa`` runs on rank 0) on gathered entries as an inpainting run leaves them: a full-atom ground
    truth, backbone samples of two structures of different length.  ``sasa.json`` carries the reference's eight keys of a direct
    ``sasa_metrics`` call over the diffused rows, with the run's aatype in the RSA denominators."""
    import json

    from framedipt_amd import run_sharded, sasa
    records, gathered, structures = [], {}, {"fullatom": np.r_[4:10, 20:24], "helix": np.r_[8:15]}
    for name, rows in structures.items():
        truth, _, aatype = _case(name)
        diffused = np.zeros(len(truth), dtype=bool)
        diffused[rows] = True
        for s in range(2):
            backbone = truth.copy()
            backbone[:, 5:] = 0
            backbone[diffused[:, None] & (backbone != 0).any(-1)] += np.float32(0.4 * (s + 1))  # (the diffused rows moved: another surface)
            records.append({"item": len(records), "name": name, "sample_i": s, "file": f"{name}/sample_{s}/sample_{s}_1.pdb"})
            gathered[len(gathered)] = {"prot": backbone, "diffused": diffused, "res_mask": np.ones(len(truth), dtype=np.float32),
                                       "aatype": aatype.astype(np.float32), **({"gt": truth} if s == 0 else {})}
    summary = run_sharded.run_sasa(str(tmp_path), records, gathered, inpainting=True)
    with open(tmp_path / "sasa.json") as f:
        assert json.load(f) == json.loads(json.dumps(summary))
    assert summary["ground_truth"] and [e["sample"] for e in summary["samples"]] == [0, 1, 0, 1]
    for item, entry in enumerate(summary["samples"]):
        name = entry["pdb_name"]
        truth, _, aatype = _case(name)
        gt, mine = sasa.solvent_accessibility(truth[None], None, None, aatype[None]), sasa.solvent_accessibility(gathered[item]["prot"][None], None, None, aatype[None])
        want = sasa.sasa_metrics(gt, 0, mine, 0, [(int(k), int(k)) for k in structures[name]])
        assert entry["rows"] == structures[name].tolist() and entry["asa"] == want["sample_asa"].tolist() and entry["rsa"] == want["sample_rsa"].tolist()
        assert tuple(entry["metrics"]) == sasa.METRICS
        for k in sasa.METRICS:
            assert entry["metrics"][k] == want[k].tolist(), (name, k)
        assert np.array_equal(want["gt_asa"], _stated(name)["residue_sasa"][structures[name]]) and want["asa_abs_error"].any()
    bare = {i: {k: v for k, v in it.items() if k != "gt"} for i, it in gathered.items()}
    plain = run_sharded.run_sasa(str(tmp_path), records, bare, inpainting=True)
    assert not plain["ground_truth"] and "metrics" not in plain["samples"][0] and plain["samples"][0]["asa"] == summary["samples"][0]["asa"]


def test_run_sharded_sasa_on_two_ranks(tmp_path):
    """``run_sharded --sasa`` on two ranks with the small configuration writes ``sasa.json`` and ``sasa.csv`` with the numbers of a
    direct call on every written sample."""
    import csv
    import json
    import os
    import subprocess
    import sys

    from conftest import ROOT
    from framedipt_amd import sasa

    out_dir = tmp_path / "run"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29673",
           "-m", "framedipt_amd.run_sharded", "--out-dir", str(out_dir), "--min-length", "9", "--max-length", "14", "--length-step", "5",
           "--samples-per-length", "2", "--num-t", "2", "--max-batch", "4", "--precision", "fp32", "--keep", "last", "--sasa"]
    env = dict(os.environ, FDIPT_ONE_GPU="1", FDIPT_SHARED_GPU="allow", MASTER_ADDR="127.0.0.1")  # two ranks on this box's one GPU
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    files = sorted(os.listdir(out_dir))
    assert "sasa.json" in files and "sasa.csv" in files
    with open(out_dir / "sasa.json") as f:
        summary = json.load(f)
    with open(out_dir / "sasa.csv", newline="") as f:
        table = list(csv.DictReader(f))
    with open(out_dir / "manifest.json") as f:
        records = {(r["name"], r["sample_i"]): r for r in json.load(f)["samples"]}
    assert len(summary["samples"]) == len(table) == 4 and sorted(e["n_res"] for e in summary["samples"]) == [9, 9, 14, 14]
    for entry, row in zip(summary["samples"], table):
        prot = np.load(out_dir / records[(entry["pdb_name"], entry["sample"])]["file"])["prot_traj"]
        direct = sasa.solvent_accessibility(prot[None])
        assert entry["rows"] == list(range(entry["n_res"]))  # (de novo: every row is diffused)
        assert entry["asa"] == direct["residue_sasa"][0].tolist() and entry["rsa"] == direct["rsa"][0].tolist()
        assert entry["total"] == direct["total_sasa"][0].item() == float(row["total"])
        assert float(row["mean_asa"]) == direct["residue_sasa"][0].mean().item() and float(row["mean_rsa"]) == direct["rsa"][0].mean().item()
        assert row["pdb_name"] == str(entry["pdb_name"]) and row["sample"] == str(entry["sample"]) and row["n_res"] == str(entry["n_res"])
