"""GPU tests (-m gpu) of the structural violations (framedipt_amd/violations.py -> fdipt_sample_violations, csrc/violations.hip) against
the reference fixture tests/golden/violation_cases.npz.  ``pytest tests/test_gpu_violations.py -m gpu -s`` prints the worst device
error per output next to its bound (32 x the reference's own change under the fixture's recorded perturbations), and the distance of
the device result to the reference's float32 run next to the distance between the reference's own two runs."""
import functools

import numpy as np
import pytest
import torch

import violations_ref as vr
from conftest import load_golden

pytestmark = pytest.mark.gpu

ARRAYS = vr.FLOAT_OUTPUTS + vr.EXACT_OUTPUTS + ("radius_of_gyration",)


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("violation_cases.npz")


def _call(inp, **over):
    from framedipt_amd import violations
    kw = dict(prot=inp["prot"], diffuse_mask=inp["diffuse_mask"], res_mask=inp.get("res_mask"), residue_index=inp["residue_index"])
    kw.update(over)
    return violations.structural_violations(**kw)


@functools.lru_cache(maxsize=None)
def _single(name):
    """One case as a call of its own (NumPy inputs, uploaded)."""
    return _call(vr.case_inputs(_fix(), name))


def _same_sample(a, i, b, j, n):
    """Sample i of result a equals sample j of result b bit for bit on the first n rows (NaN = NaN); the rows behind are zero."""
    for k in ARRAYS:
        x, y = np.asarray(a[k][i]), np.asarray(b[k][j])
        if x.ndim:
            assert not x[n:].any() and not y[n:].any(), k
            x, y = x[:n], y[:n]
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), k


@pytest.mark.parametrize("name", vr.CASES)
def test_case_matches_the_reference(name):
    """Every case alone against the reference's float64 run: floats within 32 x the yardstick, masks and counts exactly; the radius of
    gyration against the restatement."""
    fix, got, inp = _fix(), _single(name), vr.case_inputs(_fix(), name)
    for s in range(inp["prot"].shape[0]):
        report = {}
        vr.check_sample(fix, name, s, vr.sample_of(got, s), lambda k, err, lim: report.__setitem__(k, (err, lim)))
        for k, (err, lim) in report.items():
            print(f"{name}[{s}]: {k}: |device - reference| = {err:.3e}, bound {lim:.3e}")
        want = vr.violations(inp["prot"][s], None, vr.keep_mask(inp["prot"][s], inp["diffuse_mask"][s]), inp["residue_index"][s])
        assert abs(got["radius_of_gyration"][s] - want["radius_of_gyration"]) <= 1e-13 * want["radius_of_gyration"]
    if name == "clean":
        for k in vr.FLOAT_OUTPUTS + vr.EXACT_OUTPUTS:
            if k != "n_clash_pairs":
                assert not got[k].any(), k  # exact zeros


@pytest.mark.parametrize("name", vr.CASES)
def test_device_is_as_near_the_float32_run_as_the_float64_reference(name):
    """The reference as shipped runs in float32: the device result is no farther from it than the reference's own float64 run plus the
    float64 bound."""
    fix, got = _fix(), _single(name)
    for k in vr.FLOAT_OUTPUTS:
        shipped, exact = fix[f"{name}.{k}.f32"], fix[f"{name}.{k}"]
        own, dev = float(np.abs(exact - shipped).max()), float(np.abs(got[k] - shipped).max())
        print(f"{name}: {k}: |device - float32 run| = {dev:.3e}, |float64 run - float32 run| = {own:.3e}")
        assert dev <= own + vr.bound(fix, name, k), k


def test_all_cases_in_one_padded_launch_equal_their_own_launches():
    """Nine samples of N = 1 .. 260 padded to 261 rows with res_mask = 0 rows that hold garbage: every output equals the case's own launch
    bit for bit, and the rows behind a sample stay zero."""
    joint, first = vr.joint_batch(_fix())
    got = _call(joint)
    for name, b0 in zip(vr.CASES, first):
        one = _single(name)
        n = one["connections_per_residue_loss_sum"].shape[1]
        for s in range(one["clashes_mean_loss"].shape[0]):
            _same_sample(got, b0 + s, one, s, n)


def test_rows_missing_inside_a_sample_are_as_if_removed():
    """res_mask = 0 rows INSIDE a sample: the outputs of the remaining rows are those of the sample without them (the bond joins the rows
    around the hole)."""
    inp = vr.case_inputs(_fix(), "clashy")
    hole = np.ones((1, 30), dtype=np.float32)
    hole[0, [0, 7, 8, 19]] = 0
    rows = np.nonzero(hole[0])[0]
    got = _call(inp, res_mask=hole)
    cut = _call({k: v[:, rows] for k, v in inp.items()})
    limit = lambda key: vr.bound(_fix(), "clashy", key)  # noqa: E731
    for k in ARRAYS:
        if got[k][0].ndim:
            assert not np.delete(got[k][0], rows, axis=0).any(), k
    # (a hole moves the rows behind it to other lanes: the sums agree within the bound, not bit for bit)
    vr.check_outputs(vr.sample_of(cut, 0), {k: (v[0][rows] if v[0].ndim else v[0]) for k, v in got.items()}, limit)
    want = vr.violations(inp["prot"][0], hole[0], vr.keep_mask(inp["prot"][0]), inp["residue_index"][0])
    vr.check_outputs(want, vr.sample_of(got, 0), limit)


def test_input_routes_agree():
    """A device tensor against a NumPy array, [B,N,5,3] against [B,N,37,3], and garbage in atoms 5..36: all equal."""
    inp = vr.case_inputs(_fix(), "n260")
    one = _single("n260")
    on_device = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    dev = _call(on_device)
    noisy = inp["prot"].copy()
    noisy[:, :, 5:] = np.random.default_rng(1).normal(size=noisy[:, :, 5:].shape) * 50
    zero_rows = inp["prot"].copy()
    zero_rows[:, 3, :5] = 0  # (a row without a non-zero backbone coordinate sits at the origin whatever its other atoms hold)
    for other in (dev, _call(inp, prot=np.ascontiguousarray(inp["prot"][:, :, :5])), _call(inp, prot=noisy),
                  _call(inp, prot=torch.from_numpy(noisy).cuda()[:, :, :5])):
        for s in range(2):
            _same_sample(other, s, one, s, 260)
    noisy[:, 3, :5] = 0
    a, b = _call(inp, prot=zero_rows), _call(inp, prot=noisy)
    for s in range(2):
        _same_sample(a, s, b, s, 260)
    # row 3 (no clash of its own in this case) now sits at the origin: its atoms coincide and its bonds stretch, as in the restatement
    assert a["within_per_atom_violations"][:, 3].all() and not one["within_per_atom_violations"][:, 3].any()
    assert (a["connections_per_residue_loss_sum"][:, 3] > one["connections_per_residue_loss_sum"][:, 3]).all()
    for s in range(2):
        want = vr.violations(zero_rows[s], None, vr.keep_mask(zero_rows[s]), inp["residue_index"][s])
        vr.check_outputs(want, vr.sample_of(a, s), lambda key: vr.bound(_fix(), "n260", key))


def test_atoms_option():
    """``atoms="all"`` on ``masked`` is the restatement with every row kept; ``atoms="diffused"`` differs from it."""
    fix, inp = _fix(), vr.case_inputs(_fix(), "masked")
    everything = _call(inp, atoms="all")
    want = vr.violations(inp["prot"][0], None, vr.keep_mask(inp["prot"][0]), inp["residue_index"][0])
    vr.check_outputs(want, vr.sample_of(everything, 0), lambda key: vr.bound(fix, "masked", key))
    assert abs(everything["radius_of_gyration"][0] - want["radius_of_gyration"]) <= 1e-13 * want["radius_of_gyration"]
    diffused = _single("masked")
    assert diffused["n_clash_pairs"][0] == everything["n_clash_pairs"][0]
    assert diffused["clashes_mean_loss"][0] > everything["clashes_mean_loss"][0]
    assert not np.array_equal(diffused["clashes_per_atom_clash_mask"], everything["clashes_per_atom_clash_mask"])
    assert diffused["radius_of_gyration"][0] != everything["radius_of_gyration"][0]


def test_no_kept_row_and_no_row_at_all():
    inp = vr.case_inputs(_fix(), "n65")
    got = _call(inp, diffuse_mask=np.zeros((1, 65), dtype=np.float32))  # all 65 rows at the origin
    assert np.isnan(got["radius_of_gyration"][0]) and got["clashes_per_atom_clash_mask"].all() and got["num_residue_violations"][0] == 65
    assert got["n_clash_pairs"][0] == 65 * 64 // 2 * 25 - 64
    none = _call(inp, res_mask=np.zeros((1, 65), dtype=np.float32))
    assert np.isnan(none["radius_of_gyration"][0]) and all(not none[k].any() for k in vr.FLOAT_OUTPUTS + vr.EXACT_OUTPUTS)


def test_end_to_end_sampler_small_config():
    """Two de novo samples (small config, N = 24, T = 6), the result left on the device: the violations of the device tensor agree with
    the restatement on the downloaded coordinates; nothing between the two calls waits for the device."""
    from framedipt_amd import config, inference, violations
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import UnconditionalSampler
    n, b, num_t = 24, 2, 6
    conf = config.small_config()
    d = SE3Diffuser(conf.diffuser, device="cuda:0")
    net = ScoreNetwork(conf.model, d, precision="fp32").load_synthetic(3).to("cuda:0")
    ds = UnconditionalSampler(config.to_conf({"min_length": n, "max_length": n, "length_step": 1, "samples_per_length": b}), d, "cuda:0")
    np.random.seed(11)
    items = [ds[i][2] for i in range(b)]
    feats = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    res = inference.inference_fn(net, d, feats, num_t=num_t, min_t=0.01, aux_traj=True, noise_scale=0.1, return_device=True)
    prot = res["prot_traj"][0]
    assert prot.is_cuda and tuple(prot.shape) == (b, n, 37, 3)
    got = violations.structural_violations(prot)
    host = prot.cpu().numpy()
    fix = _fix()
    for s in range(b):
        want = vr.violations(host[s])
        report = {}
        try:
            vr.check_outputs(want, vr.sample_of(got, s), lambda key: vr.widest_bound(fix, key), lambda k, err, lim: report.__setitem__(k, (err, lim)))
        finally:
            for k, (err, lim) in report.items():
                print(f"sampler[{s}]: {k}: |device - restatement| = {err:.3e}, bound {lim:.3e}")
        assert abs(got["radius_of_gyration"][s] - want["radius_of_gyration"]) <= 1e-13 * want["radius_of_gyration"]
    assert list(violations.violation_metrics(got, 1)) == list(violations.METRIC_KEYS)


def test_run_sharded_violations_on_a_de_novo_run(tmp_path):
    """``run_sharded --violations`` on a de novo run of two lengths: ``violations.json`` and ``violations.csv`` hold the numbers of a
    direct call on every written sample; without the flag the run writes the same files but these two."""
    import csv
    import json
    import os
    import subprocess
    import sys

    from conftest import ROOT
    from framedipt_amd import violations

    def run(out_dir, *flags):
        cmd = [sys.executable, "-m", "framedipt_amd.run_sharded", "--out-dir", str(out_dir), "--min-length", "9", "--max-length", "14", "--length-step", "5",
               "--samples-per-length", "2", "--num-t", "2", "--max-batch", "4", "--precision", "fp32", "--keep", "last", *flags]
        r = subprocess.run(cmd, env=dict(os.environ, FDIPT_SHARED_GPU="allow"), cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return sorted(os.listdir(out_dir))

    with_flag, without = run(tmp_path / "a", "--violations"), run(tmp_path / "b")
    assert [f for f in with_flag if not f.startswith("violations.")] == without and "violations.json" in with_flag and "violations.csv" in with_flag
    for f in without:
        if f.endswith(".npz"):
            x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
            assert all(np.array_equal(x[k], y[k]) for k in x.files) and x.files == y.files
    with open(tmp_path / "a" / "violations.json") as f:
        summary = json.load(f)
    with open(tmp_path / "a" / "violations.csv", newline="") as f:
        table = list(csv.DictReader(f))
    with open(tmp_path / "a" / "manifest.json") as f:
        records = {(r["name"], r["sample_i"]): r for r in json.load(f)["samples"]}
    assert len(summary["samples"]) == len(table) == 4 and sorted(e["n_res"] for e in summary["samples"]) == [9, 9, 14, 14]
    for entry, row in zip(summary["samples"], table):
        prot = np.load(tmp_path / "a" / records[(entry["pdb_name"], entry["sample"])]["file"])["prot_traj"]
        assert prot.shape == (entry["n_res"], 37, 3)
        direct = violations.structural_violations(prot[None])
        for k in violations.SCALARS + violations.COUNTS:
            assert entry[k] == direct[k][0].item() and float(row[k]) == direct[k][0].item(), k
        assert entry["residue_violations"] == violations.residue_violations(direct, 0)
        assert row["pdb_name"] == str(entry["pdb_name"]) and row["sample"] == str(entry["sample"])
