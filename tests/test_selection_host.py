"""CPU tests of sample selection: the NumPy restatement (tests/selection_ref.py) against the reference fixture
(tests/golden/selection_cases.npz), the host side of framedipt_amd/selection.py, the C entry's argument checks and the grouping
helper of ``run_sharded --select``."""
import ctypes as C

import numpy as np
import pytest

import selection_ref as sr
from conftest import load_golden

_CACHE = {}


def fixture_and_restatement(name):
    """The fixture and, computed once per case, the restatement's outputs with both forms of the median."""
    if "fix" not in _CACHE:
        _CACHE["fix"] = load_golden("selection_cases.npz")
    fix = _CACHE["fix"]
    if name not in _CACHE:
        prot, mask = sr.case_inputs(fix, name)
        x = sr.gather(prot, np.nonzero(mask[0])[0])
        _CACHE[name] = (x, sr.select(x, median="weights"), sr.select(x, median="plain") if x.shape[0] > 1 else None)
    return (fix,) + _CACHE[name]


@pytest.mark.parametrize("name", [c for c in sr.CASES if c != "s1_l4"])
def test_restatement_matches_the_reference(name):
    """Plain and weight-space iteration against the reference's outputs: coordinates within 32 x the reference's own spread under a
    permutation of its samples, densities to 1e-12 relative (the argument of exp is a sum of M <= 480 squares: relative error of order
    M eps = 1e-13), indices exactly (the fixture's gaps are >= 1e-6)."""
    fix, x, weights, plain = fixture_and_restatement(name)
    bound = sr.coordinate_bound(fix, name)
    for got in (weights, plain):
        assert np.abs(got["mean"] - fix[f"{name}.mean"]).max() <= bound
        assert np.abs(got["median"] - fix[f"{name}.median"]).max() <= bound
        np.testing.assert_allclose(got["density"], fix[f"{name}.density"], rtol=1e-12)
        for k in ("mode", "mean_closest", "median_closest"):
            assert got[k] == int(fix[f"{name}.{k}"]), k
    assert weights["status"] == 0 and abs(weights["weights"].sum() - 1) <= 1e-12
    # the weights reproduce the median: every iterate is an affine combination of the samples
    assert np.abs(x.mean(0) + np.tensordot(weights["weights"], x - x.mean(0)[None], axes=1) - weights["median"]).max() == 0


def test_single_sample_takes_the_zero_distance_rule():
    fix, x, weights, _ = fixture_and_restatement("s1_l4")
    assert np.isnan(sr.plain_median(x, 3)).all()  # the reference: 0 / 0
    assert weights["status"] == sr.ZERO_DISTANCE and np.array_equal(weights["median"], x[0]) and weights["weights"].tolist() == [1.0]
    assert np.array_equal(weights["mean"], fix["s1_l4.mean"]) and weights["mode"] == 0 == weights["median_closest"]
    # ... and a median that falls on a sample exactly stops there too: three collinear points, the middle one is the median
    line = np.zeros((3, 1, 4, 3))
    line[0, ..., 0], line[2, ..., 0] = -1.0, 1.0
    med, w, status = sr.weight_median(line + 40.0)
    assert status == sr.ZERO_DISTANCE and w.tolist() == [0, 1, 0] and np.array_equal(med, line[1] + 40.0)


def test_argument_validation_raises():
    from framedipt_amd import selection
    prot = np.zeros((6, 8, 37, 3), dtype=np.float32)
    mask = np.zeros((6, 8), dtype=np.float32)
    mask[:, 2:5] = 1
    ids, members, residues = selection.plan_groups(mask, [7, 3, 7, 3, 3, 7])
    assert ids == [7, 3] and [m.tolist() for m in members] == [[0, 2, 5], [1, 3, 4]] and residues[1].tolist() == [2, 3, 4]
    differ = mask.copy()
    differ[2, 5] = 1
    with pytest.raises(ValueError, match="share"):
        selection.select_samples(prot, differ, [7, 3, 7, 3, 3, 7])
    selection.plan_groups(differ, [0, 1, 2, 1, 1, 0])  # (the odd one in a group of its own is fine)
    empty = mask.copy()
    empty[[1, 3, 4]] = 0
    with pytest.raises(ValueError, match="no diffused"):
        selection.select_samples(prot, empty, [7, 3, 7, 3, 3, 7])
    with pytest.raises(ValueError, match="at most 64"):
        selection.select_samples(np.zeros((65, 8, 37, 3), dtype=np.float32), np.ones((65, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="one id per sample"):
        selection.select_samples(prot, mask, [0, 1])
    with pytest.raises(ValueError, match="37, 3"):
        selection.select_samples(prot[:, :, :5], mask)
    with pytest.raises(ValueError, match="sigma"):
        selection.select_samples(prot, mask, sigma=0.0)


def test_selected_structure_replaces_the_backbone_columns_only():
    from framedipt_amd import selection
    rng = np.random.default_rng(5)
    prot = rng.normal(size=(4, 9, 37, 3)).astype(np.float32)
    residues = np.array([2, 3, 7])
    sel = {"members": [np.array([3, 1])], "residues": [residues], "mean": [rng.normal(size=(3, 4, 3))], "median": [rng.normal(size=(3, 4, 3))],
           "mode": np.array([1]), "mean_closest": np.array([0]), "median_closest": np.array([1])}
    for strategy in ("mean", "median"):
        out = selection.selected_structure(sel, 0, strategy, prot)
        changed = np.zeros((9, 37), dtype=bool)
        changed[np.ix_(residues, [2, 0, 1, 4])] = True
        assert out.dtype == np.float32 and np.array_equal(out[~changed], prot[3][~changed])  # the first member carries; CB (3) stays
        for a, col in enumerate((2, 0, 1, 4)):  # C, N, CA, O
            assert np.array_equal(out[residues, col], sel[strategy][0][:, a].astype(np.float32))
    assert np.array_equal(selection.selected_structure(sel, 0, "mode", prot), prot[1])
    assert np.array_equal(selection.selected_structure(sel, 0, "mean_closest", prot), prot[3])
    assert selection.carrier(sel, 0, "median") == 0 and selection.carrier(sel, 0, "median_closest") == 1
    with pytest.raises(ValueError):
        selection.selected_structure(sel, 0, "best", prot)


def test_grouping_by_structure_name_keeps_sample_order():
    from framedipt_amd import run_sharded
    recs = [{"item": i, "name": n, "sample_i": s, "file": f"{n}/sample_{s}/sample_{s}_1.pdb"}
            for i, n, s in ((5, "7abc", 2), (0, "1xyz", 0), (3, "7abc", 0), (1, "1xyz", 1), (4, "7abc", 1), (2, "1xyz", 2))]
    groups = run_sharded.group_records_by_name(recs)
    assert list(groups) == ["1xyz", "7abc"]
    assert [[r["item"] for r in rs] for rs in groups.values()] == [[0, 1, 2], [3, 4, 5]]
    assert [r["sample_i"] for r in groups["7abc"]] == [0, 1, 2]


def test_entry_refuses_bad_groups_before_any_launch():
    """fdipt_sample_select: FDIPT_ESIZE for a group of 65, FDIPT_EINVAL for an empty group or L = 0 - decided on the host counts, before
    the device is touched (the pointers here are never dereferenced)."""
    from framedipt_amd import _lib
    lib = _lib.load()
    assert lib.fdipt_select_workspace_bytes(3, 10, 5) == 3 * 64 * 64 * 8 + 64 and lib.fdipt_select_workspace_bytes(0, 10, 5) == 0

    def call(start, n_diffused, l_max=4, b=70):
        start, n_diffused = np.asarray(start, dtype=np.int32), np.asarray(n_diffused, dtype=np.int32)
        fake = {k: 64 for k in ("atom37", "diffuse_mask", "group_start", "member", "mean", "median", "weights", "density", "dist_to_mean",
                                "dist_to_median", "index", "status", "n_diffused", "workspace")}
        args = _lib.SelectArgs(B=b, N=8, G=len(n_diffused), L_max=l_max, group_start_host=start.ctypes.data, n_diffused_host=n_diffused.ctypes.data,
                               sigma=30.0, max_iterations=10, workspace_bytes=0, **fake)
        return lib.fdipt_sample_select(C.byref(args), None)

    assert call([0, 65], [3]) == -3
    assert call([0, 5, 70], [3, 3]) == -3
    assert call([0, 5, 5], [3, 3]) == -1      # empty group
    assert call([0, 5], [0]) == -1            # L = 0
    assert call([0, 5], [5]) == -1            # L > L_max
    assert call([0, 5], [3]) == -3            # workspace too small
