"""CPU tests of sample evaluation: the NumPy restatement (tests/evaluation_ref.py) against the reference fixture
(tests/golden/evaluation_cases.npz), the host side of framedipt_amd/evaluation.py (region planning, the reference's nested dicts and
column names, argument checks) and the C entry's argument checks."""
import ctypes as C

import numpy as np
import pytest

import evaluation_ref as er
from conftest import load_golden

_CACHE = {}


def fixture():
    if "fix" not in _CACHE:
        _CACHE["fix"] = load_golden("evaluation_cases.npz")
    return _CACHE["fix"]


def restated(name):
    """The restatement's outputs for every sample of a case, computed once."""
    if name not in _CACHE:
        inp = er.case_inputs(fixture(), name)
        _CACHE[name] = [er.evaluate(inp["prot"][s], inp["ref"][0], inp["diffuse_mask"][s], inp["chain_idx"][s], inp["res_mask"][s])
                        for s in range(inp["prot"].shape[0])]
    return _CACHE[name]


def as_result(name):
    """A case's restated outputs in the form ``evaluate_samples`` returns (what ``as_eval_dicts`` reads)."""
    per = restated(name)
    out = {k: np.stack([np.asarray(p[k]) for p in per]) for k in er.FLOAT_OUTPUTS + er.EXACT_OUTPUTS if k not in ("gt_dihedral", "region_bb_rmsd")}
    out.update(gt_dihedral=per[0]["gt_dihedral"][None], region_bb_rmsd=[p["region_bb_rmsd"] for p in per], regions=[p["regions"] for p in per],
               region_rows=[p["region_rows"] for p in per], ref_index=np.zeros(len(per), dtype=np.int64))
    return out


@pytest.mark.parametrize("name", er.CASES)
def test_restatement_matches_the_reference(name):
    """Every float output within 32 x the reference's own change under the recorded perturbations (the fixture's largest where the
    case's own is 0), NaN positions equal; clash counts, reflection flags and regions exactly."""
    fix = fixture()
    for s, got in enumerate(restated(name)):
        er.check_sample(fix, name, s, got)


def test_fixture_reaches_the_branches_it_is_for():
    fix = fixture()
    assert fix["mirror.reflection"].tolist() == [1, 1] and all(not fix[f"{c}.reflection"].any() for c in er.CASES if c != "mirror")
    assert (fix["clashy.num_ca_steric_clashes"] >= 3).all() and (fix["clashy.bb"][:, 17] == 0).all()
    valid = fix["clashy.ca_ca_valid_percent"]
    assert ((valid > 0) & (valid < 1)).all()  # bonds above and below ca_ca + 0.1
    # chain-end zeros inside the regions of region_at_chain_ends: phi at a chain's first row, psi and omega at another's last
    d = fix["region_at_chain_ends.dihedral"]
    assert (d[:, 0, 0] == 0).all() and (d[:, 1:, 13] == 0).all() and (d[:, 0, 1] != 0).all()
    wrapped = np.abs(fix["wrap.gt_dihedral"][None] - fix["wrap.dihedral"]) > 180
    assert wrapped.any() and (np.abs(fix["wrap.angle_error"]) <= 180).all()


def test_plan_regions_matches_the_fixture_and_the_diffusion_info_regions():
    from framedipt_amd import evaluation, output
    fix = fixture()
    for name in er.CASES:
        mask, chain = fix[f"{name}.diffuse_mask"], fix[f"{name}.chain_idx"]
        regions = evaluation.plan_regions(mask, chain)
        assert regions == er.case_regions(fix, name), name
        chains, starts, ends = output.get_diffused_region_per_chain(mask, chain)
        assert regions == list(zip(chains, starts, ends))
        planned, rows = evaluation.region_rows(mask, chain)
        assert planned == regions and rows == er.regions_of(mask, chain, np.ones(len(mask)))[1]
    # chain ids that do not start at 0, a float chain index, two runs in one chain, padding behind
    mask = np.array([0, 1, 1, 0, 1, 0, 1, 1, 1, 0, 0], dtype=np.float32)
    chain = np.array([5, 5, 5, 5, 5, 9, 9, 9, 9, 0, 0], dtype=np.float64)
    res = np.array([1] * 9 + [0, 0], dtype=np.float32)
    regions, rows = evaluation.region_rows(mask, chain, res)
    assert regions == [(0, 1, 2), (0, 4, 4), (1, 1, 3)] and rows == [(1, 2), (4, 4), (6, 8)]
    with pytest.raises(ValueError, match="not one run"):
        evaluation.region_rows(mask, np.array([5, 5, 9, 9, 5, 5, 9, 9, 9, 0, 0]), res)
    with pytest.raises(ValueError, match="not one run"):
        evaluation.region_rows(mask, chain, np.array([1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 0]))


@pytest.mark.parametrize("name", er.CASES)
def test_eval_dicts_and_column_names_match_the_reference(name):
    """``as_eval_dicts`` + ``flatten`` on the restated arrays against the reference's flatten(...) of its own metric functions for sample
    0: the same column names in the same order, values within the yardstick bounds (dict values are entries of the arrays)."""
    from framedipt_amd import evaluation
    fix = fixture()
    row = evaluation.eval_columns(as_result(name), 0, evaluation.default_region_names(len(er.case_regions(fix, name)), tcr=True))
    assert list(row) == fix[f"{name}.columns"].tolist()
    lim = max(er.bound(fix, name, k) for k in ("res_bb_rmsd", "region_bb_rmsd", "bb_rmsd", "dihedral", "gt_dihedral", "angle_error"))
    assert np.abs(np.array(list(row.values())) - fix[f"{name}.column_values"]).max() <= lim
    assert "bb_rmsd" in row and "bb_rmsd_alpha" in row and "bb_rmsd_alpha_-4" in row and "signed_angle_error_psi_alpha_-1" in row
    dicts = evaluation.as_eval_dicts(as_result(name), 0)
    assert list(dicts["chain_metrics"]["bb_rmsd"])[0] == "region1" and list(dicts["residue_group_metrics"]["gt"]) == ["psi", "omega", "phi"]
    first, last = as_result(name)["region_rows"][0][0]
    keys = list(dicts["residue_metrics"]["bb_rmsd"]["region1"])
    assert keys == [-4, -3, -2, -1] + list(range(1, last - first + 1 - 3))
    signed, unsigned = dicts["residue_group_metrics"]["signed_angle_error"], dicts["residue_group_metrics"]["angle_error"]
    assert all(unsigned[a][r][k] == abs(v) for a in signed for r in signed[a] for k, v in signed[a][r].items())


def test_host_helpers_restate_the_reference():
    from framedipt_amd import evaluation
    assert evaluation.convert_to_eval_idx(list("abcdefg")) == {-4: "d", -3: "e", -2: "f", -1: "g", 1: "a", 2: "b", 3: "c"} == er.convert_to_eval_idx(list("abcdefg"))
    assert evaluation.flatten({"a": {"x": 1, "y": [2, {"z": 3}]}, "b": 4}) == {"a_x": 1, "a_y_1": 2, "a_y_2_z": 3, "b": 4}
    assert evaluation.default_region_names(3, tcr=True) == ["alpha", "beta", "region3"] and evaluation.default_region_names(2) == ["region1", "region2"]


def test_argument_validation_raises():
    from framedipt_amd import evaluation
    prot, ref = np.zeros((3, 8, 37, 3), dtype=np.float32), np.zeros((1, 8, 37, 3), dtype=np.float32)
    mask = np.zeros((3, 8), dtype=np.float32)
    mask[:, 2:6] = 1
    with pytest.raises(ValueError, match="37, 3"):
        evaluation.evaluate_samples(prot[:, :, :5], ref, mask)
    with pytest.raises(ValueError, match="reference should be"):
        evaluation.evaluate_samples(prot, ref[:, :7], mask)
    with pytest.raises(ValueError, match="diffuse_mask"):
        evaluation.evaluate_samples(prot, ref, mask[:, :7])
    with pytest.raises(ValueError, match="chain_idx"):
        evaluation.evaluate_samples(prot, ref, mask, chain_idx=np.zeros((3, 7)))
    with pytest.raises(ValueError, match="out of range"):
        evaluation.evaluate_samples(prot, ref, mask, ref_index=[0, 1, 0])
    with pytest.raises(ValueError, match="one row per sample"):
        evaluation.evaluate_samples(prot, ref, mask, ref_index=[0, 0])
    with pytest.raises(ValueError, match="ref_index is needed"):
        evaluation.evaluate_samples(prot, np.zeros((2, 8, 37, 3), dtype=np.float32), mask)
    # a region shorter than 4 residues: refused by the dict form only
    short = as_result("l4")
    short["region_rows"] = [[(3, 5)]]
    with pytest.raises(ValueError, match="shorter than the 4"):
        evaluation.as_eval_dicts(short, 0)


def test_entry_refuses_bad_arguments_before_any_launch():
    """fdipt_sample_evaluate: FDIPT_EINVAL for a null pointer, R = 0, a ref_index out of range or a region table that does not add up,
    FDIPT_ESIZE for a workspace too small - decided on the host copies, before the device is touched (the pointers are never read)."""
    from framedipt_amd import _lib
    lib = _lib.load()
    assert lib.fdipt_eval_workspace_bytes(3, 10) == 3 * 10 * 12 and lib.fdipt_eval_workspace_bytes(0, 10) == 0
    device = [n for n, t in _lib.EvalArgs._fields_ if t is C.c_void_p and not n.endswith("_host")]

    def call(ref_index, start, r=2, n_regions=None, max_regions=2, workspace_bytes=0, **over):
        ref_index, start = np.asarray(ref_index, dtype=np.int32), np.asarray(start, dtype=np.int32)
        args = _lib.EvalArgs(B=len(ref_index), N=8, R=r, n_regions=int(start[-1]) if n_regions is None else n_regions, max_regions=max_regions,
                             ref_index_host=ref_index.ctypes.data, region_start_host=start.ctypes.data, workspace_bytes=workspace_bytes,
                             **{**{k: 64 for k in device}, **over})
        return lib.fdipt_sample_evaluate(C.byref(args), None)

    assert call([0, 1], [0, 1, 2]) == -3                      # everything in order but the workspace
    assert call([0, 1], [0, 1, 2], r=0) == -1
    assert call([0, 2], [0, 1, 2]) == -1                      # ref_index out of range
    assert call([0, -1], [0, 1, 2]) == -1
    assert call([0, 1], [0, 3, 4]) == -1                      # more regions than max_regions
    assert call([0, 1], [0, 2, 1]) == -1                      # not ascending
    assert call([0, 1], [1, 1, 2]) == -1                      # does not start at 0
    assert call([0, 1], [0, 1, 2], n_regions=3) == -1
    assert call([0, 1], [0, 1, 2], ref37=None) == -1
    assert call([0, 1], [0, 1, 2], rotation=None) == -1
