"""CPU tests of the structural violations: the NumPy restatement (tests/violations_ref.py) against the reference fixture
(tests/golden/violation_cases.npz), the library's constants against the reference's, the C entry's argument checks, the host helpers of
framedipt_amd/violations.py and the command line of run_sharded."""
import ctypes as C

import numpy as np
import pytest

import violations_ref as vr
from conftest import load_golden

_CACHE = {}


def fixture():
    if "fix" not in _CACHE:
        _CACHE["fix"] = load_golden("violation_cases.npz")
    return _CACHE["fix"]


def restated(name):
    """The restatement's outputs for every sample of a case, computed once."""
    if name not in _CACHE:
        inp = vr.case_inputs(fixture(), name)
        _CACHE[name] = [vr.violations(inp["prot"][s], None, vr.keep_mask(inp["prot"][s], inp["diffuse_mask"][s]), inp["residue_index"][s])
                        for s in range(inp["prot"].shape[0])]
    return _CACHE[name]


@pytest.mark.parametrize("name", vr.CASES)
def test_restatement_matches_the_reference(name):
    """Every float output within 32 x the reference's own change under the recorded perturbations (the fixture's largest where the
    case's own is 0); masks, counts and num_residue_violations exactly."""
    fix = fixture()
    for s, got in enumerate(restated(name)):
        vr.check_sample(fix, name, s, got)


def test_fixture_reaches_the_branches_it_is_for():
    fix = fixture()
    kinds = {k: sum(st["kinds"][k] for name in vr.CASES for st in restated(name)) for k in vr.MASK_KINDS}
    assert all(v > 0 for v in kinds.values()), kinds
    assert all(v == 0 for v in restated("clean")[0]["kinds"].values())
    for k in vr.FLOAT_OUTPUTS + vr.EXACT_OUTPUTS:
        if k != "n_clash_pairs":
            assert not fix[f"clean.{k}"].any(), k
    # the pile of undiffused rows at the origin: all of their atoms carry the clash flag
    undiffused = fix["masked.diffuse_mask"][0] == 0
    assert undiffused.sum() == 13 and fix["masked.clashes_per_atom_clash_mask"][0][undiffused].all()
    steps = np.diff(fix["gaps.residue_index"][0]).tolist()
    assert steps.count(2) == 1 and steps.count(200) == 1 and steps.count(0) == 1
    assert fix["n1.n_clash_pairs"].tolist() == [0] and fix["n2.n_clash_pairs"].tolist() == [24]  # (one pair, C - N exempt)
    assert fix["n260.bb"].shape == (2, 260, 5, 3) and fix["n65.bb"].shape[1] == 65
    assert all(restated(name)[s]["margin"] >= 1e-3 for name in vr.CASES for s in range(len(restated(name))))


def test_float32_run_is_near_the_float64_run():
    """The reference as shipped (float32) against its float64 run: about 1e-7 relative, far above the yardsticks - the distance the
    device result is allowed to the tables users hold."""
    fix = fixture()
    for name in vr.CASES:
        for k in vr.FLOAT_OUTPUTS:
            a, b = fix[f"{name}.{k}"], fix[f"{name}.{k}.f32"]
            assert np.abs(a - b).max() <= 1e-4 * max(1.0, np.abs(a).max()), (name, k)


def test_library_constants_match_the_reference():
    from framedipt_amd import violations
    fix = fixture()
    got = violations.constants()
    assert [got[k] for k in violations.CONSTANT_NAMES] == fix["constants.head"].tolist()
    assert np.array_equal(got["lower"], fix["constants.lower"]) and np.array_equal(got["upper"], fix["constants.upper"])
    # the restatement's own copy
    assert fix["constants.head"].tolist() == [vr.RADIUS[1], vr.RADIUS[0], vr.RADIUS[4], vr.C_N_LENGTH, float(np.float32(0.014)), vr.C_N_TOLERANCE,
                                              vr.COS_CA_C_N, vr.CA_C_N_TOLERANCE / 12, vr.COS_C_N_CA, vr.C_N_CA_TOLERANCE / 12, vr.CA_CA]
    assert np.array_equal(vr.LOWER, fix["constants.lower"]) and np.array_equal(vr.UPPER, fix["constants.upper"])


def test_entry_refuses_bad_arguments_before_any_launch():
    """fdipt_sample_violations: FDIPT_EINVAL for a null pointer, B or N < 1 or an atom count it does not read, FDIPT_ESIZE for a workspace
    too small - decided before the device is touched (the pointers are never read)."""
    from framedipt_amd import _lib
    lib = _lib.load()
    assert lib.fdipt_sample_violations_workspace(3, 10) == 3 * 10 * 16 and lib.fdipt_sample_violations_workspace(0, 10) == 0
    assert lib.fdipt_sample_violations_workspace(3, 0) == 0
    pointers = [n for n, t in _lib.ViolationArgs._fields_ if t is C.c_void_p]

    def call(b=2, n=8, atoms=37, workspace_bytes=0, **over):
        args = _lib.ViolationArgs(B=b, N=n, atoms=atoms, workspace_bytes=workspace_bytes, **{**{k: 64 for k in pointers}, **over})
        return lib.fdipt_sample_violations(C.byref(args), None)

    assert call() == -3                                          # everything in order but the workspace
    assert call(workspace_bytes=2 * 8 * 16 - 1) == -3
    assert call(atoms=5) == -3
    assert call(b=0) == -1 and call(n=0) == -1 and call(b=-1) == -1
    assert call(atoms=14) == -1
    for name in pointers:
        assert call(workspace_bytes=1 << 20, **{name: None}) == -1, name
    assert lib.fdipt_sample_violations(None, None) == -1
    assert lib.fdipt_violation_constants(None) == -1


def test_violation_metrics_names_and_argument_checks():
    from framedipt_amd import violations
    res = {k: np.array([0.5, 1.5]) for k in violations.SCALARS}
    res["total_per_residue_violations_mask"] = np.array([[0, 1, 1, 0], [0, 0, 0, 0]], dtype=np.uint8)
    got = violations.violation_metrics(res, 1)
    assert list(got) == ["bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "clashes_mean_loss", "radius_of_gyration"]
    assert all(type(v) is float and v == 1.5 for v in got.values())
    assert violations.residue_violations(res, 0) == [1, 2] and violations.residue_violations(res, 1) == []
    assert set(vr.FLOAT_OUTPUTS) | {"radius_of_gyration"} == set(violations.SCALARS + violations.PER_RESIDUE + violations.PER_ATOM)
    assert set(vr.EXACT_OUTPUTS) == set(violations.COUNTS + violations.PER_RESIDUE_MASKS + violations.PER_ATOM_MASKS)
    with pytest.raises(ValueError, match="37, 3"):
        violations.structural_violations(np.zeros((2, 8, 14, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="'diffused' or 'all'"):
        violations.structural_violations(np.zeros((2, 8, 37, 3), dtype=np.float32), atoms="kept")
    with pytest.raises(ValueError, match="no samples"):
        violations.structural_violations(np.zeros((0, 8, 37, 3), dtype=np.float32))


def test_run_sharded_parses_the_violations_flag(monkeypatch, capsys):
    """The flag is an option of the command line (its help names the two files) and main() gathers and scores when it is set."""
    import sys

    from framedipt_amd import run_sharded
    monkeypatch.setattr(sys, "argv", ["run_sharded", "--help"])
    with pytest.raises(SystemExit) as done:
        run_sharded.main()
    text = " ".join(capsys.readouterr().out.split())
    assert done.value.code == 0 and "--violations" in text and "violations.json and violations.csv" in text
    monkeypatch.setattr(sys, "argv", ["run_sharded", "--out-dir", "x", "--violations=1"])
    with pytest.raises(SystemExit) as done:  # (a switch: it takes no value)
        run_sharded.main()
    assert done.value.code == 2
    a = run_sharded.parse_args(["--out-dir", "x", "--violations"])
    for inp in (False, True):  # the samples are gathered, the stage alone runs, and it needs no ground truth
        plan = run_sharded.stage_plan(a, inp)
        assert plan.collect and [s.flag for s in plan.stages] == ["violations"] and not plan.ground_truth and not plan.keep_selection
