"""CPU tests of the superposition-free accuracy scores: the NumPy restatement (tests/lddt_ref.py) against the reference fixture
(tests/golden/lddt_cases.npz), the C entry's argument checks, the host side of framedipt_amd/lddt.py and the command line of run_sharded."""
import ctypes as C

import numpy as np
import pytest

import lddt_ref as lr
from conftest import load_golden

_CACHE = {}


def fixture():
    if "fix" not in _CACHE:
        _CACHE["fix"] = load_golden("lddt_cases.npz")
    return _CACHE["fix"]


def restated(name, mode, same_residue):
    key = (name, mode, same_residue)
    if key not in _CACHE:
        _CACHE[key] = lr.restate_case(fixture(), name, mode, same_residue)
    return _CACHE[key]


def score_rows(fix, name):
    """[P,N] bool: the score rows of every pair of a case."""
    models = lr.case_pairs(fix, name)[:, 0]
    return (fix[f"{name}.res_mask"][models] != 0) & (fix[f"{name}.score_mask"][models] != 0)


@pytest.mark.parametrize("name,mode", lr.CASE_MODES)
def test_restatement_equals_the_reference_lddt_bit_for_bit(name, mode):
    """Where the reference's function applies - ``lddt_ca`` for the ``ca`` set, ``lddt`` on the flattened atoms for ``same_residue`` in the
    multi-atom sets; per score row always, globally where every existing row is a score row - the restatement holds its float64 bits."""
    fix = fixture()
    got = restated(name, mode, mode != "ca")
    keep = score_rows(fix, name)
    assert np.array_equal(got["atom_lddt"][keep], fix[f"{name}.{mode}.ref_atom"][keep])
    if mode == "ca":
        assert np.array_equal(got["res_lddt"][keep], fix[f"{name}.{mode}.ref_atom"][..., 0][keep])
    if lr.reference_applies_globally(fix, name):
        assert np.array_equal(got["lddt"], fix[f"{name}.{mode}.ref_lddt"])
    assert not got["res_lddt"][~keep].any() and not got["n_scored"][~keep].any()
    # the float32 run of the reference is near: the thresholds are decided alike up to a few pairs
    assert np.abs(fix[f"{name}.{mode}.ref_atom.f32"][keep] - fix[f"{name}.{mode}.ref_atom"][keep]).max(initial=0.0) <= 0.05


@pytest.mark.parametrize("name", lr.CASES)
def test_restatement_matches_drmsd_and_fape_within_the_yardstick(name):
    """dRMSD against ``compute_drmsd`` on float64 tensors, FAPE against the recorded restatement (the reference's ``Rigid`` is float32: its
    number is within 1e-5 relative, asserted by the generator and here), each within 32 x the recorded change under row permutations."""
    fix = fixture()
    got = restated(name, lr.CASES[name][0], False)
    lr.check_floats({k: fix[f"{name}.{k}"] for k in lr.FLOAT_OUTPUTS}, got, lambda k: lr.bound(fix, name, k))
    assert 0 <= float(fix[f"{name}.fape.ref_distance"]) <= 1e-5
    framed = (got["status"] & lr.NO_FRAME) == 0
    assert np.all(np.abs(fix[f"{name}.fape.f32"] - got["fape"])[framed] <= 1e-5 * got["fape"][framed])
    assert np.all(np.abs(fix[f"{name}.drmsd.f32"] - got["drmsd"]) <= 1e-4 * np.maximum(got["drmsd"], 1e-3))


def test_fixture_reaches_the_edges_it_is_for():
    from framedipt_amd import _lib
    fix = fixture()
    assert fix["tile"] == _lib.LDDT_TILE and fix["tile_all"] == _lib.LDDT_TILE_ALL
    assert fix["tile.xa"].shape == (1, _lib.LDDT_TILE + 1, 5, 3) and fix["tile_all.xa"].shape == (1, _lib.LDDT_TILE_ALL + 1, 37, 3)
    assert [fix[f"{n}.xa"].shape[1] for n in ("n1", "n2", "n63", "n64", "n65")] == [1, 2, 63, 64, 65]
    assert all(float(fix[f"{name}.margin"]) >= 1e-9 for name in lr.CASES)
    assert all(np.abs(fix[f"{name}.xa"]).max() <= 100 and fix[f"{name}.xa"].dtype == np.float32 for name in lr.CASES)
    # N = 1: no partner, lDDT 1.0 with the status bit, dRMSD 0
    one = restated("n1", "ca", False)
    assert one["lddt"].tolist() == [1.0] and one["res_lddt"].tolist() == [[1.0]] and one["status"].tolist() == [lr.NO_PARTNER] and one["drmsd"].tolist() == [0.0]
    assert restated("n2", "ca", False)["status"].tolist() == [0]
    # 13 rows that do not exist, inside the chain too; a 12-row loop of a two-chain complex
    gone = np.flatnonzero(fix["masked.res_mask"][0] == 0)
    assert len(gone) == 13 and gone.min() > 0 and gone.max() < 47
    assert np.flatnonzero(fix["loop.score_mask"][0]).tolist() == list(range(10, 22)) and np.bincount(fix["loop.chain_index"]).tolist() == [30, 18]
    ctx = fix["loop.score_mask"][0] == 0
    assert np.array_equal(fix["loop.xa"][0][ctx], fix["loop.xb"][0][ctx]) and restated("loop", "ca", False)["n_scored"][0][10:22].min() > 12
    # atoms count only where both structures have them
    assert not fix["sidechain.xa"][0, :, 5:].any() and fix["sidechain.xb"][0, :, 5:].any()
    side, bare = restated("sidechain", "all", False), fix["sidechain.xb"][0].copy()
    bare[:, 5:] = 0  # (the reference without its side chains scores the same pairs: N, CA, C, CB, O of both)
    same = lr.local_accuracy(fix["sidechain.xa"][0], bare, "all")
    assert np.array_equal(side["n_scored"][0], same["n_scored"]) and np.array_equal(side["res_lddt"][0], same["res_lddt"])
    assert side["n_scored"][0].max() <= 5 * 5 * 23 and (side["n_scored"] > restated("sidechain", "backbone", False)["n_scored"]).all()
    # the planted pair: (1, 8) inside the cutoff, (2, 9) outside, 1e-3 from it
    ref = fix["cutoff.xb"][0].astype(np.float64)
    (i, j), (k, l) = fix["cutoff.planted"]
    inside, outside = np.linalg.norm(ref[i, 1] - ref[j, 1]), np.linalg.norm(ref[k, 1] - ref[l, 1])
    assert 15 - 1.5e-3 < inside < 15 - 0.5e-3 and 15 + 0.5e-3 < outside < 15 + 1.5e-3
    near = lr.local_accuracy(fix["cutoff.xa"][0], fix["cutoff.xb"][0], "ca", cutoff=15.0 - 2e-3)
    far = lr.local_accuracy(fix["cutoff.xa"][0], fix["cutoff.xb"][0], "ca", cutoff=15.0 + 2e-3)
    base = restated("cutoff", "ca", False)
    assert base["n_scored"][0, [i, j]].tolist() == (near["n_scored"][[i, j]] + 1).tolist()
    assert base["n_scored"][0, [k, l]].tolist() == (far["n_scored"][[k, l]] - 1).tolist()
    # a row whose N is missing has no frame and is still a point
    no_n = restated("no_n", "ca", False)
    assert no_n["res_fape"][0, 5] == 0 and np.count_nonzero(no_n["res_fape"][0]) == 11 and no_n["n_scored"][0, 5] > 0
    assert fix["b2.ref_index"].tolist() == [1, 0] and fix["b2.pairs"].tolist() == [[0, 1], [1, 0]]
    assert len(fix["s3.pairs"]) == 6 and "s3.xb" not in fix
    s3 = restated("s3", "ca", False)["lddt"]
    assert s3[0] != s3[2]  # (0, 1) against (1, 0): the reference structure chooses the pairs


def test_mariani_and_openfold_definitions_differ_by_the_pairs_inside_a_residue():
    fix = fixture()
    mariani, openfold = restated("n65", "backbone", False), restated("n65", "backbone", True)
    assert np.array_equal(openfold["n_scored"], mariani["n_scored"] + 12) and np.array_equal(openfold["n_passed"], mariani["n_passed"] + 12)
    assert (openfold["lddt"] > mariani["lddt"]).all()
    # the CA set scores the same distances whatever the layout
    trace = lr.local_accuracy(fix["n65.xa"][0][:, 1], fix["n65.xb"][0][:, 1], "ca")
    whole = restated("n65", "ca", False)
    assert np.array_equal(trace["res_lddt"], whole["res_lddt"][0]) and trace["drmsd"] == whole["drmsd"][0]
    assert trace["status"] == lr.NO_FRAME and trace["fape"] == 0 and not trace["res_fape"].any()


def test_status_macros_are_bound():
    from framedipt_amd import _lib, lddt
    assert (_lib.LDDT_NO_PARTNER, _lib.LDDT_NO_FRAME, _lib.LDDT_SKIPPED) == (lr.NO_PARTNER, lr.NO_FRAME, lr.SKIPPED) == (1, 2, 4)
    assert (_lib.LDDT_CA, _lib.LDDT_BACKBONE, _lib.LDDT_ALL) == (0, 1, 2) and (_lib.LDDT_TILE, _lib.LDDT_TILE_ALL) == (256, 64)
    assert lddt.SET_ATOMS == lr.SET_ATOMS and lddt.THRESHOLDS == lr.THRESHOLDS and list(lddt.BACKBONE_COLUMNS) == lr.columns("backbone", 37)
    assert dict(_lib.LddtArgs._fields_)["cutoff"] is C.c_double and dict(_lib.LddtArgs._fields_)["atom_lddt"] is C.c_void_p


def test_entry_refuses_bad_arguments_before_any_launch():
    """fdipt_sample_lddt: FDIPT_EINVAL for a null pointer, a size below 1, a layout or an atom set it does not have, FDIPT_ESIZE for a
    workspace too small or a row counter that N A A overflows - decided before the device is touched (the pointers are never read)."""
    from framedipt_amd import _lib
    lib = _lib.load()
    assert lib.fdipt_sample_lddt_workspace(3, 10) == 3 * 10 * 20 and lib.fdipt_sample_lddt_workspace(0, 10) == 0 == lib.fdipt_sample_lddt_workspace(3, 0)
    pointers = [n for n, t in _lib.LddtArgs._fields_ if t is C.c_void_p]
    optional = ("prot_b", "atom_mask_a", "atom_mask_b", "atom_lddt")

    def call(workspace_bytes=0, **over):
        kw = dict(S=2, N=8, atoms=37, S_b=2, atoms_b=37, P=2, mode=0, same_residue=0, cutoff=15.0, workspace_bytes=workspace_bytes)
        kw.update({k: 64 for k in pointers})
        kw.update(over)
        return lib.fdipt_sample_lddt(C.byref(_lib.LddtArgs(**kw)), None)

    assert call() == -3 and call(workspace_bytes=2 * 8 * 20 - 1) == -3        # everything in order but the workspace
    assert call(atoms=5, atoms_b=1) == -3 and call(mode=2) == -3 and call(mode=1, atoms_b=5) == -3
    assert call(S=0) == -1 and call(N=0) == -1 and call(P=0) == -1 and call(S_b=0) == -1
    assert call(atoms=14) == -1 and call(atoms_b=4) == -1 and call(mode=3) == -1 and call(mode=-1) == -1
    assert call(mode=2, atoms_b=5) == -1 and call(mode=1, atoms=1) == -1 and call(mode=1, atoms_b=1) == -1
    assert call(cutoff=0.0) == -1 and call(cutoff=float("nan")) == -1
    assert call(prot_b=None, S_b=0, atoms_b=0) == -3                          # (S_b and atoms_b are ignored without prot_b)
    for name in set(pointers) - set(optional):  # (never a call that would pass every check: the pointers are no memory)
        assert call(workspace_bytes=1 << 20, **{name: None}) == -1, name
    assert lib.fdipt_sample_lddt(None, None) == -1


def test_shape_and_argument_errors_come_before_the_library(monkeypatch):
    from framedipt_amd import _call, _lib, lddt

    def boom(*a, **kw):
        raise AssertionError("the library or the device was touched")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_call, "upload", boom)
    x = np.zeros((2, 8, 37, 3), dtype=np.float32)
    bad = [(dict(prot_a=np.zeros((2, 8, 14, 3))), "37, 3"), (dict(prot_a=np.zeros((2, 8, 2))), "37, 3"), (dict(prot_a=np.zeros((0, 8, 3))), "no structures"),
           (dict(prot_a=x, atoms="heavy"), "'ca', 'backbone' or 'all'"), (dict(prot_a=x, prot_b=np.zeros((2, 9, 37, 3))), "8 rows"),
           (dict(prot_a=x, prot_b=np.zeros((2, 8, 5, 3)), atoms="all"), "atom37"), (dict(prot_a=np.zeros((2, 8, 3)), atoms="backbone"), "backbone atoms"),
           (dict(prot_a=x, prot_b=np.zeros((3, 8, 37, 3))), "ref_index or pairs"), (dict(prot_a=x, res_mask=np.ones((2, 9))), "res_mask"),
           (dict(prot_a=x, score_mask=np.ones((1, 8))), "score_mask"), (dict(prot_a=x, atom_mask_a=np.ones((2, 8, 5))), "atom_mask_a"),
           (dict(prot_a=x, atom_mask_b=np.ones((2, 8, 37))), "without prot_b"), (dict(prot_a=x, prot_b=x[:, :, :5], atom_mask_b=np.ones((2, 8, 37))), "atom_mask_b"),
           (dict(prot_a=x, cutoff=0.0), "positive")]
    for kw, message in bad:
        with pytest.raises(ValueError, match=message):
            lddt.local_accuracy(**kw)
    # one structure against itself alone: no pair, nothing to launch
    alone = lddt.local_accuracy(x[:1])
    assert alone["lddt"].shape == (0,) and alone["matrix"].tolist() == [[1.0]] and alone["consensus"].shape == (1, 8) and alone["res_lddt"].shape == (0, 8)
    assert lddt.ordered_pairs(3).tolist() == [[0, 1], [0, 2], [1, 0], [1, 2], [2, 0], [2, 1]]


def test_lddt_metrics_and_consensus():
    from framedipt_amd import lddt
    res = {"atoms": "backbone", "lddt": np.array([0.5, 0.75]), "drmsd": np.array([1.0, 2.0]), "fape": np.array([0.1, 0.2]), "region_fape": np.array([0.3, 0.4])}
    got = lddt.lddt_metrics(res, 1)
    assert got == {"lddt_bb": 0.75, "drmsd": 2.0, "fape": 0.2, "region_fape": 0.4} and all(type(v) is float for v in got.values())
    assert list(lddt.lddt_metrics(dict(res, atoms="ca"), 0))[0] == "lddt_ca" and list(lddt.lddt_metrics(dict(res, atoms="all"), 0))[0] == "lddt_all"
    rows = np.arange(12, dtype=np.float64).reshape(6, 2)
    want = np.stack([rows[[0, 1]].mean(0), rows[[2, 3]].mean(0), rows[[4, 5]].mean(0)])
    assert np.array_equal(lddt.consensus(rows, lddt.ordered_pairs(3), 3), want)


def test_run_sharded_parses_the_lddt_flag(monkeypatch, capsys):
    """The flag is an option of the command line (its help names the files) and main() gathers and scores when it is set."""
    import sys

    from framedipt_amd import run_sharded
    monkeypatch.setattr(sys, "argv", ["run_sharded", "--help"])
    with pytest.raises(SystemExit) as done:
        run_sharded.main()
    text = " ".join(capsys.readouterr().out.split())
    assert done.value.code == 0 and "--lddt" in text and "lddt.json and lddt.csv" in text and "consistency.json" in text
    monkeypatch.setattr(sys, "argv", ["run_sharded", "--out-dir", "x", "--lddt=1"])
    with pytest.raises(SystemExit) as done:  # (a switch: it takes no value)
        run_sharded.main()
    assert done.value.code == 2
    a = run_sharded.parse_args(["--out-dir", "x", "--lddt"])
    for inp in (False, True):  # the samples are gathered, the stage alone runs, the ground truth is built in inpainting runs only
        plan = run_sharded.stage_plan(a, inp)
        assert plan.collect and [s.flag for s in plan.stages] == ["lddt"] and plan.ground_truth == inp and not plan.keep_selection
