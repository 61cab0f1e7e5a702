"""CPU tests of the five-start mode of the structural alignment search (``inits="all"``; DESIGN.md section 7.9, "The two fragment
starts"): the NumPy restatement tests/tma_inits_ref.py against plain loops and hand-made traces, the fixture
tests/golden/tma_inits_cases.npz against the restatement, and the host side of the option."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import tma_inits_ref as ti
import tma_ref as ta
from conftest import GOLDEN, load_golden
from framedipt_amd import _lib, run_sharded, structure_search, tm_align

sys.path.insert(0, GOLDEN)
from make_goldens_tm import walk  # noqa: E402
from make_goldens_tma_inits import with_gaps  # noqa: E402


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("tma_inits_cases.npz")


def _trace(fix, name, side):
    prot_a, prot_b, mask_a, mask_b = ti.case_inputs(fix, name)
    return ta.compact(prot_a, mask_a)[0] if side == "a" else ta.compact(prot_b, mask_b)[0]


def test_jump_fragment_lengths_and_the_candidate_counts():
    assert [ti.jump(n) for n in (5, 6, 44, 45, 46, 150, 151, 200, 201, 250, 251, 512)] == [1, 2, 14, 15, 15, 15, 25, 25, 35, 35, 45, 45]
    assert ti.fragment_lengths(5) == [] and ti.fragment_lengths(6) == [3] and ti.fragment_lengths(8) == [4] and ti.fragment_lengths(9) == [3, 4]
    assert ti.fragment_lengths(60) == [20, 30] and ti.fragment_lengths(300) == [20, 100] and ti.fragment_lengths(19) == [6, 9]
    assert ti.candidates(5, 5) == [] and ti.candidates(5, 300) == []  # Ls = 5: I4 is skipped
    assert ti.candidates(6, 9) == [(3, i, j) for i in (0, 2) for j in (0, 3, 6)]
    count = lambda n1, n2: [sum(1 for c in ti.candidates(n1, n2) if c[0] == l) for l in ti.fragment_lengths(min(n1, n2))]  # noqa: E731
    assert count(300, 300) == [49, 25] and count(512, 512) == [121, 100]
    for n1, n2 in ((19, 22), (151, 150), (201, 200), (251, 250)):  # every fragment lies inside both traces, the order is (length, i, j)
        cands = ti.candidates(n1, n2)
        assert all(i + l <= n1 and j + l <= n2 for l, i, j in cands)
        assert cands == sorted(cands, key=lambda c: (ti.fragment_lengths(min(n1, n2)).index(c[0]), c[1], c[2]))


def test_frag_on_hand_made_traces():
    rng = np.random.default_rng(3)
    w = walk(rng, 40)
    assert ti.frag(w) == (0, 40)
    assert ti.frag(with_gaps(w, (15,))) == (15, 25)         # the longer side of one gap
    assert ti.frag(with_gaps(w, (25,))) == (0, 25)
    assert ti.frag(with_gaps(w[:28], (14,))) == (0, 14)     # two equal runs: the first
    assert ti.frag(with_gaps(walk(rng, 41), (14, 28))) == (0, 14)
    wide = w[0] + (w - w[0]) * (4.5 / 3.8)                   # 4.5 Angstrom throughout: singletons at 4.25, everything at 4.25 x 1.1
    assert ti.frag(wide) == (0, 40)
    assert ti.frag(w[:5]) == (0, 5) and ti.frag(with_gaps(w[:5], (1, 2, 3, 4), 100.0)) == (0, 1)  # r = min(4, 5 / 3) = 1: one row is a run
    far = w[0] + (w - w[0]) * 1e4                             # no cut within 64 rounds (4.25 x 1.1^63 = 1 722 Angstrom): the whole trace
    assert ti.frag(far) == (0, 40)
    c = 4.25
    for _ in range(2):
        c = c * 1.1
    just = w[0] + (w - w[0]) * (0.999 * c / 3.8)              # inside after two widening rounds
    assert ti.frag(just) == (0, 40) and ti.frag(with_gaps(just, (30,), 1.05 * c)) == (0, 30)
    # exactly at the cut is outside, the comparison is strict: steps of 4.25 (exact in binary) with one of 4.5 pass in the second round
    line = np.stack([np.arange(9) * 4.25, np.zeros(9), np.zeros(9)], axis=1)
    line[6:, 0] += 0.25
    assert ti.frag(line) == (0, 9) and ti.frag(with_gaps(line, (6,), 4.25 * 1.1 + 0.01)) == (0, 6)


def test_frag_of_the_fixture_constructions():
    fix = _fix()
    assert ti.frag(_trace(fix, "gap12", "b")) == (15, 25) and ti.frag(_trace(fix, "gap12", "a")) == (0, 40)
    assert ti.frag(_trace(fix, "equal_runs", "b")) == (0, 14)
    assert ti.frag(_trace(fix, "wide45", "b")) == (0, 36)
    assert ti.frag(_trace(fix, "donor_x", "a")) == (10, 20) and ti.frag(_trace(fix, "donor_x", "b")) == (0, 20)
    assert ti.frag(_trace(fix, "n5", "b")) == (0, 5)


def _plain_offsets(n1, n2, donor, f0, f1, mn):
    """I5's qualifying offsets by counting pairs one by one."""
    out = []
    for k in range(-n2, n1 + 1):
        js = [j for j in range(n2) if 0 <= j + k < n1 and (f0 <= j + k < f1 if donor == "x" else f0 <= j < f1)]
        if len(js) >= mn:
            assert js == list(range(js[0], js[-1] + 1))
            out.append((k, js[0], js[-1] + 1))
    return out


def test_fragment_threading_donor_trim_and_offsets():
    fix = _fix()
    x, y = _trace(fix, "donor_x", "a"), _trace(fix, "donor_x", "b")
    assert (len(x), len(y)) == (30, 36)
    assert ti.fragment_plan(x, y) == ("x", 10, 30, 8)           # equal runs, n1 <= n2: x gives; mn = max(2 min(20, 36) / 5, 3)
    assert ti.fragment_plan(y, x) == ("y", 10, 30, 8)           # n1 > n2: y gives
    x, y = _trace(fix, "gap12", "a"), _trace(fix, "gap12", "b")
    assert ti.fragment_plan(x, y) == ("y", 15, 40, 10) and ti.fragment_plan(y, x) == ("x", 15, 40, 10)  # the shorter run gives
    w = walk(np.random.default_rng(5), 130)
    assert ti.fragment_plan(w[:120], w[:125]) == ("x", 12, 107, 48)   # L == Ls: rows Ls / 10 .. 89 Ls / 100
    assert ti.fragment_plan(w[:125], w[:120]) == ("y", 12, 107, 48)
    assert ti.fragment_plan(w[:5], w[:5]) == ("x", 0, 5, 3) and ti.fragment_plan(w[:100], w[:100]) == ("x", 10, 90, 40)
    short = with_gaps(w[:8], (2, 4, 6), 30.0)                          # runs of two rows, r = 8 / 3 = 2: L = 2 < mn = 3, I5 is skipped
    assert ti.fragment_plan(short, w[:12]) == ("x", 0, 2, 3) and ti.fragment_offsets(8, 12, *ti.fragment_plan(short, w[:12])) == []
    assert ti.fragment_threading(short, w[:12], *ta.search_params(8)[:2])[0] is None
    for n1, n2, plan in ((30, 36, ("x", 10, 30, 8)), (36, 30, ("y", 10, 30, 8)), (120, 125, ("x", 12, 107, 48)), (5, 5, ("x", 0, 5, 3)), (40, 40, ("y", 15, 40, 10)),
                         (7, 9, ("y", 3, 5, 3))):
        assert ti.fragment_offsets(n1, n2, *plan) == _plain_offsets(n1, n2, *plan), (n1, n2, plan)
    # the map of the winning offset holds the fragment's rows only
    x, y = _trace(fix, "donor_x", "a"), _trace(fix, "donor_x", "b")
    m, f, k = ti.fragment_threading(x, y, *ta.search_params(30)[:2])
    rows = np.flatnonzero(m >= 0)
    assert k == 10 and (m[rows] == rows + k).all() and m[rows].min() >= 10 and len(rows) >= 8 and f > 0


def test_local_superposition_picks_the_first_best_candidate():
    fix = _fix()
    x, y = _trace(fix, "motif03", "a"), _trace(fix, "motif03", "b")
    d0s, ds, _ = ta.search_params(120)
    m, f, c, n = ti.local_superposition(x, y, d0s, ds)
    assert n == len(ti.candidates(120, 125)) == 81 and ti.candidates(120, 125)[c] == (20, 15, 90)  # a fragment pair on the motif's diagonal
    on = np.flatnonzero(m >= 0)
    assert ((m[on] - on) == -75).sum() >= 30
    assert f == ta.fast(m[None], x, y, d0s, ds)[0][0]
    assert ti.local_superposition(x[:5], y[:5], *ta.search_params(5)[:2]) == (None, -1.0, -1, 0)


@pytest.mark.parametrize("name", ti.PLANTED)
def test_planted_motif_is_found(name):
    """Two walks of 120 and 125 rows that share 40 rigid rows: the three default starts miss them, I4 finds them."""
    fix = _fix()
    default = ta.align_structures(*ti.case_inputs(fix, name))
    assert default["tm_b"] == float(fix[f"{name}.default_tm_b"])
    assert int(fix[f"{name}.best_init"]) >= 3 and float(fix[f"{name}.tm_b"]) >= default["tm_b"] + 0.1
    assert float(fix[f"{name}.tm_a"]) >= 0.3 and default["tm_a"] < 0.25  # 40 shared rows of 120 are 0.33
    got = fix[f"{name}.alignment"]
    on = np.flatnonzero(got >= 0)
    assert ((got[on] - on) == -75).sum() >= 36  # rows 80 .. 119 of the second on rows 5 .. 44 of the first


@pytest.mark.parametrize("name", ti.HOST_CASES)
def test_fixture_records_the_restatement_and_columns_0_to_2_are_the_default_search(name):
    """The cases up to 130 rows: the fixture holds what the restatement computes today, bit for bit; columns 0 .. 2 of ``init_tm`` and
    ``init_dp`` are tma_ref.tm_align's; where one of I1 - I3 wins, every output is."""
    fix = _fix()
    got = ti.align_structures(*ti.case_inputs(fix, name))
    for k in ti.FLOAT_OUTPUTS + ("d0_a", "d0_b", "rotation", "translation") + ti.EXACT_OUTPUTS:
        assert np.array_equal(np.asarray(got[k]), fix[f"{name}.{k}"], equal_nan=True), k
    assert float(fix[f"{name}.tm.yard"]) <= 1e-9
    default = ta.align_structures(*ti.case_inputs(fix, name))
    assert np.array_equal(got["init_tm"][:3], default["init_tm"]) and np.array_equal(got["init_dp"][:3], default["init_dp"])
    assert got["init_tm"].shape == (5,) and got["init_dp"].shape == (5,) and 0 <= got["best_init"] <= 4
    if got["best_init"] <= 2:
        for k in ("tm", "tm_a", "tm_b", "rmsd", "rotation", "translation", "alignment", "n_aligned", "best_init", "status"):
            assert np.array_equal(np.asarray(got[k]), np.asarray(default[k]), equal_nan=True), k
    else:
        assert got["init_tm"][got["best_init"]] > -1 and got["init_tm"].max() >= default["init_tm"].max()


def test_fixture_holds_the_named_cases():
    fix = _fix()
    assert tuple(fix["cases"]) == ti.CASES
    shape = {name: (int(fix[f"{name}.mask_a"].sum()), int(fix[f"{name}.mask_b"].sum())) for name in ti.CASES}
    assert shape == {"n5": (5, 5), "n6x9": (6, 9), "n19x22": (19, 22), "n64x65": (64, 65), "n151x150": (151, 150), "n201x200": (201, 200),
                     "n251x250": (251, 250), "n300": (300, 300), "n512": (512, 512), "gap12": (40, 40), "equal_runs": (41, 41), "wide45": (34, 36),
                     "donor_x": (30, 36), "donor_y": (36, 30), "masked": (69, 75), "motif03": (120, 125), "motif005": (120, 125)}
    assert fix["n5.init_tm"][3] == -1 and fix["n5.init_dp"][3] == 0 and fix["n5.init_tm"][4] > 0   # no candidate of I4 at Ls = 5; I5 runs
    assert fix["n6x9.init_tm"][3] > 0
    old = load_golden("tma_cases.npz")
    for side in ("ca_a", "ca_b", "mask_a", "mask_b"):
        assert np.array_equal(fix[f"masked.{side}"], old[f"masked.{side}"])
    assert np.array_equal(fix["masked.init_tm"][:3], old["masked.init_tm"]) and fix["masked.tm"] == old["masked.tm"]
    for name in ti.CASES:
        assert fix[f"{name}.init_tm"].shape == (5,) and fix[f"{name}.init_dp"].shape == (5,) and int(fix[f"{name}.status"]) == 0
        assert float(fix[f"{name}.tm.yard"]) <= 1e-9
    for key in fix:
        assert fix[key].dtype != object and (not key.endswith((".ca_a", ".ca_b")) or fix[key].dtype == np.float32)
    assert os.path.getsize(os.path.join(GOLDEN, "tma_inits_cases.npz")) <= 2 * os.path.getsize(os.path.join(GOLDEN, "tma_cases.npz"))


def test_a_bad_inits_is_refused_before_any_launch(tmp_path):
    prot = np.zeros((2, 9, 5, 3), dtype=np.float32)
    db = structure_search.StructureSet.from_arrays([np.zeros((9, 3))])
    for bad in ("both", "ALL", "", None, 1, 5):
        with pytest.raises(ValueError, match="inits"):
            tm_align.tm_align(prot, inits=bad)
        with pytest.raises(ValueError, match="inits"):
            structure_search.search(prot, db, inits=bad)
        with pytest.raises(ValueError, match="inits"):
            run_sharded.run_tm_align(str(tmp_path), [], {}, inits=bad)
    assert tm_align.INITS == {"default": _lib.TMA_INITS_DEFAULT, "all": _lib.TMA_INITS_ALL} == {"default": 0, "all": 1}
    assert tm_align.N_INITS == {"default": 3, "all": 5}
    members = [m for m, _ in _lib.TmAlignArgs._fields_]
    assert members[-1] == "inits" and "inits" not in [m for m, _ in _lib.SearchArgs._fields_]  # (the search takes the mode as an argument)
    import ctypes as C
    res, args = _lib.SIGNATURES["fdipt_structure_search_inits"]
    assert res == C.c_int and len(args) == 3 and args[1] == C.c_int32 and args[0] == _lib.SIGNATURES["fdipt_structure_search"][1][0]


def test_writers_of_run_sharded_record_the_mode(tmp_path):
    one = np.ones((1, 1))
    assert run_sharded.write_diversity_aligned(str(tmp_path), {16: one}, {16: one})["inits"] == "default"
    done = run_sharded.write_diversity_aligned(str(tmp_path), {16: one}, {16: one}, inits="all")
    assert done["inits"] == "all" and json.load(open(tmp_path / "diversity_aligned.json")) == done
    table = run_sharded.write_tm_align_table(str(tmp_path), {"1abc": {"samples": ["0"], "rows": 40, "matrix": one}}, inits="all")
    assert table["inits"] == "all" and json.load(open(tmp_path / "tm_align.json"))["inits"] == "all"
    assert run_sharded.write_tm_align_table(str(tmp_path), {})["inits"] == "default"
