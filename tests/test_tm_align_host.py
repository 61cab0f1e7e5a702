"""CPU tests of the structural-alignment contract as tests/tma_ref.py restates it - the closed forms a search
over alignments must reach (a copy, a shifted window, a deletion), Sec, the dynamic programme and its tie rules, the start step of the
seeds, the statuses, the recorded fixture - and of the host side: the ABI struct of framedipt_amd/tm_align.py against the host C
compiler, the writers of ``run_sharded --tm-align``."""
import csv
import ctypes as C
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import tm_ref as tr
import tma_ref as ta
from conftest import ROOT, load_golden
from framedipt_amd import _lib, run_sharded, tm_align

ORIGIN = np.array([31.0, -47.0, 58.0])


def _walk(rng, n, persist=0.7):
    d, out = rng.normal(size=3), [np.zeros(3)]
    for _ in range(n - 1):
        d = persist * d + (1.0 - persist) * 1.5 * rng.normal(size=3)
        d /= np.linalg.norm(d)
        out.append(out[-1] + 3.8 * d)
    return (np.array(out) + ORIGIN).astype(np.float32).astype(np.float64)


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def _move(rng, x):
    return x @ _rotation(rng).T + rng.normal(size=3) * 20.0


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("tma_cases.npz")


@functools.lru_cache(maxsize=None)
def _walk86():
    return _walk(np.random.default_rng(5), 86)


def test_rigid_copy_scores_one_with_the_identity_alignment():
    rng = np.random.default_rng(1)
    y = _walk86()[:80]
    got = ta.tm_align(_move(rng, y), y)
    assert abs(got["tm_a"] - 1.0) <= 1e-12 and abs(got["tm_b"] - 1.0) <= 1e-12 and got["tm"] == got["tm_b"]
    assert np.array_equal(got["alignment"], np.arange(80)) and got["n_aligned"] == 80 and got["status"] == 0 and got["rmsd"] < 1e-6
    assert np.abs(got["init_tm"] - 1.0).max() <= 1e-12 and got["best_init"] == 0


def test_window_shifted_by_six_is_found_and_the_fixed_correspondence_scores_below():
    """Rows 6 .. 85 against rows 0 .. 79 of one walk: the 74 shared rows superpose exactly, so tm >= 74 / 80; row j of y is row j - 6
    of x, and j + 6 with the two structures swapped.  The row-by-row score of section 7.8 is far below."""
    rng = np.random.default_rng(2)
    w = _walk86()
    x, y = _move(rng, w[6:]), w[:80]
    got = ta.tm_align(x, y)
    assert got["tm"] >= 74.0 / 80.0 - 1e-9 and got["tm"] <= 1.0
    assert np.array_equal(got["alignment"][6:], np.arange(74)) and got["offset"] == -6
    fixed = tr.tm_score(x, y)["tm"]
    assert fixed < got["tm"] and fixed < 0.5
    back = ta.tm_align(w[:80], _move(rng, w[6:]))  # the other way round: row j of y is row j + 6 of x
    assert back["tm"] >= 74.0 / 80.0 - 1e-9 and np.array_equal(back["alignment"][:74], np.arange(74) + 6) and back["offset"] == 6
    assert back["n_aligned"] == 74 and (back["alignment"][74:] == -1).all()


def test_deletion_is_bridged_exactly():
    """80 rows against the same 80 with rows 30 - 36 deleted: every row of the shorter chain has its partner."""
    rng = np.random.default_rng(3)
    x = _walk86()[:80]
    keep = np.delete(np.arange(80), np.arange(30, 37))
    got = ta.tm_align(x, _move(rng, x[keep]))
    assert got["tm_b"] >= 1.0 - 1e-9 and got["tm_a"] >= 73.0 / 80.0 - 1e-9 and got["tm_a"] < 74.0 / 80.0
    assert np.array_equal(got["alignment"], keep) and got["n_aligned"] == 73
    assert got["d0_a"] == tr.d0_of(80) and got["d0_b"] == tr.d0_of(73)


def _helix(n):
    k = np.arange(n)
    return np.stack([2.3 * np.cos(np.radians(100.0) * k), 2.3 * np.sin(np.radians(100.0) * k), 1.5 * k], axis=1)


def _strand(n):
    k = np.arange(n)
    return np.stack([3.3 * k, 0.9 * (-1.0) ** k, np.zeros(n)], axis=1)


def test_sec_on_an_ideal_helix_and_strand():
    """An alpha helix (radius 2.3, rise 1.5, 100 degrees per residue: CA distances i,i+2 5.45 and i,i+3 5.03, i,i+4 6.2) and a pleated strand
    (3.3 per residue: 6.6, 10.1, 13.2): every row but the two at either end is H, respectively E; a straight line with 3.8 steps is
    neither, and its (i - 2, i + 2) distance of 15.2 is beyond 8, so it is coil."""
    assert ta.sec_string(_helix(12)) == "CC" + "H" * 8 + "CC"
    assert ta.sec_string(_strand(12)) == "CC" + "E" * 8 + "CC"
    line = np.stack([3.8 * np.arange(9), np.zeros(9), np.zeros(9)], axis=1)
    assert ta.sec_string(line) == "C" * 9
    turn = _helix(9) * np.array([1.0, 1.0, 0.2])  # the rise squeezed: no helix distances, but rows i - 2 and i + 2 are close
    assert set(ta.sec_string(turn)[2:-2]) == {"T"}
    assert ta.sec_string(_helix(4)) == "CCCC"


def test_dp_on_hand_made_matrices():
    """3 x 4 score matrices: the diagonal, a forced gap, the gap penalty changing the choice, and the tie rules (the diagonal wins ties;
    in the traceback the move along y wins a tie with the move along x)."""
    one = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    assert ta.dp(one, -1.0).tolist() == [0, 1, 2, -1]
    shifted = np.array([[0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])
    assert ta.dp(shifted, -1.0).tolist() == [-1, 0, 1, 2]
    gapped = np.array([[1.0, 0, 0, 0], [0, 0, 0.9, 0], [0, 0, 0, 0.9]])  # rows 1, 2 of x fit columns 2, 3: a gap of one column
    assert ta.dp(gapped, 0.0).tolist() == [0, -1, 1, 2]
    # with a penalty of -1 the gap costs what row 0's pair brings (1.0): cell (1, 2) is a three-way tie at 0, which the diagonal wins,
    # so the path is the shifted diagonal (0 + 0.9 + 0.9) and row 0 of x pairs with column 1 at a score of 0
    assert ta.dp(gapped, -1.0).tolist() == [-1, 0, 1, 2]
    zeros = np.zeros((3, 4))  # all ties: d >= h and d >= v everywhere, the path is the diagonal from the far corner
    assert ta.dp(zeros, 0.0).tolist() == [-1, 0, 1, 2]
    assert ta.dp(zeros, -0.6).tolist() == [-1, 0, 1, 2]
    assert ta.dp(np.zeros((4, 3)), 0.0).tolist() == [1, 2, 3]


def test_dp_is_monotone_and_matches_a_plain_double_loop():
    rng = np.random.default_rng(4)
    for n1, n2, g in ((7, 11, -0.6), (12, 5, 0.0), (9, 9, -1.0)):
        score = rng.random((n1, n2))
        val, path = np.zeros((n1 + 1, n2 + 1)), np.zeros((n1 + 1, n2 + 1), dtype=bool)
        for i in range(1, n1 + 1):
            for j in range(1, n2 + 1):
                d = val[i - 1, j - 1] + score[i - 1, j - 1]
                h = val[i - 1, j] + (g if path[i - 1, j] else 0.0)
                v = val[i, j - 1] + (g if path[i, j - 1] else 0.0)
                path[i, j] = d >= h and d >= v
                val[i, j] = d if path[i, j] else (v if v >= h else h)
        want, i, j = np.full(n2, -1), n1, n2
        while i > 0 and j > 0:
            if path[i, j]:
                want[j - 1], i, j = i - 1, i - 1, j - 1
            else:
                h = val[i - 1, j] + (g if path[i - 1, j] else 0.0)
                v = val[i, j - 1] + (g if path[i, j - 1] else 0.0)
                i, j = (i, j - 1) if v >= h else (i - 1, j)
        got = ta.dp(score, g)
        assert np.array_equal(got, want)
        assert np.all(np.diff(got[got >= 0]) > 0)


def test_start_step_seed_counts():
    """Starts 0, step, 2 step, ... up to k - l plus k - l itself: k = 300 at step 40 has 1 + 5 + 7 + 8 + 9 + 9 seeds, step 1 the 1 222 of
    section 7.8; the last start of every level is k - l."""
    assert ta.starts(300, 150, 40).tolist() == [0, 40, 80, 120, 150] and ta.starts(300, 300, 40).tolist() == [0]
    assert ta.starts(80, 40, 40).tolist() == [0, 40] and ta.starts(81, 40, 40).tolist() == [0, 40, 41]
    length, start = ta.seeds(300, 40)
    assert len(length) == 1 + 5 + 7 + 8 + 9 + 9
    assert len(ta.seeds(300, 1)[0]) == 1222 == len(tr.seeds(300)[0])
    for k in (3, 5, 9, 80, 130):
        assert np.array_equal(ta.seeds(k, 1)[0], tr.seeds(k)[0]) and np.array_equal(ta.seeds(k, 1)[1], tr.seeds(k)[1])
        length, start = ta.seeds(k, 40)
        assert np.all(start + length <= k) and all((start[length == l] == k - l).any() for l in set(length.tolist()))


def test_search_at_step_one_without_d8_is_the_search_of_the_tm_score():
    rng = np.random.default_rng(6)
    y = _walk(rng, 37)
    x = _move(rng, y + rng.normal(size=y.shape) * 0.6)
    d0 = tr.d0_of(37)
    s, t = ta.search(x, y, d0, min(max(d0, 4.5), 8.0)), tr.tm_score(x, y)
    assert s["S"] / 37 == t["tm"] and s["best_seed"] == t["best_seed"] and s["passes"] == t["passes"]
    far = ta.search(x, y, d0, min(max(d0, 4.5), 8.0), 1, 0.5)  # a d8 of 0.5: only pairs within 0.5 score
    assert far["S"] < s["S"]


def test_widening_of_the_fast_cut_is_the_smallest_number_of_half_steps():
    """``widened`` against counting the steps one by one: the first cut ``first + 0.5 n``, n >= 1, with the third smallest squared
    distance inside, also where the distance lies on a step and where the limit ends the widening."""
    rng = np.random.default_rng(9)
    first = np.concatenate([rng.uniform(20.25, 65.0, 200), [20.25, 20.25, 64.0, 30.0]])
    m3 = np.concatenate([first[:200] + rng.uniform(1e-9, 3e4, 200), [20.75, 20.75 + 1e-12, 5e5, 3e6]])
    got = ta.widened(first, m3)
    for f, m, g in zip(first, m3, got):
        n = 1
        while not m <= f + 0.5 * n and f + 0.5 * n < ta.C2_LIMIT:
            n += 1
        assert g == f + 0.5 * n, (f, m)
    assert got[-1] >= ta.C2_LIMIT and got[-1] < ta.C2_LIMIT + 0.5 and got[-4] == 20.75 and got[-3] == 21.25


def test_scores_stay_in_range():
    rng = np.random.default_rng(7)
    for n1, n2 in ((30, 30), (24, 41), (50, 18)):
        got = ta.tm_align(_walk(rng, n1), _walk(rng, n2))
        for k in ("tm", "tm_a", "tm_b"):
            assert 0.0 < got[k] <= 1.0
        assert np.all(got["init_tm"][got["init_tm"] >= 0] <= 1.0 + 1e-12) and got["init_dp"].min() >= 0 and got["init_dp"].max() <= 60
        rows = got["alignment"][got["alignment"] >= 0]
        assert len(rows) == got["n_aligned"] and np.all(np.diff(rows) > 0) and rows.max() < n1


def test_statuses():
    rng = np.random.default_rng(8)
    y = _walk(rng, 12)
    short = ta.tm_align(y[:4], y)
    assert short["status"] == ta.TOO_SHORT and np.isnan(short["tm"]) and short["n_aligned"] == 0 and np.all(short["alignment"] == -1)
    assert ta.tm_align(y, y[:4])["status"] == ta.TOO_SHORT and ta.tm_align(y[:5], y[:5])["status"] == 0
    bad = y.copy()
    bad[3, 1] = np.inf
    assert ta.tm_align(bad, y)["status"] == ta.NOT_FINITE and np.isnan(ta.tm_align(y, bad)["tm"])
    k = np.arange(5.0)  # points 100 Angstrom apart against a chain: no three pairs fit within d8 under any transform
    far = ta.tm_align(y[:5], np.stack([np.zeros(5), 100.0 * k, 0.3 * k * k], axis=1))
    assert far["status"] == ta.NO_ALIGNMENT and np.isnan([far["tm"], far["tm_a"], far["tm_b"], far["rmsd"]]).all() and far["n_aligned"] < 3
    assert (far["alignment"] >= 0).sum() == far["n_aligned"] and far["best_init"] >= 0 and np.array_equal(far["rotation"], np.eye(3))
    assert (ta.TOO_SHORT, ta.SKIPPED, ta.NOT_FINITE, ta.NO_ALIGNMENT) == (_lib.TMA_TOO_SHORT, _lib.TMA_SKIPPED, _lib.TMA_NOT_FINITE, _lib.TMA_NO_ALIGNMENT)
    assert ta.MAX_ROWS == _lib.TMA_MAX_ROWS == tm_align.MAX_ROWS == 512


def test_masks_compact_the_structures_separately():
    fix = _fix()
    a, b, ma, mb = ta.case_inputs(fix, "masked")
    got = ta.align_structures(a, b, ma, mb)
    assert int(ma.sum()) == 69 and int(mb.sum()) == 75 and not np.array_equal(ma, mb)
    set_rows = got["alignment"] >= 0
    assert not set_rows[mb == 0].any() and (ma[got["alignment"][set_rows]] != 0).all()


SMALL = tuple(c for c in ta.CASES if c not in ("shift4_300", "n512"))


@pytest.mark.parametrize("name", SMALL)
def test_fixture_records_the_restatement(name):
    """The cases up to 130 rows: the fixture holds what the restatement computes today, bit for bit."""
    fix = _fix()
    got = ta.align_structures(*ta.case_inputs(fix, name))
    for k in ta.FLOAT_OUTPUTS + ("d0_a", "d0_b", "rotation", "translation") + ta.EXACT_OUTPUTS:
        assert np.array_equal(np.asarray(got[k]), fix[f"{name}.{k}"], equal_nan=True), k
    assert float(fix[f"{name}.tm.yard"]) <= 1e-9


def test_fixture_holds_the_named_cases():
    fix = _fix()
    assert tuple(fix["cases"]) == ta.CASES
    shape = {name: (len(fix[f"{name}.ca_a"]), len(fix[f"{name}.ca_b"])) for name in ta.CASES}
    assert shape["n5"] == (5, 5) and shape["n5x9"] == (5, 9) and shape["n19x22"] == (19, 22) and shape["n64x65"] == (64, 65) and shape["n61x80"] == (61, 80)
    assert shape["deletion"] == (80, 73) and shape["partial"] == (45, 64) and shape["shift4_300"] == (300, 300) and shape["n512"] == (512, 512)
    assert float(fix["n19x22.d0_a"]) == 0.5 and float(fix["n19x22.d0_b"]) > 0.5
    assert float(fix["shift6.tm"]) >= 74 / 80 - 1e-9 and float(fix["shift4_300.tm"]) >= 296 / 300 - 1e-9 and abs(float(fix["copy80.tm"]) - 1) <= 1e-12
    assert float(fix["deletion.tm_b"]) >= 1 - 1e-9 and float(fix["deletion.tm_a"]) >= 73 / 80 - 1e-9
    for name in ("tcr80", "tcr130"):
        assert fix[f"{name}.init_tm"][1] > 0
        for side in ("ca_a", "ca_b"):
            assert set("HE") & set(ta.sec_string(fix[f"{name}.{side}"].astype(np.float64)))
    assert int(fix["far.status"]) == ta.NO_ALIGNMENT and np.isnan(fix["far.tm"]) and int(fix["far.n_aligned"]) < 3
    assert fix["all8.ca"].shape == (8, 40, 3) and fix["all8.tm"].shape == (28,) and fix["all8.alignment"].shape == (28, 40)
    for key in fix:
        assert fix[key].dtype != object and (not key.endswith((".ca_a", ".ca_b", ".ca")) or fix[key].dtype == np.float32)


def test_struct_layout_matches_the_host_compiler(tmp_path):
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host C compiler")
    cls = _lib.TmAlignArgs
    lines = ["#include <stdio.h>", '#include "fdipt.h"', "int main(void) {", '  printf("size %zu\\n", sizeof(FdiptTmAlignArgs));']
    lines += [f'  printf("{m} %zu\\n", offsetof(FdiptTmAlignArgs, {m}));' for m, _ in cls._fields_]
    lines += ['  printf("FDIPT_TMA_MAX_ROWS %d\\n", FDIPT_TMA_MAX_ROWS);', "  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert got == {"size": C.sizeof(cls), **{m: getattr(cls, m).offset for m, _ in cls._fields_}, "FDIPT_TMA_MAX_ROWS": 512}
    members = [m for m, _ in cls._fields_]
    assert members[:8] == ["S", "N_a", "atoms", "ca", "S_b", "N_b", "atoms_b", "P"] and set(tm_align.OUTPUTS) <= set(members)
    assert _lib.SIGNATURES["fdipt_sample_tm_align_workspace"][1] == [C.c_int] * 4


def test_writers_of_run_sharded(tmp_path):
    """``--tm-align``: the larger of the searched and the fixed score is written and clustered, the entries the fixed score won are
    counted, a NaN on one side gives way to the other side and a pair without either score stops the clustering of its length; the
    inpainting table holds the matrix per structure and the structures that were skipped."""
    nan = np.nan
    aligned = np.array([[1.0, 0.9, 0.2], [0.9, 1.0, nan], [0.2, nan, 1.0]])
    fixed = np.array([[1.0, 0.4, 0.25], [0.4, 1.0, 0.3], [0.25, 0.3, 1.0]])
    holes = np.array([[1.0, nan], [nan, 1.0]])
    done = run_sharded.write_diversity_aligned(str(tmp_path), {24: aligned, 16: np.ones((1, 1)), 30: holes}, {24: fixed, 16: np.ones((1, 1)), 30: holes},
                                               tm_score_th=0.5, skipped=[600])
    assert [e["length"] for e in done["lengths"]] == [16, 24, 30] and done["skipped_lengths"] == [600]
    e = done["lengths"][1]
    assert (e["samples"], e["clusters"], e["fixed_won"], e["nan_pairs"], e["pairs"]) == (3, 2, 2, 0, 3) and e["diversity"] == 2 / 3 and e["labels"] == [1, 1, 2]
    written = np.load(tmp_path / "pairwise_tm_score_aligned_length_24.npy")
    assert np.array_equal(written, [[1.0, 0.9, 0.25], [0.9, 1.0, 0.3], [0.25, 0.3, 1.0]])
    e = done["lengths"][2]
    assert (e["samples"], e["clusters"], e["diversity"], e["labels"], e["fixed_won"], e["nan_pairs"]) == (2, None, None, None, 0, 1)
    assert json.load(open(tmp_path / "diversity_aligned.json")) == done
    rows = list(csv.DictReader(open(tmp_path / "diversity_aligned.csv")))
    assert [r["length"] for r in rows] == ["16", "24", "30"] and rows[1]["clusters"] == "2" and rows[1]["fixed_won"] == "2" and float(rows[1]["diversity"]) == 2 / 3
    assert (rows[2]["clusters"], rows[2]["diversity"], rows[2]["nan_pairs"]) == ("", "", "1")
    assert not (tmp_path / "pairwise_tm_score_length_24.npy").exists() and not (tmp_path / "diversity.json").exists()
    table = run_sharded.write_tm_align_table(str(tmp_path), {"1abc": {"samples": ["0", "1"], "rows": 40, "matrix": np.array([[1.0, nan], [nan, 1.0]])}},
                                             {"2xyz": 530})
    assert table["structures"]["1abc"] == {"samples": ["0", "1"], "rows": 40, "matrix": [[1.0, None], [None, 1.0]]}
    assert table["skipped_structures"] == {"2xyz": 530}
    assert json.load(open(tmp_path / "tm_align.json")) == table


def test_compact_rows_brings_a_large_complex_under_the_row_limit():
    """Three samples of a 724-row complex with 40, 38 and 0 diffused rows: the rows go to the front in order, 40 rows remain (the search
    limits the rows of the arrays it is given, not the rows it uses), and the restatement aligns the compacted pair as it does the
    whole structures under their masks."""
    rng = np.random.default_rng(10)
    ca = _walk(rng, 724).astype(np.float32)
    prot = np.stack([ta.five_atoms(ca + rng.normal(size=ca.shape).astype(np.float32) * 0.4) for _ in range(3)])
    mask = np.zeros((3, 724), dtype=np.float32)
    mask[0, 570:610], mask[1, 571:609] = 1, 1
    rows, rows_mask = run_sharded.compact_rows(prot, mask)
    assert rows.shape == (3, 40, 5, 3) and rows.dtype == np.float32 and rows.shape[1] <= tm_align.MAX_ROWS < prot.shape[1]
    assert rows_mask.sum(1).tolist() == [40, 38, 0] and rows_mask[1, :38].all()
    assert np.array_equal(rows[0], prot[0, 570:610]) and np.array_equal(rows[1, :38], prot[1, 571:609]) and not rows[1, 38:].any()
    whole, packed = ta.align_structures(prot[0], prot[1], mask[0], mask[1]), ta.align_structures(rows[0], rows[1], rows_mask[0], rows_mask[1])
    for k in ("tm", "tm_a", "tm_b", "rmsd", "n_aligned", "init_dp", "best_init"):
        assert np.array_equal(whole[k], packed[k]), k
    assert np.array_equal(whole["alignment"][571:609], np.where(packed["alignment"][:38] >= 0, packed["alignment"][:38] + 570, -1))
    empty, empty_mask = run_sharded.compact_rows(prot[:1], np.zeros((1, 724)))
    assert empty.shape == (1, 1, 5, 3) and not empty_mask.any()
