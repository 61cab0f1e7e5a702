"""CPU tests of the sequence-alignment contract: the NumPy restatement (tests/seqalign_ref.py) against a
brute-force enumeration and closed forms, the tie rule on planted ties, the hand-entered BLOSUM62 table, the host part of
``seq_align.chain_row_map`` and the argument errors ``align_sequences`` raises before torch or the library is touched."""
import sys

import numpy as np
import pytest

import seqalign_ref as ref
from framedipt_amd import _lib, row_map, seq_align

B62, IDENT = 2 * seq_align.BLOSUM62.astype(np.int64), 2 * seq_align.IDENTITY.astype(np.int64)
M, X, Y = 0, 1, 2


@pytest.mark.parametrize("table", [B62, IDENT], ids=["blosum62", "identity"])
@pytest.mark.parametrize("o,e", [(-20, -1), (-2, -2)], ids=["-10/-0.5", "-1/-1"])
def test_score_equals_the_enumeration_of_all_alignments(table, o, e):
    """(a) 300 random pairs of lengths 1 .. 6 (letters 0 .. 20, a small alphabet in every third pair so that matches occur): the
    restatement's score is the maximum over every alignment, and its own path scores that by the definition."""
    rng = np.random.default_rng(62)
    for k in range(300):
        la, lb = rng.integers(1, 7, 2)
        letters = 3 if k % 3 == 0 else 21
        a, b = rng.integers(0, letters, la), rng.integers(0, letters, lb)
        got = ref.align(a, b, table, o, e)
        assert got["score_half"] == ref.brute_force_score(a, b, table, o, e), (a, b)
        assert ref.path_score(a, b, got["path"], table, o, e) == got["score_half"]
        assert got["n_aligned"] + got["n_gaps_b"] == la and got["n_aligned"] + got["n_gaps_a"] == lb


def test_vectorised_fill_equals_the_triple_loop():
    """The anti-diagonal fill against the plain loops up to 64 rows: the path (so the tie rule), the map and every count."""
    rng = np.random.default_rng(5)
    for la, lb, letters, (o, e) in [(1, 1, 21, (-20, -1)), (1, 9, 4, (-2, -2)), (9, 1, 4, (-2, -2)), (17, 23, 2, (-2, -2)), (23, 17, 3, (0, -2)),
                                    (40, 35, 21, (-20, -1)), (64, 64, 4, (-4, -1)), (64, 50, 21, (-2, 0))]:
        a, b = rng.integers(0, letters, la), rng.integers(0, letters, lb)
        for table in (B62, IDENT):
            fast, slow = ref.align(a, b, table, o, e), ref.align_loops(a, b, table, o, e)
            assert fast["path"] == slow["path"] and np.array_equal(fast["alignment"], slow["alignment"])
            assert {k: v for k, v in fast.items() if k not in ("path", "alignment")} == {k: v for k, v in slow.items() if k not in ("path", "alignment")}


def test_closed_forms():
    """(b) A sequence against itself scores the sum of its diagonal entries with the identity map; a 40-letter sequence against itself
    without rows 15 .. 19 scores sum diag(b) - 10 - 4 * 0.5 with the known map (a[15] != a[20] and a[14] != a[19]: no other placement of
    the gap scores as much, whatever the tie rule)."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 20, 40)
    a[15], a[20], a[14], a[19] = 0, 1, 2, 3
    same = ref.align(a, a, B62, -20, -1)
    assert same["score_half"] == B62[a, a].sum() and np.array_equal(same["alignment"], np.arange(40)) and same["path"] == [M] * 40
    assert (same["n_identical"], same["n_gap_runs"]) == (40, 0)
    b = np.delete(a, np.arange(15, 20))
    cut = ref.align(a, b, B62, -20, -1)
    assert cut["score"] == B62[b, b].sum() / 2 - 10 - 4 * 0.5
    assert np.array_equal(cut["alignment"], np.delete(np.arange(40), np.arange(15, 20)))
    assert (cut["n_aligned"], cut["n_identical"], cut["n_gaps_a"], cut["n_gaps_b"], cut["n_gap_runs"]) == (35, 35, 0, 5, 1)
    back = ref.align(b, a, B62, -20, -1)  # the gap on the other side
    assert back["score_half"] == cut["score_half"] and (back["n_gaps_a"], back["n_gaps_b"]) == (5, 0)
    assert np.array_equal(back["alignment"], row_map.invert(cut["alignment"], 40))


def test_tie_rule_on_planted_ties():
    """(c) With equal open and extend every placement of a gap in a run of equal letters scores the same: the first of M, X, Y wins in
    every maximum, which is decided walking BACK from the end - so matches are taken at the end and the gap lands at the start."""
    A, R = 0, 1
    r = ref.align([A, A, A, A], [A, A], IDENT, -2, -2)  # AAAA / --AA
    assert r["score"] == 2 - 2 and r["path"] == [X, X, M, M] and r["alignment"].tolist() == [2, 3] and r["n_gap_runs"] == 1
    r = ref.align([A, A], [A, A, A, A], IDENT, -2, -2)
    assert r["path"] == [Y, Y, M, M] and r["alignment"].tolist() == [-1, -1, 0, 1]
    r = ref.align([A, R, A], [A, A], IDENT, -2, -2)     # ARA / A-A (score 1) beats every other alignment: no tie here
    assert r["score"] == 1 and r["path"] == [M, X, M] and r["alignment"].tolist() == [0, 2]
    r = ref.align([A, R, A], [A, A], B62, -8, -8)       # 4 + 4 - 4 = 4 against ARA / -AA = -4 - 1 + 4: still A-A
    assert r["path"] == [M, X, M]
    # a mismatch or two gaps, both -2 in whole units under -1 / -1: M is first
    r = ref.align([A], [R], IDENT, -2, -2)
    assert r["score"] == -1 and r["path"] == [M]
    r = ref.align([A], [R], IDENT, -1, -1)              # -1 (mismatch) against -0.5 - 0.5 (two gaps): equal; M wins
    assert r["score"] == -1 and r["path"] == [M]
    r = ref.align([A], [R], IDENT, 0, 0)                # free gaps: X at the end cell is first of the two gap states
    assert r["score"] == 0 and r["path"] == [Y, X] and r["n_gap_runs"] == 2 and r["alignment"].tolist() == [-1]


def test_blosum62_invariants():
    """(d) The table was entered by hand: symmetric, trace 116, sum -426, the row sums, the extremes, and the X row."""
    t = seq_align.BLOSUM62
    assert t.shape == (21, 21) and t.dtype == np.int32 and np.array_equal(t, t.T)
    b = t[:20, :20]
    assert np.trace(b) == 116 and b.sum() == -426 and (b.min(), b.max()) == (-4, 11)
    assert b.sum(axis=1).tolist() == [-16, -21, -18, -26, -31, -12, -17, -34, -17, -27, -25, -17, -13, -25, -32, -11, -14, -32, -16, -22]
    order = "ARNDCQEGHILKMFPSTWYV"
    assert seq_align.LETTERS == order + "X" and seq_align.X == 20
    assert [t[20, order.index(c)] for c in "AST"] == [0, 0, 0] and [t[20, order.index(c)] for c in "CPW"] == [-2, -2, -2]
    assert (t[20] == -1).sum() == 21 - 6 and t[20, 20] == -1
    assert (b[order.index("W"), order.index("W")], b[order.index("C"), order.index("C")], b[order.index("I"), order.index("V")]) == (11, 9, 3)
    i = seq_align.IDENTITY
    assert np.array_equal(np.diag(i), [1] * 20 + [-1]) and (i - np.diag(np.diag(i)) == -1 + np.eye(21)).all()
    assert np.array_equal(seq_align.table_half_units("blosum62"), 2 * t) and np.array_equal(seq_align.table_half_units(t), 2 * t)
    assert seq_align.encode("ARNDCQEGHILKMFPSTWYVXBZ-a").tolist() == list(range(21)) + [20, 20, 20, 0]


def test_chain_maps_on_the_host():
    """(e) The host part of ``chain_row_map``: chains as runs of one label, pairing by label or by list, per-chain maps offset into whole
    rows, an unpaired chain left at -1, a returning label refused; the maps pass ``row_map.validate`` and ``invert`` round-trips them."""
    rng = np.random.default_rng(8)
    chain_a = np.array(["A"] * 12 + ["B"] * 9 + ["C"] * 5)
    chain_b = np.array(["B"] * 7 + ["D"] * 4 + ["A"] * 12)
    a, b = rng.integers(0, 20, 26), np.zeros(23, dtype=np.int64)
    b[:7], b[11:] = np.delete(a[12:21], [3, 4]), a[:12]
    plan = seq_align.plan_chains(chain_a, 26, chain_b, 23)
    assert plan == [("B", "B", (12, 21), (0, 7)), ("A", "A", (0, 12), (11, 23))]
    per_chain = [ref.align(a[s:e], b[u:v], B62, -20, -1)["alignment"] for _, _, (s, e), (u, v) in plan]
    padded = [np.concatenate([m, np.full(12 - len(m), -1)]) for m in per_chain]  # as the device pads to the launch's N_b
    m = seq_align.assemble_map(plan, padded, 23)
    want = np.concatenate([np.delete(np.arange(12, 21), [3, 4]), [-1] * 4, np.arange(12)])
    assert np.array_equal(m, want) and m.dtype == np.int32
    assert np.array_equal(row_map.validate(m, 26), m) and np.array_equal(row_map.invert(row_map.invert(m, 26), 23), m)
    listed = seq_align.plan_chains(chain_a, 26, chain_b, 23, chain_pairs=[("C", "D")])
    assert listed == [("C", "D", (21, 26), (7, 11))]
    assert seq_align.plan_chains(None, 26, None, 23) == [(None, None, (0, 26), (0, 23))]
    assert seq_align.chain_runs("H", 5) == [("H", 0, 5)]
    with pytest.raises(ValueError, match="returns at row 3"):
        seq_align.chain_runs(np.array([1, 1, 2, 1]), 4)
    with pytest.raises(ValueError, match="4 rows"):
        seq_align.chain_runs(np.array([1, 1, 2]), 4)
    for bad in ([("A", "Z")], [("A", "A"), ("A", "B")]):
        with pytest.raises(ValueError, match="chain_pairs"):
            seq_align.plan_chains(chain_a, 26, chain_b, 23, chain_pairs=bad)


def test_argument_errors_need_neither_torch_nor_the_library(monkeypatch):
    """(f) Every shape and argument error is raised before torch is imported or the library loaded."""
    monkeypatch.setitem(sys.modules, "torch", None)  # an import of torch would raise ImportError
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    seqs = np.zeros((2, 5), dtype=np.int64)
    cases = [(dict(open_gap=-0.3), "open_gap"), (dict(extend_gap=0.5), "extend_gap"), (dict(open_gap=-5000.0), "open_gap"),
             (dict(matrix=np.zeros((20, 20), dtype=np.int64)), r"\[21, 21\]"), (dict(matrix=np.zeros((21, 21))), "integers"),
             (dict(matrix="pam250"), "matrix"), (dict(len_a=[5, 6]), "padded width"), (dict(len_a=[5]), "lengths"),
             (dict(len_b=[1, 1]), "len_b without seq_b"), (dict(pairs=[[0, 2]]), "pairs"), (dict(max_workspace_bytes=-1), "max_workspace_bytes")]
    for kwargs, match in cases:
        with pytest.raises(ValueError, match=match):
            seq_align.align_sequences(seqs, **kwargs)
    with pytest.raises(ValueError, match="letter outside"):
        seq_align.align_sequences(np.array([[0, 21, 3]]), np.array([[1, 2, 3]]))
    with pytest.raises(ValueError, match="integer"):
        seq_align.align_sequences(np.zeros((2, 5)))
    with pytest.raises(ValueError, match="ragged"):
        seq_align.align_sequences(["ARN", "AR"], len_a=[3, 2])
    # a bad letter beyond a sequence's length is padding, not an error: the call gets as far as the device
    with pytest.raises(ImportError):
        seq_align.align_sequences(np.array([[0, 1, 99]]), np.array([[0, 1, 2]]), len_a=[2])
    assert (_lib.SEQ_EMPTY, _lib.SEQ_BAD_LETTER, _lib.SEQ_SKIPPED, _lib.SEQ_MAX_ROWS) == (1, 2, 4, 2048)
    assert {"fdipt_seq_align", "fdipt_seq_align_workspace_bytes"} <= set(_lib.SIGNATURES)
