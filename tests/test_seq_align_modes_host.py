"""CPU tests of the local and semi-global modes of sequence alignment: the NumPy restatement
(tests/seqalign_modes_ref.py) against an enumeration by the definitions and against closed forms, ``free_ends`` parsing, the host side of
``seq_align.chain_row_map(exclude_a=, exclude_b=)`` with a stub in place of the device call, and the ABI."""
import sys

import numpy as np
import pytest

import seqalign_modes_ref as mr
import seqalign_ref as ref
from framedipt_amd import _lib, seq_align

B62, IDENT = 2 * seq_align.BLOSUM62.astype(np.int64), 2 * seq_align.IDENTITY.astype(np.int64)
M, X, Y = 0, 1, 2
PENALTIES = [(-4, -1), (-2, -2), (0, 0), (-6, 0), (-1, -3)]
# the package's constants drive the restatement: its modes and bits are the ABI's
MODES = [(seq_align.MODES["semiglobal"], f) for f in range(16)] + [(seq_align.MODES["local"], 0)]
BITS = {k: seq_align.free_end_bits("semiglobal", k) for k in ("a", "b", "all")}


def _span(r, a, b):
    return a[r["begin_a"]:r["end_a"]], b[r["begin_b"]:r["end_b"]]


@pytest.mark.parametrize("o,e", PENALTIES, ids=[f"{o}/{e}" for o, e in PENALTIES])
def test_restatement_equals_the_enumeration(o, e):
    """(1, 2, 3) 12 random pairs of lengths 1 .. 5 over three letters for each of the sixteen flag sets and local, under five penalty
    pairs (1 020 cases): the recurrence's score is the enumeration's, the charged path re-scored by the global rule over its span is
    the score, the counts are the span's, and without a flag the path is ``seqalign_ref.align``'s."""
    rng = np.random.default_rng(100 - o * 10 - e)
    for mode, free in MODES:
        for _ in range(12):
            la, lb = rng.integers(1, 6, 2)
            a, b = rng.integers(0, 3, la), rng.integers(0, 3, lb)
            got = mr.align(a, b, IDENT, o, e, mode, free)
            assert got["score_half"] == mr.brute_force_score(a, b, IDENT, o, e, mode, free), (a, b, mode, free)
            sa, sb = _span(got, a, b)
            assert mr.path_score(sa, sb, got["path"], IDENT, o, e) == got["score_half"], (a, b, mode, free)
            assert got["n_aligned"] + got["n_gaps_b"] == len(sa) and got["n_aligned"] + got["n_gaps_a"] == len(sb)
            assert (got["status"] == mr.NO_ALIGNED) == (got["n_aligned"] == 0)
            outside = np.r_[got["alignment"][:got["begin_b"]], got["alignment"][got["end_b"]:]]
            assert (outside == -1).all() and (got["alignment"] >= 0).sum() == got["n_aligned"]
            if mode == mr.LOCAL and got["path"]:
                assert got["path"][0] == M and got["path"][-1] == M and got["score_half"] > 0
            if free == 0 and mode == mr.SEMIGLOBAL:
                want = ref.align(a, b, IDENT, o, e)
                assert got["path"] == want["path"] and got["score_half"] == want["score_half"] and np.array_equal(got["alignment"], want["alignment"])
                assert (got["begin_a"], got["end_a"], got["begin_b"], got["end_b"]) == (0, la, 0, lb)
                assert mr.align(a, b, IDENT, o, e, mr.GLOBAL)["path"] == want["path"]


def test_vectorised_fill_equals_the_loops():
    """The anti-diagonal fill against the plain loops up to 64 rows, in every output."""
    rng = np.random.default_rng(6)
    for la, lb, letters, (o, e) in [(1, 1, 21, (-20, -1)), (1, 9, 4, (-2, -2)), (9, 1, 4, (-2, -2)), (17, 23, 2, (-2, -2)), (23, 17, 3, (0, -2)),
                                    (40, 35, 21, (-20, -1)), (64, 50, 4, (-4, -1))]:
        a, b = rng.integers(0, letters, la), rng.integers(0, letters, lb)
        for table in (B62, IDENT):
            for mode, free in [(mr.LOCAL, 0)] + [(mr.SEMIGLOBAL, f) for f in (0, 1, 8, 3, 12, 15, 6)]:
                fast, slow = mr.align(a, b, table, o, e, mode, free), mr.align_loops(a, b, table, o, e, mode, free)
                assert fast["path"] == slow["path"] and np.array_equal(fast["alignment"], slow["alignment"])
                skip = ("path", "alignment")
                assert {k: v for k, v in fast.items() if k not in skip} == {k: v for k, v in slow.items() if k not in skip}


def test_a_word_inside_unrelated_letters():
    """(4) A 7-letter word inside 20 unrelated letters: under local and under free_ends "a" the span is the word, with identity 1."""
    word = seq_align.encode("WCHMFYW")
    a = np.concatenate([seq_align.encode("AGSTAGSTAGST"), word, seq_align.encode("GASTGAST")])
    for mode, free in ((mr.LOCAL, 0), (mr.SEMIGLOBAL, BITS["a"])):
        r = mr.align(a, word, B62, -20, -1, mode, free)
        assert (r["begin_a"], r["end_a"], r["begin_b"], r["end_b"]) == (12, 19, 0, 7) and r["path"] == [M] * 7
        assert r["n_identical"] == r["n_aligned"] == 7 and r["score_half"] == B62[word, word].sum() and r["status"] == 0
        assert r["alignment"].tolist() == list(range(12, 19)) and r["n_gap_runs"] == r["n_gaps_a"] == r["n_gaps_b"] == 0
    glob = mr.align(a, word, B62, -20, -1, mr.GLOBAL)  # the same word, and both tails charged
    assert glob["score_half"] == B62[word, word].sum() + (-20 - 11) + (-20 - 7) and glob["n_gap_runs"] == 2


def test_overlap_of_a_suffix_and_a_prefix():
    """(4) Two sequences that overlap by a suffix of a and a prefix of b, under "all": the span is the overlap, the overhangs are free."""
    shared = seq_align.encode("WCHMFYWKDE")
    a = np.concatenate([seq_align.encode("AGSTAGSTAG"), shared])
    b = np.concatenate([shared, seq_align.encode("PLVPLVPL")])
    r = mr.align(a, b, B62, -20, -1, mr.SEMIGLOBAL, BITS["all"])
    assert (r["begin_a"], r["end_a"], r["begin_b"], r["end_b"]) == (10, 20, 0, 10) and r["path"] == [M] * 10
    assert r["score_half"] == B62[shared, shared].sum() and r["alignment"].tolist() == list(range(10, 20)) + [-1] * 8
    assert (r["n_gaps_a"], r["n_gaps_b"], r["n_gap_runs"]) == (0, 0, 0)
    back = mr.align(b, a, B62, -20, -1, mr.SEMIGLOBAL, BITS["all"])  # a prefix of the first against a suffix of the second
    assert (back["begin_a"], back["end_a"], back["begin_b"], back["end_b"]) == (0, 10, 10, 20)
    assert back["alignment"].tolist() == [-1] * 10 + list(range(10))


def test_no_aligned_column():
    """(4) All-X input has no positive cell: the empty local result; under "all" the best is a pair of free runs, score 0, no column; a
    length of 0 stays EMPTY."""
    x = np.full(5, 20)
    r = mr.align(x, x[:3], B62, -20, -1, mr.LOCAL)
    assert r["status"] == mr.NO_ALIGNED and r["score_half"] == 0 and r["path"] == [] and (r["alignment"] == -1).all()
    assert (r["begin_a"], r["end_a"], r["begin_b"], r["end_b"]) == (0, 0, 0, 0)
    r = mr.align(x, x[:3], B62, -20, -1, mr.SEMIGLOBAL, 15)
    assert r["status"] == mr.NO_ALIGNED and r["score_half"] == 0 and r["n_aligned"] == 0 and r["path"] == []
    assert (r["end_a"] - r["begin_a"], r["end_b"] - r["begin_b"]) == (0, 0)
    for mode in (mr.LOCAL, mr.SEMIGLOBAL):
        r = mr.align(x, [], B62, -20, -1, mode)
        assert r["status"] == mr.EMPTY and r["score_half"] == 0


def test_two_equal_motifs_the_earlier_diagonal_wins():
    """(4) The word twice in a: local ends at the smallest i + j among equal scores, so the first copy is taken; the semi-global key runs
    the other way (i + j descending) and takes the last."""
    word = seq_align.encode("WCHMFYW")
    a = np.concatenate([seq_align.encode("AGST"), word, seq_align.encode("GASTGA"), word, seq_align.encode("ST")])
    r = mr.align(a, word, B62, -20, -1, mr.LOCAL)
    assert (r["begin_a"], r["end_a"]) == (4, 11) and r["alignment"].tolist() == list(range(4, 11))
    r = mr.align(a, word, B62, -20, -1, mr.SEMIGLOBAL, BITS["a"])
    assert (r["begin_a"], r["end_a"]) == (17, 24) and r["alignment"].tolist() == list(range(17, 24))
    # equal i + j: the word at b's start against a's end and the reverse - the smaller i wins
    r = mr.align(np.concatenate([word, [0, 0, 0], [5, 5, 5, 5]]), np.concatenate([[7, 7, 7, 7], [1, 1, 1], word]), B62, -20, -1, mr.LOCAL)
    assert (r["begin_a"], r["end_a"], r["begin_b"], r["end_b"]) == (0, 7, 7, 14)


def test_free_ends_parsing_and_refusals(monkeypatch):
    """(5) Names, shorthands and the default; an unknown mode or name and ``free_ends`` with another mode are refused before torch or the
    library is touched."""
    monkeypatch.setitem(sys.modules, "torch", None)
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    bits = seq_align.free_end_bits
    assert seq_align.FREE_ENDS == {"a_left": 1, "a_right": 2, "b_left": 4, "b_right": 8}
    assert seq_align.MODES == {"global": 0, "semiglobal": 1, "local": 2} and seq_align.NO_ALIGNED == 8
    assert bits("semiglobal", None) == 15 == bits("semiglobal", "all") and bits("semiglobal", "a") == 3 and bits("semiglobal", "b") == 12
    assert bits("semiglobal", ["a_left", "b_right"]) == 9 and bits("semiglobal", ("b_left",)) == 4 and bits("semiglobal", "a_right") == 2
    assert bits("semiglobal", []) == 0 and bits("global", None) == 0 == bits("local", None)
    seqs = np.zeros((2, 5), dtype=np.int64)
    for kwargs, match in [(dict(mode="overlap"), "mode"), (dict(mode=1), "mode"), (dict(mode="local", free_ends="a"), "free_ends"),
                          (dict(free_ends="all"), "free_ends"), (dict(mode="semiglobal", free_ends="left"), "free_ends"),
                          (dict(mode="semiglobal", free_ends=["a_left", 3]), "free_ends"), (dict(mode="semiglobal", open_gap=-0.3), "open_gap")]:
        with pytest.raises(ValueError, match=match):
            seq_align.align_sequences(seqs, **kwargs)
    with pytest.raises(ValueError, match="free_ends"):
        seq_align.chain_row_map("ARN", None, "ARN", None, free_ends="a")
    with pytest.raises(ImportError):  # a good call gets as far as the device
        seq_align.align_sequences(seqs, mode="local")


def _stub(monkeypatch, table=B62, o=-20, e=-1):
    """``align_sequences`` of ragged lists answered by the restatement: the keys ``chain_row_map`` reads."""
    def align_sequences(seqs_a, seqs_b, traceback=True, mode="global", free_ends=None, **_):
        free = seq_align.free_end_bits(mode, free_ends)
        n_b = max(len(s) for s in seqs_b)
        rows = [mr.align(sa, sb, table, o, e, seq_align.MODES[mode], free) for sa, sb in zip(seqs_a, seqs_b)]
        out = {k: np.array([r[k] for r in rows]) for k in mr.KEYS}
        out["score"] = out.pop("score_half") / 2.0
        out["alignment"] = np.stack([np.concatenate([r["alignment"], np.full(n_b - len(r["alignment"]), -1)]) for r in rows])
        la, lb = np.array([len(s) for s in seqs_a]), np.array([len(s) for s in seqs_b])
        out.update(seq_align.identities(out["n_identical"], out["n_aligned"], la, lb))
        out["identity_span_b"] = out["n_identical"] / np.maximum(out["end_b"] - out["begin_b"], 1)
        out["coverage_b"] = (out["end_b"] - out["begin_b"]) / lb
        return out

    monkeypatch.setattr(seq_align, "align_sequences", align_sequences)


def test_exclude_regions_on_hand_cases(monkeypatch):
    """(6) ``exclude_a`` / ``exclude_b``: an aligned column whose row of a lies inside the region leaves the map, its row of b has to lie
    inside b's region (ValueError otherwise; the converse is not checked), the counts stay those of the alignment, ``n_excluded`` counts
    the dropped columns; and the modes reach the per-chain call."""
    _stub(monkeypatch)
    rng = np.random.default_rng(9)
    a = rng.integers(0, 20, 30)
    chain = np.array(["H"] * 18 + ["L"] * 12)
    plain = seq_align.chain_row_map(a, chain, a, chain)
    assert np.array_equal(plain["alignment"], np.arange(30)) and plain["n_excluded"].tolist() == [0, 0]
    got = seq_align.chain_row_map(a, chain, a, chain, exclude_a=[(4, 8), None], exclude_b=[(4, 8), None])
    want = np.arange(30)
    want[4:9] = -1
    assert np.array_equal(got["alignment"], want) and got["alignment"].dtype == np.int32
    assert got["n_excluded"].tolist() == [5, 0] and got["n_aligned"].tolist() == [18, 12] and got["identity"].tolist() == [1.0, 1.0]
    got = seq_align.chain_row_map(a, chain, a, chain, exclude_a=[None, (0, 2)], exclude_b=[(0, 99), (0, 3)])  # (b's region may be wider)
    want = np.arange(30)
    want[18:21] = -1
    assert np.array_equal(got["alignment"], want) and got["n_excluded"].tolist() == [0, 3]
    with pytest.raises(ValueError, match="same excluded region"):
        seq_align.chain_row_map(a, chain, a, chain, exclude_a=[(4, 8), None], exclude_b=[(5, 8), None])
    with pytest.raises(ValueError, match="same excluded region"):
        seq_align.chain_row_map(a, chain, a, chain, exclude_a=[(4, 8), None])
    for bad in ([(4, 8)], [(4, 8, 9), None]):
        with pytest.raises(ValueError, match="exclude_a"):
            seq_align.chain_row_map(a, chain, a, chain, exclude_a=bad)
    # the regions are chain-relative rows of each side: b lacks 3 leading rows of H, its region is shifted by 3
    b, chain_b = a[3:], chain[3:]
    got = seq_align.chain_row_map(a, chain, b, chain_b, mode="semiglobal", free_ends="a", exclude_a=[(6, 7), None], exclude_b=[(3, 4), None])
    want = np.arange(3, 30)
    want[3:5] = -1
    assert np.array_equal(got["alignment"], want) and got["begin_a"].tolist() == [3, 0] and got["end_a"].tolist() == [18, 12]
    assert got["n_excluded"].tolist() == [2, 0] and got["coverage_b"].tolist() == [1.0, 1.0] and got["identity_span_b"].tolist() == [1.0, 1.0]
    # a chain pair without an aligned column leaves its rows at -1
    lone = seq_align.chain_row_map(np.r_[a[:18], np.full(12, 20)], chain, np.r_[a[:18], np.full(12, 20)], chain, mode="local")
    assert lone["status"].tolist() == [0, seq_align.NO_ALIGNED] and np.array_equal(lone["alignment"], np.r_[np.arange(18), np.full(12, -1)])


def test_the_abi_declares_the_mode_entry():
    """(7) Both new symbols and the struct are read from the header; the struct repeats the global one field by field."""
    assert {"fdipt_seq_align_modes", "fdipt_seq_align_modes_workspace_bytes"} <= set(_lib.SIGNATURES)
    assert _lib.SIGNATURES["fdipt_seq_align_modes_workspace_bytes"] == _lib.SIGNATURES["fdipt_seq_align_workspace_bytes"]
    old, new = dict(_lib.SeqAlignArgs._fields_), dict(_lib.SeqAlignModeArgs._fields_)
    assert set(new) - set(old) == {"mode", "free_ends", "begin_a", "end_a", "begin_b", "end_b"} and all(new[k] is old[k] for k in old)
    assert (_lib.SEQ_MODE_GLOBAL, _lib.SEQ_MODE_SEMIGLOBAL, _lib.SEQ_MODE_LOCAL, _lib.SEQ_NO_ALIGNED) == (0, 1, 2, 8)
    assert (_lib.SEQ_FREE_A_LEFT, _lib.SEQ_FREE_A_RIGHT, _lib.SEQ_FREE_B_LEFT, _lib.SEQ_FREE_B_RIGHT) == (1, 2, 4, 8)
    assert "Fdipt" in _lib.SeqAlignModeArgs.__doc__
