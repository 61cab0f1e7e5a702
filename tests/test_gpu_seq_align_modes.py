"""GPU tests (-m gpu) of the local and semi-global modes of sequence alignment: ``seq_align.align_sequences(mode=,
free_ends=)`` (fdipt_seq_align_modes, csrc/seqalign_modes.hip) against the NumPy restatement (tests/seqalign_modes_ref.py) in every
output - all integers, so equality is ``np.array_equal`` -, the score-only launch against the traceback launch, the C entry's own
refusals, then the callers: ``seq_align.chain_row_map``, ``compare.sequence_aligned_accuracy`` and ``run_sharded.run_seq_diversity``."""
import json

import numpy as np
import pytest
import torch

import seqalign_modes_ref as mr
import tm_ref as tr
from framedipt_amd import _call, _lib, compare, run_sharded, seq_align

pytestmark = pytest.mark.gpu

INTS = ("n_aligned", "n_identical", "n_gaps_a", "n_gaps_b", "n_gap_runs", "begin_a", "end_a", "begin_b", "end_b", "status")
SCORINGS = {"blosum62": ("blosum62", -10.0, -0.5), "ties": ("identity", -1.0, -1.0)}
# (mode, free_ends as the Python entry takes them, the restatement's bits)
FLAGS = {"local": ("local", None, 0), "none": ("semiglobal", [], 0), "a_left": ("semiglobal", ["a_left"], 1), "b_right": ("semiglobal", ("b_right",), 8),
         "a": ("semiglobal", "a", 3), "b": ("semiglobal", "b", 12), "all": ("semiglobal", "all", 15)}
enc = seq_align.encode


def _half(matrix, o, e):
    return seq_align.table_half_units(matrix).astype(np.int64), int(2 * o), int(2 * e)


def _equal(got, want, keys=("score", "alignment") + INTS):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


def _check(seqs_a, seqs_b, pairs, flags, scoring="blosum62", **kw):
    """One launch with the traceback over ragged lists against the restatement in every output, then the score-only launch against it."""
    matrix, o, e = SCORINGS[scoring]
    mode, free_ends, bits = FLAGS[flags]
    call = dict(pairs=pairs, matrix=matrix, open_gap=o, extend_gap=e, mode=mode, free_ends=free_ends, **kw)
    got = seq_align.align_sequences(seqs_a, seqs_b, **call)
    n_b = max(max(len(s) for s in seqs_b), 1)
    want = mr.batch(seqs_a, seqs_b, pairs, *_half(matrix, o, e), n_b, seq_align.MODES[mode], bits)
    assert got["alignment"].shape == want["alignment"].shape and got["mode"] == mode
    _equal(got, want)
    span = got["end_b"] - got["begin_b"]
    assert np.array_equal(got["identity_span_b"], np.where(span > 0, got["n_identical"] / np.maximum(span, 1), 0.0))
    assert np.array_equal(got["coverage_b"], np.where(got["len_b"] > 0, span / np.maximum(got["len_b"], 1), 0.0))
    fast = seq_align.align_sequences(seqs_a, seqs_b, traceback=False, **call)
    assert "alignment" not in fast and set(fast) == set(got) - {"alignment"}
    for k in fast:
        assert np.array_equal(fast[k], got[k]), k
    return got


def _letters(rng, n, scoring):
    return rng.integers(0, 3 if scoring == "ties" else 20, n)


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
@pytest.mark.parametrize("la,lb", [(1, 1), (1, 64), (64, 1), (2, 3), (63, 65), (64, 64), (65, 63), (129, 127), (300, 287)])
def test_lengths_at_the_lane_stride_and_diagonal_edges(la, lb, scoring):
    """One pair per launch under local and the six flag sets.  blosum62: b is a stretch of a with substitutions between unrelated ends, so
    the free ends matter; ties: three letters, identity table, equal open and extend, so that most cells tie."""
    rng = np.random.default_rng(1000 * la + lb)
    a, b = _letters(rng, la, scoring), _letters(rng, lb, scoring)
    if min(la, lb) > 60 and scoring == "blosum62":
        n = min(la, lb) - 20
        b[7:7 + n] = a[13:13 + n]
        flip = rng.random(lb) < 0.2
        b[flip] = rng.integers(0, 20, int(flip.sum()))
    for flags in FLAGS:
        _check([a], [b], [(0, 0)], flags, scoring)


BACK_A, BACK_B, WORD = "AGST", "PLV", "WCHMFYW"  # two backgrounds that never score above 0 against each other (BLOSUM62), and a word


def _background(rng, letters, n):
    return enc("".join(rng.choice(list(letters), n)))


@pytest.mark.parametrize("end", [64, 65])
def test_a_local_end_cell_at_the_chunk_edge(end):
    """The word planted so that the local end cell sits at i = 64 (the last lane of a diagonal's first chunk of 64 inner cells begins at
    i = 1) and at i = 65."""
    rng = np.random.default_rng(end)
    a, b = _background(rng, BACK_A, 100), _background(rng, BACK_B, 30)
    a[end - 7:end], b[11:18] = enc(WORD), enc(WORD)
    got = _check([a], [b], [(0, 0)], "local")
    assert (got["begin_a"][0], got["end_a"][0], got["begin_b"][0], got["end_b"][0]) == (end - 7, end, 11, 18)
    assert got["n_identical"][0] == 7 and got["identity_span_b"][0] == 1.0 and got["score"][0] == seq_align.BLOSUM62[enc(WORD), enc(WORD)].sum()


@pytest.mark.parametrize("la", [65, 129])
def test_an_end_cell_in_the_last_row_and_in_the_last_column(la):
    """a ends inside b (the end cell (la, j) lies in the last row; index la lives in another chunk than most candidates of its diagonal)
    and, with the sides swapped, b ends inside a (the last column)."""
    rng = np.random.default_rng(la)
    shared = rng.integers(0, 20, 40)
    a = np.concatenate([_background(rng, BACK_A, la - 40), shared])
    b = np.concatenate([_background(rng, BACK_B, 9), shared, _background(rng, BACK_B, 31)])
    for flags in ("b_right", "b", "all"):
        got = _check([a], [b], [(0, 0)], flags)
        assert (got["end_a"][0], got["end_b"][0]) == (la, 49)
    for flags in ("a", "all"):
        got = _check([b], [a], [(0, 0)], flags)
        assert (got["end_a"][0], got["end_b"][0]) == (49, la)
    _check([b], [a], [(0, 0)], "local")


def test_a_free_leading_run_across_a_chunk():
    """70 leading rows of a are free under A_LEFT: the origin is the corner (70, 0); without the flag the run is walked and counted."""
    rng = np.random.default_rng(70)
    b = rng.integers(0, 20, 40)
    a = np.concatenate([_background(rng, BACK_A, 70), b])
    for flags in ("a_left", "a", "all"):
        got = _check([a], [b], [(0, 0)], flags)
        assert (got["begin_a"][0], got["end_a"][0], got["n_gaps_b"][0], got["n_gap_runs"][0]) == (70, 110, 0, 0)
        assert np.array_equal(got["alignment"][0], np.arange(70, 110)) and got["score"][0] == seq_align.BLOSUM62[b, b].sum()
    got = _check([a], [b], [(0, 0)], "none")
    assert (got["begin_a"][0], got["n_gaps_b"][0], got["n_gap_runs"][0]) == (0, 70, 1)


def test_tied_motifs_and_pairs_without_an_aligned_column():
    """The word twice in a: local takes the earlier diagonal, the semi-global key the later one.  All-X and disjoint alphabets between two
    ordinary pairs: NO_ALIGNED, and no bit of a neighbour changes."""
    word = enc(WORD)
    twice = np.concatenate([enc("AGST"), word, enc("GASTGA"), word, enc("ST")])
    seqs_a = [twice, np.full(9, 20), enc("AGSTAGSTAG"), twice]
    seqs_b = [word, np.full(6, 20), enc("PLVPLV")]
    pairs = [(0, 0), (1, 1), (2, 2), (3, 0)]
    got = _check(seqs_a, seqs_b, pairs, "local")
    assert got["begin_a"].tolist() == [4, 0, 0, 4] and got["end_a"].tolist() == [11, 0, 0, 11]
    assert got["status"].tolist() == [0, seq_align.NO_ALIGNED, seq_align.NO_ALIGNED, 0] and (got["alignment"][1:3] == -1).all()
    got = _check(seqs_a, seqs_b, pairs, "a")
    assert got["begin_a"][[0, 3]].tolist() == [17, 17] and got["status"][[0, 3]].tolist() == [0, 0]
    got = _check(seqs_a, seqs_b, pairs, "all")
    assert got["status"].tolist() == [0, seq_align.NO_ALIGNED, seq_align.NO_ALIGNED, 0] and got["score"][1:3].tolist() == [0.0, 0.0]
    _check(seqs_a, seqs_b, pairs, "all", "ties")
    _check(seqs_a, seqs_b, pairs, "local", "ties")


def test_one_wave_serves_every_pair_from_one_slab():
    """A padded ragged batch with ``max_workspace_bytes`` of one slab: a single wave serves every pair through the same LDS, the same
    direction bytes and the same running bests.  A high-scoring pair stands before low ones (a best that survived a pair would win the
    next); the result is the default launch's and the restatement's."""
    rng = np.random.default_rng(14)
    long = rng.integers(0, 20, 90)
    seqs_a = [long] + [rng.integers(0, 4, n) for n in (5, 64, 33, 1, 77, 12, 65)]
    seqs_b = [long[2:88]] + [rng.integers(0, 4, n) for n in (3, 63, 40, 70, 1)]
    pairs = [(0, 0)] + [(i, j) for i in range(1, 8) for j in range(1, 6)] + [(0, 0), (4, 5), (0, 0), (1, 1)]
    for flags in ("local", "all", "a", "b_right"):
        for scoring in sorted(SCORINGS):
            matrix, o, e = SCORINGS[scoring]
            mode, free_ends, _ = FLAGS[flags]
            default = _check(seqs_a, seqs_b, pairs, flags, scoring)
            one = seq_align.align_sequences(seqs_a, seqs_b, pairs=pairs, matrix=matrix, open_gap=o, extend_gap=e, mode=mode, free_ends=free_ends,
                                            max_workspace_bytes=90 * 86)
            assert set(one) == set(default)
            for k in default:
                assert np.array_equal(one[k], default[k]), k
    lib = _lib.load()
    assert lib.fdipt_seq_align_modes_workspace_bytes(40, 90, 86, 1, 90 * 86) == 90 * 86 == lib.fdipt_seq_align_modes_workspace_bytes(40, 90, 86, 1, 0)
    assert lib.fdipt_seq_align_modes_workspace_bytes(40, 90, 86, 1, 2 ** 30) == 40 * 90 * 86 and lib.fdipt_seq_align_modes_workspace_bytes(40, 90, 86, 0, 2 ** 30) == 0


def test_device_tensors_and_strings():
    """Padded arrays whose pad region holds valid letters, as NumPy arrays and as device tensors, and one-letter strings."""
    rng = np.random.default_rng(11)
    xa, xb = rng.integers(0, 20, (5, 70)), rng.integers(0, 20, (4, 66))
    xb[1, :30] = xa[2, 5:35]
    xb[0, 20:60] = xa[0, 3:43]
    la, lb = np.array([70, 17, 64, 1, 33]), np.array([66, 30, 65, 2])
    pairs = [(0, 0), (2, 1), (1, 3), (3, 2), (4, 0), (2, 1), (0, 2), (4, 3)]
    seqs_a, seqs_b = [xa[i, :la[i]] for i in range(5)], [xb[j, :lb[j]] for j in range(4)]
    dev = torch.device("cuda", torch.cuda.current_device())
    for flags in ("local", "all", "a_left"):
        mode, free_ends, bits = FLAGS[flags]
        want = mr.batch(seqs_a, seqs_b, pairs, *_half("blosum62", -10, -0.5), 66, seq_align.MODES[mode], bits)
        for a, b in ((xa, xb), (torch.from_numpy(xa).to(dev), torch.from_numpy(xb).to(dev)), (torch.from_numpy(xa).to(dev).int(), xb)):
            for traceback in (True, False):
                got = seq_align.align_sequences(a, b, len_a=la, len_b=lb, pairs=pairs, mode=mode, free_ends=free_ends, traceback=traceback)
                _equal(got, want, ("score",) + INTS + (("alignment",) if traceback else ()))
    strings = seq_align.align_sequences(["GGARNDBGG", "wyv-"], ["ARNDX", "ZZ"], pairs=[(0, 0), (1, 0), (1, 1)], matrix="identity", open_gap=-1, extend_gap=-1, mode="local")
    assert strings["n_identical"].tolist() == [4, 0, 0] and strings["begin_a"].tolist() == [2, 0, 0] and strings["end_b"].tolist() == [4, 0, 0]
    assert strings["status"].tolist() == [0, seq_align.NO_ALIGNED, seq_align.NO_ALIGNED]


def _raw(xa, la, xb, lb, pairs, mode, free_ends, traceback=True, **over):
    """``fdipt_seq_align_modes`` as a C caller reaches it: nothing is checked on the host.  BLOSUM62, -10 / -0.5."""
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)  # noqa: E731
    p, n_b = len(pairs), xb.shape[1]
    scalars = dict(S_a=xa.shape[0], N_a=xa.shape[1], S_b=xb.shape[0], N_b=n_b, P=p, max_len_a=int(max(la)), max_len_b=int(max(lb)), open_gap=-20,
                   extend_gap=-1, traceback=int(traceback), mode=mode, free_ends=free_ends)
    scalars.update(over)
    keys = ("score",) + INTS + (("alignment",) if traceback else ())
    outputs = {k: ("int32", (p, n_b) if k == "alignment" else (p,)) for k in keys}
    return _call.run("fdipt_seq_align_modes", _lib.SeqAlignModeArgs, dev, scalars,
                     dict(seq_a=up(xa), len_a=up(la), seq_b=up(xb), len_b=up(lb), pairs=up(pairs), table=up(seq_align.table_half_units("blosum62"))),
                     outputs, widen=keys, workspace=("fdipt_seq_align_modes_workspace_bytes", p, scalars["max_len_a"], scalars["max_len_b"], int(traceback), 2 ** 30))


def test_empty_bad_letter_and_skipped_pairs_change_no_neighbour():
    """Between ordinary pairs: a length of 0 (EMPTY alone, zeros, a map of -1), a letter outside 0 .. 20 (scored as X and flagged) and a
    pair index out of range (SKIPPED; only a C caller can send one) - in both new modes, with and without the traceback."""
    rng = np.random.default_rng(13)
    xa, xb = rng.integers(0, 20, (3, 40)), rng.integers(0, 20, (3, 44))
    xb[0, 10:34], xb[2, :12] = xa[0, 4:28], xa[1, :12]
    bad = xa.copy()
    bad[1, 4], bad[1, 9], bad[2, 39] = 25, -3, 21  # (row 2's lies beyond its length)
    la, lb = np.array([40, 12, 7]), np.array([44, 0, 30])
    pairs = np.array([(0, 0), (0, 1), (0, 0), (1, 2), (0, 0), (7, 0), (0, 0), (2, 3), (2, 2), (0, 0)])
    as_x = np.where((bad < 0) | (bad > 20), 20, bad)
    seqs_a, seqs_b = [as_x[i, :la[i]] for i in range(3)], [xb[j, :lb[j]] for j in range(3)]
    served = [k for k, (i, j) in enumerate(pairs) if i < 3 and j < 3]
    for mode, free in ((mr.LOCAL, 0), (mr.SEMIGLOBAL, 15), (mr.SEMIGLOBAL, 3), (mr.GLOBAL, 0)):
        want = mr.batch(seqs_a, seqs_b, [tuple(pairs[k]) for k in served], *_half("blosum62", -10, -0.5), 44, mode, free)
        want["status"][[served.index(3)]] |= _lib.SEQ_BAD_LETTER
        for traceback in (True, False):
            got = _raw(bad, la, xb, lb, pairs, mode, free, traceback)
            for k in ("score",) + INTS + (("alignment",) if traceback else ()):
                full = got[k] * (2 if k == "score" else 1)
                assert np.array_equal(full[served] if k != "score" else got[k][served], want["score_half" if k == "score" else k]), (k, mode, free)
                assert not np.delete(got[k], served, axis=0).any() or k in ("status", "alignment")
            assert got["status"][[1, 5, 7]].tolist() == [_lib.SEQ_EMPTY, _lib.SEQ_SKIPPED, _lib.SEQ_SKIPPED]
            if traceback:
                assert (got["alignment"][[1, 5, 7]] == -1).all()
            for k in (2, 4, 6, 9):  # the repeated ordinary pair, whatever stands before it
                assert all(np.array_equal(got[key][k], got[key][0]) for key in got)


def test_the_longest_pair_and_the_size_limit():
    """2048 x 2040 (one wave per block, the largest LDS layout and slab) per mode; 2049 letters are refused with FDIPT_ESIZE."""
    rng = np.random.default_rng(15)
    a = rng.integers(0, 20, 2048)
    b = np.delete(a, np.arange(700, 708))
    flip = rng.random(2040) < 0.4
    b[flip] = rng.integers(0, 20, int(flip.sum()))
    b[:25], b[2000:] = _background(rng, BACK_B, 25), _background(rng, BACK_B, 40)
    for flags in ("local", "all"):
        got = _check([a], [b], [(0, 0)], flags)
        assert got["n_aligned"][0] > 1800 and got["begin_b"][0] > 0 and got["end_b"][0] < 2040
    glob = seq_align.align_sequences([a], [b])
    new = _raw(a[None], [2048], b[None], [2040], np.array([(0, 0)]), mr.GLOBAL, 0)
    assert np.array_equal(new["alignment"], glob["alignment"]) and new["score"][0] == 2 * glob["score"][0]
    for mode in ("local", "semiglobal"):
        for traceback in (True, False):
            with pytest.raises(_lib.FdiptError, match="ESIZE"):
                seq_align.align_sequences(np.zeros((1, 2049), dtype=np.int64), np.zeros((1, 8), dtype=np.int64), traceback=traceback, mode=mode)


def test_the_global_mode_of_the_new_entry_and_its_refusals():
    """``mode = GLOBAL`` through fdipt_seq_align_modes equals ``align_sequences(mode="global")`` (fdipt_seq_align) in every shared output,
    with the span the host forms there; SEMIGLOBAL without a flag is the same launch.  A bad mode, flags outside 0 .. 15, flags with
    another mode and a null span output are FDIPT_EINVAL."""
    rng = np.random.default_rng(21)
    xa, xb = rng.integers(0, 20, (6, 130)), rng.integers(0, 20, (5, 127))
    xb[0, 5:100], xb[3, :64] = xa[1, :95], xa[4, 60:124]
    la, lb = np.array([130, 129, 64, 65, 127, 1]), np.array([127, 63, 1, 100, 0])
    pairs = np.array([(i, j) for i in range(6) for j in range(5)])
    for traceback in (True, False):
        old = seq_align.align_sequences(xa, xb, len_a=la, len_b=lb, pairs=pairs, traceback=traceback)
        for mode in (mr.GLOBAL, mr.SEMIGLOBAL):
            new = _raw(xa, la, xb, lb, pairs, mode, 0, traceback)
            for k in new:
                assert np.array_equal(new[k], 2 * old[k] if k == "score" else old[k]), (k, mode)
    assert old["n_aligned"].min() == 0 and old["mode"] == "global" and np.array_equal(old["end_a"][old["status"] == 0], old["len_a"][old["status"] == 0])
    one = (xa[:1], [130], xb[:1], [127], np.array([(0, 0)]))
    for over in (dict(mode=3), dict(mode=-1), dict(mode=mr.SEMIGLOBAL, free_ends=16), dict(mode=mr.SEMIGLOBAL, free_ends=-1),
                 dict(mode=mr.LOCAL, free_ends=1), dict(mode=mr.GLOBAL, free_ends=15), dict(mode=mr.LOCAL, open_gap=1)):
        with pytest.raises(_lib.FdiptError, match="EINVAL"):
            _raw(*one, over.pop("mode"), over.pop("free_ends", 0), **over)
    dev = torch.device("cuda", torch.cuda.current_device())
    with pytest.raises(_lib.FdiptError, match="EINVAL"):  # no span outputs
        _call.run("fdipt_seq_align_modes", _lib.SeqAlignModeArgs, dev, dict(S_a=1, N_a=4, P=1, max_len_a=4, max_len_b=4, mode=mr.LOCAL),
                  dict(seq_a=torch.zeros(4, dtype=torch.int32, device=dev), len_a=torch.full((1,), 4, dtype=torch.int32, device=dev),
                       pairs=torch.zeros(2, dtype=torch.int32, device=dev), table=torch.zeros(441, dtype=torch.int32, device=dev)),
                  {k: ("int32", (1,)) for k in ("score", "n_aligned", "n_identical", "n_gaps_a", "n_gaps_b", "n_gap_runs", "status")})


def _structure(rng):
    """60 rows in two chains; the reference lacks 5 leading and 4 trailing rows of chain H."""
    ca = np.cumsum(rng.normal(size=(60, 3)) * 2.2, axis=0).astype(np.float32)
    model = tr.five_atoms(ca)[None]
    kept = np.r_[np.arange(5, 26), np.arange(30, 60)]
    aatype = rng.integers(0, 20, 60)
    chain = np.array(["H"] * 30 + ["L"] * 30)
    return model, model[:, kept], aatype, chain, kept


def test_chain_row_map_fits_a_reference_without_termini():
    """``chain_row_map(mode="semiglobal", free_ends="a")`` on the 60-row structure: the map is the offset map and the model's overhangs
    cost nothing; the global alignment at the same scoring pays for both tails - what the restatement gives for each."""
    rng = np.random.default_rng(31)
    _, _, aatype, chain, kept = _structure(rng)
    half = _half("blosum62", -10, -0.5)
    fit = seq_align.chain_row_map(aatype, chain, aatype[kept], chain[kept], mode="semiglobal", free_ends="a")
    assert np.array_equal(fit["alignment"], kept) and fit["chains"] == [("H", "H"), ("L", "L")] and not fit["status"].any()
    assert fit["begin_a"].tolist() == [5, 0] and fit["end_a"].tolist() == [26, 30] and fit["n_gap_runs"].tolist() == [0, 0]
    assert fit["n_excluded"].tolist() == [0, 0] and fit["coverage_b"].tolist() == [1.0, 1.0] and fit["identity_span_b"].tolist() == [1.0, 1.0]
    glob = seq_align.chain_row_map(aatype, chain, aatype[kept], chain[kept])
    want_fit = mr.align(aatype[:30], aatype[kept][:21], *half, mr.SEMIGLOBAL, 3)
    want_glob = mr.align(aatype[:30], aatype[kept][:21], *half, mr.GLOBAL)
    assert fit["score"][0] == want_fit["score"] == seq_align.BLOSUM62[aatype[5:26], aatype[5:26]].sum()
    assert glob["score"][0] == want_glob["score"] <= fit["score"][0] - (10 + 4 * 0.5) - (10 + 3 * 0.5) and glob["n_gap_runs"][0] == want_glob["n_gap_runs"] >= 2
    assert np.array_equal(glob["alignment"][:21], np.where(want_glob["alignment"] >= 0, want_glob["alignment"], -1))
    assert glob["begin_a"].tolist() == [0, 0] and glob["end_a"].tolist() == [30, 30]
    cut = seq_align.chain_row_map(aatype, chain, aatype[kept], chain[kept], mode="semiglobal", free_ends="a", exclude_a=[(10, 12), None], exclude_b=[(5, 7), None])
    assert np.array_equal(cut["alignment"], np.where((kept >= 10) & (kept <= 12), -1, kept)) and cut["n_excluded"].tolist() == [3, 0]
    with pytest.raises(ValueError, match="same excluded region"):
        seq_align.chain_row_map(aatype, chain, aatype[kept], chain[kept], mode="semiglobal", free_ends="a", exclude_a=[(10, 12), None], exclude_b=[(10, 12), None])


def test_sequence_aligned_accuracy_with_the_fitted_map():
    """``compare.sequence_aligned_accuracy(mode="semiglobal", free_ends="a")``: the reference is the model's own rows, so every covered
    row scores lDDT 1 and every reference row is covered."""
    rng = np.random.default_rng(32)
    model, truth, aatype, chain, kept = _structure(rng)
    got = compare.sequence_aligned_accuracy(model, aatype, truth, aatype[kept], chain_a=chain, chain_b=chain[kept], mode="semiglobal", free_ends="a")
    assert np.array_equal(got["alignment"], kept) and got["n_covered"].tolist() == [51] and got["n_reference"].tolist() == [51]
    # a perfect score is (1 / (eps + c)) * (eps + 0.25 * 4 c) in float64 (lddt_body.hpp: ld_score): four roundings of half an ulp each
    ulps = 4 * np.finfo(np.float64).eps
    assert got["res_lddt"].shape == (1, 51) and np.abs(got["res_lddt"] - 1.0).max() <= ulps and abs(got["lddt"][0] - 1.0) <= ulps
    assert not got["seq_status"].any() and got["gdt_ts"].tolist() == [1.0]


def test_run_seq_diversity_in_the_local_and_semiglobal_modes(tmp_path):
    """``run_sharded.run_seq_diversity(mode=)`` (``--seq-align-mode``) on gathered entries of two lengths: the matrix file carries the mode
    in its name, the JSON records it, the numbers are the direct score-only call's and the restatement's, and the global files of an
    earlier run stay."""
    rng = np.random.default_rng(17)
    text = lambda n: "".join(seq_align.LETTERS[c] for c in rng.integers(0, 20, n))  # noqa: E731
    base = text(31)
    designed = {0: [base, base[:12] + text(19)], 1: [text(24), base[4:28]], 2: [base[:20] + text(11)]}
    records = [{"item": i, "name": f"length_{len(designed[i][0])}", "sample_i": i, "file": f"sample_{i:06d}.npz"} for i in range(3)]
    gathered = {i: {"designed_sequences": designed[i]} for i in range(3)}
    run_sharded.run_seq_diversity(str(tmp_path), records, gathered)
    before = np.load(tmp_path / "pairwise_seq_identity.npy")
    seqs = [enc(s) for i in range(3) for s in designed[i]]
    for mode, bits in (("local", 0), ("semiglobal", 15)):
        done = run_sharded.run_seq_diversity(str(tmp_path), records, gathered, mode=mode)
        direct = seq_align.align_sequences(seqs, traceback=False, mode=mode)
        want = mr.batch(seqs, seqs, direct["pairs"], *_half("blosum62", -10, -0.5), 31, seq_align.MODES[mode], bits)
        assert np.array_equal(direct["n_identical"], want["n_identical"]) and np.array_equal(direct["score"], want["score"])
        matrix = np.load(tmp_path / f"pairwise_seq_identity_{mode}.npy")
        assert np.array_equal(matrix, direct["matrix"]) and matrix.shape == (5, 5)
        with open(tmp_path / "seq_diversity.json") as f:
            assert json.load(f) == json.loads(json.dumps(done))
        assert done["matrix"] == f"pairwise_seq_identity_{mode}.npy" and done["scoring"]["mode"] == mode
        assert done["scoring"].get("free_ends") == ("all" if mode == "semiglobal" else None)
        assert matrix[0, 3] == 1.0  # base[4:28] lies inside base
        assert np.array_equal(np.load(tmp_path / "pairwise_seq_identity.npy"), before)
    with pytest.raises(ValueError, match="mode"):
        run_sharded.run_seq_diversity(str(tmp_path), records, gathered, mode="overlap")
