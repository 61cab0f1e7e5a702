"""GPU tests (-m gpu) of sequence alignment on the device: ``seq_align.align_sequences`` (fdipt_seq_align,
csrc/seqalign.hip) against the NumPy restatement (tests/seqalign_ref.py) on every output - all of them integers or formed from integers,
so equality is ``np.array_equal`` -, the score-only mode against the traceback mode, then the callers: ``seq_align.chain_row_map`` through
``compare.sequence_aligned_accuracy`` and ``run_sharded.run_seq_diversity``.  Every case runs in seconds."""
import json

import numpy as np
import pytest
import torch

import seqalign_ref as ref
import tm_ref as tr
from framedipt_amd import _lib, compare, gdt, lddt, row_map, run_sharded, seq_align

pytestmark = pytest.mark.gpu

INTS = ("n_aligned", "n_identical", "n_gaps_a", "n_gaps_b", "n_gap_runs")
SCORINGS = {"blosum62": ("blosum62", -10.0, -0.5), "ties": ("identity", -1.0, -1.0)}


def _half(matrix, o, e):
    return seq_align.table_half_units(matrix).astype(np.int64), int(2 * o), int(2 * e)


def _check(seqs_a, seqs_b, pairs, scoring="blosum62", **kw):
    """One launch with the traceback over ragged lists against the restatement, then the score-only launch against the first."""
    matrix, o, e = SCORINGS[scoring]
    got = seq_align.align_sequences(seqs_a, seqs_b, pairs=pairs, matrix=matrix, open_gap=o, extend_gap=e, **kw)
    n_b = max(len(s) for s in seqs_b)
    want = ref.batch(seqs_a, seqs_b, pairs, *_half(matrix, o, e), max(n_b, 1))
    assert got["alignment"].shape == want["alignment"].shape
    for k in ("score", "alignment") + INTS:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    empty = np.array([len(seqs_a[i]) == 0 or len(seqs_b[j]) == 0 for i, j in pairs])
    assert np.array_equal(got["status"], np.where(empty, _lib.SEQ_EMPTY, 0))
    la, lb = np.array([len(seqs_a[i]) for i, _ in pairs]), np.array([len(seqs_b[j]) for _, j in pairs])
    assert np.array_equal(got["len_a"], la) and np.array_equal(got["len_b"], lb)
    for k, d in (("identity", got["n_aligned"]), ("identity_b", lb), ("identity_short", np.minimum(la, lb))):
        assert np.array_equal(got[k], np.where(d > 0, got["n_identical"] / np.maximum(d, 1), 0.0))
    _score_only_equals(got, seqs_a, seqs_b, pairs, matrix, o, e)
    return got


def _score_only_equals(got, seqs_a, seqs_b, pairs, matrix, o, e, **kw):
    fast = seq_align.align_sequences(seqs_a, seqs_b, pairs=pairs, matrix=matrix, open_gap=o, extend_gap=e, traceback=False, **kw)
    assert "alignment" not in fast and set(fast) == set(got) - {"alignment"}
    for k in fast:
        assert np.array_equal(fast[k], got[k]), k


def _letters(rng, n, scoring):
    return rng.integers(0, 3 if scoring == "ties" else 20, n)


@pytest.mark.parametrize("scoring", sorted(SCORINGS))
@pytest.mark.parametrize("la,lb", [(1, 1), (1, 64), (64, 1), (2, 3), (63, 65), (64, 64), (65, 63), (127, 129), (128, 128), (129, 127), (300, 287)])
def test_lengths_at_the_lane_stride_and_diagonal_edges(la, lb, scoring):
    """One pair per launch, so that every length sizes its own LDS layout: a diagonal of exactly one, one more and one fewer than a whole
    number of 64-lane chunks, N_a > N_b and N_b > N_a.  ``ties``: three letters, identity table, equal open and extend - ties at most
    cells, so the whole path is the tie rule's."""
    rng = np.random.default_rng(1000 * la + lb)
    a = _letters(rng, la, scoring)
    b = _letters(rng, lb, scoring)
    if min(la, lb) > 60 and scoring == "blosum62":  # related sequences: b is a with substitutions (an unrelated pair is covered by ties)
        b = np.resize(a, lb)
        flip = rng.random(lb) < 0.3
        b[flip] = rng.integers(0, 20, int(flip.sum()))
    _check([a], [b], [(0, 0)], scoring)


def test_padded_batches_read_nothing_beyond_a_length():
    """Arrays [S,N] whose lengths lie below the padded width, the pad region full of valid letters: NumPy arrays and device tensors give the
    restatement's numbers on the sequences cut to their lengths; pairs repeat and cross."""
    rng = np.random.default_rng(11)
    xa, xb = rng.integers(0, 20, (5, 70)), rng.integers(0, 20, (4, 66))
    xb[1, :30] = xa[2, 5:35]
    la, lb = np.array([70, 17, 64, 1, 33]), np.array([66, 30, 65, 2])
    pairs = [(0, 0), (2, 1), (1, 3), (3, 2), (4, 0), (2, 1), (0, 2), (4, 3)]
    seqs_a, seqs_b = [xa[i, :la[i]] for i in range(5)], [xb[j, :lb[j]] for j in range(4)]
    want = ref.batch(seqs_a, seqs_b, pairs, *_half("blosum62", -10, -0.5), 66)
    dev = torch.device("cuda", torch.cuda.current_device())
    for a, b in ((xa, xb), (torch.from_numpy(xa).to(dev), torch.from_numpy(xb).to(dev)), (torch.from_numpy(xa).to(dev).int(), xb)):
        got = seq_align.align_sequences(a, b, len_a=la, len_b=lb, pairs=pairs)
        for k in ("score", "alignment") + INTS:
            assert np.array_equal(got[k], want[k]), k
        assert not got["status"].any()
    _score_only_equals(got, xa, xb, pairs, "blosum62", -10.0, -0.5, len_a=la, len_b=lb)
    # one array and no pairs: all i < j and the mirrored matrix of identity_short
    sq = seq_align.align_sequences(xa, len_a=la, traceback=False)
    assert sq["pairs"].tolist() == [[i, j] for i in range(5) for j in range(i + 1, 5)]
    m = sq["matrix"]
    assert m.shape == (5, 5) and np.array_equal(m, m.T) and np.array_equal(np.diag(m), np.ones(5)) and np.array_equal(m[sq["pairs"][:, 0], sq["pairs"][:, 1]], sq["identity_short"])
    assert np.array_equal(sq["n_identical"], ref.batch(seqs_a, seqs_a, sq["pairs"], *_half("blosum62", -10, -0.5), 70)["n_identical"])


def test_a_gap_run_across_a_stride_edge():
    """A 70-row deletion: the X run crosses a 64-lane chunk edge and the map is the known one."""
    rng = np.random.default_rng(12)
    a = rng.integers(0, 20, 200)
    a[60], a[130], a[59], a[129] = 0, 1, 2, 3  # the run cannot slide
    b = np.delete(a, np.arange(60, 130))
    got = _check([a], [b], [(0, 0)])
    assert np.array_equal(got["alignment"][0], np.delete(np.arange(200), np.arange(60, 130)))
    assert (got["n_gaps_b"][0], got["n_gap_runs"][0], got["n_identical"][0]) == (70, 1, 130)
    assert got["score"][0] == seq_align.BLOSUM62[b, b].sum() - 10 - 69 * 0.5
    back = _check([b], [a], [(0, 0)])
    assert np.array_equal(back["alignment"][0], row_map.invert(got["alignment"][0], 200)) and back["n_gaps_a"][0] == 70


def test_planted_ties_all_x_and_strings():
    """AAAA / AA and ARA / AA with equal open and extend (the first of M, X, Y wins: the gap lands at the start), a pair of all-X sequences
    (no letter is identical to X), and one-letter strings with letters outside the twenty."""
    got = _check([seq_align.encode(s) for s in ("AAAA", "ARA", "AA", "XXXXX")], [seq_align.encode(s) for s in ("AA", "AAAA", "XXX")],
                 [(0, 0), (1, 0), (2, 1), (3, 2), (3, 0)], "ties")
    assert got["alignment"].tolist() == [[2, 3, -1, -1], [0, 2, -1, -1], [-1, -1, 0, 1], [2, 3, 4, -1], [3, 4, -1, -1]]
    assert got["score"].tolist() == [0.0, 1.0, 0.0, -5.0, -5.0] and got["n_identical"].tolist() == [2, 2, 2, 0, 0]
    strings = seq_align.align_sequences(["ARNDB", "wyv-"], ["ARNDX"], matrix="identity", open_gap=-1, extend_gap=-1)
    assert strings["n_identical"].tolist() == [4, 0] and strings["n_aligned"].tolist() == [5, 4] and strings["pairs"].tolist() == [[0, 0], [1, 0]]


def test_empty_and_bad_letters_through_device_tensors():
    """A device tensor is judged on the device: a length of 0 answers EMPTY with zeros and a map of -1, a letter outside 0 .. 20 inside a
    length is scored as X and flagged, and neither changes another pair."""
    rng = np.random.default_rng(13)
    dev = torch.device("cuda", torch.cuda.current_device())
    xa, xb = rng.integers(0, 20, (3, 20)), rng.integers(0, 20, (2, 24))
    xb[0, :20] = xa[0]
    bad = xa.copy()
    bad[1, 4], bad[1, 9], bad[2, 19] = 25, -3, 21  # (row 2's lies beyond its length)
    la, lb = np.array([20, 12, 7]), np.array([24, 0])
    pairs = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1)]
    as_x = bad.copy()
    as_x[(bad < 0) | (bad > 20)] = 20
    want = ref.batch([as_x[i, :la[i]] for i in range(3)], [xb[j, :lb[j]] for j in range(2)], pairs, *_half("blosum62", -10, -0.5), 24)
    for traceback in (True, False):
        got = seq_align.align_sequences(torch.from_numpy(bad).to(dev), torch.from_numpy(xb).to(dev), len_a=la, len_b=lb, pairs=pairs, traceback=traceback)
        assert got["status"].tolist() == [0, _lib.SEQ_BAD_LETTER, 0, _lib.SEQ_EMPTY, _lib.SEQ_EMPTY]
        for k in ("score",) + INTS + (("alignment",) if traceback else ()):
            assert np.array_equal(got[k], want[k]), k
        assert not got["score"][3:].any() and not got["n_gaps_a"][3:].any() and not got["identity"][3:].any()
    with pytest.raises(ValueError, match="letter outside"):
        seq_align.align_sequences(bad, xb, len_a=la, len_b=lb, pairs=pairs)


def test_one_wave_serves_every_pair_from_one_slab():
    """A pair list longer than the persistent waves with shapes that change from pair to pair: with ``max_workspace_bytes`` of one slab a
    single wave walks all of them through the same direction bytes and the same LDS, and the result is the default launch's bit for bit."""
    rng = np.random.default_rng(14)
    seqs_a = [rng.integers(0, 4, n) for n in (90, 5, 64, 33, 1, 77, 12, 65)]
    seqs_b = [rng.integers(0, 4, n) for n in (3, 88, 63, 40, 70, 1)]
    pairs = [(i, j) for i in range(8) for j in range(6)]
    rng.shuffle(pairs)
    for scoring in sorted(SCORINGS):
        matrix, o, e = SCORINGS[scoring]
        default = _check(seqs_a, seqs_b, pairs, scoring)
        one = seq_align.align_sequences(seqs_a, seqs_b, pairs=pairs, matrix=matrix, open_gap=o, extend_gap=e, max_workspace_bytes=90 * 88)
        few = seq_align.align_sequences(seqs_a, seqs_b, pairs=pairs, matrix=matrix, open_gap=o, extend_gap=e, max_workspace_bytes=5 * 90 * 88 + 17)
        assert set(one) == set(default)
        for k in default:
            assert np.array_equal(one[k], default[k]) and np.array_equal(few[k], default[k]), k
    lib = _lib.load()
    assert lib.fdipt_seq_align_workspace_bytes(48, 90, 88, 1, 90 * 88) == 90 * 88 == lib.fdipt_seq_align_workspace_bytes(48, 90, 88, 1, 0)
    assert lib.fdipt_seq_align_workspace_bytes(48, 90, 88, 1, 2 ** 30) == 48 * 90 * 88 and lib.fdipt_seq_align_workspace_bytes(48, 90, 88, 0, 2 ** 30) == 0


def test_the_longest_pair_and_the_size_limit():
    """2048 x 2040 (one wave per block, the largest LDS layout and slab) in both modes; 2049 letters are refused with FDIPT_ESIZE."""
    rng = np.random.default_rng(15)
    a = rng.integers(0, 20, 2048)
    b = np.delete(a, np.arange(700, 708))
    flip = rng.random(2040) < 0.4
    b[flip] = rng.integers(0, 20, int(flip.sum()))
    got = _check([a], [b], [(0, 0)])
    assert got["n_aligned"][0] > 1900
    for traceback in (True, False):
        with pytest.raises(_lib.FdiptError, match="ESIZE"):
            seq_align.align_sequences(np.zeros((1, 2049), dtype=np.int64), np.zeros((1, 8), dtype=np.int64), traceback=traceback)
    assert seq_align.MAX_ROWS == 2048


def test_sequence_aligned_accuracy_on_a_60_row_structure():
    """A model of 60 rows against a reference that lacks rows 10 .. 14 and 40 (one chain, then two): the map equals
    ``row_map.from_residue_numbers`` on the true numbering, and the lDDT / GDT outputs equal the mapped calls with that map."""
    rng = np.random.default_rng(16)
    ca = np.cumsum(rng.normal(size=(60, 3)) * 2.2, axis=0).astype(np.float32)
    model = tr.five_atoms((ca + 0.5 * rng.normal(size=ca.shape)).astype(np.float32))[None]
    kept = np.delete(np.arange(60), [10, 11, 12, 13, 14, 40])
    truth = tr.five_atoms(ca[kept])[None]
    aatype = rng.integers(0, 20, 60)
    aatype[[9, 14, 10, 15, 39, 40, 41]] = [0, 1, 2, 3, 4, 5, 6]  # neither gap can slide
    chain = np.array(["H"] * 30 + ["L"] * 30)
    want_map = row_map.from_residue_numbers(chain, np.arange(60), chain[kept], kept)
    for chains in ((None, None), (chain, chain[kept])):
        got = compare.sequence_aligned_accuracy(model, aatype, truth, aatype[kept], chain_a=chains[0], chain_b=chains[1])
        assert np.array_equal(got["alignment"], want_map) and got["alignment"].shape == (54,)
        assert got["chains"] == ([(None, None)] if chains[0] is None else [("H", "H"), ("L", "L")])
        assert got["identity"].tolist() == [1.0] * len(got["chains"]) and int(got["n_aligned"].sum()) == 54 and not got["seq_status"].any()
        local = lddt.local_accuracy(model, truth, alignment=want_map, coverage="penalise")
        glob = gdt.gdt_scores(model, truth, alignment=want_map, norm_length="reference")
        for k in ("lddt", "res_lddt", "n_covered", "n_reference", "drmsd"):
            assert np.array_equal(got[k], local[k]), k
        for k in ("gdt_ts", "gdt_ha", "counts", "res_within"):
            assert np.array_equal(got[k], glob[k]), k
        assert got["n_covered"].tolist() == [54] and got["res_lddt"].shape == (1, 54)
    one = ref.align(aatype[:30], aatype[kept][:25], *_half("blosum62", -10, -0.5))
    assert got["score"][0] == one["score"] == seq_align.BLOSUM62[aatype[kept][:25], aatype[kept][:25]].sum() - 10 - 4 * 0.5
    # an unpaired chain stays open
    lone = seq_align.chain_row_map(aatype, chain, aatype[kept], np.array(["H"] * 25 + ["K"] * 29))
    assert np.array_equal(lone["alignment"], np.concatenate([want_map[:25], np.full(29, -1)])) and lone["chains"] == [("H", "H")]


def test_run_seq_diversity_on_gathered_entries(tmp_path):
    """``run_sharded.run_seq_diversity`` (what ``--design --seq-diversity`` runs on rank 0) on gathered entries of two lengths as
    ``run_design`` leaves them: the matrix file and the JSON carry the numbers of the direct score-only call."""
    rng = np.random.default_rng(17)
    text = lambda n: "".join(seq_align.LETTERS[c] for c in rng.integers(0, 20, n))  # noqa: E731
    base = text(31)
    designed = {0: [base, base[:12] + text(19)], 1: [text(24), base[4:28]], 2: [base[:20] + text(11)]}
    records = [{"item": i, "name": f"length_{len(designed[i][0])}", "sample_i": i, "file": f"sample_{i:06d}.npz"} for i in range(3)]
    gathered = {i: {"designed_sequences": designed[i]} for i in range(3)}
    done = run_sharded.run_seq_diversity(str(tmp_path), records, gathered)
    seqs = [s for i in range(3) for s in designed[i]]
    direct = seq_align.align_sequences(seqs, traceback=False)
    want = ref.batch([seq_align.encode(s) for s in seqs], [seq_align.encode(s) for s in seqs], direct["pairs"], *_half("blosum62", -10, -0.5), 31)
    assert np.array_equal(direct["n_identical"], want["n_identical"]) and np.array_equal(direct["score"], want["score"])
    matrix = np.load(tmp_path / "pairwise_seq_identity.npy")
    assert np.array_equal(matrix, direct["matrix"]) and matrix.shape == (5, 5)
    with open(tmp_path / "seq_diversity.json") as f:
        assert json.load(f) == json.loads(json.dumps(done))
    assert done["n_sequences"] == 5 and done["sequences"][3] == {"sample": "sample_000001", "index": 1}
    assert done["mean_identity"] == matrix[~np.eye(5, dtype=bool)].mean()
    assert done["max_identity_to_other_sample"] == {"sample_000000": float(matrix[:2, 2:].max()), "sample_000001": float(matrix[2:4][:, [0, 1, 4]].max()),
                                                    "sample_000002": float(matrix[4, :4].max())}
    assert done["max_identity_to_other_sample"]["sample_000001"] == 1.0  # base[4:28] lies inside base
    assert done["scoring"] == {"matrix": "blosum62", "open_gap": -10.0, "extend_gap": -0.5, "mode": "global"}
    with pytest.raises(ValueError, match="designed sequences"):
        run_sharded.run_seq_diversity(str(tmp_path), records, {i: {} for i in range(3)})
