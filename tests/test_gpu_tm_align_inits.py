"""GPU tests (-m gpu) of the five-start mode of the structural alignment search (``inits="all"``: tm_align5_kernel of csrc/tmalign.hip,
ss_score5_kernel / ss_detail5_kernel of csrc/structsearch.hip; DESIGN.md section 7.9, "The two fragment starts") against the NumPy
restatement tests/tma_inits_ref.py as recorded in tests/golden/tma_inits_cases.npz, and against the default mode where the contract says
the two agree bit for bit.  ``-s`` prints the device's error per case next to its bound, max(32 x yard, 1e-13)."""
import functools
import json

import numpy as np
import pytest

import tma_inits_ref as ti
import tma_ref as ta
from conftest import load_golden
from framedipt_amd import _lib, run_sharded, structure_search as ss, tm_align
from test_gpu_tm_align import _check_pair, _same_pair

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("tma_inits_cases.npz")


@functools.lru_cache(maxsize=None)
def _single(name, inits="all"):
    """One recorded case as a launch of its own."""
    a, b, ma, mb = ti.case_inputs(_fix(), name)
    return tm_align.tm_align(a[None], b[None], ma[None], mb[None], inits=inits)


@pytest.mark.parametrize("name", ti.CASES)
def test_case_matches_the_restatement(name):
    """5 x 5 (no candidate of I4), 6 x 9 (one fragment length), 19 x 22, 64 x 65, the thresholds of I4's jump (151, 201, 251 rows), 300 x
    300 (two rows per thread), 512 x 512 (221 candidates, the LDS limit), Frag's constructions (a gap, equal runs, one widening round, the
    donor either way), separate masks, and the two planted motifs that only I4 finds."""
    fix, got = _fix(), _single(name)
    a, b, ma, mb = ti.case_inputs(fix, name)
    assert got["init_tm"].shape == (1, 5) and got["init_dp"].shape == (1, 5)
    _check_pair(got, 0, fix, name, None, a, b, ma, mb)


@pytest.mark.parametrize("name", ti.CASES)
def test_columns_0_to_2_and_pairs_won_by_the_first_three_equal_the_default_mode(name):
    got, default = _single(name), _single(name, "default")
    assert default["init_tm"].shape == (1, 3) and default["init_dp"].shape == (1, 3)
    assert np.array_equal(got["init_tm"][:, :3], default["init_tm"]) and np.array_equal(got["init_dp"][:, :3], default["init_dp"])
    if got["best_init"][0] <= 2:
        for k in tm_align.OUTPUTS:
            if k not in ("init_tm", "init_dp"):
                assert np.array_equal(got[k], default[k], equal_nan=True), k
    else:
        assert got["init_tm"][0, got["best_init"][0]] > -1 and default["best_init"][0] <= 2


@pytest.mark.parametrize("name", ti.PLANTED)
def test_planted_motif_is_found_where_the_default_mode_misses_it(name):
    got, default = _single(name), _single(name, "default")
    print(f"{name}: tm_b {got['tm_b'][0]:.4f} (best_init {got['best_init'][0]}), default {default['tm_b'][0]:.4f}")
    assert default["tm_b"][0] == float(_fix()[f"{name}.default_tm_b"])
    assert got["best_init"][0] >= 3 and got["tm_b"][0] >= default["tm_b"][0] + 0.1 and got["tm_a"][0] >= 0.3
    on = np.flatnonzero(got["alignment"][0] >= 0)
    assert ((got["alignment"][0][on] - on) == -75).sum() >= 36


BATCH = ("n5", "n6x9", "n19x22", "gap12", "masked", "donor_y", "motif03")


def test_padded_batch_equals_the_pairs_alone_in_any_order():
    """Seven cases of 5 .. 125 rows padded to 130 rows in one launch, the pair list in order and permuted: every pair's outputs equal
    its own launch bit for bit."""
    fix = _fix()
    prot = np.full((2 * len(BATCH), 130, 5, 3), 7.5, dtype=np.float32)
    mask = np.zeros((2 * len(BATCH), 130), dtype=np.float32)
    for k, name in enumerate(BATCH):
        a, b, ma, mb = ti.case_inputs(fix, name)
        prot[2 * k, :len(a)], prot[2 * k + 1, :len(b)] = a, b
        mask[2 * k, :len(a)], mask[2 * k + 1, :len(b)] = ma, mb
    pairs = np.array([[2 * k, 2 * k + 1] for k in range(len(BATCH))])
    got = tm_align.tm_align(prot, mask_a=mask, pairs=pairs, inits="all")
    order = np.array([4, 0, 6, 2, 5, 1, 3])
    mixed = tm_align.tm_align(prot, mask_a=mask, pairs=pairs[order], inits="all")
    assert got["init_tm"].shape == (7, 5)
    for k, name in enumerate(BATCH):
        rows = len(fix[f"{name}.ca_b"])
        _same_pair(got, k, _single(name), 0, rows)
        _same_pair(mixed, int(np.flatnonzero(order == k)[0]), _single(name), 0, rows)


def test_statuses_and_limits():
    fix = _fix()
    a, b, _, _ = ti.case_inputs(fix, "n6x9")
    mask_b = np.ones((1, 9), dtype=np.float32)
    mask_b[0, [0, 2, 4, 6, 8]] = 0
    got = tm_align.tm_align(a[None], b[None], None, mask_b, inits="all")  # n2 = 4
    assert got["status"].tolist() == [_lib.TMA_TOO_SHORT] and np.isnan(got["tm"][0]) and got["n_aligned"].tolist() == [0]
    assert got["best_init"].tolist() == [-1] and got["init_tm"].shape == (1, 5) and (got["init_tm"] == -1).all() and not got["init_dp"].any()
    assert (got["alignment"] == -1).all() and np.array_equal(got["rotation"][0], np.eye(3))
    bad = a.copy()
    bad[2, 1, 0] = np.nan
    got = tm_align.tm_align(np.stack([a, bad]), b[None], ref_index=[0, 0], inits="all")
    assert got["status"].tolist() == [0, _lib.TMA_NOT_FINITE] and np.isnan(got["tm"][1]) and (got["init_tm"][1] == -1).all() and not got["init_dp"][1].any()
    _same_pair(got, 0, _single("n6x9"), 0)
    both = np.stack([b, b[::-1].copy()])
    got = tm_align.tm_align(both, pairs=[[0, 1], [0, 2], [-1, 0], [1, 0]], inits="all")  # an index out of range
    assert got["status"].tolist() == [0, _lib.TMA_SKIPPED, _lib.TMA_SKIPPED, 0] and np.isnan(got["tm"][1:3]).all() and np.isfinite(got["tm"][[0, 3]]).all()
    assert (got["init_tm"][1:3] == -1).all() and (got["init_tm"][[0, 3], 0] > 0).all()
    long = np.zeros((1, tm_align.MAX_ROWS + 1, 5, 3), dtype=np.float32)
    with pytest.raises(_lib.FdiptError, match="ESIZE"):
        tm_align.tm_align(long, long, inits="all")
    with pytest.raises(_lib.FdiptError, match="ESIZE"):
        tm_align.tm_align(b[None], long, inits="all")


def test_the_entries_refuse_an_inits_that_is_none_of_the_two():
    import ctypes as C

    import torch
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    bufs = {k: torch.zeros(64, dtype=torch.float64, device=dev) for k in tm_align.OUTPUTS + ("prot", "mask", "pairs")}
    fields = dict(S=1, N_a=9, atoms=5, ca=1, S_b=1, N_b=9, atoms_b=5, P=1, prot_b=None, mask_b=None, workspace=None, workspace_bytes=0,
                  **{k: _lib.ptr(v) for k, v in bufs.items()})
    for bad in (2, -1, 5):
        assert lib.fdipt_sample_tm_align(C.byref(_lib.TmAlignArgs(inits=bad, **fields)), _lib.stream_ptr()) == _lib.EINVAL
    # the search takes the mode as an argument of a second entry
    scalars = ("Q", "N_q", "atoms", "ca", "D", "top_k", "rank_by", "prune", "details", "n_buckets", "detail_cap", "R", "min_score", "bucket_start", "bucket_cap",
               "workspace", "workspace_bytes")
    bufs = {k: torch.zeros(4096, dtype=torch.float64, device=dev) for k, _ in _lib.SearchArgs._fields_ if k not in scalars or k == "workspace"}
    start, cap = np.array([0, 1], dtype=np.int32), np.array([16], dtype=np.int32)
    args = _lib.SearchArgs(Q=1, N_q=9, atoms=5, ca=1, D=1, top_k=1, rank_by=0, prune=1, details=1, n_buckets=1, detail_cap=16, R=9, min_score=0.0,
                           bucket_start=start.ctypes.data_as(C.c_void_p), bucket_cap=cap.ctypes.data_as(C.c_void_p), workspace_bytes=4096 * 8,
                           **{k: _lib.ptr(v) for k, v in bufs.items()})
    for bad in (2, -1, 5):
        assert lib.fdipt_structure_search_inits(C.byref(args), bad, _lib.stream_ptr()) == _lib.EINVAL


@functools.lru_cache(maxsize=None)
def _search_case():
    """3 queries (70 rows: 70, 45 and 24 set) and 12 entries of 20 .. 70 rows in the buckets of 32 and of 96 rows: windows of the
    queries' walk with noise, among them the second trace of a planted pair cut to 70 rows."""
    rng = np.random.default_rng(31)
    fix = _fix()
    w = fix["motif03.ca_a"][:70].astype(np.float64)
    prot = np.stack([ta.five_atoms((w + s * 0.4 * rng.normal(size=w.shape)).astype(np.float32)) for s in range(3)])
    mask = np.ones((3, 70), dtype=np.float32)
    mask[1, 45:], mask[2, :30], mask[2, 54:] = 0, 0, 0
    entries = []
    for n, first in zip((20, 24, 28, 30, 31, 32, 65, 66, 67, 68, 69), (0, 5, 10, 30, 35, 38, 0, 1, 2, 0, 1)):
        entries.append((w[first:first + n] + 0.5 * rng.normal(size=(n, 3))).astype(np.float32))
    entries.append(fix["motif03.ca_b"][55:125])  # 70 rows that hold the motif at rows 25 .. 64
    return prot, mask, entries


def test_search_equals_the_brute_force_tm_align_bit_for_bit():
    prot, mask, entries = _search_case()
    db = ss.StructureSet.from_arrays(entries)
    work = ss.plan(db.lengths)
    assert work["bucket_cap"].tolist() == [96, 32] and db.lengths.min() == 20 and db.lengths.max() == 70
    padded = np.full((12, 70, 5, 3), 7.5, dtype=np.float32)
    padded_mask = np.zeros((12, 70), dtype=np.float32)
    for e, t in enumerate(entries):
        padded[e, :len(t)], padded_mask[e, :len(t)] = ta.five_atoms(t), 1
    pairs = np.array([[q, e] for q in range(3) for e in range(12)])
    dense = tm_align.tm_align(prot, padded, mask, padded_mask, pairs=pairs, inits="all")
    plain = tm_align.tm_align(prot, padded, mask, padded_mask, pairs=pairs)
    print("pairs won by I4 or I5:", int((dense["best_init"] >= 3).sum()), "of 36; tm_b rose in", int((dense["tm_b"] > plain["tm_b"]).sum()))
    brute = ss.search(prot, db, mask, top_k=4, prune=False, details=True, return_scores=True, inits="all")
    assert brute["inits"] == "all"
    assert np.array_equal(brute["scores_q"], dense["tm_a"].reshape(3, 12)) and np.array_equal(brute["scores_t"], dense["tm_b"].reshape(3, 12))
    assert np.array_equal(brute["pair_status"], dense["status"].reshape(3, 12)) and not brute["pair_status"].any()
    order = np.lexsort((np.arange(12)[None, :].repeat(3, 0), -brute["scores_q"]), axis=1)[:, :4]
    assert np.array_equal(brute["hit"], order)
    assert np.array_equal(brute["detail_tm_q"], brute["tm_q"]) and np.array_equal(brute["detail_tm_t"], brute["tm_t"])
    for q in range(3):
        for j, e in enumerate(brute["hit"][q]):
            p, rows = q * 12 + e, len(entries[e])
            assert brute["tm_q"][q, j] == dense["tm_a"][p] and brute["tm_t"][q, j] == dense["tm_b"][p] and brute["rmsd"][q, j] == dense["rmsd"][p]
            assert np.array_equal(brute["rotation"][q, j], dense["rotation"][p]) and np.array_equal(brute["translation"][q, j], dense["translation"][p])
            assert np.array_equal(brute["alignment"][q, j, :rows], dense["alignment"][p, :rows]) and brute["best_init"][q, j] == dense["best_init"][p]
    pruned = ss.search(prot, db, mask, top_k=4, prune=True, details=True, return_scores=True, inits="all")
    for k in ("hit", "tm_q", "tm_t", "rmsd", "n_aligned", "status", "pdb_tm", "rotation", "translation", "alignment", "best_init"):
        assert np.array_equal(pruned[k], brute[k]), k
    ran = (pruned["pair_status"] & ss.PRUNED) == 0
    assert np.array_equal(pruned["scores_q"][ran], brute["scores_q"][ran]) and np.isnan(pruned["scores_q"][~ran]).all()
    default = ss.search(prot, db, mask, top_k=4, prune=False, details=True, return_scores=True)
    assert default["inits"] == "default" and np.array_equal(default["scores_t"], plain["tm_b"].reshape(3, 12))


def test_run_tm_align_with_the_mode_on_a_small_de_novo_set(tmp_path):
    """Three de novo samples of 125 rows (the planted pair and a noisy copy of its second trace; the first has 120 rows set): the mode
    reaches the search, is recorded, and the planted pair scores what ``tm_align`` gives it."""
    fix = _fix()
    rng = np.random.default_rng(5)
    prot = np.zeros((3, 125, 5, 3), dtype=np.float32)
    prot[0, :120], prot[1] = ta.five_atoms(fix["motif03.ca_a"]), ta.five_atoms(fix["motif03.ca_b"])
    prot[2] = ta.five_atoms((fix["motif03.ca_b"] + 0.2 * rng.normal(size=(125, 3))).astype(np.float32))
    res_mask = np.ones((3, 125), dtype=np.float32)
    res_mask[0, 120:] = 0
    records = [{"item": s, "name": "denovo", "sample_i": s} for s in range(3)]
    gathered = {s: {"prot": prot[s], "res_mask": res_mask[s]} for s in range(3)}
    done = run_sharded.run_tm_align(str(tmp_path), records, gathered, inpainting=False, inits="all")
    assert done["inits"] == "all" and json.load(open(tmp_path / "diversity_aligned.json")) == done
    (e,) = done["lengths"]
    assert (e["length"], e["samples"], e["nan_pairs"]) == (125, 3, 0)
    matrix = np.load(tmp_path / "pairwise_tm_score_aligned_length_125.npy")
    want = tm_align.tm_align(prot, mask_a=res_mask, inits="all")["matrix"]
    assert (matrix >= want).all() and matrix[0, 1] == want[0, 1] == _single("motif03")["tm_b"][0]  # (the larger of searched and fixed)
    plain = run_sharded.run_tm_align(str(tmp_path), records, gathered, inpainting=False)
    assert plain["inits"] == "default" and np.load(tmp_path / "pairwise_tm_score_aligned_length_125.npy")[0, 1] <= matrix[0, 1] - 0.1
