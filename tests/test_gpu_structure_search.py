"""GPU tests (-m gpu) of the novelty search (framedipt_amd/structure_search.py -> fdipt_structure_search, csrc/structsearch.hip;
DESIGN.md section 7.15): for every query the search returns exactly what a brute force over all entries returns - the NumPy restatement
(tests/search_ref.py on tests/tma_ref.py) and the existing ``tm_align`` on the padded set, both bit for bit - whatever the bucket, with
and without the length bound.  The cases are tests/search_ref.py:case_a: the smallest shapes at which each mechanism can go wrong."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import search_ref as sr
from framedipt_amd import _lib, run_sharded, structure_search as ss, tm_align

pytestmark = pytest.mark.gpu
FLOATS = ("tm_q", "tm_t", "rmsd", "scores_q", "scores_t", "pdb_tm")
EXACT = ("hit", "n_aligned", "status", "pair_status")


def _bits(a, b):
    """Equal bit for bit, NaN where NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@functools.lru_cache(maxsize=None)
def _db():
    _, _, entries, names = sr.case_a()
    return ss.StructureSet.from_arrays(entries, names)


@functools.lru_cache(maxsize=None)
def _brute():
    """Case A without the bound: top 4, every pair's scores, the details."""
    prot, mask, _, _ = sr.case_a()
    return ss.search(prot, _db(), mask, top_k=4, prune=False, details=True, return_scores=True)


@functools.lru_cache(maxsize=None)
def _padded():
    """The parent's capability: ``tm_align`` of every (query, entry) pair against the set padded to its longest entry."""
    prot, mask, entries, _ = sr.case_a()
    longest = max(len(t) for t in entries)
    padded = np.full((len(entries), longest, 5, 3), 7.5, dtype=np.float32)
    padded_mask = np.zeros((len(entries), longest), dtype=np.float32)
    for e, t in enumerate(entries):
        padded[e, :len(t)], padded_mask[e, :len(t)] = sr.ta.five_atoms(t), 1
    pairs = np.array([[q, e] for q in range(len(prot)) for e in range(len(entries))])
    return tm_align.tm_align(prot, padded, mask, padded_mask, pairs=pairs), len(entries)


def test_case_a_equals_the_brute_force_of_the_restatement_bit_for_bit():
    got, want = _brute(), sr.case_a_ref(top_k=4)
    for k in FLOATS + EXACT:
        print(k, "device", np.asarray(got[k]).ravel()[:6], "restatement", np.asarray(want[k]).ravel()[:6])
    for k in FLOATS + EXACT:
        assert _bits(got[k], want[k]), k
    lengths = _db().lengths
    assert got["n_pruned"].tolist() == [0, 0, 0] and got["n_skipped"].tolist() == [0, 0, 0] and got["n_scored"].tolist() == [len(lengths)] * 3
    assert (got["pair_status"][:, 0] == _lib.TMA_TOO_SHORT).all() and (got["pair_status"][:, sr.NAN_ENTRY] == _lib.TMA_NOT_FINITE).all()
    assert ss.novelty_metrics(got, 1) == {"pdbTM": float(got["tm_q"][1, 0]), "hit": got["names"][1][0], "tm_t": float(got["tm_t"][1, 0]),
                                          "n_aligned": int(got["n_aligned"][1, 0])}


def test_the_bucketed_ragged_path_equals_tm_align_on_the_padded_set_bit_for_bit():
    got, (dense, n_db) = _brute(), _padded()
    assert _bits(got["scores_q"], dense["tm_a"].reshape(3, n_db)) and _bits(got["scores_t"], dense["tm_b"].reshape(3, n_db))
    assert _bits(got["pair_status"], dense["status"].reshape(3, n_db))
    for q in range(3):
        for j, e in enumerate(got["hit"][q]):
            p = q * n_db + e
            assert e >= 0 and got["tm_q"][q, j] == dense["tm_a"][p] and got["tm_t"][q, j] == dense["tm_b"][p]
            assert got["rmsd"][q, j] == dense["rmsd"][p] and got["n_aligned"][q, j] == dense["n_aligned"][p]


def test_the_detail_pass_equals_tm_align_and_the_score_pass():
    got, (dense, n_db) = _brute(), _padded()
    lengths = _db().lengths
    assert _bits(got["detail_tm_q"], got["tm_q"]) and _bits(got["detail_tm_t"], got["tm_t"])
    assert got["alignment"].shape == (3, 4, lengths[got["hit"]].max())
    for q in range(3):
        for j, e in enumerate(got["hit"][q]):
            p, rows = q * n_db + e, lengths[e]
            assert _bits(got["rotation"][q, j], dense["rotation"][p]) and _bits(got["translation"][q, j], dense["translation"][p])
            assert _bits(got["alignment"][q, j, :rows], dense["alignment"][p, :rows]) and (got["alignment"][q, j, rows:] == -1).all()
            assert got["best_init"][q, j] == dense["best_init"][p] and got["names"][q][j] == _db().names[e]


def test_duplicates_come_back_lower_index_first_and_the_self_hit_scores_one():
    got = _brute()
    row = got["hit"][1].tolist()
    assert sr.SELF in row and row.index(sr.DUPLICATE) == row.index(sr.SELF) + 1
    j = row.index(sr.SELF)
    assert got["tm_q"][1, j] == 1.0 and got["tm_t"][1, j] == 1.0 and got["tm_q"][1, j + 1] == 1.0 and got["n_aligned"][1, j] == 60
    other = got["hit"][0].tolist()  # the 72-row query sees the two copies as a tie too
    assert other.index(sr.DUPLICATE) == other.index(sr.SELF) + 1


def test_the_length_bound_prunes_what_cannot_enter_and_changes_no_bit():
    """The 60-row query alone, top 1 by the query's length.  The longest buckets run first; after the launch of the bucket that holds
    the query itself the floor is 1.0, and every entry of fewer than 60 rows lies in a later bucket with a bound strictly below it."""
    prot, mask, _, _ = sr.case_a()
    db, lengths = _db(), _db().lengths
    brute = _brute()
    got = ss.search(prot[1:2], db, mask[1:2], top_k=1, rank_by="query", prune=True, details=False, return_scores=True)
    assert got["hit"][0, 0] == brute["hit"][1, 0] and _bits(got["tm_q"][0, 0], brute["tm_q"][1, 0]) and _bits(got["tm_t"][0, 0], brute["tm_t"][1, 0])
    assert got["tm_q"][0, 0] == 1.0 == got["pdb_tm"][0]
    work = ss.plan(lengths, "query")
    caps = work["bucket_cap"].tolist()
    own = caps.index(ss.BUCKET_CAPS[work["bucket_of"][sr.SELF]])
    later = {int(e) for b in range(own + 1, len(caps)) for e in work["entries"][work["bucket_start"][b]:work["bucket_start"][b + 1]]}
    valid_short = {e for e, n in enumerate(lengths) if 5 <= n < 60}
    assert valid_short <= later  # (known from the plan alone)
    pruned = (got["pair_status"][0] & ss.PRUNED) != 0
    print("n_pruned", got["n_pruned"], "valid entries of fewer than 60 rows", len(valid_short))
    assert got["n_pruned"].tolist() == [len(valid_short)] == [11] and set(np.flatnonzero(pruned)) == valid_short
    assert not pruned[lengths >= 60].any() and got["pair_status"][0, 0] == _lib.TMA_TOO_SHORT  # (strict: a bound of 1.0 is not below the floor)
    assert np.isnan(got["scores_q"][0, pruned]).all() and _bits(got["scores_q"][0, ~pruned], brute["scores_q"][1, ~pruned])
    assert got["n_scored"].tolist() == [len(lengths) - 11] and got["n_skipped"].tolist() == [0] and "rotation" not in got


def test_the_bound_by_the_entry_length_equals_the_brute_force():
    prot, mask, _, _ = sr.case_a()
    want = sr.case_a_ref(top_k=2, rank_by="target")
    for prune in (False, True):
        got = ss.search(prot, _db(), mask, top_k=2, rank_by="target", prune=prune, details=False)
        for k in ("hit", "tm_q", "tm_t", "rmsd", "n_aligned", "status", "pdb_tm"):
            assert _bits(got[k], want[k]), (k, prune)
        print("rank_by target, prune", prune, "n_pruned", got["n_pruned"])
        # the 60-row query holds its two copies (tm_t = 1.0) after the bucket of cap 64: the entries of 70 and 130 rows run later, bound below 1
        assert got["n_pruned"][1] == 2 if prune else not got["n_pruned"].any()


def test_min_score_and_a_top_k_beyond_the_set():
    prot, mask, _, _ = sr.case_a()
    want = sr.case_a_ref(top_k=8, min_score=0.5)
    got = ss.search(prot, _db(), mask, top_k=8, min_score=0.5)
    for k in ("hit", "tm_q", "tm_t", "rmsd", "n_aligned", "status", "pdb_tm"):
        assert _bits(got[k], want[k]), k
    assert ((got["tm_q"] >= 0.5) == (got["hit"] >= 0)).all() and (got["hit"][2] == -1).all() and np.isnan(got["pdb_tm"][2])
    assert got["names"][2] == [None] * 8 and np.isnan(got["detail_tm_q"][2]).all() and (got["alignment"][2] == -1).all()
    assert _bits(got["detail_tm_q"], got["tm_q"]) and _bits(got["detail_tm_t"], got["tm_t"])
    wide, ref = ss.search(prot, _db(), mask, top_k=64, prune=False, details=False), sr.case_a_ref(top_k=64)
    assert _bits(wide["hit"], ref["hit"]) and _bits(wide["tm_q"], ref["tm_q"]) and ((wide["hit"] >= 0).sum(1) == 14).all()


def test_an_atom37_device_tensor_is_used_in_place_and_equals_the_numpy_path():
    prot, mask, _, _ = sr.case_a()
    wide = np.zeros((3, 72, 37, 3), dtype=np.float32)
    wide[:, :, :5] = prot
    tensor = torch.from_numpy(wide).cuda()
    before = tensor.clone()
    got, base = ss.search(tensor, _db(), torch.from_numpy(mask).cuda(), top_k=4, prune=False, return_scores=True), _brute()
    assert torch.equal(tensor, before)
    for k in FLOATS + EXACT + ("rotation", "translation", "alignment", "best_init", "n_scored"):
        assert _bits(got[k], base[k]), k


def test_an_entry_beyond_the_row_limit_is_skipped_and_counted():
    prot, mask, entries, _ = sr.case_a()
    long = np.cumsum(np.random.default_rng(2).normal(size=(ss.MAX_ROWS + 1, 3)) * 2.2, axis=0).astype(np.float32)
    db = ss.StructureSet.from_arrays([entries[sr.SELF], long, entries[9]])
    got = ss.search(prot[1:2], db, mask[1:2], top_k=3, return_scores=True)
    assert got["hit"].tolist() == [[0, 2, -1]] and got["n_skipped"].tolist() == [1] and got["pair_status"][0].tolist() == [0, ss.TOO_LONG, 0]
    assert np.isnan(got["scores_q"][0, 1]) and _bits(got["tm_q"][0, :2], _brute()["scores_q"][1, [sr.SELF, 9]])
    only = ss.search(prot[1:2], ss.StructureSet.from_arrays([long]), mask[1:2])  # no launch of the score pass at all
    assert only["hit"].tolist() == [[-1]] and only["n_skipped"].tolist() == [1] and only["n_scored"].tolist() == [0] and only["alignment"].shape == (1, 1, 0)


def test_refusals_before_any_launch():
    prot, mask, _, _ = sr.case_a()
    db = _db()
    for bad in (dict(top_k=0), dict(top_k=65), dict(rank_by="length")):
        with pytest.raises(ValueError):
            ss.search(prot, db, mask, **bad)
    with pytest.raises(ValueError, match="empty"):
        ss.search(prot, ss.StructureSet.from_arrays([]), mask)
    with pytest.raises(_lib.FdiptError, match="ESIZE"):
        ss.search(np.zeros((1, ss.MAX_ROWS + 1, 5, 3), dtype=np.float32), db)
    # the entry itself
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    names = [n for n, _ in _lib.SearchArgs._fields_ if n not in ("Q", "N_q", "atoms", "ca", "D", "top_k", "rank_by", "prune", "details", "n_buckets", "detail_cap", "R",
                                                                 "min_score", "bucket_start", "bucket_cap", "workspace", "workspace_bytes")]
    bufs = {k: torch.zeros(4096, dtype=torch.float64, device=dev) for k in names + ["workspace"]}
    start, cap = np.array([0, 1], dtype=np.int32), np.array([16], dtype=np.int32)

    def call(**change):
        fields = dict(Q=1, N_q=9, atoms=5, ca=1, D=1, top_k=1, rank_by=0, prune=1, details=1, n_buckets=1, detail_cap=16, R=9, min_score=0.0,
                      bucket_start=start.ctypes.data_as(C.c_void_p), bucket_cap=cap.ctypes.data_as(C.c_void_p), workspace_bytes=4096 * 8,
                      **{k: _lib.ptr(v) for k, v in bufs.items()})
        fields.update(change)
        return lib.fdipt_structure_search(C.byref(_lib.SearchArgs(**fields)), _lib.stream_ptr())

    assert call(top_k=0) == _lib.EINVAL and call(top_k=65) == _lib.EINVAL and call(rank_by=2) == _lib.EINVAL and call(D=0) == _lib.EINVAL
    assert call(hit=None) == _lib.EINVAL and call(rotation=None) == _lib.EINVAL and call(atoms=4) == _lib.EINVAL and call(detail_cap=513) == _lib.EINVAL
    wrong = np.array([600], dtype=np.int32)
    assert call(bucket_cap=wrong.ctypes.data_as(C.c_void_p)) == _lib.EINVAL and call(plan_entries=None) == _lib.EINVAL
    assert call(N_q=513) == _lib.ESIZE and call(workspace_bytes=8) == _lib.ESIZE
    assert lib.fdipt_structure_search_workspace(3, 4, 0) == 8 * (12 + 3) and lib.fdipt_structure_search_workspace(3, 4, 1) > 8 * 15


def test_run_novelty_writes_what_search_returns(tmp_path):
    """``run_sharded --novelty`` on one rank: two samples of 48 rows against a set of five entries; the files hold the numbers of a
    direct call on the written samples.  Inpainting runs are refused."""
    import os
    import subprocess
    import sys

    from conftest import ROOT
    prot, mask, entries, _ = sr.case_a()
    db = ss.StructureSet.from_arrays([entries[k] for k in (9, 10, 11, 12, sr.SELF)], names=["a", "b", "c", "d", "e"])
    db.save(tmp_path / "set.npz")
    out_dir = tmp_path / "run"
    cmd = [sys.executable, "-m", "framedipt_amd.run_sharded", "--out-dir", str(out_dir), "--num-t", "2", "--max-batch", "4", "--keep", "last", "--min-length", "48",
           "--max-length", "48", "--length-step", "5", "--samples-per-length", "2", "--precision", "fp32", "--novelty", str(tmp_path / "set.npz")]
    r = subprocess.run(cmd, env=dict(os.environ, FDIPT_SHARED_GPU="allow"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (out_dir / "novelty.json").exists() and (out_dir / "novelty.csv").exists()
    with open(out_dir / "novelty.json") as f:
        summary = json.load(f)
    with open(out_dir / "manifest.json") as f:
        records = json.load(f)["samples"]
    assert summary["entries"] == 5 and summary["top_k"] == 1 and "sample itself" in summary["query"] and "foldseek" in summary["search"]
    assert [(s["length"], s["sample"]) for s in summary["samples"]] == [(48, 0), (48, 1)] and summary["skipped_lengths"] == []
    samples = np.stack([np.load(out_dir / rec["file"])["prot_traj"] for rec in records])
    assert samples.shape == (2, 48, 37, 3)
    direct = ss.search(samples.astype(np.float32), db)
    lines = (out_dir / "novelty.csv").read_text().split()
    assert lines[0] == "length,sample,pdbTM,hit" and len(lines) == 3
    for q, s in enumerate(summary["samples"]):
        assert s["pdbTM"] == float(direct["pdb_tm"][q]) == float(direct["tm_q"][q, 0]) and s["hit"] == direct["names"][q][0] and s["tm_t"] == float(direct["tm_t"][q, 0])
        assert s["n_aligned"] == int(direct["n_aligned"][q, 0]) and s["n_scored"] + s["n_pruned"] + s["n_skipped"] == 5
        assert lines[1 + q] == f"48,{q},{s['pdbTM']!r},{s['hit']}"
    gathered = {q: {"prot": samples[q]} for q in range(2)}
    again = run_sharded.run_novelty(str(tmp_path), [{"item": q, "name": "length_48", "sample_i": q} for q in range(2)], gathered, tmp_path / "set.npz", top_k=2)
    assert [s["pdbTM"] for s in again["samples"]] == [s["pdbTM"] for s in summary["samples"]] and len(again["samples"][0]["hits"]) == 2
    with pytest.raises(ValueError, match="de novo"):
        run_sharded.run_novelty(str(tmp_path), [], {}, tmp_path / "set.npz", inpainting=True)
