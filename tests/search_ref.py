"""The brute force the novelty search (framedipt_amd/structure_search.py) must equal: every (query, entry) pair
scored by the NumPy restatement of the alignment search (tests/tma_ref.py, imported, not edited), the pairs sorted by the order rule
(ranked score descending, entry index ascending, NaN never ranks), ``min_score`` and ``top_k`` applied.  It never prunes.  A pair's
result is computed once per process and shared (``pair``), so the host tests and the GPU tests pay for the restatement once.  The
cases of the tests are at the end."""
from __future__ import annotations

import functools

import numpy as np

import tma_ref as ta
from conftest import load_golden

MAX_ROWS = ta.MAX_ROWS
PRUNED, TOO_LONG = 16, 32
_PAIRS: dict = {}


def pair(x, y) -> dict:
    """``tma_ref.tm_align`` of the compacted traces x (query) and y (entry), computed once per distinct pair of arrays."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    key = (x.tobytes(), y.tobytes())
    if key not in _PAIRS:
        _PAIRS[key] = ta.tm_align(x, y)
    return _PAIRS[key]


def bound(n1: int, n2: int, rank_by: str = "query") -> float:
    """A score is a sum of at most min(n1, n2) terms of at most 1 over the normalisation length."""
    return float(min(n1, n2)) / float(n2 if rank_by == "target" else n1)


def search_ref(queries, entries, top_k=1, rank_by="query", min_score=0.0) -> dict:
    """queries: compacted CA traces [n1,3]; entries: CA traces [n2,3] (an entry beyond MAX_ROWS rows is skipped: TOO_LONG).  The
    outputs of ``search(..., return_scores=True)`` without the detail pass."""
    n_q, n_db = len(queries), len(entries)
    out = {"scores_q": np.full((n_q, n_db), np.nan), "scores_t": np.full((n_q, n_db), np.nan), "pair_status": np.zeros((n_q, n_db), dtype=np.int64),
           "pair_n_aligned": np.zeros((n_q, n_db), dtype=np.int64), "pair_rmsd": np.full((n_q, n_db), np.nan),
           "hit": np.full((n_q, top_k), -1, dtype=np.int64), "tm_q": np.full((n_q, top_k), np.nan), "tm_t": np.full((n_q, top_k), np.nan),
           "n_aligned": np.zeros((n_q, top_k), dtype=np.int64), "rmsd": np.full((n_q, top_k), np.nan), "status": np.zeros((n_q, top_k), dtype=np.int64),
           "pdb_tm": np.full(n_q, np.nan), "n_skipped": np.zeros(n_q, dtype=np.int64)}
    for q, x in enumerate(queries):
        for e, y in enumerate(entries):
            if len(y) > MAX_ROWS:
                out["pair_status"][q, e] = TOO_LONG
                out["n_skipped"][q] += 1
                continue
            got = pair(x, y)
            out["scores_q"][q, e], out["scores_t"][q, e], out["pair_status"][q, e] = got["tm_a"], got["tm_b"], got["status"]
            out["pair_n_aligned"][q, e], out["pair_rmsd"][q, e] = got["n_aligned"], got["rmsd"]
        ranked = out["scores_t" if rank_by == "target" else "scores_q"][q]
        order = sorted((e for e in range(n_db) if ranked[e] >= min_score), key=lambda e: (-ranked[e], e))[:top_k]  # (NaN >= x is False)
        for j, e in enumerate(order):
            out["hit"][q, j], out["tm_q"][q, j], out["tm_t"][q, j] = e, out["scores_q"][q, e], out["scores_t"][q, e]
            out["n_aligned"][q, j], out["rmsd"][q, j], out["status"][q, j] = out["pair_n_aligned"][q, e], out["pair_rmsd"][q, e], out["pair_status"][q, e]
        if order:
            out["pdb_tm"][q] = ranked[order[0]]
    return out


# ------------------------------------------------------------------------------------------------------ the cases of the tests
SELF, DUPLICATE = 13, 14  # entries of case A: the 60-row query itself, and again
NAN_ENTRY = 15


@functools.lru_cache(maxsize=None)
def case_a():
    """(prot [3,72,5,3] float32, mask [3,72] float32, entries: a list of [n,3] float32, names).  The queries are 72-row windows of the
    recorded TCR variable domains (tests/golden/tma_cases.npz) with 72, 60 and 41 rows set, the third with masked rows in the middle.
    Entries: 4 rows (TOO_SHORT), 5, 19 .. 22 (the edges of the d0 and d0s formulas), cap - 1, cap, cap + 1 of the two smallest bucket
    caps (16, 32), 130 rows, the 60-row query itself and again (a tie), and 70 rows with a NaN coordinate."""
    from framedipt_amd import structure_search
    fix = load_golden("tma_cases.npz")
    a, b, long = fix["tcr130.ca_a"].astype(np.float32), fix["tcr130.ca_b"].astype(np.float32), fix["shift4_300.ca_a"].astype(np.float32)
    prot = np.stack([ta.five_atoms(a[20:92]), ta.five_atoms(b[10:82]), ta.five_atoms(long[100:172])]).astype(np.float32)
    mask = np.ones((3, 72), dtype=np.float32)
    mask[1, 60:] = 0
    mask[2, 8:30] = 0
    mask[2, 63:] = 0
    assert mask.sum(1).tolist() == [72, 60, 41]
    c0, c1 = structure_search.BUCKET_CAPS[:2]
    entries, start = [], 0
    for n in (4, 5, 19, 20, 21, 22, c0 - 1, c0, c0 + 1, c1 - 1, c1, c1 + 1):
        source = (a, b, long)[len(entries) % 3]
        entries.append(source[start % 40:start % 40 + n].copy())
        start += 7
    entries.append(b.copy())                   # 130 rows: holds query 1's window
    assert len(entries) == SELF
    own = prot[1, mask[1] != 0, 1].copy()      # the 60-row query itself
    entries += [own, own.copy()]
    bad = long[200:270].copy()
    bad[31, 1] = np.nan
    entries.append(bad)
    assert len(entries) == NAN_ENTRY + 1
    return prot, mask, entries, [f"e{k}_{len(t)}" for k, t in enumerate(entries)]


def case_a_queries():
    """The compacted float64 traces of case A's queries, as the restatement takes them."""
    prot, mask, _, _ = case_a()
    return [ta.compact(prot[q], mask[q])[0] for q in range(len(prot))]


def case_a_ref(top_k=4, rank_by="query", min_score=0.0):
    _, _, entries, _ = case_a()
    return search_ref(case_a_queries(), entries, top_k, rank_by, min_score)
