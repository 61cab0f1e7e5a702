"""NumPy restatement of the local and semi-global modes of sequence alignment (include/fdipt.h, "sequence
alignment: modes").  Units, table, penalties, the three states and the tie rule inside a cell are those of tests/seqalign_ref.py, which
this file imports for the global case and does not change.

``align`` fills the states along anti-diagonals with array operations, ``align_loops`` is the plain triple loop it is checked against,
``brute_force_score`` enumerates paths (and, for the local mode, substrings) by the DEFINITIONS - no recurrence, no maximum before the
end -, and ``path_score`` scores a charged path over its span by the global rule."""
import numpy as np

import seqalign_ref as gref

NEG = gref.NEG
GLOBAL, SEMIGLOBAL, LOCAL = 0, 1, 2
A_LEFT, A_RIGHT, B_LEFT, B_RIGHT = 1, 2, 4, 8
EMPTY, NO_ALIGNED = 1, 8
FRESH = 3  # M's predecessor code of a local fresh start
path_score = gref.path_score


def _boundary(la, lb, o, e, mode, free):
    st = np.full((3, la + 1, lb + 1), NEG, dtype=np.int64)  # M, X, Y
    prev = np.zeros((3, la + 1, lb + 1), dtype=np.uint8)
    if mode == LOCAL:
        return st, prev  # no boundary scores
    st[0, 0, 0] = 0
    if free & A_LEFT:
        st[0, 1:, 0] = 0  # corners
    else:
        st[1, 1:, 0] = o + np.arange(la) * e
    if free & B_LEFT:
        st[0, 0, 1:] = 0
    else:
        st[2, 0, 1:] = o + np.arange(lb) * e
    return st, prev


def _fill_loops(a, b, table, o, e, mode, free):
    la, lb = len(a), len(b)
    st, prev = _boundary(la, lb, o, e, mode, free)
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            t_ab = int(table[a[i - 1], b[j - 1]])
            for s, (pi, pj, add) in enumerate(((i - 1, j - 1, (0, 0, 0)), (i - 1, j, (o, e, o)), (i, j - 1, (o, o, e)))):
                cand = [int(st[t, pi, pj]) + add[t] for t in range(3)]
                best = 0
                for t in (1, 2):
                    if cand[t] > cand[best]:
                        best = t
                value = cand[best]
                if s == 0:
                    if mode == LOCAL and value <= 0:  # the fresh start wins the tie
                        value, best = 0, FRESH
                    value += t_ab
                st[s, i, j], prev[s, i, j] = value, best
    return st, prev


def _fill_diagonals(a, b, table, o, e, mode, free):
    la, lb = len(a), len(b)
    st, prev = _boundary(la, lb, o, e, mode, free)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    for d in range(2, la + lb + 1):
        i = np.arange(max(1, d - lb), min(la, d - 1) + 1)
        j = d - i
        for s, (pi, pj, add) in enumerate(((i - 1, j - 1, (0, 0, 0)), (i - 1, j, (o, e, o)), (i, j - 1, (o, o, e)))):
            cand = st[:, pi, pj] + np.array(add, dtype=np.int64)[:, None]
            best = np.argmax(cand, axis=0)  # the first of equal maxima
            value = cand[best, np.arange(len(i))]
            if s == 0:
                if mode == LOCAL:
                    fresh = value <= 0
                    value, best = np.where(fresh, 0, value), np.where(fresh, FRESH, best)
                value = value + table[a[i - 1], b[j - 1]]
            st[s, i, j], prev[s, i, j] = value, best
    return st, prev


def _end_cell(st, la, lb, mode, free):
    """(score, i, j, state) of the end cell, or None for the empty local result."""
    if mode == LOCAL:
        m = st[0, 1:, 1:]
        top = int(m.max())
        i, j = np.nonzero(m == top)  # score descending, then i + j ascending, then i ascending (np.nonzero lists i ascending)
        k = np.flatnonzero(i + j == (i + j).min())[0]
        return (top, int(i[k]) + 1, int(j[k]) + 1, 0) if top > 0 else None
    cells = [(la, lb)] + [(i, lb) for i in range(la) if free & A_RIGHT] + [(la, j) for j in range(lb) if free & B_RIGHT]
    best = None
    for i, j in cells:
        for s in range(3):
            key = (int(st[s, i, j]), i + j, i, -s)  # score, i + j and i descending, then the first of M, X, Y
            if best is None or key > best[0]:
                best = (key, i, j, s)
    return best[0][0], best[1], best[2], best[3]


def _walk(st, prev, end, lb, mode, free):
    """The charged path from the end cell back to its origin: (path, map [lb], (begin_a, begin_b))."""
    _, i, j, cur = end
    path, m = [], np.full(lb, -1, dtype=np.int64)
    while i > 0 or j > 0:
        if i == 0 or j == 0:
            if mode != LOCAL and ((j == 0 and free & A_LEFT) or (i == 0 and free & B_LEFT)):
                break  # a corner: the origin
            cur = nxt = 1 if j == 0 else 2  # a leading gap that is not free is walked and counted
        else:
            nxt = int(prev[cur, i, j])
        path.append(cur)
        if cur == 0:
            m[j - 1] = i - 1
            i, j = i - 1, j - 1
        elif cur == 1:
            i -= 1
        else:
            j -= 1
        if nxt == FRESH:
            break
        cur = nxt
    path.reverse()
    return path, m, (i, j)


def _result(a, b, fill, table, o, e, mode, free):
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    if mode not in (GLOBAL, SEMIGLOBAL, LOCAL) or not 0 <= free <= 15 or (free and mode != SEMIGLOBAL):
        raise ValueError((mode, free))
    out = {"score_half": 0, "path": [], "alignment": np.full(len(b), -1, dtype=np.int64), "n_aligned": 0, "n_identical": 0, "n_gaps_a": 0,
           "n_gaps_b": 0, "n_gap_runs": 0, "begin_a": 0, "end_a": 0, "begin_b": 0, "end_b": 0, "status": EMPTY}
    if len(a) and len(b):
        out["status"] = NO_ALIGNED
        st, prev = fill(a, b, np.asarray(table, dtype=np.int64), int(o), int(e), mode, free)
        end = _end_cell(st, len(a), len(b), mode, free)
        if end is not None:
            path, m, (bi, bj) = _walk(st, prev, end, len(b), mode, free)
            out.update(score_half=end[0], path=path, alignment=m, begin_a=bi, end_a=end[1], begin_b=bj, end_b=end[2],
                       **gref.counts(a[bi:], b[bj:], path))
            out["status"] = 0 if out["n_aligned"] else NO_ALIGNED
    out["score"] = out["score_half"] / 2.0
    return out


def align(a, b, table, o, e, mode=SEMIGLOBAL, free_ends=0):
    """a, b: letters 0 .. 20; table [21,21] and o, e in HALF units; mode GLOBAL (= SEMIGLOBAL without a flag), SEMIGLOBAL with the
    ``free_ends`` bits, or LOCAL.  Returns ``score_half``, ``score``, the charged ``path``, ``alignment`` [len b], the counts, the span
    ``begin_a``, ``end_a``, ``begin_b``, ``end_b`` and ``status`` (EMPTY for a length of 0, NO_ALIGNED for no aligned column)."""
    return _result(a, b, _fill_diagonals, table, o, e, mode, free_ends)


def align_loops(a, b, table, o, e, mode=SEMIGLOBAL, free_ends=0):
    return _result(a, b, _fill_loops, table, o, e, mode, free_ends)


def _paths(a, b, i0, j0, table):
    """Every path of M / X / Y steps from (i0, j0), as (i, j, steps, table sum) at EVERY cell it passes, the start included."""
    la, lb = len(a), len(b)
    stack = [(i0, j0, (), 0)]
    while stack:
        i, j, steps, total = stack.pop()
        yield i, j, steps, total
        if i < la and j < lb:
            stack.append((i + 1, j + 1, steps + (0,), total + int(table[a[i], b[j]])))
        if i < la:
            stack.append((i + 1, j, steps + (1,), total))
        if j < lb:
            stack.append((i, j + 1, steps + (2,), total))


def _runs(steps):
    runs = []
    for s in steps:
        if runs and runs[-1][0] == s:
            runs[-1][1] += 1
        else:
            runs.append([s, 1])
    return runs


def brute_force_score(a, b, table, o, e, mode=SEMIGLOBAL, free_ends=0):
    """The best score by the definitions.  SEMIGLOBAL (GLOBAL: no flag): every path from the corner to the end, each gap run charged
    open + (k - 1) extend except a first run that is X with A_LEFT or Y with B_LEFT and a last run that is X with A_RIGHT or Y with
    B_RIGHT.  LOCAL: every pair of substrings and every path between their corners that starts and ends with M, or the empty
    alignment with score 0."""
    la, lb = len(a), len(b)
    if mode == LOCAL:
        best = 0
        for i0 in range(la):
            for j0 in range(lb):
                for _, _, steps, total in _paths(a, b, i0, j0, table):
                    if steps and steps[0] == 0 and steps[-1] == 0:
                        best = max(best, total + sum(o + (k - 1) * e for s, k in _runs(steps) if s))
        return best
    best = None
    for i, j, steps, total in _paths(a, b, 0, 0, table):
        if (i, j) != (la, lb):
            continue
        runs = _runs(steps)
        for n, (s, k) in enumerate(runs):
            first_free = n == 0 and ((s == 1 and free_ends & A_LEFT) or (s == 2 and free_ends & B_LEFT))
            last_free = n == len(runs) - 1 and ((s == 1 and free_ends & A_RIGHT) or (s == 2 and free_ends & B_RIGHT))
            if s and not first_free and not last_free:
                total += o + (k - 1) * e
        best = total if best is None or total > best else best
    return best


KEYS = ("score_half", "n_aligned", "n_identical", "n_gaps_a", "n_gaps_b", "n_gap_runs", "begin_a", "end_a", "begin_b", "end_b", "status")


def batch(seqs_a, seqs_b, pairs, table, o, e, n_b, mode=SEMIGLOBAL, free_ends=0):
    """The device's outputs for ``pairs`` over lists of sequences: integer arrays [P] and ``alignment`` [P,n_b]."""
    out = {k: np.zeros(len(pairs), dtype=np.int64) for k in KEYS}
    out["alignment"] = np.full((len(pairs), n_b), -1, dtype=np.int64)
    for p, (ia, ib) in enumerate(pairs):
        r = align(seqs_a[ia], seqs_b[ib], table, o, e, mode, free_ends)
        for k in KEYS:
            out[k][p] = r[k]
        out["alignment"][p, :len(seqs_b[ib])] = r["alignment"]
    out["score"] = out["score_half"] / 2.0
    return out
