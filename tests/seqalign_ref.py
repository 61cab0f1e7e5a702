"""NumPy restatement of the sequence-alignment contract (include/fdipt.h, "sequence alignment"): Gotoh's three
states in int64 half units with the project's tie rule (the first of M, X, Y wins among equals), the path walked back from the end cell,
the map and the counts.  ``align`` fills the states along anti-diagonals with array operations (2048 x 2040 in about a second);
``align_loops`` is the plain triple loop the vectorised fill is checked against; ``brute_force_score`` enumerates every alignment."""
import numpy as np

NEG = -(1 << 30)
X_LETTER = 20


def _boundary(la, lb, o, e):
    st = np.full((3, la + 1, lb + 1), NEG, dtype=np.int64)  # M, X, Y
    st[0, 0, 0] = 0
    st[1, 1:, 0] = o + np.arange(la) * e
    st[2, 0, 1:] = o + np.arange(lb) * e
    return st, np.zeros((3, la + 1, lb + 1), dtype=np.uint8)  # the predecessor state of each state of each cell


def _fill_loops(a, b, table, o, e):
    la, lb = len(a), len(b)
    st, prev = _boundary(la, lb, o, e)
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            t_ab = int(table[a[i - 1], b[j - 1]])
            for s, (pi, pj, add) in enumerate(((i - 1, j - 1, (t_ab, t_ab, t_ab)), (i - 1, j, (o, e, o)), (i, j - 1, (o, o, e)))):
                cand = [int(st[t, pi, pj]) + add[t] for t in range(3)]
                best = 0
                for t in (1, 2):
                    if cand[t] > cand[best]:
                        best = t
                st[s, i, j], prev[s, i, j] = cand[best], best
    return st, prev


def _fill_diagonals(a, b, table, o, e):
    la, lb = len(a), len(b)
    st, prev = _boundary(la, lb, o, e)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    for d in range(2, la + lb + 1):
        i = np.arange(max(1, d - lb), min(la, d - 1) + 1)
        j = d - i
        for s, (pi, pj, add) in enumerate(((i - 1, j - 1, None), (i - 1, j, (o, e, o)), (i, j - 1, (o, o, e)))):
            src = st[:, pi, pj]
            cand = src + table[a[i - 1], b[j - 1]][None, :] if s == 0 else src + np.array(add, dtype=np.int64)[:, None]
            best = np.argmax(cand, axis=0)  # the first of equal maxima
            st[s, i, j], prev[s, i, j] = cand[best, np.arange(len(i))], best
    return st, prev


def _walk(a, b, st, prev):
    la, lb = len(a), len(b)
    end = [int(st[s, la, lb]) for s in range(3)]
    cur = 0
    for s in (1, 2):
        if end[s] > end[cur]:
            cur = s
    score, i, j, path = end[cur], la, lb, []
    m = np.full(lb, -1, dtype=np.int64)
    while i > 0 or j > 0:
        path.append(cur)
        nxt = int(prev[cur, i, j]) if i > 0 and j > 0 else cur  # (row 0 is Y throughout, column 0 is X)
        if cur == 0:
            m[j - 1] = i - 1
            i, j = i - 1, j - 1
        elif cur == 1:
            i -= 1
        else:
            j -= 1
        cur = nxt
    path.reverse()
    return score, path, m


def counts(a, b, path):
    """The integer outputs of a path (states 0 = M, 1 = X: a letter of a against a gap, 2 = Y: a letter of b against a gap)."""
    i = j = aligned = identical = runs = 0
    last = None
    for s in path:
        if s == 0:
            aligned += 1
            identical += int(a[i] == b[j] and a[i] != X_LETTER)
            i, j = i + 1, j + 1
        elif s == 1:
            i += 1
        else:
            j += 1
        runs += int(s != 0 and s != last)
        last = s
    return {"n_aligned": aligned, "n_identical": identical, "n_gaps_a": path.count(2), "n_gaps_b": path.count(1), "n_gap_runs": runs}


def _result(a, b, fill, table, o, e):
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    out = {"score_half": 0, "path": [], "alignment": np.full(len(b), -1, dtype=np.int64), "n_aligned": 0, "n_identical": 0, "n_gaps_a": 0,
           "n_gaps_b": 0, "n_gap_runs": 0}
    if len(a) and len(b):
        score, path, m = _walk(a, b, *fill(a, b, np.asarray(table, dtype=np.int64), int(o), int(e)))
        out.update(score_half=score, path=path, alignment=m, **counts(a, b, path))
    out["score"] = out["score_half"] / 2.0
    return out


def align(a, b, table, o, e):
    """a, b: letters 0 .. 20; table [21,21] and o, e in HALF units.  Returns ``score_half``, ``score``, ``path``, ``alignment`` [len b] and
    the counts; zeros and a map of -1 where a length is 0 (the device's EMPTY)."""
    return _result(a, b, _fill_diagonals, table, o, e)


def align_loops(a, b, table, o, e):
    return _result(a, b, _fill_loops, table, o, e)


def path_score(a, b, path, table, o, e):
    """The score (half units) of a path by the definition: table entries of the aligned pairs, open + (k - 1) extend per gap run."""
    i = j = total = 0
    last = None
    for s in path:
        if s == 0:
            total += int(table[a[i], b[j]])
            i, j = i + 1, j + 1
        else:
            total += e if s == last else o
            i, j = i + (s == 1), j + (s == 2)
        last = s
    return total


def brute_force_score(a, b, table, o, e):
    """The largest ``path_score`` over EVERY alignment of a and b (each a sequence of M, X, Y steps from the corner to the end), by
    enumeration: no recurrence, no maximum before the end."""
    la, lb = len(a), len(b)
    best = [None]

    def go(i, j, last, total):
        if i == la and j == lb:
            if best[0] is None or total > best[0]:
                best[0] = total
            return
        if i < la and j < lb:
            go(i + 1, j + 1, 0, total + int(table[a[i], b[j]]))
        if i < la:
            go(i + 1, j, 1, total + (e if last == 1 else o))
        if j < lb:
            go(i, j + 1, 2, total + (e if last == 2 else o))

    go(0, 0, None, 0)
    return best[0]


def batch(seqs_a, seqs_b, pairs, table, o, e, n_b):
    """The device's outputs for ``pairs`` over lists of sequences: integer arrays [P] and ``alignment`` [P,n_b]."""
    keys = ("score_half", "n_aligned", "n_identical", "n_gaps_a", "n_gaps_b", "n_gap_runs")
    out = {k: np.zeros(len(pairs), dtype=np.int64) for k in keys}
    out["alignment"] = np.full((len(pairs), n_b), -1, dtype=np.int64)
    for p, (ia, ib) in enumerate(pairs):
        r = align(seqs_a[ia], seqs_b[ib], table, o, e)
        for k in keys:
            out[k][p] = r[k]
        out["alignment"][p, :len(seqs_b[ib])] = r["alignment"]
    out["score"] = out["score_half"] / 2.0
    return out
