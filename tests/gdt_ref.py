"""NumPy restatement of the GDT contract (include/fdipt.h, "GDT-TS / GDT-HA"), written in the evaluation order of
framedipt_amd/csrc/gdt.hip: the search vectorised over the work items and serial over the rows, on the superposition and distance
primitives of the TM-score restatement (tests/tm_ref.py: every sum over rows is a ``cumsum``, which adds in index order as the
device's row walk does).  ``gdt`` returns every output of the device for one pair and, for the fixture generator, ``margin``: the
smallest distance in Angstrom between any |T x_i - y_i| and a threshold it was compared with (the five cutoffs in every pass of every
item, every selection cut tried).  Helpers for the cases of tests/golden/gdt_cases.npz are at the end."""
from __future__ import annotations

import numpy as np

import tm_ref as tr

CUTOFFS = (0.5, 1.0, 2.0, 4.0, 8.0)
MODES = ("none", "global", "search")
MAX_PASSES, CUT_LIMIT = tr.MAX_PASSES, tr.CUT_LIMIT
TOO_SHORT, SKIPPED, NOT_FINITE = 1, 2, 4
CASES = ("n1", "n2", "n3", "n4", "n5", "n9", "n37", "n64", "n65", "n130", "masked", "planted", "hinge", "exact", "unrelated", "n1024", "nan")
CHUNK = 2048  # items of the search evaluated at once (memory of the restatement only: the result does not depend on it)
C2 = np.array([c * c for c in CUTOFFS])

compact = tr.compact
five_atoms = tr.five_atoms


def _margin(d2, thresholds, skip_exact=False):
    """The smallest | |d| - threshold | over d2 [..., n] and the thresholds; ``skip_exact``: distances that equal a threshold in float64
    are decided by ``<=`` itself and do not count."""
    d = np.sqrt(d2)
    best = np.inf
    for c in np.unique(np.asarray(thresholds, dtype=np.float64)):
        gap = np.abs(d - c)
        if skip_exact:
            gap = np.where(d2 == c * c, np.inf, gap)
        if gap.size:
            best = min(best, float(np.nanmin(gap)))
    return best


def counts_under(rotation, translation, x, y):
    """[5] int64: the rows within each cutoff under one transform (what the tests recount from the device's transforms)."""
    d2 = tr.dist2(np.asarray(rotation, dtype=np.float64).reshape(1, 9), np.asarray(translation, dtype=np.float64).reshape(1, 3), x, y)[0]
    return (d2[None, :] <= C2[:, None]).sum(1).astype(np.int64)


def _search(x, y):
    """The winners of the five cutoffs over every pass of every item: (count [5], item [5], pass [5], r [5,9], t [5,3], passes, margin,
    widened: the passes in which the cut grew)."""
    n = x.shape[0]
    frag, start = tr.seeds(n)
    n_seeds = len(frag)
    rows = np.arange(n)[None, :]
    b_cnt, b_item, b_pass = np.full(5, -1, dtype=np.int64), np.full(5, np.iinfo(np.int64).max), np.zeros(5, dtype=np.int64)
    b_r, b_t = np.zeros((5, 9)), np.zeros((5, 3))
    passes, margin, widened = 0, np.inf, 0
    for lo in range(0, 5 * n_seeds, CHUNK):
        item = np.arange(lo, min(lo + CHUNK, 5 * n_seeds))
        seed, k = item % n_seeds, item // n_seeds
        sel = (rows >= start[seed][:, None]) & (rows < (start[seed] + frag[seed])[:, None])
        cut0 = np.array(CUTOFFS)[k]
        active = np.ones(len(item), dtype=bool)
        for it in range(MAX_PASSES):
            idx = np.flatnonzero(active)
            r, t = tr.superpose(sel[idx], x, y)
            d2 = tr.dist2(r, t, x, y)
            passes += len(idx)
            cnt = (d2[:, None, :] <= C2[None, :, None]).sum(2)
            margin = min(margin, _margin(d2, CUTOFFS))
            cut = cut0[idx].copy()
            inside = d2 < (cut * cut)[:, None]
            widened += int(((inside.sum(1) < 3) & (n > 3)).sum())
            while True:
                need = (inside.sum(1) < 3) & (n > 3) & (cut < CUT_LIMIT)
                if not need.any():
                    break
                cut[need] += 0.5
                inside[need] = d2[need] < (cut[need] * cut[need])[:, None]
                margin = min(margin, float(np.min(np.abs(np.sqrt(d2[need]) - cut[need][:, None]))))
            for j in range(5):  # the largest count, the lowest item among equals, its earliest pass
                w = int(np.argmax(cnt[:, j]))
                if cnt[w, j] > b_cnt[j] or (cnt[w, j] == b_cnt[j] and item[idx[w]] < b_item[j]):
                    b_cnt[j], b_item[j], b_pass[j], b_r[j], b_t[j] = cnt[w, j], item[idx[w]], it, r[w], t[w]
            done = (inside == sel[idx]).all(1) | (it == MAX_PASSES - 1)
            sel[idx] = inside
            active[idx[done]] = False
            if not active.any():
                break
    return b_cnt, b_item, b_pass, b_r, b_t, passes, margin, widened


def gdt(x, y, mode="search", norm=None) -> dict:
    """x, y [n,3] float64, the compacted CA traces of a pair (model, reference).  Returns the device's outputs of the pair -
    ``res_within`` over the n compacted rows - and ``margin``."""
    assert mode in MODES
    x, y = np.asarray(x, dtype=np.float64).reshape(-1, 3), np.asarray(y, dtype=np.float64).reshape(-1, 3)
    n = x.shape[0]
    length = int(norm) if norm is not None and int(norm) > 0 else n
    out = {"gdt_ts": np.nan, "gdt_ha": np.nan, "counts": np.zeros(5, dtype=np.int64), "n_scored": n, "rotation": np.tile(np.eye(3), (5, 1, 1)),
           "translation": np.zeros((5, 3)), "best_item": np.full(5, -1, dtype=np.int64), "best_pass": np.full(5, -1, dtype=np.int64), "passes": 0,
           "res_within": np.zeros(n, dtype=np.int32), "status": 0, "length": length, "margin": np.inf}
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return {**out, "status": NOT_FINITE}
    if n < (1 if mode == "none" else 3):
        return {**out, "status": TOO_SHORT}
    with np.errstate(all="ignore"):
        if mode == "search":
            cnt, item, pas, r, t, passes, margin, widened = _search(x, y)
            out.update(counts=cnt, best_item=item, best_pass=pas, passes=passes, margin=margin, widened=widened)
        else:
            if mode == "global":
                r, t = tr.superpose(np.ones((1, n), dtype=bool), x, y)
                out["passes"] = 1
            else:
                r, t = np.eye(3).reshape(1, 9), np.zeros((1, 3))
            r, t = np.repeat(r, 5, axis=0), np.repeat(t, 5, axis=0)
            out["counts"] = counts_under(r[0], t[0], x, y)
            out["margin"] = _margin(tr.dist2(r[:1], t[:1], x, y), CUTOFFS, skip_exact=mode == "none")
        d2 = tr.dist2(r, t, x, y)  # [5,n]: row i under cutoff j's transform
    out["res_within"] = ((d2 <= C2[:, None]) * (1 << np.arange(5))[:, None]).sum(0).astype(np.int32)
    c = [int(v) for v in out["counts"]]
    out.update(rotation=r.reshape(5, 3, 3), translation=t, gdt_ts=(c[1] + c[2] + c[3] + c[4]) / (4.0 * length), gdt_ha=(c[0] + c[1] + c[2] + c[3]) / (4.0 * length))
    return out


# ---------------------------------------------------------------------------------------------- the fixture's cases
INT_OUTPUTS = ("counts", "n_scored", "best_item", "best_pass", "passes", "res_within", "status")
RECORDED = ("gdt_ts", "gdt_ha", "rotation", "translation") + INT_OUTPUTS


def case_inputs(fix, name):
    """(prot_a [N,5,3] f32, prot_b [N,5,3] f32, mask_a [N], mask_b [N], norm_length or None) of a recorded case."""
    norm = int(fix[f"{name}.norm_length"])
    return five_atoms(fix[f"{name}.ca_a"]), five_atoms(fix[f"{name}.ca_b"]), fix[f"{name}.mask_a"], fix[f"{name}.mask_b"], (norm if norm > 0 else None)


def scored_rows(mask_a, mask_b):
    return np.flatnonzero((np.asarray(mask_a) != 0) & (np.asarray(mask_b) != 0))


def spread(res_within, rows, n_rows):
    """``res_within`` of the compacted rows as the device reports it: [N] int32, 0 at the rows that are not scored."""
    out = np.zeros(n_rows, dtype=np.int32)
    out[rows] = res_within
    return out
