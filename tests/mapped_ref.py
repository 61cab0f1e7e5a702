"""NumPy restatement of the mapped accuracy contract (include/fdipt.h, "accuracy through a row map"): gather the
model's rows through the map, then the restatements of the un-mapped entries (tests/lddt_ref.py, tests/gdt_ref.py).  The penalise rule is
written out with its integer counts, and ``far_points`` is the construction the contract names as its oracle: the gathered model with
every absent atom at a far, distinct point and marked present.
"""
from __future__ import annotations

import numpy as np

import gdt_ref as gr
import lddt_ref as lr
from mapped_cases import FAR

OUT_OF_RANGE, DUPLICATE = 8, 16
LDDT_INTS = ("n_scored", "n_passed")


def covered_rows(m, n_a, res_mask_a=None, res_mask_b=None):
    """[N_b] bool: the reference row exists, its entry is a model row, and that row exists."""
    m = np.asarray(m)
    exists_b = np.ones(len(m), dtype=bool) if res_mask_b is None else np.asarray(res_mask_b) != 0
    inside = (m >= 0) & (m < n_a)
    rows_a = np.ones(n_a, dtype=bool) if res_mask_a is None else np.asarray(res_mask_a) != 0
    return exists_b & inside & rows_a[np.where(inside, m, 0)]


def gathered(xa, m, covered, mask_a=None):
    """(G [N_b,A,3] float32, present [N_b,A] bool): model row m[j] at the covered rows, zeros and nothing present elsewhere."""
    xa = lr._layout(np.asarray(xa))
    g = np.zeros((len(m),) + xa.shape[1:], dtype=np.float32)
    present = np.zeros((len(m), xa.shape[1]), dtype=bool)
    rows = np.flatnonzero(covered)
    g[rows] = xa[np.asarray(m)[rows]]
    present[rows] = lr.exists(xa, mask_a)[np.asarray(m)[rows]]
    return g, present


def far_points(g, present):
    """G with every absent atom at a far point of its own: on a line from FAR on, 1000 Angstrom apart (exact in float32)."""
    out = g.copy()
    rows, cols = np.nonzero(~present)
    out[rows, cols] = np.stack([FAR + 1000.0 * np.arange(len(rows)), np.full(len(rows), -FAR), np.full(len(rows), 2 * FAR)], axis=1).astype(np.float32)
    return out


def local_accuracy(xa, xb, m, mode="ca", coverage="ignore", res_mask_a=None, res_mask_b=None, score_mask=None, mask_a=None, mask_b=None, cutoff=15.0,
                   same_residue=False) -> dict:
    """One pair through its map: the outputs of ``fdipt_sample_lddt_mapped`` over the N_b rows of the reference, ``n_covered`` and
    ``n_reference``."""
    xa, xb, m = lr._layout(np.asarray(xa)), lr._layout(np.asarray(xb)), np.asarray(m)
    n_b, k = len(m), lr.SET_ATOMS[mode]
    exists_b = np.ones(n_b, dtype=bool) if res_mask_b is None else np.asarray(res_mask_b) != 0
    covered = covered_rows(m, xa.shape[0], res_mask_a, res_mask_b)
    g, present = gathered(xa, m, covered, mask_a)
    out = lr.local_accuracy(g, xb, mode, exists_b, score_mask, mask_a=present, mask_b=mask_b, cutoff=cutoff, same_residue=same_residue)
    out.update(n_covered=int(covered.sum()), n_reference=int(exists_b.sum()))
    if coverage == "ignore":
        return out
    # penalise: scored by the reference alone, passed where the model has both atoms too
    score_rows = exists_b & (np.ones(n_b, dtype=bool) if score_mask is None else np.asarray(score_mask) != 0)
    cols_a, cols_b = lr.columns(mode, g.shape[1]), lr.columns(mode, xb.shape[1])
    in_ref = (lr.exists(xb, mask_b)[:, cols_b] & exists_b[:, None]).reshape(-1)          # [N_b K]
    in_both = in_ref & present[:, cols_a].reshape(-1)
    pa, pb = g[:, cols_a].astype(np.float64).reshape(n_b * k, 3), xb[:, cols_b].astype(np.float64).reshape(n_b * k, 3)
    d_b, d_a = np.sqrt(lr.EPS + lr._pair_sq(pb)), np.sqrt(lr.EPS + lr._pair_sq(pa))
    rows_of = np.repeat(np.arange(n_b), k)
    candidate = in_ref[:, None] & in_ref[None, :] & ~np.eye(n_b * k, dtype=bool)
    if k > 1 and not same_residue:
        candidate &= rows_of[:, None] != rows_of[None, :]
    scored = candidate & (d_b < cutoff)
    both = in_both[:, None] & in_both[None, :]
    l1 = np.abs(d_b - d_a)
    c_atom = scored.sum(1).reshape(n_b, k)
    n_atom = np.stack([(scored & both & (l1 < t)).sum(1).reshape(n_b, k) for t in lr.THRESHOLDS], axis=-1)
    keep = score_rows[:, None]
    out["atom_lddt"] = np.where(keep, lr.score(c_atom, n_atom), 0.0)
    out["n_scored"], out["n_passed"] = c_atom.sum(1) * score_rows, n_atom.sum(1) * keep
    out["res_lddt"] = np.where(score_rows, lr.score(out["n_scored"], out["n_passed"]), 0.0)
    out["lddt"] = float(lr.score(out["n_scored"].sum(), out["n_passed"].sum(0)))
    out["status"] = (out["status"] & ~lr.NO_PARTNER) | (lr.NO_PARTNER if np.any(score_rows & (out["n_scored"] == 0)) else 0)
    return out


def far_point_oracle(xa, xb, m, mode, res_mask_a=None, res_mask_b=None, score_mask=None, mask_a=None, mask_b=None, same_residue=False) -> dict:
    """The un-mapped restatement on the gathered model with absent atoms far away and marked present: the integers and scores of penalise."""
    xa, xb, m = lr._layout(np.asarray(xa)), lr._layout(np.asarray(xb)), np.asarray(m)
    exists_b = np.ones(len(m), dtype=bool) if res_mask_b is None else np.asarray(res_mask_b) != 0
    g, present = gathered(xa, m, covered_rows(m, xa.shape[0], res_mask_a, res_mask_b), mask_a)
    return lr.local_accuracy(far_points(g, present), xb, mode, exists_b, score_mask, mask_a=np.ones_like(present), mask_b=mask_b, same_residue=same_residue)


def gdt_rows(m, n_a, mask_a=None, mask_b=None):
    """The reference rows a mapped GDT scores, ascending."""
    return np.flatnonzero(covered_rows(m, n_a, mask_a, mask_b))


def gdt(ca_a, ca_b, m, mode="search", mask_a=None, mask_b=None, norm=None) -> dict:
    """One pair of CA traces through its map: the outputs of ``fdipt_sample_gdt_mapped``, ``res_within`` over the N_b rows."""
    m = np.asarray(m)
    rows = gdt_rows(m, len(ca_a), mask_a, mask_b)
    out = gr.gdt(np.asarray(ca_a)[m[rows]], np.asarray(ca_b)[rows], mode, norm)
    out["res_within"] = gr.spread(out["res_within"], rows, len(m))
    out["n_covered"] = len(rows)
    out["n_reference"] = len(m) if mask_b is None else int(np.count_nonzero(mask_b))
    return out


def map_flags(m, n_a):
    m = np.asarray(m)
    used = m[m >= 0]
    return (OUT_OF_RANGE if np.any((m < -1) | (m >= n_a)) else 0) | (DUPLICATE if len(np.unique(used)) != len(used) else 0)
