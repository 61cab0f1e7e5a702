"""Dense NumPy restatement of the superposition-free accuracy contract (include/fdipt.h): lDDT with its integer
counts, dRMSD and backbone FAPE of one (model, reference) pair in float64, including what the reference's functions cannot produce by
themselves (Mariani's definition without the pairs inside a residue, ``score_mask``, the per-residue FAPE).  Also the readers of the
fixture tests/golden/lddt_cases.npz (tests/golden/make_goldens_lddt.py) and the bounds the tests share.

The distances, the frames and the local points are written component by component, in the order of the reference's expressions: a term
of a sum here is the term the kernel forms, and only the order of the sums differs.
"""
from __future__ import annotations

import numpy as np

MODES = ("ca", "backbone", "all")
SET_ATOMS = {"ca": 1, "backbone": 4, "all": 37}
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
NO_PARTNER, NO_FRAME, SKIPPED = 1, 2, 4
EPS, FRAME_EPS, FAPE_EPS, CLAMP, UNIT = 1e-10, 1e-8, 1e-4, 10.0, 10.0
# case -> the atom sets it runs in; tests/golden/make_goldens_lddt.py builds the inputs
CASES = {"n1": ("ca", "backbone"), "n2": ("ca", "backbone"), "n63": ("ca", "backbone"), "n64": ("ca", "backbone"), "n65": ("ca", "backbone"),
         "tile": ("ca", "backbone"), "tile_all": ("all",), "masked": ("ca", "backbone"), "loop": ("ca", "backbone"), "sidechain": ("all", "backbone"),
         "all48": ("all",), "cutoff": ("ca", "backbone"), "no_n": ("ca", "backbone"), "b2": ("ca", "backbone"), "s3": ("ca", "backbone")}
CASE_MODES = [(name, mode) for name, modes in CASES.items() for mode in modes]
FLOAT_OUTPUTS = ("drmsd", "fape", "res_fape", "region_fape")
EXACT_OUTPUTS = ("lddt", "res_lddt", "n_scored", "n_passed", "atom_lddt", "status")
PERM_SEEDS = (3000, 3001, 3002)
MOTION_CASES = ("n65",)  # the generator asserts that the fixture's rigid motion of the model keeps every integer of these


def move(x, rot, shift):
    """The rigid motion of [..., 3] float32 coordinates, formed in float64 and rounded to float32; an absent atom (all zero) stays absent."""
    moved = (np.asarray(x, dtype=np.float64) @ np.asarray(rot).T + np.asarray(shift)).astype(np.float32)
    return np.where(np.any(np.asarray(x) != 0, axis=-1, keepdims=True), moved, np.float32(0))


def columns(mode: str, layout: int):
    """The columns of the atom set in a layout of ``layout`` atoms per row (1: a CA trace)."""
    if mode == "ca":
        return [0 if layout == 1 else 1]
    return [0, 1, 2, 4] if mode == "backbone" else list(range(37))


def _layout(x):
    x = np.asarray(x)
    return x[:, None, :] if x.ndim == 2 else x


def _sum_sq(dx, dy, dz):
    return (dx * dx + dy * dy) + dz * dz


def _pair_sq(x):
    """[M,M] squared distances of the points [M,3]."""
    return _sum_sq(x[:, None, 0] - x[None, :, 0], x[:, None, 1] - x[None, :, 1], x[:, None, 2] - x[None, :, 2])


def exists(x, mask=None):
    """[N,A] bool: the project's convention (any non-zero coordinate) unless a mask is given."""
    return np.any(x != 0, axis=-1) if mask is None else np.asarray(mask) != 0


def score(c, n):
    """The reference's score from the integers: c [...], n [...,4]."""
    norm = 1.0 / (EPS + np.asarray(c, dtype=np.float64))
    return norm * (EPS + 0.25 * np.asarray(n, dtype=np.int64).sum(-1).astype(np.float64))


def frames(n, ca, c):
    """from_3_points(C, CA, N, eps 1e-8): the axes e0, e1, e2 [N,3] (the frame's columns are -e0, e1, -e2) and the origin."""
    e0, b = ca - c, n - ca
    e0 = e0 / np.sqrt(_sum_sq(e0[:, 0], e0[:, 1], e0[:, 2]) + FRAME_EPS)[:, None]
    dot = (e0[:, 0] * b[:, 0] + e0[:, 1] * b[:, 1]) + e0[:, 2] * b[:, 2]
    e1 = b - e0 * dot[:, None]
    e1 = e1 / np.sqrt(_sum_sq(e1[:, 0], e1[:, 1], e1[:, 2]) + FRAME_EPS)[:, None]
    e2 = np.stack([e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1], e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2], e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]], axis=1)
    return e0, e1, e2, ca


def local_points(frame, x):
    """[frames, points, 3]: R^T (x - t) with R's columns -e0, e1, -e2."""
    e0, e1, e2, t = frame
    dx, dy, dz = (x[None, :, k] - t[:, None, k] for k in range(3))
    along = lambda e: (e[:, None, 0] * dx + e[:, None, 1] * dy) + e[:, None, 2] * dz  # noqa: E731
    return np.stack([-along(e0), along(e1), -along(e2)], axis=-1)


def local_accuracy(xa, xb, mode="ca", res_mask=None, score_mask=None, mask_a=None, mask_b=None, cutoff=15.0, same_residue=False) -> dict:
    """One pair: model xa, reference xb, each [N,37,3], [N,5,3] or [N,3].  Returns the outputs of the pair as ``fdipt_sample_lddt`` defines
    them (``atom_lddt`` always) and ``margin``, the smallest distance of a thresholded quantity from its threshold."""
    xa, xb = _layout(xa), _layout(xb)
    n, k = xa.shape[0], SET_ATOMS[mode]
    row = np.ones(n, dtype=bool) if res_mask is None else np.asarray(res_mask) != 0
    scored_rows = row & (np.ones(n, dtype=bool) if score_mask is None else np.asarray(score_mask) != 0)
    ex_a, ex_b = exists(xa, mask_a), exists(xb, mask_b)
    cols_a, cols_b = columns(mode, xa.shape[1]), columns(mode, xb.shape[1])
    part = ex_a[:, cols_a] & ex_b[:, cols_b] & row[:, None]                                  # [N,K]
    pa, pb = xa[:, cols_a].astype(np.float64).reshape(n * k, 3), xb[:, cols_b].astype(np.float64).reshape(n * k, 3)
    rows_of = np.repeat(np.arange(n), k)
    d_b, d_a = np.sqrt(EPS + _pair_sq(pb)), np.sqrt(EPS + _pair_sq(pa))
    flat = part.reshape(-1)
    candidate = flat[:, None] & flat[None, :] & ~np.eye(n * k, dtype=bool)
    if k > 1 and not same_residue:
        candidate &= rows_of[:, None] != rows_of[None, :]
    scored = candidate & (d_b < cutoff)
    l1 = np.abs(d_b - d_a)
    margin = np.min(np.abs(d_b - cutoff)[candidate], initial=np.inf)
    c_atom = scored.sum(1).reshape(n, k)
    n_atom = np.stack([(scored & (l1 < t)).sum(1).reshape(n, k) for t in THRESHOLDS], axis=-1)   # [N,K,4]
    for t in THRESHOLDS:
        margin = min(margin, np.min(np.abs(l1 - t)[scored], initial=np.inf))
    keep = scored_rows[:, None]
    out = {"atom_lddt": np.where(keep, score(c_atom, n_atom), 0.0), "n_scored": c_atom.sum(1) * scored_rows,
           "n_passed": n_atom.sum(1) * keep, "margin": float(margin)}
    out["res_lddt"] = np.where(scored_rows, score(out["n_scored"], out["n_passed"]), 0.0)
    out["lddt"] = float(score(out["n_scored"].sum(), out["n_passed"].sum(0)))
    status = NO_PARTNER if np.any(scored_rows & (out["n_scored"] == 0)) else 0
    # dRMSD over the CA atoms of the score rows that take part
    ca_a, ca_b = (0 if xa.shape[1] == 1 else 1), (0 if xb.shape[1] == 1 else 1)
    point = row & ex_a[:, ca_a] & ex_b[:, ca_b]
    ca_xa, ca_xb = xa[:, ca_a].astype(np.float64), xb[:, ca_b].astype(np.float64)
    kept = np.flatnonzero(point & scored_rows)
    m = len(kept)
    if m > 1:
        diff = np.sqrt(_pair_sq(ca_xa[kept])) - np.sqrt(_pair_sq(ca_xb[kept]))
        np.fill_diagonal(diff, 0.0)
        out["drmsd"] = float(np.sqrt(np.sum(diff * diff) * (1.0 / (m * (m - 1.0)))))
    else:
        out["drmsd"] = 0.0
    # backbone FAPE
    out.update(fape=0.0, res_fape=np.zeros(n), region_fape=0.0)
    framed = np.zeros(n, dtype=bool)
    if xa.shape[1] > 1 and xb.shape[1] > 1:
        framed = point & ex_a[:, 0] & ex_b[:, 0] & ex_a[:, 2] & ex_b[:, 2]
    if framed.any():
        f, pts = np.flatnonzero(framed), np.flatnonzero(point)
        fa = frames(*(xa[f][:, c].astype(np.float64) for c in (0, 1, 2)))
        fb = frames(*(xb[f][:, c].astype(np.float64) for c in (0, 1, 2)))
        d = local_points(fa, ca_xa[pts]) - local_points(fb, ca_xb[pts])
        err = np.minimum(np.sqrt(_sum_sq(d[..., 0], d[..., 1], d[..., 2]) + FAPE_EPS), CLAMP) / UNIT       # [frames, points]
        sums = err.sum(1)
        out["res_fape"][f] = sums / (FAPE_EPS + len(pts))
        out["fape"] = float(np.sum(sums / (FAPE_EPS + len(f))) / (FAPE_EPS + len(pts)))
        region = framed & scored_rows
        if region.any():
            out["region_fape"] = float(np.sum(out["res_fape"][region]) / region.sum())
    else:
        status |= NO_FRAME
    out["status"] = status
    return out


# ------------------------------------------------------------------ the fixture

def case_inputs(fix, name):
    """The inputs of a case as ``local_accuracy`` of the product takes them (float32 arrays as stored)."""
    inp = {"prot_a": fix[f"{name}.xa"], "res_mask": fix[f"{name}.res_mask"], "score_mask": fix[f"{name}.score_mask"]}
    if f"{name}.xb" in fix:
        inp["prot_b"] = fix[f"{name}.xb"]
    if f"{name}.ref_index" in fix:
        inp["ref_index"] = fix[f"{name}.ref_index"]
    return inp


def case_pairs(fix, name):
    return fix[f"{name}.pairs"]


def restate_case(fix, name, mode, same_residue=False, transform=None):
    """The restatement for every pair of a case: a dict of arrays stacked over the pairs.  ``transform``: applied to the model."""
    xa = fix[f"{name}.xa"]
    xb = fix[f"{name}.xb"] if f"{name}.xb" in fix else xa
    per = []
    for ia, ib in case_pairs(fix, name):
        model = xa[ia] if transform is None else transform(xa[ia])
        per.append(local_accuracy(model, xb[ib], mode, fix[f"{name}.res_mask"][ia], fix[f"{name}.score_mask"][ia], same_residue=same_residue))
    return {key: np.stack([np.asarray(p[key]) for p in per]) for key in per[0]}


def reference_applies_globally(fix, name):
    """The reference's ``lddt`` says what the contract says per score row always (with ``same_residue`` in the multi-atom sets), and with
    ``per_residue=False`` where every existing row is a score row: whether that holds for a case."""
    return bool(np.all((fix[f"{name}.score_mask"] != 0) | (fix[f"{name}.res_mask"] == 0)))


def bound(fix, name, key):
    """32 x the yardstick of the case, or of the fixture's largest for that output where the case's own is 0."""
    own = float(fix[f"{name}.{key}.yard"])
    return 32.0 * (own if own > 0 else max(float(fix[f"{c}.{key}.yard"]) for c in CASES))


def widest_bound(fix, key):
    return 32.0 * max(float(fix[f"{c}.{key}.yard"]) for c in CASES)


def check_floats(want, got, limit, report=None):
    """Every float output of ``got`` within ``limit(key)`` of ``want``."""
    for key in FLOAT_OUTPUTS:
        err = float(np.max(np.abs(np.asarray(got[key], dtype=np.float64) - np.asarray(want[key], dtype=np.float64)), initial=0.0))
        if report is not None:
            report(key, err, limit(key))
        assert err <= limit(key), (key, err, limit(key))


def check_exact(want, got, keys=EXACT_OUTPUTS):
    for key in keys:
        x, y = np.asarray(got[key]), np.asarray(want[key])
        assert x.shape == y.shape and np.array_equal(x.astype(y.dtype) if y.dtype.kind in "iu" else x, y), key


def to_atom37(x):
    """[S,N,5,3] or [S,N,37,3] -> [S,N,37,3] with zeros in the columns the input does not have."""
    if x.shape[2] == 37:
        return x.copy()
    out = np.zeros(x.shape[:2] + (37, 3), dtype=x.dtype)
    out[:, :, :5] = x
    return out


def joint_batch(fix, mode, seed=5):
    """Every case that runs in ``mode`` as one launch in atom37: padded to the longest with res_mask = 0 rows that hold garbage, garbage
    also in the columns the mode does not read.  Returns (inputs, [(case, first pair, pairs)])."""
    rng = np.random.default_rng(seed)
    names = [name for name, modes in CASES.items() if mode in modes]
    n_max = max(fix[f"{name}.xa"].shape[1] for name in names)
    read = columns(mode, 37) if mode != "ca" else [0, 1, 2]  # (the frames read N, CA, C in every mode)
    unread = [c for c in range(37) if c not in set(read) | {0, 1, 2}]
    xa, xb, rm, sm, pairs, where = [], [], [], [], [], []

    def padded(x):
        x = to_atom37(x)
        out = (rng.normal(size=(x.shape[0], n_max, 37, 3)) * 40).astype(np.float32)
        out[:, :x.shape[1]] = x
        if unread:
            out[:, :, unread] = (rng.normal(size=(x.shape[0], n_max, len(unread), 3)) * 40).astype(np.float32)
        return out

    for name in names:
        a = fix[f"{name}.xa"]
        b = fix[f"{name}.xb"] if f"{name}.xb" in fix else a
        p = case_pairs(fix, name) + np.array([sum(len(x) for x in xa), sum(len(x) for x in xb)])
        where.append((name, sum(len(x) for x in pairs), len(p)))
        xa.append(padded(a))
        xb.append(padded(b))
        pairs.append(p)
        for src, dst in ((fix[f"{name}.res_mask"], rm), (fix[f"{name}.score_mask"], sm)):
            m = np.zeros((a.shape[0], n_max), dtype=np.float32)
            m[:, :a.shape[1]] = src
            dst.append(m)
    sm = np.concatenate(sm)
    sm[np.concatenate(rm) == 0] = 1  # (a score mask set on a row that does not exist changes nothing)
    return ({"prot_a": np.concatenate(xa), "prot_b": np.concatenate(xb), "res_mask": np.concatenate(rm), "score_mask": sm,
             "pairs": np.concatenate(pairs).astype(np.int32)}, where)
