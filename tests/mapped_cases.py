"""Cases of the mapped accuracy tests: a reference structure b, a model a with other rows and a row map from
the rows of b to those of a.  Sizes sit at the kernels' edges (tiles of 256 and 64 partner rows, four rows per block, 256 threads), not
at the workload's.  Built from fixed seeds with NumPy only; the three cases whose reference numbers are recorded
(tests/golden/mapped_cases.npz, tests/golden/make_goldens_mapped.py) are stored there with their inputs.
"""
from __future__ import annotations

import os

import numpy as np

import lddt_ref as lr
from gdt_ref import five_atoms  # noqa: F401  (the GDT tests put CA traces into the five-atom layout with it)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mapped_cases.npz")
GOLDEN_CASES = {"g_ca": "ca", "g_bb": "backbone", "g_all": "all"}  # recorded case -> its atom set
FAR = 1.0e5  # where the far-point construction starts to put absent atoms (Angstrom)

# name: (N_a, N_b, atoms per row, seed, kind)
SPEC = {
    "identity70": (70, 70, 37, 11, "identity"),
    "perm66": (66, 66, 5, 12, "permutation"),
    "edge257": (90, 257, 5, 13, "tail"),       # covered reference rows 255 and 256 (the second tile of 256), a masked reference row
    "edge40": (257, 40, 5, 14, "scatter"),     # model rows beyond 256
    "all65": (50, 65, 37, 15, "missing"),      # the ALL set: a second tile of 64, atoms missing on both sides
    "tiny5": (3, 5, 5, 16, "scatter"),
    "one": (1, 1, 5, 17, "identity"),
}


def structure(n: int, rng, atoms: int = 5) -> np.ndarray:
    """[n, atoms, 3] float64: a CA walk of 3.8 Angstrom steps that stays compact, N, C, CB, O around each CA at bond-like distances, and
    in atom37 up to 6 side-chain atoms per row within 4 Angstrom of CB (the other columns absent: zeros)."""
    ca = np.zeros((n, 3))
    for i in range(1, n):
        step = rng.normal(size=3) - 0.02 * ca[i - 1]
        ca[i] = ca[i - 1] + 3.8 * step / np.linalg.norm(step)
    ca += np.array([12.0, -9.0, 15.0])
    x = np.zeros((n, atoms, 3))
    for col, dist in ((0, 1.46), (1, 0.0), (2, 1.52), (3, 1.53), (4, 2.4)):
        off = rng.normal(size=(n, 3))
        x[:, col] = ca + dist * off / np.linalg.norm(off, axis=1, keepdims=True)
    if atoms == 37:
        for i in range(n):
            for col in rng.choice(np.arange(5, 37), size=int(rng.integers(0, 7)), replace=False):
                off = rng.normal(size=3)
                x[i, col] = x[i, 3] + off / np.linalg.norm(off) * rng.uniform(1.4, 4.0)
    return x


def model_of(xb, m, n_a: int, rng) -> np.ndarray:
    """[n_a, A, 3] float64: row m[j] is reference row j with per-row errors of 0.05 .. 2 Angstrom (so that every threshold is crossed),
    moved rigidly as a whole; the model rows without a partner are a structure of their own."""
    xa = structure(n_a, rng, xb.shape[1]) + 30.0
    rows = np.flatnonzero((m >= 0) & (m < n_a))
    scale = rng.choice([0.05, 0.3, 0.8, 2.0], size=(len(rows), 1, 1), p=[0.4, 0.3, 0.2, 0.1])
    noisy = xb[rows] + scale * rng.normal(size=(len(rows), 1, 3)) + 0.05 * rng.normal(size=xb[rows].shape)
    xa[m[rows]] = np.where(np.any(xb[rows] != 0, axis=-1, keepdims=True), noisy, 0.0)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.linalg.det(q))
    present = np.any(xa != 0, axis=-1, keepdims=True)
    return np.where(present, xa @ q.T + np.array([5.0, -3.0, 8.0]), 0.0)


def row_map_of(kind: str, n_a: int, n_b: int, rng) -> np.ndarray:
    m = np.full(n_b, -1, dtype=np.int32)
    if kind == "identity":
        m[:] = np.arange(n_b)
    elif kind == "permutation":  # non-monotone: a permutation of all rows
        m[:] = rng.permutation(n_a)[:n_b]
    elif kind == "tail":  # the model covers a scattered part of the reference, the last two rows of the second tile among it
        rows = np.sort(np.concatenate([rng.choice(n_b - 2, size=n_a - 12, replace=False), [n_b - 2, n_b - 1]]))
        m[rows] = rng.permutation(n_a)[:len(rows)]
    else:  # scatter, missing: about two thirds of the reference rows, model rows in any order
        count = max(1, min(n_a, (2 * n_b) // 3))
        rows = np.sort(rng.choice(n_b, size=count, replace=False))
        m[rows] = rng.permutation(n_a)[:count]
    return m


def build(name: str) -> dict:
    """The inputs of a case as float32 / int32 arrays with a leading structure axis of 1: prot_a, prot_b, alignment [N_b], res_mask
    [1,N_a], res_mask_b, score_mask [1,N_b]."""
    n_a, n_b, atoms, seed, kind = SPEC[name]
    rng = np.random.default_rng(seed)
    xb = structure(n_b, rng, atoms)
    m = row_map_of(kind, n_a, n_b, rng)
    xa = model_of(xb, m, n_a, rng)
    res_mask, res_mask_b, score_mask = np.ones((1, n_a), dtype=np.float32), np.ones((1, n_b), dtype=np.float32), np.ones((1, n_b), dtype=np.float32)
    if kind in ("tail", "missing", "scatter") and n_b > 8:
        covered = np.flatnonzero(m >= 0)
        res_mask_b[0, covered[1]] = 0          # a reference row that does not exist, although the map names a partner for it
        res_mask[0, m[covered[3]]] = 0         # a model row that does not exist: its reference row is not covered
        score_mask[0, covered[5]] = 0          # a covered row that is context only
        score_mask[0, np.flatnonzero(m < 0)[0]] = 0
    if kind == "missing":  # atoms the model lacks, atoms the reference lacks (the CA of one row among them)
        covered = np.flatnonzero(m >= 0)
        xa[m[covered[::4]], 5:] = 0.0
        xa[m[covered[2]], 1] = 0.0
        xb[covered[7], 0] = 0.0
        xb[::5, 20:] = 0.0
    return {"prot_a": xa[None].astype(np.float32), "prot_b": xb[None].astype(np.float32), "alignment": m, "res_mask": res_mask,
            "res_mask_b": res_mask_b, "score_mask": score_mask}


def golden():
    """The recorded fixture as a dict of arrays."""
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def golden_inputs(fix, name: str) -> dict:
    return {key: fix[f"{name}.{key}"] for key in ("prot_a", "prot_b", "alignment", "res_mask", "res_mask_b", "score_mask")}


def modes_of(case: dict):
    """The atom sets a case can run in."""
    return lr.MODES if case["prot_a"].shape[2] == 37 else ("ca", "backbone")


def straight_trace(n: int = 60, first: int = 20, last: int = 30):
    """The closed form: a straight CA trace of ``n`` rows spaced 3.8 Angstrom as the reference, the model the same trace without the rows
    ``first`` .. ``last`` - 1 and rigidly moved.  Returns (model [1,n - gap,3], reference [1,n,3], alignment [n])."""
    ref = np.zeros((n, 3))
    ref[:, 0] = 3.8 * np.arange(n)
    ref += np.array([4.0, -7.0, 2.5])
    keep = np.r_[0:first, last:n]
    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, 0.8, -0.6], [0.0, 0.6, 0.8]])
    model = ref[keep] @ rot.T + np.array([20.0, 3.0, -11.0])
    m = np.full(n, -1, dtype=np.int32)
    m[keep] = np.arange(len(keep))
    return model[None].astype(np.float32), ref[None].astype(np.float32), m
