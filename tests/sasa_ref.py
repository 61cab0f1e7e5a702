"""NumPy restatement of the solvent-accessibility contract (include/fdipt.h, "solvent accessibility"): Shrake &
Rupley's point test on the golden-spiral sphere, written from the contract's text with whole-array operations - the kernel
(csrc/sasa.hip) gives an atom to a wave and walks tiles of 64 atoms - so that the two share the rules and nothing else.  float64
throughout, the operations in the order the contract states them.

``shrake_rupley`` takes one set of atoms; ``sasa`` takes ONE sample: prot [N,37,3] or [N,5,3] float32.  Two forms: ``filtered=False``
tests every point against every other atom, ``filtered=True`` only against the atoms with ``|c_i - c_j| < R_i + R_j``.
"""
from __future__ import annotations

import numpy as np

ATOM37 = ("N", "CA", "C", "CB", "O", "CG", "CG1", "CG2", "OG", "OG1", "SG", "CD", "CD1", "CD2", "ND1", "ND2", "OD1", "OD2", "SD", "CE", "CE1",
          "CE2", "CE3", "NE", "NE1", "NE2", "OE1", "OE2", "CH2", "NH1", "NH2", "OH", "CZ", "CZ2", "CZ3", "NZ", "OXT")
ATOM5 = ("N", "CA", "C", "CB", "O")
ELEMENT_RADII = {"N": 1.55, "C": 1.70, "O": 1.52, "S": 1.80}
RESTYPES = ("ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE", "LEU", "LYS", "MET", "PHE", "PRO", "SER", "THR", "TRP", "TYR", "VAL")
MAX_ASA = {"ALA": 121.0, "ARG": 265.0, "ASN": 187.0, "ASP": 187.0, "CYS": 148.0, "GLU": 214.0, "GLN": 214.0, "GLY": 97.0, "HIS": 216.0,
           "ILE": 195.0, "LEU": 191.0, "LYS": 230.0, "MET": 203.0, "PHE": 228.0, "PRO": 154.0, "SER": 143.0, "THR": 163.0, "TRP": 264.0,
           "TYR": 255.0, "VAL": 165.0}  # Tien et al. 2013, empirical
COMPLEXES = ("1fyt", "5ksa", "7t2d")
BACKBONE_EXCERPTS = ("anti", "helix", "boundary")
DENSE_TILE = 512


def sphere_points(n):
    """[n,3] float64: the golden spiral, formed in float64, rounded to float32 and widened again."""
    dl, dz = np.pi * (3.0 - np.sqrt(5.0)), 2.0 / n
    out = np.zeros((n, 3), dtype=np.float64)
    z, lon = 1.0 - dz / 2.0, 0.0
    for k in range(n):
        r = np.sqrt(1.0 - z * z)
        out[k] = np.cos(lon) * r, np.sin(lon) * r, z
        z -= dz
        lon += dl
    return out.astype(np.float32).astype(np.float64)


def radii(atoms):
    names = ATOM37 if atoms == 37 else ATOM5
    return np.array([ELEMENT_RADII[name[0]] for name in names], dtype=np.float64)


def max_sasa(aatype):
    table = np.array([MAX_ASA[r] for r in RESTYPES] + [np.nan], dtype=np.float64)
    return table[np.clip(np.asarray(aatype, dtype=np.int64), 0, 20)]


def _d2(p, c):
    """((dx dx + dy dy) + dz dz) of p [...,3] and c [...,3], broadcast."""
    dx, dy, dz = p[..., 0] - c[..., 0], p[..., 1] - c[..., 1], p[..., 2] - c[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _dense_free(p, i, c, R2, tile=DENSE_TILE):
    """The states of the points p [m,3] of atom i against EVERY other atom, the atoms taken in tiles so that the temporaries stay in cache."""
    m, n = len(p), len(c)
    a, b, hit = np.empty((m, tile)), np.empty((m, tile)), np.empty((m, tile), dtype=bool)
    buried = np.zeros(m, dtype=bool)
    for j0 in range(0, n, tile):
        w = min(tile, n - j0)
        A, B, H = a[:, :w], b[:, :w], hit[:, :w]
        np.subtract(p[:, 0:1], c[None, j0:j0 + w, 0], out=A)
        np.multiply(A, A, out=A)
        np.subtract(p[:, 1:2], c[None, j0:j0 + w, 1], out=B)
        np.multiply(B, B, out=B)
        np.add(A, B, out=A)
        np.subtract(p[:, 2:3], c[None, j0:j0 + w, 2], out=B)
        np.multiply(B, B, out=B)
        np.add(A, B, out=A)
        np.less_equal(A, R2[None, j0:j0 + w], out=H)
        if j0 <= i < j0 + w:
            H[:, i - j0] = False
        buried |= H.any(axis=1)
    return ~buried


def shrake_rupley(xyz, R, sphere, filtered=True, details=False):
    """xyz [n,3] (widened to float64), R [n] float64 (probe included), sphere [m,3] float64 -> accessible [n] int64; with ``details``
    (filtered form) also the smallest |d^2 - R_j^2| over every tested (point, neighbour) pair (inf without one) and the points'
    states [n,m] bool (True: accessible)."""
    c, R = np.asarray(xyz).astype(np.float64), np.asarray(R, dtype=np.float64)
    n, R2 = len(c), R * R
    out, margin, free = np.zeros(n, dtype=np.int64), np.inf, np.ones((n, len(sphere)), dtype=bool)
    if not filtered:
        ct = np.ascontiguousarray(c.T).T  # (the columns contiguous: the tiles are read along j)
        for i in range(n):
            free[i] = _dense_free(sphere * R[i] + c[i], i, ct, R2)
        return (free.sum(axis=1), margin, free) if details else free.sum(axis=1)
    nbrs = []
    for lo in range(0, n, 512):
        near = np.sqrt(_d2(c[lo:lo + 512, None], c[None])) < R[lo:lo + 512, None] + R[None]
        near[np.arange(len(near)), lo + np.arange(len(near))] = False
        nbrs += [np.flatnonzero(row) for row in near]
    for i in range(n):
        js = nbrs[i]
        if len(js) == 0:
            out[i] = len(sphere)
            continue
        d2 = _d2((sphere * R[i] + c[i])[:, None], c[None, js])
        free[i] = ~(d2 <= R2[None, js]).any(axis=1)
        out[i] = int(free[i].sum())
        if details:
            margin = min(margin, float(np.abs(d2 - R2[None, js]).min()))
    return (out, margin, free) if details else out


def existing_atoms(prot, atom_mask=None, res_mask=None):
    """[N,A] bool."""
    prot = np.asarray(prot)
    exists = np.any(prot != 0, axis=-1) if atom_mask is None else np.asarray(atom_mask) != 0
    if res_mask is not None:
        exists = exists & (np.asarray(res_mask) != 0)[:, None]
    return exists


def sasa(prot, atom_mask=None, res_mask=None, aatype=None, probe_radius=1.40, n_points=100, atom_radii=None, filtered=True):
    """One sample -> accessible, atom_sasa [N,A], residue_sasa, rsa [N], n_atoms and ``total_sasa``."""
    prot = np.asarray(prot)
    n_res, atoms = prot.shape[:2]
    exists = existing_atoms(prot, atom_mask, res_mask)
    R = (radii(atoms) if atom_radii is None else np.asarray(atom_radii, dtype=np.float64)) + np.float64(probe_radius)
    rows, cols = np.nonzero(exists)  # (row, column) order
    counts = shrake_rupley(prot[rows, cols], R[cols], sphere_points(n_points), filtered)
    accessible = np.zeros((n_res, atoms), dtype=np.int64)
    accessible[rows, cols] = counts
    atom_sasa = accessible * ((R * R) * (4.0 * np.pi / n_points))[None]
    residue = np.zeros(n_res, dtype=np.float64)
    for a in range(atoms):
        residue = residue + atom_sasa[:, a]
    denominator = max_sasa(np.zeros(n_res, dtype=np.int64) if aatype is None else aatype)
    with np.errstate(invalid="ignore"):
        rsa = residue / denominator
    return {"accessible": accessible, "atom_sasa": atom_sasa, "residue_sasa": residue, "rsa": rsa, "n_atoms": int(exists.sum()),
            "total_sasa": residue.sum()}


def cap_fraction(d, ri, rj):
    """The fraction of the sphere of radius ri that lies inside a sphere of radius rj at distance d (|ri - rj| < d < ri + rj)."""
    return (1.0 - (d * d + ri * ri - rj * rj) / (2.0 * d * ri)) / 2.0


# ---- the fixture (tests/golden/sasa_cases.npz): compact atom lists
def case_names(fix):
    return [str(c) for c in fix["cases"]]


def case_atoms(fix, name):
    """-> (xyz [n,3] float32, row [n], col [n] atom37 column, aatype [N], chain [N]) of a case."""
    return (fix[f"{name}.xyz"], fix[f"{name}.row"].astype(np.int64), fix[f"{name}.col"].astype(np.int64), fix[f"{name}.aatype"].astype(np.int64),
            fix[f"{name}.chain"].astype(np.int64))


def case_prot(fix, name, atoms=37):
    """-> (prot [N,atoms,3] float32, atom_mask [N,atoms] uint8, aatype [N]); ``atoms=5`` keeps the columns N, CA, C, CB, O."""
    xyz, row, col, aatype, _ = case_atoms(fix, name)
    keep = col < atoms
    prot, mask = np.zeros((len(aatype), atoms, 3), dtype=np.float32), np.zeros((len(aatype), atoms), dtype=np.uint8)
    prot[row[keep], col[keep]], mask[row[keep], col[keep]] = xyz[keep], 1
    return prot, mask, aatype
