"""Solvent accessibility of samples on the device: the per-residue ASA / RSA block of the reference's TCR metric table
(evaluation/utils/metrics.py:get_sasa -> ``Bio.PDB.SASA.ShrakeRupley().compute(model, level="R")`` over the whole complex after a PDB
round trip, and its eight callers ``gt_asa``, ``sample_asa``, ``gt_rsa``, ``sample_rsa``, ``asa_abs_error``, ``asa_square_error``,
``rsa_abs_error``, ``rsa_square_error``):

* ``accessible`` [B,N,A]: of the ``n_points`` sphere points of every atom, how many no other atom of the sample buries;
* ``atom_sasa`` [B,N,A], ``residue_sasa`` [B,N], ``total_sasa`` [B] in square Angstrom; ``rsa`` [B,N] = residue_sasa / MAX_SASA[aatype].

``solvent_accessibility`` is one call of ``fdipt_sample_sasa`` (csrc/sasa.hip, ABI in include/fdipt.h) for any number of samples, all
in float64.  The algorithm is Shrake & Rupley (1973) on the golden-spiral sphere with element radii by atom name; DESIGN.md section
7.7 is its contract, with the points in which it is known or suspected to differ from Biopython.  No Biopython was at hand: the
numbers are pinned by that contract, a NumPy restatement and closed-form two-atom cases, not by ``Bio.PDB.SASA`` itself.
"""
from __future__ import annotations

import numpy as np

from . import _call, _lib
from .data import features as F

ATOM_RADII = {"N": 1.55, "C": 1.70, "O": 1.52, "S": 1.80}  # Angstrom, by element: the first letter of the atom37 name
ATOM5 = ("N", "CA", "C", "CB", "O")  # the five-atom layout (violations.py)
# Tien et al. 2013, empirical maximal ASA per residue type in square Angstrom (the reference's residue_constants.MAX_SASAs)
_MAX_BY_NAME = {"ALA": 121.0, "ARG": 265.0, "ASN": 187.0, "ASP": 187.0, "CYS": 148.0, "GLU": 214.0, "GLN": 214.0, "GLY": 97.0, "HIS": 216.0,
                "ILE": 195.0, "LEU": 191.0, "LYS": 230.0, "MET": 203.0, "PHE": 228.0, "PRO": 154.0, "SER": 143.0, "THR": 163.0, "TRP": 264.0,
                "TYR": 255.0, "VAL": 165.0}
MAX_SASA = np.array([_MAX_BY_NAME[r] for r in F.RESTYPE_3], dtype=np.float64)  # indexed by the project's aatype
METRICS = ("gt_asa", "sample_asa", "gt_rsa", "sample_rsa", "asa_abs_error", "asa_square_error", "rsa_abs_error", "rsa_square_error")
MAX_POINTS = 1024


def sphere_points(n: int) -> np.ndarray:
    """[n,3] float64: the golden-spiral unit points (dl = pi (3 - sqrt 5), dz = 2 / n, z_0 = 1 - dz / 2, lon_0 = 0), formed in
    float64, rounded to float32 - Biopython keeps its sphere in a float32 array - and widened again.  The one place that forms the
    table the device receives."""
    if not 1 <= n <= MAX_POINTS:
        raise ValueError(f"n_points should be 1 .. {MAX_POINTS}, got {n}")
    dl, dz = np.pi * (3.0 - np.sqrt(5.0)), 2.0 / n
    out = np.empty((n, 3), dtype=np.float64)
    z, lon = 1.0 - dz / 2.0, 0.0
    for k in range(n):
        r = np.sqrt(1.0 - z * z)
        out[k] = np.cos(lon) * r, np.sin(lon) * r, z
        z -= dz
        lon += dl
    return out.astype(np.float32).astype(np.float64)


def default_radii(atoms: int) -> np.ndarray:
    """[atoms] float64: the element radius of every atom column, atoms = 37 (atom37) or 5 (N, CA, C, CB, O)."""
    if atoms not in (37, 5):
        raise ValueError(f"atoms should be 37 or 5, got {atoms}")
    return np.array([ATOM_RADII[name[0]] for name in (F.ATOM_TYPES if atoms == 37 else ATOM5)], dtype=np.float64)


def solvent_accessibility(prot, atom_mask=None, res_mask=None, aatype=None, probe_radius: float = 1.40, n_points: int = 100, radii=None) -> dict:
    """prot [B,N,37,3] or [B,N,5,3] float32, a device tensor (used in place: ``inference_fn(..., return_device=True)["prot_traj"][0]``)
    or a NumPy array (uploaded).  atom_mask [B,N,A] (default: the atoms with a non-zero coordinate, as the PDB writer keeps them),
    res_mask [B,N] (default: ones), aatype [B,N] integers for the RSA denominator (default: ALA; 20 or more gives NaN), radii [A]
    (default: ``default_radii``).  All atoms of a sample that exist, of every chain, shield each other.  Returns NumPy arrays:
    ``accessible`` [B,N,A] int64, ``atom_sasa`` [B,N,A], ``residue_sasa`` [B,N], ``rsa`` [B,N] float64, ``n_atoms`` [B] int64 and
    ``total_sasa`` [B] = residue_sasa.sum(1).  The host does not wait for the device before the read-back."""
    b, n, n_atoms = _call.structure_shape(prot)
    n_points = int(n_points)
    sphere = sphere_points(n_points)
    reach = (default_radii(n_atoms) if radii is None else np.asarray(radii, dtype=np.float64)) + np.float64(probe_radius)
    if reach.shape != (n_atoms,) or not np.all(np.isfinite(reach)) or not np.all(reach > 0):
        raise ValueError(f"radii should be {n_atoms} positive numbers (with the probe radius added), got {reach!r}")

    import torch
    dev, (x,) = _call.upload("solvent_accessibility", prot=prot)
    atom = _call.per_row(atom_mask, (b, n, n_atoms), "atom_mask", dev=dev)
    atom = (x != 0).any(-1) if atom is None else atom != 0
    res = _call.per_row(res_mask, (b, n), "res_mask", "mask", default=1, dev=dev)
    kind = _call.per_row(aatype, (b, n), "aatype", "int", default=0, dev=dev).to(torch.int64)
    table = torch.from_numpy(np.append(MAX_SASA, np.nan)).to(dev)
    largest = table[torch.where((kind >= 0) & (kind < 20), kind, torch.full_like(kind, 20))]
    per_atom = (b, n, n_atoms)
    out = _call.run("fdipt_sample_sasa", _lib.SasaArgs, dev, dict(B=b, N=n, atoms=n_atoms, n_points=n_points),
                    dict(prot=x, atom_mask=atom.to(torch.uint8).contiguous(), res_mask=res, atom_radius=torch.from_numpy(reach).to(dev),
                         sphere=torch.from_numpy(sphere).to(dev), max_sasa=largest.contiguous()),
                    dict(accessible=("int32", per_atom), atom_sasa=("float64", per_atom), residue_sasa=("float64", (b, n)), rsa=("float64", (b, n)),
                         n_atoms=("int32", (b,))),
                    widen=("accessible", "n_atoms"), workspace=("fdipt_sample_sasa_workspace", b, n, n_atoms))
    out["total_sasa"] = out["residue_sasa"].sum(1)
    return out


def region_rows(regions) -> np.ndarray:
    """The row indices of ``regions``, a sequence of (start, end) row ranges with ``end`` inclusive (as
    ``secondary_structure.region_counts`` takes them), in the order given."""
    return np.concatenate([np.arange(int(lo), int(hi) + 1) for lo, hi in regions]) if len(regions) else np.zeros(0, dtype=np.int64)


def sasa_metrics(gt: dict, b_gt: int, sample: dict, b_sample: int, regions) -> dict:
    """The reference's eight ASA / RSA keys (METRICS) as float64 arrays over the rows of ``regions``: sample ``b_gt`` of the result
    ``gt`` is the ground truth (``model_1``), sample ``b_sample`` of ``sample`` the sample (``model_2``); the two results may come from
    different calls, a full-atom structure and a backbone as in the reference.  Errors are ground truth minus sample."""
    rows = region_rows(regions)
    out = {}
    for kind, key in (("asa", "residue_sasa"), ("rsa", "rsa")):
        truth, mine = np.asarray(gt[key][b_gt])[rows], np.asarray(sample[key][b_sample])[rows]
        error = truth - mine
        out.update({f"gt_{kind}": truth, f"sample_{kind}": mine, f"{kind}_abs_error": np.abs(error), f"{kind}_square_error": error ** 2})
    return {k: out[k] for k in METRICS}
