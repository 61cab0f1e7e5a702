"""Structural violations of samples on the device: the violation block of the reference's metric tables
(framedipt/analysis/metrics.py:protein_metrics -> openfold/np/relax/amber_minimize.py:get_violation_metrics ->
openfold/utils/loss.py find_structural_violations / compute_violation_metrics, tolerance factor 12, overlap tolerance 1.5):

* ``bonds_c_n_loss_mean``, ``angles_ca_c_n_loss_mean``, ``angles_c_n_ca_loss_mean``: flat-bottom errors of the peptide bond between
  consecutive residues; ``clashes_mean_loss``: overlap of the van der Waals spheres of atoms of different residues;
* the ``violations_*`` fractions of ``compute_violation_metrics``, ``num_residue_violations`` and the per-residue / per-atom sums and
  masks they come from (within-residue bounds included);
* ``radius_of_gyration`` in Angstrom over the atoms of the kept rows (``md.compute_rg`` of the written PDB gives it in nm; no mdtraj
  here, so this number is pinned by its NumPy restatement only).

``structural_violations`` is one call of ``fdipt_sample_violations`` (csrc/violations.hip, contract in include/fdipt.h) for any number
of samples, all in float64.  As in the reference's call, every residue is ALA (five atoms N, CA, C, CB, O: the per-atom arrays have
these five columns in atom37 order) and a row that does not keep its coordinates sits at the origin and counts: undiffused rows clash
with each other and enter the bond terms.  ``atoms="all"`` scores the diffused region against its real context instead.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _call, _lib

SCALARS = ("bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "angles_c_n_ca_loss_mean", "clashes_mean_loss",
           "violations_extreme_ca_ca_distance", "violations_between_residue_bond", "violations_between_residue_clash",
           "violations_within_residue", "violations_per_residue", "radius_of_gyration")
COUNTS = ("num_residue_violations", "n_clash_pairs")
PER_RESIDUE = ("connections_per_residue_loss_sum",)
PER_RESIDUE_MASKS = ("connections_per_residue_violation_mask", "total_per_residue_violations_mask")
PER_ATOM = ("clashes_per_atom_loss_sum", "within_per_atom_loss_sum")
PER_ATOM_MASKS = ("clashes_per_atom_clash_mask", "within_per_atom_violations")
METRIC_KEYS = ("bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "clashes_mean_loss", "radius_of_gyration")  # protein_metrics' metrics_dict
CONSTANT_NAMES = ("vdw_c", "vdw_n", "vdw_o", "c_n_length", "c_n_stddev", "c_n_tolerance", "cos_ca_c_n", "ca_c_n_stddev", "cos_c_n_ca",
                  "c_n_ca_stddev", "ca_ca")  # then lower [5,5] and upper [5,5]


def constants() -> dict:
    """The constants of the kernel as it uses them (``fdipt_violation_constants``): CONSTANT_NAMES, ``lower`` and ``upper`` [5,5] in the
    atom order N, CA, C, CB, O."""
    buf = (C.c_double * _lib.VIOLATION_CONSTANTS)()
    n = _lib.load().fdipt_violation_constants(buf)
    if n != _lib.VIOLATION_CONSTANTS:
        raise _lib.FdiptError(f"fdipt_violation_constants wrote {n} values, expected {_lib.VIOLATION_CONSTANTS}")
    vals = np.array(buf[:])
    k = len(CONSTANT_NAMES)
    out = {name: float(v) for name, v in zip(CONSTANT_NAMES, vals[:k])}
    out.update(lower=vals[k:k + 25].reshape(5, 5), upper=vals[k + 25:k + 50].reshape(5, 5))
    return out


def structural_violations(prot, diffuse_mask=None, res_mask=None, residue_index=None, atoms: str = "diffused") -> dict:
    """prot [B,N,37,3] or [B,N,5,3] float32, a device tensor (used in place: ``inference_fn(..., return_device=True)["prot_traj"][0]``)
    or a NumPy array (uploaded); only atoms 0..4 are read.  diffuse_mask, res_mask [B,N] (default: ones), residue_index [B,N] integers
    (default: 0 .. N - 1, what ``create_full_prot`` builds).  ``atoms="diffused"`` is the reference: a row keeps its coordinates where it
    is diffused and has a non-zero coordinate, every other existing row sits at the origin; ``atoms="all"`` keeps every row with a
    non-zero coordinate.  Returns NumPy arrays: SCALARS [B] float64, COUNTS [B] int64, PER_RESIDUE [B,N] and PER_ATOM [B,N,5] float64,
    their masks uint8.  The host does not wait for the device before the read-back."""
    if atoms not in ("diffused", "all"):
        raise ValueError(f"atoms should be 'diffused' or 'all', got {atoms!r}")
    b, n, n_atoms = _call.structure_shape(prot)

    import torch
    dev, (x,) = _call.upload("structural_violations", prot=prot)
    res = _call.per_row(res_mask, (b, n), "res_mask", "mask", default=1, dev=dev)
    nonzero = (x[:, :, :5] != 0).flatten(2).any(dim=-1).to(torch.float32)  # (protein_metrics :149 on the atoms that exist)
    keep = nonzero if atoms == "all" else nonzero * _call.per_row(diffuse_mask, (b, n), "diffuse_mask", "mask", default=1, dev=dev)
    index = _call.per_row(residue_index, (b, n), "residue_index", "int", dev=dev)
    if index is None:
        index = torch.arange(n, dtype=torch.int32, device=dev).repeat(b, 1)
    outputs = {k: ("float64", (b,)) for k in SCALARS}
    outputs.update(num_residue_violations=("int32", (b,)), n_clash_pairs=("int64", (b,)))
    outputs.update({k: ("float64", (b, n)) for k in PER_RESIDUE})
    outputs.update({k: ("uint8", (b, n)) for k in PER_RESIDUE_MASKS})
    outputs.update({k: ("float64", (b, n, 5)) for k in PER_ATOM})
    outputs.update({k: ("uint8", (b, n, 5)) for k in PER_ATOM_MASKS})
    return _call.run("fdipt_sample_violations", _lib.ViolationArgs, dev, dict(B=b, N=n, atoms=n_atoms),
                     dict(prot=x, res_mask=res, keep_mask=keep.contiguous(), residue_index=index), outputs, widen=("num_residue_violations",),
                     workspace=("fdipt_sample_violations_workspace", b, n))

def violation_metrics(result: dict, b: int) -> dict:
    """The flat ``metrics_dict`` entries of ``protein_metrics`` for sample ``b``: METRIC_KEYS as Python floats."""
    return {k: float(result[k][b]) for k in METRIC_KEYS}


def residue_violations(result: dict, b: int) -> list:
    """Rows of sample ``b`` with any violation (``get_violation_metrics``' residue_violations)."""
    return np.flatnonzero(result["total_per_residue_violations_mask"][b]).tolist()
