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

from . import _lib

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
    if len(prot.shape) != 4 or tuple(prot.shape[2:]) not in ((37, 3), (5, 3)):
        raise ValueError(f"prot should be [B, N, 37, 3] or [B, N, 5, 3], got {tuple(prot.shape)}")
    b, n, n_atoms = int(prot.shape[0]), int(prot.shape[1]), int(prot.shape[2])
    if b < 1 or n < 1:
        raise ValueError(f"prot {tuple(prot.shape)}: no samples or no residues")

    import torch
    lib = _lib.load()
    if torch.is_tensor(prot):
        _lib.require_cuda(prot, "structural_violations")
        if prot.dtype != torch.float32:
            raise ValueError(f"prot should be float32, got {prot.dtype}")
        dev = prot.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())

    def mask(x, what):
        if x is None:
            return torch.ones((b, n), dtype=torch.float32, device=dev)
        x = x.to(dev) if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        if tuple(x.shape) != (b, n):
            raise ValueError(f"{what} {tuple(x.shape)} does not match prot {tuple(prot.shape)}")
        return (x != 0).to(torch.float32)

    with torch.cuda.device(dev):
        x = prot.contiguous() if torch.is_tensor(prot) else torch.from_numpy(np.ascontiguousarray(prot, dtype=np.float32)).to(dev)
        res = mask(res_mask, "res_mask")
        nonzero = (x[:, :, :5] != 0).flatten(2).any(dim=-1).to(torch.float32)  # (protein_metrics :149 on the atoms that exist)
        keep = (nonzero if atoms == "all" else nonzero * mask(diffuse_mask, "diffuse_mask")).contiguous()
        if residue_index is None:
            index = torch.arange(n, dtype=torch.int32, device=dev).repeat(b, 1)
        else:
            index = residue_index.to(dev) if torch.is_tensor(residue_index) else torch.from_numpy(np.ascontiguousarray(residue_index)).to(dev)
            if tuple(index.shape) != (b, n):
                raise ValueError(f"residue_index {tuple(index.shape)} does not match prot {tuple(prot.shape)}")
            if index.is_floating_point():
                index = torch.round(index)
            index = index.to(torch.int32).contiguous()
        zeros = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
        out = {k: zeros(torch.float64, b) for k in SCALARS}
        out.update(num_residue_violations=zeros(torch.int32, b), n_clash_pairs=zeros(torch.int64, b))
        out.update({k: zeros(torch.float64, b, n) for k in PER_RESIDUE})
        out.update({k: zeros(torch.uint8, b, n) for k in PER_RESIDUE_MASKS})
        out.update({k: zeros(torch.float64, b, n, 5) for k in PER_ATOM})
        out.update({k: zeros(torch.uint8, b, n, 5) for k in PER_ATOM_MASKS})
        ws_bytes = lib.fdipt_sample_violations_workspace(b, n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        p = _lib.ptr
        args = _lib.ViolationArgs(B=b, N=n, atoms=n_atoms, prot=p(x), res_mask=p(res), keep_mask=p(keep), residue_index=p(index),
                                  workspace=p(ws), workspace_bytes=ws_bytes, **{k: p(v) for k, v in out.items()})
        _lib.check(lib.fdipt_sample_violations(C.byref(args), _lib.stream_ptr()), "fdipt_sample_violations")
        out = {k: v.cpu().numpy() for k, v in out.items()}
    out["num_residue_violations"] = out["num_residue_violations"].astype(np.int64)
    return out


def violation_metrics(result: dict, b: int) -> dict:
    """The flat ``metrics_dict`` entries of ``protein_metrics`` for sample ``b``: METRIC_KEYS as Python floats."""
    return {k: float(result[k][b]) for k in METRIC_KEYS}


def residue_violations(result: dict, b: int) -> list:
    """Rows of sample ``b`` with any violation (``get_violation_metrics``' residue_violations)."""
    return np.flatnonzero(result["total_per_residue_violations_mask"][b]).tolist()
