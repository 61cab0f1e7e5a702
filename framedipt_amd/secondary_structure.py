"""Secondary structure of samples on the device: the SHAPE_METRICS of the reference's metric tables
(framedipt/analysis/metrics.py:calc_mdtraj_metrics -> ``md.compute_dssp(traj, simplified=True)`` of the written PDB; per diffused region
in evaluation/utils/metrics.py:get_coil_helix_sheet):

* ``coil_percent``, ``helix_percent``, ``strand_percent``, ``non_coil_percent``: fractions of the rows that exist;
* ``ss`` [B,N]: the class per row (0 coil, 1 helix: alpha, 3-10 or pi, 2 strand, 255 where the row does not exist) and ``ss_string``,
  its ``C`` / ``H`` / ``E`` letters over the rows that exist;
* the hydrogen bonds they come from: per donor its two acceptors and their energies in kcal/mol, and the counts of bonds, bridges and
  ladders.

``secondary_structure`` is one call of ``fdipt_sample_dssp`` (csrc/dssp.hip, ABI in include/fdipt.h) for any number of samples, all in
float64.  The algorithm is Kabsch & Sander (1983) as DSSP 2.x states it; DESIGN.md section 7.6 is its contract, with the corner cases
in which it is known to differ.  No mdtraj was at hand: the numbers are pinned by a NumPy restatement, by ideal backbones and by the
deposited annotation of three complexes, not by ``md.compute_dssp`` itself.
"""
from __future__ import annotations

import numpy as np

from . import _call, _lib

FRACTIONS = ("non_coil_percent", "coil_percent", "helix_percent", "strand_percent")  # calc_mdtraj_metrics' keys before radius_of_gyration
COUNTS = ("n_rows", "n_hbonds", "n_bridges", "n_ladders", "status")
LETTERS = {_lib.DSSP_COIL: "C", _lib.DSSP_HELIX: "H", _lib.DSSP_STRAND: "E"}
PRO = 14  # the project's index of proline in aatype (data/features.py: RESTYPE_3_TO_INDEX)


def secondary_structure(prot, res_mask=None, chain_idx=None, aatype=None) -> dict:
    """prot [B,N,37,3] or [B,N,5,3] float32, a device tensor (used in place: ``inference_fn(..., return_device=True)["prot_traj"][0]``)
    or a NumPy array (uploaded); atoms 0, 1, 2, 4 (N, CA, C, O) are read.  res_mask [B,N] (default: ones), chain_idx [B,N] integers
    (default: one chain), aatype [B,N] integers (default: no prolines; a row with aatype 14 donates no hydrogen bond).  A row exists where
    res_mask != 0 and each of its four atoms has a non-zero coordinate: an undiffused row left at the origin is absent, as it is from
    the PDB the reference writes.  Returns NumPy arrays: FRACTIONS [B] float64 (NaN without a row or with a status bit), COUNTS [B]
    int64, ``ss`` [B,N] uint8, ``acceptor`` [B,N,2] int64 (row index, -1: none), ``acceptor_energy`` [B,N,2] float64, and ``ss_string``, a
    list of B strings.  The host does not wait for the device before the read-back."""
    b, n, n_atoms = _call.structure_shape(prot)

    import torch
    dev, (x,) = _call.upload("secondary_structure", prot=prot)
    res = _call.per_row(res_mask, (b, n), "res_mask", "mask", default=1, dev=dev)
    chain = _call.per_row(chain_idx, (b, n), "chain_idx", "int", default=0, dev=dev)
    kind = _call.per_row(aatype, (b, n), "aatype", "int", dev=dev)
    proline = torch.zeros((b, n), dtype=torch.uint8, device=dev) if kind is None else (kind == PRO).to(torch.uint8)
    outputs = {k: ("float64", (b,)) for k in FRACTIONS}
    outputs.update({k: ("int32", (b,)) for k in COUNTS})
    outputs.update(ss=("uint8", (b, n)), acceptor=("int32", (b, n, 2)), acceptor_energy=("float64", (b, n, 2)))
    out = _call.run("fdipt_sample_dssp", _lib.DsspArgs, dev, dict(B=b, N=n, atoms=n_atoms),
                    dict(prot=x, res_mask=res, chain_idx=chain, is_proline=proline), outputs, widen=COUNTS + ("acceptor",),
                    workspace=("fdipt_sample_dssp_workspace", b, n))
    out["ss_string"] = ["".join(LETTERS[c] for c in row.tolist() if c != _lib.DSSP_ABSENT) for row in out["ss"]]
    return out


def shape_metrics(result: dict, b: int) -> dict:
    """``calc_mdtraj_metrics``' four secondary-structure keys for sample ``b`` as Python floats.  Its fifth key, ``radius_of_gyration``,
    is ``violations.structural_violations(...)["radius_of_gyration"]``: in Angstrom here, in nm there (mdtraj's unit)."""
    return {k: float(result[k][b]) for k in FRACTIONS}


def region_counts(result: dict, b: int, regions) -> tuple:
    """``(coil, helix, sheet)`` row counts of sample ``b`` over ``regions``, a sequence of (start, end) row ranges with ``end``
    inclusive, as ``get_coil_helix_sheet`` takes its starts / ends: what it returns, on row indices of the sample (its chain offsets
    added).  A row that does not exist counts in none of the three."""
    ss = np.asarray(result["ss"][b])
    rows = np.concatenate([ss[int(lo):int(hi) + 1] for lo, hi in regions]) if len(regions) else ss[:0]
    return tuple(int((rows == c).sum()) for c in (_lib.DSSP_COIL, _lib.DSSP_HELIX, _lib.DSSP_STRAND))
