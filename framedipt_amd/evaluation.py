"""Sample evaluation on the device: the numbers of the reference's evaluation tables for samples against their ground truth
(evaluation/evaluate_tcr.py with evaluation/utils/metrics.py, and the geometry checks of framedipt/analysis/metrics.py):

* backbone RMSD of the diffused regions - overall, per region, per residue - over the atoms C, N, CA, O, without superposition;
* phi / psi / omega of sample and ground truth in degrees, per chain over all residues, and their signed errors
  (``angle_error_with_sign(ground truth, sample)``, as ``residue_signed_angle_error`` calls it);
* CA-CA bond deviation and valid fraction, CA clash count and fraction (``ca_ca_distance`` / ``ca_ca_clashes``);
* the superposition of the CA atoms onto the ground truth (``rigid_transform_3D``): ``aligned_mean_dev`` is the number
  ``calc_aligned_rmsd`` returns - a MEAN of per-atom distances - and ``aligned_rmsd`` the root mean square after the same motion.

``evaluate_samples`` is one launch of ``fdipt_sample_evaluate`` (csrc/evaluate.hip, contract in include/fdipt.h) for any number of
samples, all in float64; ``as_eval_dicts`` / ``flatten`` give the nested dicts and the column names ``evaluate_tcr.py`` writes.

A chain is a run of consecutive rows with ``res_mask != 0`` and one ``chain_idx``: a chain id that comes back after another chain, or a
``res_mask = 0`` row inside a chain, is refused (the reference would join the rows around it; here ``res_mask = 0`` is padding).
"""
from __future__ import annotations

import numpy as np

from . import _call, _lib, output

ANGLES = ("phi", "psi", "omega")  # order of the [.., 3, N] arrays
DICT_ANGLES = ("psi", "omega", "phi")  # key order of the reference's dicts (calc_dihedrals)
BACKBONE_COLUMNS = (2, 0, 1, 4)  # atom37 columns of the reference's BACKBONE_ATOMS order C, N, CA, O
TCR_CHAINS = ("alpha", "beta")
NAN_DIHEDRAL, DEGENERATE_ALIGNMENT, SKIPPED = _lib.EVAL_NAN_DIHEDRAL, _lib.EVAL_DEGENERATE_ALIGNMENT, _lib.EVAL_SKIPPED
SCALARS = ("bb_rmsd", "ca_ca_bond_dev", "ca_ca_valid_percent", "num_ca_steric_clashes", "ca_steric_clash_percent", "aligned_mean_dev",
           "aligned_rmsd", "reflection")
GEOMETRY_SCALARS = ("ca_ca_bond_dev", "ca_ca_valid_percent", "num_ca_steric_clashes", "ca_steric_clash_percent")


def plan_regions(diffuse_mask, chain_idx):
    """[(chain, first, last)]: the maximal runs of diffused residues per chain in the order of ``get_diffused_region_per_chain``
    (experiments/utils.py:629-687, restated once in framedipt_amd/output.py): chains numbered 0.. in np.unique order, indices local to
    the chain."""
    chains, starts, ends = output.get_diffused_region_per_chain(_call.host(diffuse_mask).reshape(-1), _call.host(chain_idx).reshape(-1))
    return [(int(c), int(s), int(e)) for c, s, e in zip(chains, starts, ends)]


def region_rows(diffuse_mask, chain_idx, res_mask=None):
    """(regions, rows) of one sample: ``plan_regions`` over the rows of res_mask, and the absolute (first, last) row of every region.
    Raises ValueError for chains the kernel does not serve."""
    diffuse = _call.host(diffuse_mask).reshape(-1) != 0
    chain = _call.host(chain_idx).reshape(-1)
    keep = np.ones(len(diffuse), dtype=bool) if res_mask is None else _call.host(res_mask).reshape(-1) != 0
    if not (len(chain) == len(diffuse) == len(keep)):
        raise ValueError(f"diffuse_mask, chain_idx and res_mask should have one length, got {len(diffuse)}, {len(chain)}, {len(keep)}")
    kept = np.nonzero(keep)[0]
    ids = np.unique(chain[kept])
    first_row = {}
    for c in ids:
        rows = kept[chain[kept] == c]
        if rows[-1] - rows[0] + 1 != len(rows):
            raise ValueError(f"chain {c!r} is not one run of consecutive rows with res_mask != 0")
        first_row[int(np.nonzero(ids == c)[0][0])] = int(rows[0])
    regions = plan_regions((diffuse & keep)[kept], chain[kept])
    return regions, [(first_row[c] + s, first_row[c] + e) for c, s, e in regions]


def evaluate_samples(prot, reference, diffuse_mask, chain_idx=None, ref_index=None, res_mask=None, align_mask=None) -> dict:
    """prot [B,N,37,3] and reference [R,N,37,3] float32 (device tensors are used in place, NumPy arrays are uploaded), diffuse_mask
    [B,N]; chain_idx [B,N] (default: one chain), ref_index [B] (default: row 0 for R = 1, row b for R = B), res_mask [B,N] (default:
    ones), align_mask [B,N] (default: res_mask).  Returns float64 arrays ``res_bb_rmsd`` [B,N], ``bb_rmsd`` [B], ``dihedral`` and
    ``angle_error`` [B,3,N], ``gt_dihedral`` [R,3,N] (angles in ANGLES order, degrees; the error is ground truth - sample),
    ``ca_ca_bond_dev``, ``ca_ca_valid_percent``, ``ca_steric_clash_percent``, ``aligned_mean_dev``, ``aligned_rmsd`` [B], ``rotation``
    [B,3,3], ``translation`` [B,3]; int arrays ``num_ca_steric_clashes``, ``reflection``, ``status`` [B], ``ref_index`` [B]; and per
    sample the lists ``region_bb_rmsd`` ([G_b] float64), ``regions`` ((chain, first, last), chain-local as plan_regions) and
    ``region_rows`` ((first, last) rows).  A NaN dihedral raises ValueError as in the reference; a degenerate alignment (fewer than 3
    aligned rows, a covariance without a unique best rotation) only sets its ``status`` bit."""
    b, n, _ = _call.structure_shape(prot, atoms=(37,))
    if len(reference.shape) != 4 or tuple(reference.shape[1:]) != tuple(prot.shape[1:]) or reference.shape[0] < 1:
        raise ValueError(f"reference should be [R, N, 37, 3] with the N of prot {tuple(prot.shape)}, got {tuple(reference.shape)}")
    r = int(reference.shape[0])
    res = _call.per_row(res_mask, (b, n), "res_mask", "mask", default=1)
    diffuse = _call.per_row(diffuse_mask, (b, n), "diffuse_mask", "mask") * res
    align = res.copy() if align_mask is None else _call.per_row(align_mask, (b, n), "align_mask", "mask")
    chain = _call.per_row(chain_idx, (b, n), "chain_idx", "int", default=0)
    if ref_index is None:
        if r not in (1, b):
            raise ValueError(f"ref_index is needed to map {b} samples to {r} reference structures")
        ref = np.zeros(b, dtype=np.int32) if r == 1 else np.arange(b, dtype=np.int32)
    else:
        ref = np.ascontiguousarray(_call.host(ref_index).reshape(-1), dtype=np.int32)
        if ref.shape[0] != b:
            raise ValueError(f"ref_index should hold one row per sample: {ref.shape[0]} for {b} samples")
        if ((ref < 0) | (ref >= r)).any():
            raise ValueError(f"ref_index out of range: {ref.tolist()} for {r} reference structures")
    planned = [region_rows(diffuse[i], chain[i], res[i]) for i in range(b)]
    regions, rows = [p[0] for p in planned], [p[1] for p in planned]
    start = np.zeros(b + 1, dtype=np.int32)
    start[1:] = np.cumsum([len(x) for x in rows])
    table = np.array([fl for x in rows for fl in x], dtype=np.int32).reshape(-1, 2)
    max_regions = max(1, max(len(x) for x in rows))
    n_diffused = (diffuse != 0).sum(axis=1).astype(np.int32)

    import torch
    dev, (x, y) = _call.upload("evaluate_samples", prot=prot, reference=reference)
    per_sample, per_residue, int_per_sample = ("float64", (b,)), ("float64", (b, n)), ("int32", (b,))
    outputs = {"res_bb_rmsd": per_residue, "region_bb_rmsd": ("float64", (b, max_regions)), "bb_rmsd": per_sample, "dihedral": ("float64", (b, 3, n)),
               "gt_dihedral": ("float64", (r, 3, n)), "angle_error": ("float64", (b, 3, n)), "ca_ca_bond_dev": per_sample,
               "ca_ca_valid_percent": per_sample, "num_ca_steric_clashes": int_per_sample, "ca_steric_clash_percent": per_sample,
               "aligned_mean_dev": per_sample, "aligned_rmsd": per_sample, "rotation": ("float64", (b, 3, 3)), "translation": ("float64", (b, 3)),
               "reflection": int_per_sample, "status": int_per_sample, "n_diffused": int_per_sample}
    inputs = dict(ref_index=ref, diffuse_mask=diffuse, res_mask=res, align_mask=align, chain_idx=chain, region_start=start,
                  region_rows=table if len(table) else np.zeros((1, 2), dtype=np.int32))
    out = _call.run("fdipt_sample_evaluate", _lib.EvalArgs, dev,
                    dict(B=b, N=n, R=r, n_regions=len(table), max_regions=max_regions, ref_index_host=ref.ctypes.data,
                         region_start_host=start.ctypes.data),
                    dict(atom37=x, ref37=y, **{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inputs.items()}),
                    outputs, widen=("num_ca_steric_clashes", "reflection", "status"), workspace=("fdipt_eval_workspace_bytes", b, n))
    status, counted = out["status"], out.pop("n_diffused")
    if (status & SKIPPED).any() or not np.array_equal(counted, n_diffused):
        raise _lib.FdiptError(f"fdipt_sample_evaluate: the device counted {counted.tolist()} diffused residues per sample, the host "
                              f"{n_diffused.tolist()} (status {status.tolist()})")
    if (status & NAN_DIHEDRAL).any():
        raise ValueError(f"Found NaN values in computed dihedral angles (samples {np.nonzero(status & NAN_DIHEDRAL)[0].tolist()}).")
    per_region = out["region_bb_rmsd"]
    out["region_bb_rmsd"] = [per_region[i, :len(rows[i])].copy() for i in range(b)]
    out.update(regions=regions, region_rows=rows, ref_index=ref.astype(np.int64))
    return out


def convert_to_eval_idx(vals):
    """{-4: vals[-4], ..., -1: vals[-1], 1: vals[0], 2: vals[1], ...} (metrics.py:1245-1261): the last four under negative keys, the
    rest counted from 1."""
    if len(vals) < 4:
        raise ValueError(f"a region of {len(vals)} residues is shorter than the 4 the evaluation indices need")
    out = {idx: vals[idx] for idx in (-4, -3, -2, -1)}
    out.update({i + 1: v for i, v in enumerate(vals[:-4])})
    return out


def flatten(obj, delim: str = "_", parent: str = "") -> dict:
    """Nested dicts / sequences -> one dict whose keys join the levels with ``delim`` (metrics.py:1210-1239; sequence items count from 1)."""
    items = []
    if isinstance(obj, dict):
        for key, val in obj.items():
            items.extend(flatten(val, delim, f"{parent}{delim}{key}" if parent else key).items())
    elif isinstance(obj, (list, tuple)):
        for i, val in enumerate(obj):
            items.extend(flatten(val, delim, f"{parent}{delim}{i + 1}").items())
    else:
        items.append((parent, obj))
    return dict(items)


def default_region_names(n_regions: int, tcr: bool = False):
    """``alpha`` / ``beta`` for the first two regions of a TCR run (the reference's TCR_CHAINS), ``region1``, ``region2``, ... otherwise."""
    return [TCR_CHAINS[g] if tcr and g < len(TCR_CHAINS) else f"region{g + 1}" for g in range(n_regions)]


def as_eval_dicts(result: dict, b: int, region_names=None) -> dict:
    """The reference's nested dicts for sample ``b``, one entry per metric group of evaluate_tcr.py: ``model_metrics`` {bb_rmsd},
    ``chain_metrics`` {bb_rmsd: {region: value}}, ``residue_metrics`` {bb_rmsd: {region: {index: value}}}, ``residue_group_metrics``
    {angle_error | signed_angle_error | sample | gt: {angle: {region: {index: value}}}} with the indices of ``convert_to_eval_idx``.
    ``flatten`` of each group gives the columns ``evaluate_tcr.py`` writes (``bb_rmsd``, ``bb_rmsd_alpha``, ``bb_rmsd_alpha_-4``,
    ``angle_error_phi_alpha_1``, ...).  Raises ValueError for a region shorter than 4 residues."""
    rows = result["region_rows"][b]
    names = list(region_names) if region_names is not None else default_region_names(len(rows))
    if len(names) < len(rows):
        raise ValueError(f"{len(names)} region names for {len(rows)} regions")
    gt = result["gt_dihedral"][int(result["ref_index"][b])]
    cut = lambda arr, g: convert_to_eval_idx([float(v) for v in arr[rows[g][0]:rows[g][1] + 1]])  # noqa: E731
    per_angle = lambda arr, fn=float: {a: {names[g]: {k: fn(v) for k, v in cut(arr[ANGLES.index(a)], g).items()}  # noqa: E731
                                           for g in range(len(rows))} for a in DICT_ANGLES}
    return {"model_metrics": {"bb_rmsd": float(result["bb_rmsd"][b])},
            "chain_metrics": {"bb_rmsd": {names[g]: float(result["region_bb_rmsd"][b][g]) for g in range(len(rows))}},
            "residue_metrics": {"bb_rmsd": {names[g]: cut(result["res_bb_rmsd"][b], g) for g in range(len(rows))}},
            "residue_group_metrics": {"angle_error": per_angle(result["angle_error"][b], abs),
                                      "signed_angle_error": per_angle(result["angle_error"][b]),
                                      "sample": per_angle(result["dihedral"][b]), "gt": per_angle(gt)}}


def eval_columns(result: dict, b: int, region_names=None) -> dict:
    """One row of the reference's metrics table for sample ``b``: every group of ``as_eval_dicts`` flattened, in its order."""
    row = {}
    for group in as_eval_dicts(result, b, region_names).values():
        row.update(flatten(group))
    return row
