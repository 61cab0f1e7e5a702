"""Sample selection on the device: the five structures the reference reports for an inpainting run
(evaluation/utils/sample_selection.py ``get_selected_models``): ``mean``, ``median``, ``mode``, ``mean_closest``, ``median_closest``
of the samples of a complex, over the backbone atoms C, N, CA, O of its diffused residues.

``select_samples`` is one launch of ``fdipt_sample_select`` (csrc/select.hip, contract in include/fdipt.h) for any number of
complexes; ``selected_structure`` assembles the atom37 of a strategy as ``replace_coords`` does.  The samples are compared in the
frame they share - the fixed context of an inpainting run - without superposition, as in the reference: for de novo batches the
numbers carry no structural meaning.

One divergence from the reference: where its Weiszfeld iteration divides by a distance of exactly 0 and returns NaN (always for a
single sample), the iteration here stops and returns that sample as the median, with ``status`` bit ``ZERO_DISTANCE`` set.
"""
from __future__ import annotations

import numpy as np

from . import _call, _lib

STRATEGIES = ("mean", "median", "mode", "mean_closest", "median_closest")
BACKBONE_COLUMNS = (2, 0, 1, 4)  # atom37 columns of the reference's BACKBONE_ATOMS order C, N, CA, O
MAX_SAMPLES = _lib.SELECT_MAX_SAMPLES
ZERO_DISTANCE, SKIPPED = _lib.SELECT_ZERO_DISTANCE, _lib.SELECT_SKIPPED


def plan_groups(diffuse_mask, groups=None):
    """Host-side plan of a launch: (ids, members, residues) with one entry per group in order of first appearance - the group's id,
    its batch indices in batch order and the indices of its diffused residues.  Raises ValueError for what the kernel cannot serve."""
    mask = _call.host(diffuse_mask) != 0
    if mask.ndim != 2:
        raise ValueError(f"diffuse_mask should be [B, N], got shape {mask.shape}")
    b = mask.shape[0]
    groups = np.zeros(b, dtype=np.int64) if groups is None else _call.host(groups).reshape(-1)
    if groups.shape[0] != b:
        raise ValueError(f"groups should hold one id per sample: {groups.shape[0]} ids for {b} samples")
    ids, members, residues = [], [], []
    for gid in dict.fromkeys(groups.tolist()):
        mem = np.nonzero(groups == gid)[0]
        if len(mem) > MAX_SAMPLES:
            raise ValueError(f"group {gid!r} has {len(mem)} samples: at most {MAX_SAMPLES} (one wave lane per sample)")
        if not (mask[mem] == mask[mem[0]]).all():
            raise ValueError(f"the samples of group {gid!r} do not share one diffuse_mask")
        res = np.nonzero(mask[mem[0]])[0]
        if len(res) == 0:
            raise ValueError(f"group {gid!r} has no diffused residue")
        ids.append(gid)
        members.append(mem.astype(np.int32))
        residues.append(res.astype(np.int32))
    if not ids:
        raise ValueError("no samples")
    return ids, members, residues


def select_samples(prot, diffuse_mask, groups=None, sigma: float = 30.0, max_iterations: int = 10000) -> dict:
    """prot [B,N,37,3] float32 (a device tensor is used in place, a NumPy array is uploaded), diffuse_mask [B,N], groups [B] ids or
    None (one group).  Returns per-group lists under ``mean`` / ``median`` [L,4,3] float64 (atoms in BACKBONE_COLUMNS order),
    ``weights`` / ``density`` / ``dist_to_mean`` / ``dist_to_median`` [S] float64, ``residues`` [L], ``members`` [S] (batch indices),
    and int arrays [G] ``mode`` / ``mean_closest`` / ``median_closest`` (positions within the group) and ``status``; ``group_ids``
    names the groups in order."""
    b, n, _ = _call.structure_shape(prot, atoms=(37,))
    mask = _call.per_row(diffuse_mask, (b, n), "diffuse_mask", "mask")
    if not sigma > 0 or max_iterations < 0:
        raise ValueError(f"sigma = {sigma}, max_iterations = {max_iterations}: expected sigma > 0 and max_iterations >= 0")
    ids, members, residues = plan_groups(mask, groups)
    n_groups, l_max = len(ids), max(len(r) for r in residues)
    start = np.zeros(n_groups + 1, dtype=np.int32)
    start[1:] = np.cumsum([len(m) for m in members])
    n_diffused = np.array([len(r) for r in residues], dtype=np.int32)

    import torch
    dev, (x,) = _call.upload("select_samples", prot=prot)
    centre, per_sample, per_group = ("float64", (n_groups, l_max, 4, 3)), ("float64", (b,)), ("int32", (n_groups,))
    out = _call.run(
        "fdipt_sample_select", _lib.SelectArgs, dev,
        dict(B=b, N=n, G=n_groups, L_max=l_max, group_start_host=start.ctypes.data, n_diffused_host=n_diffused.ctypes.data, sigma=float(sigma),
             max_iterations=int(max_iterations)),
        dict(atom37=x, diffuse_mask=torch.from_numpy(mask).to(dev), group_start=torch.from_numpy(start).to(dev),
             member=torch.from_numpy(np.concatenate(members)).to(dev)),
        dict(mean=centre, median=centre, weights=per_sample, density=per_sample, dist_to_mean=per_sample, dist_to_median=per_sample,
             index=("int32", (n_groups, 3)), status=per_group, n_diffused=per_group),
        widen=("index", "status"), workspace=("fdipt_select_workspace_bytes", n_groups, b, l_max))
    mean, median, index, status, counted = (out[k] for k in ("mean", "median", "index", "status", "n_diffused"))
    if (status & SKIPPED).any() or not np.array_equal(counted, n_diffused):
        raise _lib.FdiptError(f"fdipt_sample_select: the device counted {counted.tolist()} diffused residues per group, the host "
                              f"{n_diffused.tolist()} (status {status.tolist()})")
    cut = lambda row: [row[start[g]:start[g + 1]].copy() for g in range(n_groups)]  # noqa: E731
    return {"mean": [mean[g, :n_diffused[g]].copy() for g in range(n_groups)],
            "median": [median[g, :n_diffused[g]].copy() for g in range(n_groups)],
            **{k: cut(out[k]) for k in ("weights", "density", "dist_to_mean", "dist_to_median")},
            "mode": index[:, 0].copy(), "mean_closest": index[:, 1].copy(), "median_closest": index[:, 2].copy(), "status": status,
            "residues": [r.astype(np.int64) for r in residues],
            "members": [m.astype(np.int64) for m in members], "group_ids": list(ids)}


def carrier(selection: dict, group: int, strategy: str) -> int:
    """Position within the group of the sample a strategy's structure is built on: the chosen sample, or the first one for ``mean`` and
    ``median`` (the reference's ``predicted_models[0]``)."""
    if strategy not in STRATEGIES:
        raise ValueError(f"strategy {strategy!r}: expected one of {STRATEGIES}")
    return 0 if strategy in ("mean", "median") else int(selection[strategy][group])


def selected_structure(selection: dict, group: int, strategy: str, prot) -> np.ndarray:
    """atom37 [N,37,3] of a strategy: the chosen member for ``mode`` / ``mean_closest`` / ``median_closest``; for ``mean`` / ``median``
    the group's first member with columns C, N, CA, O of the diffused residues replaced (``replace_coords``, sample_selection.py:535;
    CB and everything else stay the first member's, as in the reference)."""
    b = int(selection["members"][group][carrier(selection, group, strategy)])
    out = np.array(_call.host(prot[b]), dtype=np.float32)
    if strategy in ("mean", "median"):
        out[np.asarray(selection["residues"][group])[:, None], np.array(BACKBONE_COLUMNS)[None, :]] = selection[strategy][group]
    return out
