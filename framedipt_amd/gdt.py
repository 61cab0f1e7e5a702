"""GDT-TS and GDT-HA of samples on the device: the fraction of the scored rows whose CA atoms lie within 1, 2, 4, 8 (TS) or 0.5, 1, 2, 4
(HA) Angstrom of the reference's - openfold/utils/validation_metrics.py ``gdt``, ``gdt_ts``, ``gdt_ha`` - without a superposition
(``superpose="none"``: the frame of the fixed context of an inpainting run, the reference's ``gdt`` on the raw coordinates), after one
least-squares superposition of all rows (``"global"``: ``superimpose``, then ``gdt``) or, per cutoff, under the best transform of a seed
search (``"search"``).

``gdt_scores`` is one call of ``fdipt_sample_gdt`` (csrc/gdt.hip, ABI in include/fdipt.h) for any number of pairs, all in float64;
DESIGN.md section 7.14 is the contract.  The search is this project's own - the fragment seeds of the TM-score search refined at each
of the five cutoffs - and is pinned by its NumPy restatement (tests/gdt_ref.py): no parity with the LGA program is claimed.
"""
from __future__ import annotations

import numpy as np

from . import _call, _lib
from ._call import all_pairs  # noqa: F401  (part of this module's interface)

CA = 1  # the CA column of atom37 and of the five-atom layout N, CA, C, CB, O
MAX_ROWS = _lib.TM_MAX_ROWS
CUTOFFS = (0.5, 1.0, 2.0, 4.0, 8.0)
MODES = {"none": _lib.GDT_NONE, "global": _lib.GDT_GLOBAL, "search": _lib.GDT_SEARCH}
OUTPUTS = ("gdt_ts", "gdt_ha", "counts", "n_scored", "rotation", "translation", "best_item", "best_pass", "passes", "res_within", "status")
_INTS = ("counts", "n_scored", "best_item", "best_pass", "passes", "status")  # (res_within stays int32: a bit field per row)
assert len(CUTOFFS) == _lib.GDT_CUTOFFS


def gdt_scores(prot_a, prot_b=None, mask_a=None, mask_b=None, pairs=None, norm_length=None, ref_index=None, superpose: str = "search") -> dict:
    """prot_a [S,N,37,3] or [S,N,5,3] float32, a device tensor (used in place) or a NumPy array (uploaded): the models; prot_b
    [S_b,N,37 or 5,3] likewise or None: the references.  mask_a [S,N], mask_b [S_b,N] (default: ones): a pair is scored over the rows
    where both of its structures' masks are set.  Pairs are planned as ``tm_score.tm_scores`` plans them:

    * ``prot_b`` None, ``pairs`` None: all i < j of prot_a; the result carries ``matrix_ts`` and ``matrix_ha`` [S,S] with a unit
      diagonal, entry (i, j) mirrored to (j, i).
    * ``prot_b`` given: sample i against structure ``ref_index[i]`` of prot_b (default: row i where S_b = S, row 0 where S_b = 1).
    * ``pairs`` [P,2]: first index into prot_a, second into prot_b (prot_a without it).
    ``norm_length`` [P] (or one number): the length L the counts are divided by where > 0, else the number of rows scored.
    ``superpose``: "none", "global" or "search" (above).

    Returns NumPy arrays per pair: ``gdt_ts``, ``gdt_ha`` float64 (NaN with a status bit), ``counts`` [P,5] (rows within ``CUTOFFS``),
    ``n_scored``, ``rotation`` [P,5,3,3] and ``translation`` [P,5,3] (R x + t ~ y per cutoff, x the model), ``best_item`` and
    ``best_pass`` [P,5] (-1 outside "search"), ``passes``, ``status`` int64, ``res_within`` [P,N] int32 (bit j: the row is scored and
    within ``CUTOFFS[j]`` under cutoff j's transform) and ``pairs`` [P,2]."""
    if superpose not in MODES:
        raise ValueError(f"superpose should be one of {sorted(MODES)}, got {superpose!r}")
    s_a, n, atoms_a = _call.structure_shape(prot_a, "prot_a", lead="S", items="structures")
    s_b, n_b, atoms_b = (s_a, n, atoms_a) if prot_b is None else _call.structure_shape(prot_b, "prot_b", lead="S", items="structures")
    if n_b != n:
        raise ValueError(f"prot_b {tuple(prot_b.shape)} does not have the {n} rows of prot_a")
    if prot_b is None and mask_b is not None:
        raise ValueError("mask_b without prot_b: the structures of prot_a carry mask_a")
    pair_list, square = _call.plan_pairs(s_a, s_b, prot_b is not None, pairs, ref_index)
    n_pairs = len(pair_list)
    if norm_length is not None:
        norm_length = np.broadcast_to(np.asarray(norm_length, dtype=np.int32), (n_pairs,)).copy()
    k = len(CUTOFFS)
    shapes = {"counts": (k,), "rotation": (k, 3, 3), "translation": (k, 3), "best_item": (k,), "best_pass": (k,), "res_within": (n,)}
    outputs = {key: ("float64" if key in ("gdt_ts", "gdt_ha", "rotation", "translation") else "int32", (n_pairs,) + shapes.get(key, ())) for key in OUTPUTS}
    if n_pairs == 0:  # (one structure, all-against-all)
        out = _call.empty_outputs(outputs, _INTS)
    else:
        import torch
        dev, (xa, xb) = _call.upload("gdt_scores", prot_a=prot_a, prot_b=prot_b)
        out = _call.run("fdipt_sample_gdt", _lib.GdtArgs, dev,
                        dict(S=s_a, N=n, atoms=atoms_a, ca=CA, S_b=s_b, atoms_b=atoms_b, P=n_pairs, mode=MODES[superpose]),
                        dict(prot=xa, mask=_call.per_row(mask_a, (s_a, n), "mask_a", "mask", default=1, dev=dev), prot_b=xb,
                             mask_b=None if prot_b is None else _call.per_row(mask_b, (s_b, n), "mask_b", "mask", default=1, dev=dev),
                             pairs=torch.from_numpy(pair_list).to(dev), norm_length=None if norm_length is None else torch.from_numpy(norm_length).to(dev)),
                        outputs, widen=_INTS)
    out["pairs"] = pair_list.astype(np.int64)
    if square:
        out["matrix_ts"] = _call.square_matrix(s_a, pair_list, out["gdt_ts"])
        out["matrix_ha"] = _call.square_matrix(s_a, pair_list, out["gdt_ha"])
    return out


def gdt_metrics(result: dict, p: int) -> dict:
    """``{"gdt_ts", "gdt_ha"}`` of pair ``p`` of a ``gdt_scores`` result."""
    return {"gdt_ts": float(result["gdt_ts"][p]), "gdt_ha": float(result["gdt_ha"][p])}
