"""GDT-TS and GDT-HA of samples on the device: the fraction of the scored rows whose CA atoms lie within 1, 2, 4, 8 (TS) or 0.5, 1, 2, 4
(HA) Angstrom of the reference's - openfold/utils/validation_metrics.py ``gdt``, ``gdt_ts``, ``gdt_ha`` - without a superposition
(``superpose="none"``: the frame of the fixed context of an inpainting run, the reference's ``gdt`` on the raw coordinates), after one
least-squares superposition of all rows (``"global"``: ``superimpose``, then ``gdt``) or, per cutoff, under the best transform of a seed
search (``"search"``).

``gdt_scores`` is one call of ``fdipt_sample_gdt`` (csrc/gdt.hip, ABI in include/fdipt.h) for any number of pairs, all in float64;
DESIGN.md section 7.14 is the contract.  The search is this project's own - the fragment seeds of the TM-score search refined at each
of the five cutoffs - and is pinned by its NumPy restatement (tests/gdt_ref.py): no parity with the LGA program is claimed.
With ``alignment=`` the rows of the two structures need not correspond: ``fdipt_sample_gdt_mapped`` (csrc/gdt_mapped.hip) pairs them
through a row map.
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


def gdt_scores(prot_a, prot_b=None, mask_a=None, mask_b=None, pairs=None, norm_length=None, ref_index=None, superpose: str = "search",
               alignment=None) -> dict:
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
    within ``CUTOFFS[j]`` under cutoff j's transform) and ``pairs`` [P,2].

    ``alignment`` (int [N_b], or [P,N_b] per pair; NumPy or a device tensor): the rows of prot_b need not be those of prot_a - entry j is
    the row of prot_a that corresponds to row j of prot_b, or -1 (``tm_align(...)["alignment"]``, ``row_map``); DESIGN.md section 7.16.
    prot_b is then required and may have any row count up to ``MAX_ROWS``, and both may be CA traces [S,N,3]; a pair is scored over the
    reference rows that are masked in, have a partner and whose partner is masked in, in ascending reference order; ``res_within`` is
    [P,N_b]; the result gains ``n_covered`` (= ``n_scored``), ``n_reference`` (masked reference rows) and ``coverage``, their ratio.
    ``norm_length="reference"`` then divides by the masked reference rows instead of the rows scored: a model that covers half of the
    reference perfectly scores 0.5.  Bad maps: as ``lddt.local_accuracy`` (NaN scores with the ``MAP_*`` status bits)."""
    if superpose not in MODES:
        raise ValueError(f"superpose should be one of {sorted(MODES)}, got {superpose!r}")
    if alignment is not None:
        return _mapped_scores(prot_a, prot_b, mask_a, mask_b, pairs, norm_length, ref_index, superpose, alignment)
    if isinstance(norm_length, str):
        raise ValueError(f"norm_length={norm_length!r} belongs to a call with an alignment")
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


def _trace_shape(x, what: str):
    """(structures, rows, atoms per row) of [S,N,37,3], [S,N,5,3] or a CA trace [S,N,3] (atoms = 1)."""
    shape = tuple(x.shape)
    if len(shape) == 3 and shape[2] == 3:
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"{what} {shape}: no structures or no residues")
        return int(shape[0]), int(shape[1]), 1
    return _call.structure_shape(x, what, lead="S", items="structures")


def _mapped_scores(prot_a, prot_b, mask_a, mask_b, pairs, norm_length, ref_index, superpose, alignment) -> dict:
    """``gdt_scores`` with an alignment: one call of ``fdipt_sample_gdt_mapped``."""
    if prot_b is None:
        raise ValueError("an alignment maps the rows of prot_b to those of prot_a: prot_b is required")
    s_a, n_a, atoms_a = _trace_shape(prot_a, "prot_a")
    s_b, n_b, atoms_b = _trace_shape(prot_b, "prot_b")
    if (atoms_a == 1) != (atoms_b == 1):
        raise ValueError(f"a CA trace goes with a CA trace: prot_a holds {atoms_a} atom(s) per row, prot_b {atoms_b}")
    if max(n_a, n_b) > MAX_ROWS:
        raise ValueError(f"{max(n_a, n_b)} rows: the mapped GDT takes up to {MAX_ROWS} rows per structure")
    pair_list, _ = _call.plan_pairs(s_a, s_b, True, pairs, ref_index)
    n_pairs = len(pair_list)
    by_reference = isinstance(norm_length, str)
    if by_reference and norm_length != "reference":
        raise ValueError(f"norm_length should be numbers, None or 'reference', got {norm_length!r}")
    _call.check_shapes((("mask_a", mask_a, (s_a, n_a)), ("mask_b", mask_b, (s_b, n_b))), mapped=True)
    if by_reference:  # (the masked reference rows of every pair, on the host: a device mask is read back)
        rows = np.full(s_b, n_b, dtype=np.int64) if mask_b is None else np.count_nonzero(_call.host(mask_b), axis=1)
        norm_length = rows[np.clip(pair_list[:, 1], 0, s_b - 1)].astype(np.int32)
    elif norm_length is not None:
        norm_length = np.broadcast_to(np.asarray(norm_length, dtype=np.int32), (n_pairs,)).copy()
    alignment = _call.check_map(alignment, n_pairs, n_b, n_a)
    k = len(CUTOFFS)
    shapes = {"counts": (k,), "rotation": (k, 3, 3), "translation": (k, 3), "best_item": (k,), "best_pass": (k,), "res_within": (n_b,)}
    outputs = {key: ("float64" if key in ("gdt_ts", "gdt_ha", "rotation", "translation") else "int32", (n_pairs,) + shapes.get(key, ())) for key in OUTPUTS}
    if n_pairs == 0:
        out = _call.empty_outputs(outputs, _INTS)
    else:
        import torch
        dev, (xa, xb) = _call.upload("gdt_scores", prot_a=prot_a, prot_b=prot_b)
        out = _call.run_mapped("fdipt_sample_gdt_mapped", _lib.GdtArgs, dev,
                               dict(S=s_a, N=n_b, atoms=atoms_a, ca=0 if atoms_a == 1 else CA, S_b=s_b, atoms_b=atoms_b, P=n_pairs, mode=MODES[superpose]),
                               dict(prot=xa, mask=_call.per_row(mask_a, (s_a, n_a), "mask_a", "mask", default=1, dev=dev), prot_b=xb,
                                    mask_b=_call.per_row(mask_b, (s_b, n_b), "mask_b", "mask", default=1, dev=dev), pairs=torch.from_numpy(pair_list).to(dev),
                                    norm_length=None if norm_length is None else torch.from_numpy(norm_length).to(dev)),
                               outputs, dict(N_a=n_a, coverage=0, map=_call.upload_map(alignment, n_pairs, n_b, dev), res_mask_b=None, score_mask_b=None),
                               widen=_INTS)
    out["pairs"] = pair_list.astype(np.int64)
    return _call.add_coverage(out, n_pairs)


def gdt_metrics(result: dict, p: int) -> dict:
    """``{"gdt_ts", "gdt_ha"}`` of pair ``p`` of a ``gdt_scores`` result."""
    return {"gdt_ts": float(result["gdt_ts"][p]), "gdt_ha": float(result["gdt_ha"][p])}
