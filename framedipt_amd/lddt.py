"""Superposition-free accuracy of samples on the device: lDDT, dRMSD and backbone FAPE of a model structure against a reference
structure in row correspondence (openfold/utils/loss.py: ``lddt`` / ``lddt_ca``, ``compute_drmsd``, ``compute_fape`` as ``backbone_loss``
calls it).  No frame is chosen and no superposition is searched, so the numbers say whether a region is locally right whether or not
it has hinged as a whole against its context - and they mean something for the coordinate averages ``select_samples`` builds.

* ``lddt`` / ``res_lddt``: Mariani et al.'s local distance difference test, per pair and per residue, with the integers it is formed
  from (``n_scored``, ``n_passed``); the context rows count as environment, ``score_mask`` picks the rows that are reported;
* ``drmsd``: root mean square difference of the CA distance matrices of the score rows;
* ``fape`` / ``res_fape`` / ``region_fape``: CA errors seen from every residue's own backbone frame, clamped at 10 and in units of 10
  Angstrom.

``local_accuracy`` is one call of ``fdipt_sample_lddt`` (csrc/lddt.hip, contract in include/fdipt.h and DESIGN.md section 7.13) for any
number of ordered pairs, all in float64.  With one array every ordered pair is scored - lDDT is not symmetric, the reference structure
chooses the scored distances - and ``consensus`` is the per-residue mean over the other samples as references: where the samples of a
run agree.  With ``alignment=`` the rows of the reference need not be those of the model: ``fdipt_sample_lddt_mapped``
(csrc/lddt_mapped.hip) reads the model through a row map (``row_map`` builds maps, ``compare.aligned_accuracy``
takes them from ``tm_align``).
"""
from __future__ import annotations

import numpy as np

from . import _call, _lib

MODES = {"ca": _lib.LDDT_CA, "backbone": _lib.LDDT_BACKBONE, "all": _lib.LDDT_ALL}
SET_ATOMS = {"ca": 1, "backbone": 4, "all": 37}
BACKBONE_COLUMNS = (0, 1, 2, 4)  # N, CA, C, O in atom37 and in the five-atom layout
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
PER_PAIR = ("lddt", "drmsd", "fape", "region_fape")
PER_ROW = ("res_lddt", "res_fape")
METRIC_NAMES = {"ca": "lddt_ca", "backbone": "lddt_bb", "all": "lddt_all"}
COVERAGE = {"ignore": _lib.MAP_IGNORE, "penalise": _lib.MAP_PENALISE}


def _shape(x, what: str):
    """(structures, rows, atoms per row) of [S,N,37,3], [S,N,5,3] or a CA trace [S,N,3] (atoms = 1)."""
    shape = tuple(x.shape)
    if len(shape) == 3 and shape[2] == 3:
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"{what} {shape}: no structures or no residues")
        return int(shape[0]), int(shape[1]), 1
    if len(shape) != 4:
        raise ValueError(f"{what} should be [S, N, 37, 3], [S, N, 5, 3] or [S, N, 3], got {shape}")
    return _call.structure_shape(x, what, lead="S", items="structures")


def ordered_pairs(s: int) -> np.ndarray:
    """[s (s - 1), 2] int32: every i != j, i-major."""
    i, j = np.nonzero(~np.eye(s, dtype=bool))
    return np.stack([i, j], axis=1).astype(np.int32)


def local_accuracy(prot_a, prot_b=None, atoms: str = "ca", res_mask=None, score_mask=None, atom_mask_a=None, atom_mask_b=None, pairs=None,
                   ref_index=None, cutoff: float = 15.0, same_residue: bool = False, per_atom: bool = False, alignment=None,
                   coverage: str = "ignore", res_mask_b=None) -> dict:
    """prot_a [S,N,37,3], [S,N,5,3] or a CA trace [S,N,3] float32, a device tensor (used in place:
    ``inference_fn(..., return_device=True)["prot_traj"][0]``) or a NumPy array (uploaded): the models; prot_b [S_b,N,...] likewise or
    None: the references.  ``atoms``: "ca", "backbone" (N, CA, C, O) or "all" (atom37 in both).  res_mask [S,N] (default: ones): the
    rows that exist; score_mask [S,N] (default: ones): the rows whose scores are reported and that enter the pair's numbers - partners,
    FAPE points and frames are always all existing rows.  atom_mask_a [S,N,atoms], atom_mask_b [S_b,N,atoms_b] (default: an atom exists
    where a coordinate is non-zero); an atom takes part where it exists in both structures.

    * ``prot_b`` given: model i against reference ``ref_index[i]`` (default: row i where S_b = S, row 0 where S_b = 1).
    * ``prot_b`` None, ``pairs`` None: every ordered pair i != j of prot_a; the result carries ``matrix`` [S,S] (row = model, column =
      reference, unit diagonal; not symmetric), ``drmsd_matrix`` [S,S] (zero diagonal) and ``consensus`` [S,N], the mean of ``res_lddt``
      over the other samples as references (zeros for one sample).
    * ``pairs`` [P,2]: (model: index into prot_a, reference: index into prot_b, or prot_a without it).
    ``same_residue``: atom pairs inside a row are scored too (OpenFold's ``lddt`` on the flattened atoms; the default is Mariani's
    definition).  ``per_atom``: also ``atom_lddt`` [P,N,A], A = 1, 4, 37.

    Returns NumPy arrays: ``lddt``, ``drmsd``, ``fape``, ``region_fape`` [P] float64, ``res_lddt``, ``res_fape`` [P,N] float64,
    ``n_scored`` [P,N] and ``n_passed`` [P,N,4] int64, ``status`` [P] int64 (``_lib.LDDT_*`` bits), ``pairs`` [P,2], ``atoms``.  A CA
    trace has no frames: the FAPE outputs are zero with ``LDDT_NO_FRAME`` set.  The host does not wait for the device before the
    read-back.

    ``alignment`` (int [N_b], or [P,N_b] per pair; NumPy or a device tensor): the rows of prot_b need not be those of prot_a - entry j is
    the row of the model that corresponds to row j of the reference, or -1 (``tm_align(...)["alignment"]``, ``row_map``); DESIGN.md
    section 7.16.  prot_b is then required and may have any row count; every per-row output has its N_b rows; ``score_mask`` is
    [S_b,N_b] and ``res_mask_b`` [S_b,N_b] (default: ones) says which reference rows exist, ``res_mask`` [S,N_a] which model rows do.
    ``coverage``: "ignore" - an atom takes part where it exists in the reference and its row has a present partner in the model, so
    the numbers are those of the un-mapped call on the gathered model - or "penalise" - every atom pair of the reference within the
    cutoff is scored and passes only where the model has both atoms, so a row without a partner scores eps / (eps + c); dRMSD and FAPE
    are the same under both.  The result gains ``n_covered``, ``n_reference`` [P] int64 and ``coverage`` [P], their ratio (0 for no
    reference row).  A NumPy map with an entry outside -1 .. N_a - 1 or a model row used twice raises; for a device tensor the pair's
    ``status`` carries ``MAP_OUT_OF_RANGE`` / ``MAP_DUPLICATE`` and its outputs are zero."""
    if atoms not in MODES:
        raise ValueError(f"atoms should be 'ca', 'backbone' or 'all', got {atoms!r}")
    mapped = alignment is not None
    if mapped and coverage not in COVERAGE:
        raise ValueError(f"coverage should be 'ignore' or 'penalise', got {coverage!r}")
    if not mapped and (coverage != "ignore" or res_mask_b is not None):
        raise ValueError("coverage and res_mask_b belong to a call with an alignment")
    if mapped and prot_b is None:
        raise ValueError("an alignment maps the rows of prot_b to those of prot_a: prot_b is required")
    s_a, n_a, atoms_a = _shape(prot_a, "prot_a")
    s_b, n, atoms_b = (s_a, n_a, atoms_a) if prot_b is None else _shape(prot_b, "prot_b")  # n: the rows of every per-row output, the reference's
    if not mapped and n != n_a:
        raise ValueError(f"prot_b {tuple(prot_b.shape)} does not have the {n_a} rows of prot_a")
    for what, layout in (("prot_a", atoms_a), ("prot_b", atoms_b)):
        if (atoms == "all" and layout != 37) or (atoms == "backbone" and layout == 1):
            raise ValueError(f"atoms={atoms!r} needs {'atom37' if atoms == 'all' else 'the backbone atoms'}: {what} holds {layout} atom(s) per row")
    if prot_b is None and atom_mask_b is not None:
        raise ValueError("atom_mask_b without prot_b: the structures of prot_a carry atom_mask_a")
    if not cutoff > 0:
        raise ValueError(f"cutoff should be positive, got {cutoff}")
    if prot_b is None and pairs is None and ref_index is None:
        pair_list, square = ordered_pairs(s_a), True
    else:
        pair_list, square = _call.plan_pairs(s_a, s_b, prot_b is not None, pairs, ref_index)
    n_pairs, k = len(pair_list), SET_ATOMS[atoms]
    score_rows = (s_b, n) if mapped else (s_a, n)  # (the rows that are reported are the reference's)
    # (shape errors of the optional inputs before torch or the library is touched)
    _call.check_shapes((("res_mask", res_mask, (s_a, n_a)), ("res_mask_b", res_mask_b, (s_b, n)), ("score_mask", score_mask, score_rows),
                        ("atom_mask_a", atom_mask_a, (s_a, n_a, atoms_a)), ("atom_mask_b", atom_mask_b, (s_b, n, atoms_b))), mapped)
    if mapped:
        alignment = _call.check_map(alignment, n_pairs, n, n_a)
    ints = ("n_scored", "n_passed", "status")
    outputs = {key: ("float64", (n_pairs,)) for key in PER_PAIR}
    outputs.update({key: ("float64", (n_pairs, n)) for key in PER_ROW})
    outputs.update(n_scored=("int32", (n_pairs, n)), n_passed=("int32", (n_pairs, n, 4)), status=("int32", (n_pairs,)))
    if per_atom:
        outputs["atom_lddt"] = ("float64", (n_pairs, n, k))
    if n_pairs == 0:  # (one structure, all-against-all)
        out = _call.empty_outputs(outputs, ints)
    else:
        import torch
        dev, (xa, xb) = _call.upload("local_accuracy", prot_a=prot_a, prot_b=prot_b)
        mask_a = _call.atom_mask(atom_mask_a, (s_a, n_a, atoms_a), "atom_mask_a", dev)
        mask_b = mask_a if prot_b is None else _call.atom_mask(atom_mask_b, (s_b, n, atoms_b), "atom_mask_b", dev)
        scored = _call.per_row(score_mask, score_rows, "score_mask", "mask", default=1, dev=dev)
        entry = "fdipt_sample_lddt_mapped" if mapped else "fdipt_sample_lddt"
        call = (entry, _lib.LddtArgs, dev,
                dict(S=s_a, N=n, atoms=atoms_a, S_b=s_b, atoms_b=atoms_b, P=n_pairs, mode=MODES[atoms], same_residue=int(bool(same_residue)),
                     cutoff=float(cutoff)),
                dict(prot=xa, prot_b=xb, res_mask=_call.per_row(res_mask, (s_a, n_a), "res_mask", "mask", default=1, dev=dev),
                     score_mask=None if mapped else scored, atom_mask_a=mask_a, atom_mask_b=mask_b, pairs=torch.from_numpy(pair_list).to(dev)),
                outputs)
        if mapped:
            out = _call.run_mapped(*call, dict(N_a=n_a, coverage=COVERAGE[coverage], map=_call.upload_map(alignment, n_pairs, n, dev),
                                               res_mask_b=_call.per_row(res_mask_b, (s_b, n), "res_mask_b", "mask", default=1, dev=dev), score_mask_b=scored),
                                   widen=ints, workspace=(entry + "_workspace", n_pairs, n))
        else:
            out = _call.run(*call, widen=ints, workspace=(entry + "_workspace", n_pairs, n))
    out["pairs"] = pair_list.astype(np.int64)
    out["atoms"] = atoms
    if mapped:
        _call.add_coverage(out, n_pairs)
    if square:
        out["matrix"] = np.ones((s_a, s_a), dtype=np.float64)
        out["drmsd_matrix"] = np.zeros((s_a, s_a), dtype=np.float64)
        out["matrix"][pair_list[:, 0], pair_list[:, 1]] = out["lddt"]
        out["drmsd_matrix"][pair_list[:, 0], pair_list[:, 1]] = out["drmsd"]
        out["consensus"] = consensus(out["res_lddt"], pair_list, s_a)
    return out


def consensus(res_lddt, pair_list, s: int) -> np.ndarray:
    """[s,N]: per model the mean of ``res_lddt`` over its pairs (the other samples as references); zeros for a model without a pair."""
    res_lddt = np.asarray(res_lddt, dtype=np.float64)
    out = np.zeros((s, res_lddt.shape[1]), dtype=np.float64)
    for i in range(s):
        rows = res_lddt[np.asarray(pair_list)[:, 0] == i]
        if len(rows):
            out[i] = rows.mean(axis=0)
    return out


def lddt_metrics(result: dict, p: int) -> dict:
    """The flat entries of pair ``p`` for a metrics table: ``lddt_ca`` / ``lddt_bb`` / ``lddt_all`` by the atom set of the call, ``drmsd``,
    ``fape``, ``region_fape``, as Python floats."""
    return {METRIC_NAMES[result["atoms"]]: float(result["lddt"][p]), "drmsd": float(result["drmsd"][p]), "fape": float(result["fape"][p]),
            "region_fape": float(result["region_fape"][p])}
