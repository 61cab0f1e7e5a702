"""Interface accuracy of complexes on the device: is a chain - or a redesigned loop - docked onto its partner where the reference has it?

* ``n_native``, ``n_model``, ``n_shared``: the residue-residue contacts across an interface in the reference, in the model, in both;
  ``fnat`` = shared / native, ``fnonnat`` = (model - shared) / model; per row ``res_native``, ``res_model``, ``res_shared``;
* ``irmsd``: RMSD of the backbone atoms of the interface rows (within ``interface_cutoff`` of the other side in the reference) after
  their own superposition; ``lrmsd``: RMSD of the ligand's backbone atoms after the superposition of the receptor's;
* ``dockq`` = (fnat + 1 / (1 + (irmsd / 1.5)^2) + 1 / (1 + (lrmsd / 8.5)^2)) / 3 (Basu & Wallner 2016).

``interface_accuracy`` is one call of ``fdipt_sample_interface`` (csrc/interface.hip, ABI in include/fdipt.h) for any number of pairs and
up to ``MAX_INTERFACES`` interfaces, all in float64; DESIGN.md section 7.18 is the contract.  The contract is this project's own and is
pinned by its NumPy restatement (tests/interface_ref.py): no parity with the DockQ program is claimed.  An interface is a row of
``sides`` (0 neither, 1 receptor, 2 ligand): ``chain_sides`` builds one per chain pair, ``loop_sides`` one per chain with diffused rows -
the inpainting question.

With ``alignment=`` the rows of the reference need not be those of the model: ``fdipt_sample_interface_mapped``
(csrc/interface_mapped.hip) reads the model through a row map, and ``coverage="penalise"`` charges the model
for the reference rows it lacks.  ``compare.sequence_aligned_interface`` takes the map from the sequences.
"""
from __future__ import annotations

import numpy as np

from . import _call, _lib

MODES = {"ca": _lib.IFACE_CA, "cb": _lib.IFACE_CB, "backbone": _lib.IFACE_BACKBONE, "all": _lib.IFACE_ALL}
CONTACT_CUTOFF = {"ca": 8.0, "cb": 8.0, "backbone": 5.0, "all": 5.0}
RECEPTOR, LIGAND = _lib.IFACE_RECEPTOR, _lib.IFACE_LIGAND
MAX_ROWS, MAX_INTERFACES = _lib.IFACE_MAX_ROWS, _lib.IFACE_MAX_INTERFACES
PER_INTERFACE_INTS = ("n_native", "n_model", "n_shared", "n_interface_rows", "status")
PER_INTERFACE = ("fnat", "fnonnat", "irmsd", "lrmsd", "dockq")
PER_ROW = ("res_native", "res_model", "res_shared", "interface_rows")
TRANSFORMS = {"interface_rotation": (3, 3), "interface_translation": (3,), "receptor_rotation": (3, 3), "receptor_translation": (3,)}
COVERAGE = {"ignore": _lib.MAP_IGNORE, "penalise": _lib.MAP_PENALISE}
CAPRI_BOUNDS = (0.23, 0.49, 0.80)  # DockQ at which the class becomes acceptable, medium, high


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


def chain_sides(chain_idx, chain_pairs=None):
    """``chain_idx`` [N]: the chain label of every row.  (sides int32 [I,N], labels int64 [I,2]): one interface per pair of chains - every
    pair of distinct labels in ascending order, or the listed ``chain_pairs`` [I,2] - with the chain of more rows as the receptor (ties:
    the lower label); ``labels[k]`` is (receptor label, ligand label)."""
    chain_idx = np.rint(_call.host(chain_idx)).astype(np.int64).reshape(-1)
    present = np.unique(chain_idx)
    if chain_pairs is None:
        chain_pairs = [(a, b) for i, a in enumerate(present) for b in present[i + 1:]]
    chain_pairs = np.asarray(chain_pairs, dtype=np.int64).reshape(-1, 2)
    sides, labels = np.zeros((len(chain_pairs), len(chain_idx)), dtype=np.int32), np.zeros((len(chain_pairs), 2), dtype=np.int64)
    for k, (a, b) in enumerate(chain_pairs):
        if a == b or a not in present or b not in present:
            raise ValueError(f"chain pair ({a}, {b}): two distinct labels of chain_idx are needed (labels {present.tolist()})")
        lo, hi = min(a, b), max(a, b)
        receptor, ligand = (hi, lo) if np.count_nonzero(chain_idx == hi) > np.count_nonzero(chain_idx == lo) else (lo, hi)
        sides[k, chain_idx == receptor], sides[k, chain_idx == ligand] = RECEPTOR, LIGAND
        labels[k] = receptor, ligand
    return sides, labels


def loop_sides(diffuse_mask, chain_idx, partner: str = "other_chains"):
    """``diffuse_mask`` [N] (non-zero: the row was diffused), ``chain_idx`` [N].  (sides int32 [I,N], chains int64 [I]): one interface per
    chain that has diffused rows, in ascending label order - the ligand is that chain's diffused rows, the receptor every row of the other
    chains (``partner="other_chains"``) or every undiffused row, the chain's own among them (``"rest"``)."""
    if partner not in ("other_chains", "rest"):
        raise ValueError(f"partner should be 'other_chains' or 'rest', got {partner!r}")
    diffused = _call.host(diffuse_mask).reshape(-1) != 0
    chain_idx = np.rint(_call.host(chain_idx)).astype(np.int64).reshape(-1)
    if diffused.shape != chain_idx.shape:
        raise ValueError(f"diffuse_mask {diffused.shape} and chain_idx {chain_idx.shape} differ")
    chains = np.unique(chain_idx[diffused])
    sides = np.zeros((len(chains), len(chain_idx)), dtype=np.int32)
    for k, c in enumerate(chains):
        sides[k, (chain_idx != c) if partner == "other_chains" else ~diffused] = RECEPTOR
        sides[k, diffused & (chain_idx == c)] = LIGAND
    return sides, chains.astype(np.int64)


def interface_accuracy(prot_a, prot_b=None, sides=None, atoms: str = "cb", res_mask=None, res_mask_b=None, atom_mask_a=None, atom_mask_b=None,
                       pairs=None, ref_index=None, contact_cutoff=None, interface_cutoff: float = 10.0, prune: bool = True, alignment=None,
                       coverage: str = "ignore") -> dict:
    """prot_a [S,N,37,3], [S,N,5,3] or a CA trace [S,N,3] float32, a device tensor (used in place) or a NumPy array (uploaded): the
    models; prot_b [S_b,N,...] likewise or None: the references.  ``sides`` int [I,N] (or [N]): 0 neither, 1 receptor, 2 ligand, one row
    per interface, shared by every pair.  ``atoms``: "ca", "cb" (CB where both structures have it, else CA), "backbone" (N, CA, C, CB, O)
    or "all" (atom37 in both).  res_mask [S,N], res_mask_b [S_b,N] (default: ones): a row takes part where both of its pair's structures
    have it.  atom_mask_a [S,N,atoms], atom_mask_b [S_b,N,atoms_b] (default: an atom exists where a coordinate is non-zero); an atom takes
    part where it exists in both structures, so a full-atom ground truth against a backbone sample is compared on their common atoms.

    * ``prot_b`` given: model i against reference ``ref_index[i]`` (default: row i where S_b = S, row 0 where S_b = 1).
    * ``prot_b`` None, ``pairs`` None: every ordered pair i != j of prot_a - the reference owns the native contacts - and the result carries
      ``matrix_dockq`` and ``matrix_fnat`` [I,S,S] (row = model, column = reference, unit diagonal): do the samples agree on the binding mode.
    * ``pairs`` [P,2]: (model: index into prot_a, reference: index into prot_b, or prot_a without it).
    ``contact_cutoff``: default 5 for "all" and "backbone", 8 for "ca" and "cb"; ``interface_cutoff``: which rows are interface rows.
    ``prune=False`` evaluates every residue pair across the sides; the result is the same bit for bit.

    Returns NumPy arrays: ``n_native``, ``n_model``, ``n_shared``, ``n_interface_rows``, ``status`` [P,I] int64 (``_lib.IFACE_*`` bits),
    ``fnat``, ``fnonnat``, ``irmsd``, ``lrmsd``, ``dockq`` [P,I] float64 (NaN with a status bit), ``res_native``, ``res_model``,
    ``res_shared`` [P,I,N] int64, ``interface_rows`` [P,I,N] bool, ``interface_rotation`` [P,I,3,3] and ``interface_translation`` [P,I,3]
    (R x + t ~ y, x the model: the superposition of irmsd), ``receptor_rotation`` and ``receptor_translation`` (of lrmsd), ``pairs``
    [P,2], ``atoms`` and the two cutoffs.

    ``alignment`` (int [N_b], or [P,N_b] per pair; NumPy or a device tensor): the rows of prot_b [S_b,N_b,...] need not be those of prot_a
    [S,N_a,...] - entry j is the row of the model that corresponds to row j of the reference, or -1 (``seq_align.chain_row_map``,
    ``row_map``, ``tm_align(...)["alignment"]``); the map need not be monotone (the model may store its chains in another order).  One
    call of ``fdipt_sample_interface_mapped``, DESIGN.md section 7.19.  The reference owns the rows: ``sides`` is [I,N_b], res_mask_b
    [S_b,N_b], every per-row output [P,I,N_b]; res_mask and atom_mask_a stay in the model's rows.  ``coverage``: "ignore" - a row takes part
    where it has a partner in the model, and the result is bit for bit that of the call without ``alignment`` on the gathered model;
    "penalise" - the native contacts and the interface rows are the reference's own, a model contact needs both rows in the model, so a
    missing residue costs fnat every native contact it is part of, and irmsd / lrmsd run over the rows the model has.  The result gains
    ``n_covered``, ``n_reference`` [P] int64, ``coverage`` [P] (their ratio, 0 for no reference row), ``n_interface_covered`` [P,I] (the
    interface rows that entered irmsd) and ``coverage_mode``.  A NumPy map that is out of range or uses a model row twice raises
    (``row_map.validate``); a device map sets ``_lib.IFACE_MAP_OUT_OF_RANGE`` / ``_lib.IFACE_MAP_DUPLICATE`` in ``status`` on every
    interface of its pair, whose outputs are those of a skipped pair."""
    if atoms not in MODES:
        raise ValueError(f"atoms should be 'ca', 'cb', 'backbone' or 'all', got {atoms!r}")
    if sides is None:
        raise ValueError("sides is required: chain_sides(chain_idx) or loop_sides(diffuse_mask, chain_idx) build it")
    mapped = alignment is not None
    if mapped and coverage not in COVERAGE:
        raise ValueError(f"coverage should be 'ignore' or 'penalise', got {coverage!r}")
    if not mapped and coverage != "ignore":
        raise ValueError(f"coverage={coverage!r} belongs to a call with an alignment")
    if mapped and prot_b is None:
        raise ValueError("alignment maps the rows of prot_b to those of prot_a: prot_b is required")
    s_a, n_a, atoms_a = _shape(prot_a, "prot_a")
    s_b, n, atoms_b = (s_a, n_a, atoms_a) if prot_b is None else _shape(prot_b, "prot_b")  # n: the rows of every per-row output, the reference's
    if not mapped and n != n_a:
        raise ValueError(f"prot_b {tuple(prot_b.shape)} does not have the {n_a} rows of prot_a")
    for what, layout in (("prot_a", atoms_a), ("prot_b", atoms_b)):
        if (atoms == "all" and layout != 37) or (atoms in ("cb", "backbone") and layout == 1):
            raise ValueError(f"atoms={atoms!r} needs {'atom37' if atoms == 'all' else 'the backbone atoms'}: {what} holds {layout} atom(s) per row")
    if prot_b is None and (atom_mask_b is not None or res_mask_b is not None):
        raise ValueError("atom_mask_b or res_mask_b without prot_b: the structures of prot_a carry atom_mask_a and res_mask")
    contact_cutoff = CONTACT_CUTOFF[atoms] if contact_cutoff is None else float(contact_cutoff)
    if not contact_cutoff > 0 or not interface_cutoff > 0:
        raise ValueError(f"the cutoffs should be positive, got contact_cutoff={contact_cutoff}, interface_cutoff={interface_cutoff}")
    sides_host = sides if hasattr(sides, "detach") else np.asarray(sides)
    sides_shape = tuple(sides_host.shape)
    if len(sides_shape) == 1:
        sides_shape = (1,) + sides_shape
    if len(sides_shape) != 2 or sides_shape[1] != n or sides_shape[0] < 1:
        raise ValueError(f"sides should be [I, {n}] (or [{n}]) with I >= 1{' - with an alignment the rows of prot_b, the reference -' if mapped else ''}, got "
                         f"{tuple(sides_host.shape)}")
    n_if = sides_shape[0]
    if prot_b is None and pairs is None and ref_index is None:
        pair_list, square = ordered_pairs(s_a), True
    else:
        pair_list, square = _call.plan_pairs(s_a, s_b, prot_b is not None, pairs, ref_index)
    n_pairs = len(pair_list)
    shape_a, shape_b = (s_a, n_a) + (() if atoms_a == 1 else (atoms_a,)), (s_b, n) + (() if atoms_b == 1 else (atoms_b,))
    _call.check_shapes((("res_mask", res_mask, (s_a, n_a)), ("res_mask_b", res_mask_b, (s_b, n)), ("atom_mask_a", atom_mask_a, shape_a),
                        ("atom_mask_b", atom_mask_b, shape_b)), mapped)
    if mapped:
        alignment = _call.check_map(alignment, n_pairs, n, n_a)
    per_interface_ints = PER_INTERFACE_INTS + (("n_interface_covered",) if mapped else ())
    ints = per_interface_ints + PER_ROW[:3]
    outputs = {key: ("int32", (n_pairs, n_if)) for key in per_interface_ints}
    outputs.update({key: ("float64", (n_pairs, n_if)) for key in PER_INTERFACE})
    outputs.update({key: ("int32", (n_pairs, n_if, n)) for key in PER_ROW})
    outputs.update({key: ("float64", (n_pairs, n_if) + shape) for key, shape in TRANSFORMS.items()})
    if n_pairs == 0:  # (one structure, all-against-all)
        out = _call.empty_outputs(outputs, ints)
    else:
        import torch
        dev, (xa, xb) = _call.upload("interface_accuracy", prot_a=prot_a, prot_b=prot_b)
        mask_a = _call.atom_mask(atom_mask_a, shape_a, "atom_mask_a", dev)
        mask_b = mask_a if prot_b is None else _call.atom_mask(atom_mask_b, shape_b, "atom_mask_b", dev)
        rows_b = None if prot_b is None else _call.per_row(res_mask_b, (s_b, n), "res_mask_b", "mask", default=1, dev=dev)
        entry = "fdipt_sample_interface_mapped" if mapped else "fdipt_sample_interface"
        call = (entry, _lib.InterfaceArgs, dev,
                dict(S=s_a, N=n, atoms=atoms_a, S_b=s_b, atoms_b=atoms_b, P=n_pairs, I=n_if, mode=MODES[atoms], flags=0 if prune else _lib.IFACE_NO_PRUNE,
                     contact_cutoff=contact_cutoff, interface_cutoff=float(interface_cutoff)),
                dict(prot=xa, prot_b=xb, res_mask=_call.per_row(res_mask, (s_a, n_a), "res_mask", "mask", default=1, dev=dev), res_mask_b=rows_b,
                     atom_mask_a=mask_a, atom_mask_b=mask_b, pairs=torch.from_numpy(pair_list).to(dev),
                     sides=_call.per_row(sides_host.reshape(n_if, n), (n_if, n), "sides", "int", dev=dev)),
                outputs)
        if mapped:
            out = _call.run_mapped(*call, dict(N_a=n_a, coverage=COVERAGE[coverage], map=_call.upload_map(alignment, n_pairs, n, dev), res_mask_b=rows_b,
                                               score_mask_b=None), widen=ints, workspace=(entry + "_workspace", n_pairs, n))
        else:
            out = _call.run(*call, widen=ints, workspace=(entry + "_workspace", n_pairs, n))
    out["interface_rows"] = out["interface_rows"] != 0
    out.update(pairs=pair_list.astype(np.int64), atoms=atoms, contact_cutoff=contact_cutoff, interface_cutoff=float(interface_cutoff))
    if mapped:
        _call.add_coverage(out, n_pairs)
        out["coverage_mode"] = coverage
    if square:
        for key, name in (("dockq", "matrix_dockq"), ("fnat", "matrix_fnat")):
            out[name] = np.tile(np.eye(s_a), (n_if, 1, 1))
            out[name][:, pair_list[:, 0], pair_list[:, 1]] = out[key].T
    return out


def global_dockq(result: dict, p: int) -> float:
    """This project's own one-number summary of pair ``p`` (NOT the DockQ program's global score): the mean of ``dockq[p]`` over the
    interfaces that have a native contact (``n_native > 0``).  Under ``coverage="penalise"`` (``result["coverage_mode"]``) an interface
    whose DockQ is NaN - the model lacks the rows of a superposition - counts as 0; otherwise (``"ignore"``, or a call without an
    alignment) it is left out.  NaN where no interface has a native contact, or none is left."""
    dockq = np.asarray(result["dockq"], dtype=np.float64)[p].reshape(-1)
    dockq = dockq[np.asarray(result["n_native"])[p].reshape(-1) > 0]
    dockq = np.nan_to_num(dockq, nan=0.0) if result.get("coverage_mode", "ignore") == "penalise" else dockq[~np.isnan(dockq)]
    return float(dockq.mean()) if dockq.size else float("nan")


def interface_metrics(result: dict, p: int, k: int) -> dict:
    """The flat entries of pair ``p`` on interface ``k`` for a metrics table: the four integers, ``fnat``, ``fnonnat``, ``irmsd``,
    ``lrmsd``, ``dockq`` (None for NaN), ``capri_class`` (None without a DockQ) and ``status``, as Python numbers."""
    number = lambda v: None if v != v else float(v)  # noqa: E731  (NaN: a status bit)
    dockq = number(result["dockq"][p, k])
    return {**{key: int(result[key][p, k]) for key in PER_INTERFACE_INTS[:4]}, **{key: number(result[key][p, k]) for key in PER_INTERFACE},
            "capri_class": None if dockq is None else int(capri_class(dockq)), "status": int(result["status"][p, k])}


def capri_class(dockq):
    """0 incorrect, 1 acceptable, 2 medium, 3 high: DockQ against 0.23, 0.49, 0.80 (a number or an array; NaN gives 0)."""
    with np.errstate(invalid="ignore"):
        return np.sum([np.asarray(dockq, dtype=np.float64) >= b for b in CAPRI_BOUNDS], axis=0)
