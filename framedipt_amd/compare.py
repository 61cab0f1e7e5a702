"""Accuracy of a model against a reference whose rows do not correspond: align first, then score through the alignment.

``aligned_accuracy`` runs the alignment search (``tm_align.tm_align``), hands its ``alignment`` - the row of the model aligned with each
row of the reference, or -1 - to the two mapped accuracy entries (``lddt.local_accuracy`` and ``gdt.gdt_scores`` with ``alignment=``;
DESIGN.md section 7.16) and returns one dict.  The reference owns the rows: every per-row output has the reference's N_b rows, lDDT
under ``coverage="penalise"`` charges the reference rows the model has no partner for, and GDT is divided by the reference's rows.
For a correspondence known beforehand - residue numbers, a deletion - build the map with ``row_map`` and call the two entries directly.
``sequence_aligned_accuracy`` takes the map from the sequences instead (``seq_align.chain_row_map``: a global alignment per chain, what the
reference's ``framedipt/protein/align.py`` does before it superposes).
"""
from __future__ import annotations

import numpy as np

from . import gdt, interface, lddt, seq_align, tm_align

_LDDT_KEYS = ("lddt", "res_lddt", "n_scored", "n_passed", "drmsd", "fape", "res_fape", "region_fape", "n_covered", "n_reference", "coverage")
_GDT_KEYS = ("gdt_ts", "gdt_ha", "counts", "res_within", "rotation", "translation")


def aligned_accuracy(prot_a, prot_b, mask_a=None, mask_b=None, pairs=None, ref_index=None, inits: str = "default", atoms: str = "ca",
                     coverage: str = "penalise", superpose: str = "search") -> dict:
    """prot_a [S,N_a,37,3] or [S,N_a,5,3]: the models; prot_b [S_b,N_b,37 or 5,3]: the references (device tensors or NumPy arrays, as
    ``tm_align`` takes them); mask_a [S,N_a], mask_b [S_b,N_b]: the rows of each structure; ``pairs`` / ``ref_index``: as ``tm_align``
    plans them (default: model i against reference i, or against the one reference).  ``inits``: the search's initial alignments;
    ``atoms`` / ``coverage``: the lDDT atom set and switch; ``superpose``: the GDT mode.

    Returns per pair ``tm`` (normalised by the reference), ``tm_a``, ``tm_b``, ``rmsd``, ``n_aligned``, ``alignment`` [P,N_b] and the
    search's ``rotation`` / ``translation`` as ``tm_rotation`` / ``tm_translation``; the lDDT outputs ``lddt``, ``res_lddt`` [P,N_b],
    ``n_scored``, ``n_passed``, ``drmsd``, ``fape``, ``res_fape``, ``region_fape``, ``n_covered``, ``n_reference``, ``coverage``; the GDT
    outputs ``gdt_ts``, ``gdt_ha`` (divided by the reference's masked rows), ``counts``, ``res_within`` [P,N_b], ``rotation``,
    ``translation`` [P,5,...]; the three status words ``tm_status``, ``lddt_status``, ``gdt_status``; ``pairs`` and ``atoms``."""
    if prot_b is None:
        raise ValueError("aligned_accuracy scores models against references: prot_b is required")
    found = tm_align.tm_align(prot_a, prot_b, mask_a=mask_a, mask_b=mask_b, pairs=pairs, ref_index=ref_index, inits=inits)
    pair_list, maps = found["pairs"], found["alignment"].astype("int32")
    local = lddt.local_accuracy(prot_a, prot_b, atoms=atoms, res_mask=mask_a, res_mask_b=mask_b, pairs=pair_list, alignment=maps, coverage=coverage)
    glob = gdt.gdt_scores(prot_a, prot_b, mask_a=mask_a, mask_b=mask_b, pairs=pair_list, alignment=maps, norm_length="reference", superpose=superpose)
    out = {k: found[k] for k in ("tm", "tm_a", "tm_b", "rmsd", "n_aligned", "alignment", "pairs")}
    out.update(tm_rotation=found["rotation"], tm_translation=found["translation"], tm_status=found["status"])
    out.update({k: local[k] for k in _LDDT_KEYS})
    out.update({k: glob[k] for k in _GDT_KEYS})
    out.update(lddt_status=local["status"], gdt_status=glob["status"], atoms=atoms, coverage_mode=coverage, superpose=superpose)
    return out


def sequence_aligned_accuracy(prot_a, aatype_a, prot_b, aatype_b, chain_a=None, chain_b=None, chain_pairs=None, mask_a=None, mask_b=None,
                              pairs=None, ref_index=None, atoms: str = "ca", coverage: str = "penalise", superpose: str = "search", **scoring) -> dict:
    """prot_a [S,N_a,37 or 5,3]: the models, which share the residue types aatype_a [N_a] and the chain labels chain_a [N_a]; prot_b
    [S_b,N_b,37 or 5,3]: the references with aatype_b [N_b], chain_b [N_b].  The rows are matched by ``seq_align.chain_row_map`` (chains
    with equal labels, or ``chain_pairs``; ``scoring``: its ``matrix``, ``open_gap``, ``extend_gap``, ``mode``, ``free_ends``, ``exclude_a``,
    ``exclude_b`` - ``mode="semiglobal", free_ends="a"`` for a reference that lacks termini), and the one map serves every pair of
    ``local_accuracy(..., alignment=, coverage=)`` and ``gdt_scores(..., alignment=, norm_length="reference")``.

    Returns ``alignment`` [N_b], ``chains`` and per chain pair ``score``, ``identity``, ``identity_b``, ``n_identical``, ``n_aligned``,
    ``seq_status``; per pair of structures the lDDT and GDT outputs of ``aligned_accuracy`` (``lddt``, ``res_lddt`` [P,N_b], ``gdt_ts``,
    ``gdt_ha``, ``n_covered``, ...), ``lddt_status``, ``gdt_status``; ``atoms``, ``coverage_mode``, ``superpose``."""
    if prot_b is None:
        raise ValueError("sequence_aligned_accuracy scores models against references: prot_b is required")
    n_a, n_b = int(prot_a.shape[1]), int(prot_b.shape[1])
    for what, aatype, n in (("aatype_a", aatype_a, n_a), ("aatype_b", aatype_b, n_b)):
        if len(aatype) != n:
            raise ValueError(f"{what} holds {len(aatype)} letters for {n} rows")
    found = seq_align.chain_row_map(aatype_a, chain_a, aatype_b, chain_b, chain_pairs=chain_pairs, **scoring)
    m = found["alignment"]
    local = lddt.local_accuracy(prot_a, prot_b, atoms=atoms, res_mask=mask_a, res_mask_b=mask_b, pairs=pairs, ref_index=ref_index, alignment=m, coverage=coverage)
    glob = gdt.gdt_scores(prot_a, prot_b, mask_a=mask_a, mask_b=mask_b, pairs=pairs, ref_index=ref_index, alignment=m, norm_length="reference", superpose=superpose)
    out = {k: found[k] for k in ("alignment", "chains", "score", "identity", "identity_b", "n_identical", "n_aligned")}
    out.update({k: local[k] for k in _LDDT_KEYS})
    out.update({k: glob[k] for k in _GDT_KEYS})
    out.update(seq_status=found["status"], lddt_status=local["status"], gdt_status=glob["status"], pairs=local["pairs"], atoms=atoms, coverage_mode=coverage,
               superpose=superpose)
    return out


def sequence_aligned_interface(prot_a, aatype_a, prot_b, aatype_b, chain_a, chain_b, chain_pairs=None, interfaces=None, atoms: str = "cb",
                               coverage: str = "penalise", mask_a=None, mask_b=None, atom_mask_a=None, atom_mask_b=None, pairs=None, ref_index=None,
                               contact_cutoff=None, interface_cutoff: float = 10.0, prune: bool = True, **scoring) -> dict:
    """The docking question for a model from another tool, or a ground truth read from its own file: prot_a [S,N_a,...] are the models
    with residue types aatype_a [N_a] and chain labels chain_a [N_a]; prot_b [S_b,N_b,...] the references with aatype_b, chain_b [N_b].
    The rows are matched by ``seq_align.chain_row_map`` (chains with equal labels, or ``chain_pairs`` [(label_a, label_b)]; ``scoring``:
    its ``matrix``, ``open_gap``, ``extend_gap``, ``mode``, ``free_ends``, ``exclude_a``, ``exclude_b``) - the model may store its chains in
    another order, the map is then not monotone -, the
    interfaces are ``interface.chain_sides(chain_b, interfaces)`` (``interfaces``: pairs of the REFERENCE's chain labels; default: every
    pair), and ``interface.interface_accuracy(..., alignment=, coverage=)`` scores every pair of structures in one call.  The sibling of
    ``sequence_aligned_accuracy``; no parity with the DockQ program is claimed.

    Returns ``alignment`` [N_b], ``chains`` and per chain pair ``score``, ``identity``, ``identity_b``, ``n_identical``, ``n_aligned``,
    ``seq_status``; every output of ``interface_accuracy`` with an alignment (``dockq``, ``fnat`` [P,I], ``n_covered``,
    ``n_interface_covered``, ...); ``sides`` [I,N_b], ``labels`` [I,2] (receptor, ligand: the reference's chain labels) and
    ``global_dockq`` [P] (``interface.global_dockq``: this project's own summary)."""
    if prot_b is None:
        raise ValueError("sequence_aligned_interface scores models against references: prot_b is required")
    n_a, n_b = int(prot_a.shape[1]), int(prot_b.shape[1])
    for what, x, n in (("aatype_a", aatype_a, n_a), ("aatype_b", aatype_b, n_b), ("chain_a", chain_a, n_a), ("chain_b", chain_b, n_b)):
        if x is None or len(x) != n:
            raise ValueError(f"{what} should hold one entry for each of the {n} rows" + ("" if x is None else f", got {len(x)}"))
    sides, labels = interface.chain_sides(chain_b, interfaces)
    found = seq_align.chain_row_map(aatype_a, chain_a, aatype_b, chain_b, chain_pairs=chain_pairs, **scoring)
    out = interface.interface_accuracy(prot_a, prot_b, sides, atoms=atoms, res_mask=mask_a, res_mask_b=mask_b, atom_mask_a=atom_mask_a, atom_mask_b=atom_mask_b,
                                       pairs=pairs, ref_index=ref_index, contact_cutoff=contact_cutoff, interface_cutoff=interface_cutoff, prune=prune,
                                       alignment=found["alignment"], coverage=coverage)
    out.update({k: found[k] for k in ("alignment", "chains", "score", "identity", "identity_b", "n_identical", "n_aligned")})
    out.update(seq_status=found["status"], sides=sides, labels=labels)
    out["global_dockq"] = np.array([interface.global_dockq(out, p) for p in range(len(out["pairs"]))], dtype=np.float64)
    return out


def aligned_metrics(result: dict, p: int) -> dict:
    """The flat entries of pair ``p`` for a metrics table, as Python numbers."""
    return {"tm_score": float(result["tm"][p]), lddt.METRIC_NAMES[result["atoms"]]: float(result["lddt"][p]), "gdt_ts": float(result["gdt_ts"][p]),
            "gdt_ha": float(result["gdt_ha"][p]), "drmsd": float(result["drmsd"][p]), "n_aligned": int(result["n_aligned"][p]),
            "n_covered": int(result["n_covered"][p]), "n_reference": int(result["n_reference"][p]), "coverage": float(result["coverage"][p])}
