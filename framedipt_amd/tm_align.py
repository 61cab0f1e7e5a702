"""Structural alignment of samples on the device: the alignment search behind the all-against-all matrix of
evaluation/eval_denovo.py:hierarchy_diversity, which the reference fills with ``tmtools.tm_align``.

``tm_align`` is one call of ``fdipt_sample_tm_align`` (csrc/tmalign.hip, ABI in include/fdipt.h) for any number of pairs, all in
float64: a sequence-independent search over alignments of two CA traces - gapless threading, a dynamic programme on the traces'
secondary structure, one on secondary structure plus distance, each iterated by dynamic programming under the transform of the TM-score
seed search - then the TM-score of the best alignment per chain length.  ``inits="all"`` adds two fragment-based initial alignments (a
grid of local superpositions, and the threading of the longest unbroken run) for pairs that share a motif the three cannot see.
DESIGN.md section 7.9 is the contract.  It is modelled on
Zhang & Skolnick's TM-align and is this project's own: ``tmtools`` was not at hand and no parity with it is claimed.  Where
``tm_score.tm_scores`` scores the row-by-row correspondence (the right quantity against a ground truth or a refold), this searches
for the correspondence, which is what the diversity of a de novo run needs: two samples that share a fold at a shifted or gapped
correspondence score high here and low there.
"""
from __future__ import annotations

import numpy as np

from . import _call, _lib
from .tm_score import CA, all_pairs  # noqa: F401  (all_pairs: part of this module's interface)

MAX_ROWS = _lib.TMA_MAX_ROWS
OUTPUTS = ("tm", "tm_a", "tm_b", "rotation", "translation", "alignment", "n_aligned", "rmsd", "d0_a", "d0_b", "init_tm", "init_dp", "best_init", "status")
_INTS = ("alignment", "n_aligned", "init_dp", "best_init", "status")
INITS = {"default": _lib.TMA_INITS_DEFAULT, "all": _lib.TMA_INITS_ALL}
N_INITS = {"default": 3, "all": 5}


def check_inits(inits) -> str:
    """``inits`` if it names a mode of the search; ValueError otherwise (before any launch)."""
    if not isinstance(inits, str) or inits not in INITS:
        raise ValueError(f"inits should be one of {sorted(INITS)}, got {inits!r}")
    return inits


def tm_align(prot_a, prot_b=None, mask_a=None, mask_b=None, pairs=None, ref_index=None, inits: str = "default") -> dict:
    """prot_a [S,N_a,37,3] or [S,N_a,5,3] float32, a device tensor (used in place) or a NumPy array (uploaded); prot_b [S_b,N_b,37 or
    5,3] likewise or None - N_b may differ from N_a.  mask_a [S,N_a], mask_b [S_b,N_b] (default: ones): each structure is taken over
    the rows where its own mask is set.

    * ``prot_b`` None, ``pairs`` None: all i < j of prot_a; the result carries ``matrix`` [S,S] with a unit diagonal, entry (i, j) =
      ``tm_b`` of the pair, mirrored to (j, i) as the reference mirrors it.
    * ``prot_b`` given: sample i against structure ``ref_index[i]`` of prot_b (default: row i where S_b = S, row 0 where S_b = 1).
    * ``pairs`` [P,2]: first index into prot_a, second into prot_b (prot_a without it).
    * ``inits``: ``"default"`` (gapless threading, secondary structure, secondary structure plus distance) or ``"all"``: those three
      and then a local-superposition and a fragment-threading start, each through the same iteration.  Columns 0 .. 2 of ``init_tm``
      and ``init_dp`` and every output of a pair whose ``best_init`` is at most 2 equal the default's bit for bit; the search's own score ``S / Ls`` can only rise.

    Returns NumPy arrays per pair: ``tm_a``, ``tm_b`` (normalised by the first and by the second structure's length), ``tm`` = ``tm_b``
    (NaN with a status bit), ``rotation`` [P,3,3] and ``translation`` [P,3] (R x + t ~ y, x the first structure), ``alignment`` [P,N_b]
    (the row of the first structure aligned with each row of the second, or -1), ``n_aligned``, ``rmsd``, ``d0_a``, ``d0_b``,
    ``init_tm`` [P,3], ``init_dp`` [P,3] ([P,5] with ``inits="all"``), ``best_init``, ``status``, and ``pairs`` [P,2]."""
    n_inits = N_INITS[check_inits(inits)]
    s_a, n_a, atoms_a = _call.structure_shape(prot_a, "prot_a", lead="S", items="structures")
    s_b, n_b, atoms_b = (s_a, n_a, atoms_a) if prot_b is None else _call.structure_shape(prot_b, "prot_b", lead="S", items="structures")
    if prot_b is None and mask_b is not None:
        raise ValueError("mask_b without prot_b: the structures of prot_a carry mask_a")
    pair_list, square = _call.plan_pairs(s_a, s_b, prot_b is not None, pairs, ref_index)
    n_pairs = len(pair_list)
    shapes = {"rotation": (3, 3), "translation": (3,), "alignment": (n_b,), "init_tm": (n_inits,), "init_dp": (n_inits,)}
    outputs = {k: ("int32" if k in _INTS else "float64", (n_pairs,) + shapes.get(k, ())) for k in OUTPUTS}
    if n_pairs == 0:  # (one structure, all-against-all)
        out = _call.empty_outputs(outputs, _INTS)
    else:
        import torch
        dev, (xa, xb) = _call.upload("tm_align", prot_a=prot_a, prot_b=prot_b)
        out = _call.run("fdipt_sample_tm_align", _lib.TmAlignArgs, dev,
                        dict(S=s_a, N_a=n_a, atoms=atoms_a, ca=CA, S_b=s_b, N_b=n_b, atoms_b=atoms_b, P=n_pairs, inits=INITS[inits]),
                        dict(prot=xa, mask=_call.per_row(mask_a, (s_a, n_a), "mask_a", "mask", default=1, dev=dev), prot_b=xb,
                             mask_b=None if prot_b is None else _call.per_row(mask_b, (s_b, n_b), "mask_b", "mask", default=1, dev=dev),
                             pairs=torch.from_numpy(pair_list).to(dev)),
                        outputs, widen=_INTS)
    out["pairs"] = pair_list.astype(np.int64)
    if square:
        out["matrix"] = _call.square_matrix(s_a, pair_list, out["tm_b"])
    return out

def tm_metrics(result: dict, p: int) -> dict:
    """The reference's ``{"tm_score": ...}`` entry of pair ``p`` of a ``tm_align`` result: ``calc_tm_score``'s second value, the score
    normalised by the second structure."""
    return {"tm_score": float(result["tm_b"][p])}
