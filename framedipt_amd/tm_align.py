"""Structural alignment of samples on the device: the alignment search behind the all-against-all matrix of
evaluation/eval_denovo.py:hierarchy_diversity, which the reference fills with ``tmtools.tm_align``.

``tm_align`` is one call of ``fdipt_sample_tm_align`` (csrc/tmalign.hip, ABI in include/fdipt.h) for any number of pairs, all in
float64: a sequence-independent search over alignments of two CA traces - gapless threading, a dynamic programme on the traces'
secondary structure, one on secondary structure plus distance, each iterated by dynamic programming under the transform of the TM-score
seed search - then the TM-score of the best alignment per chain length.  DESIGN.md section 7.9 is the contract.  It is modelled on
Zhang & Skolnick's TM-align and is this project's own: ``tmtools`` was not at hand and no parity with it is claimed.  Where
``tm_score.tm_scores`` scores the row-by-row correspondence (the right quantity against a ground truth or a refold), this searches
for the correspondence, which is what the diversity of a de novo run needs: two samples that share a fold at a shifted or gapped
correspondence score high here and low there.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .tm_score import CA, all_pairs

MAX_ROWS = _lib.TMA_MAX_ROWS
OUTPUTS = ("tm", "tm_a", "tm_b", "rotation", "translation", "alignment", "n_aligned", "rmsd", "d0_a", "d0_b", "init_tm", "init_dp", "best_init", "status")
_INTS = ("alignment", "n_aligned", "init_dp", "best_init", "status")


def tm_align(prot_a, prot_b=None, mask_a=None, mask_b=None, pairs=None, ref_index=None) -> dict:
    """prot_a [S,N_a,37,3] or [S,N_a,5,3] float32, a device tensor (used in place) or a NumPy array (uploaded); prot_b [S_b,N_b,37 or
    5,3] likewise or None - N_b may differ from N_a.  mask_a [S,N_a], mask_b [S_b,N_b] (default: ones): each structure is taken over
    the rows where its own mask is set.

    * ``prot_b`` None, ``pairs`` None: all i < j of prot_a; the result carries ``matrix`` [S,S] with a unit diagonal, entry (i, j) =
      ``tm_b`` of the pair, mirrored to (j, i) as the reference mirrors it.
    * ``prot_b`` given: sample i against structure ``ref_index[i]`` of prot_b (default: row i where S_b = S, row 0 where S_b = 1).
    * ``pairs`` [P,2]: first index into prot_a, second into prot_b (prot_a without it).

    Returns NumPy arrays per pair: ``tm_a``, ``tm_b`` (normalised by the first and by the second structure's length), ``tm`` = ``tm_b``
    (NaN with a status bit), ``rotation`` [P,3,3] and ``translation`` [P,3] (R x + t ~ y, x the first structure), ``alignment`` [P,N_b]
    (the row of the first structure aligned with each row of the second, or -1), ``n_aligned``, ``rmsd``, ``d0_a``, ``d0_b``,
    ``init_tm`` [P,3], ``init_dp`` [P,3], ``best_init``, ``status``, and ``pairs`` [P,2]."""
    for name, x in (("prot_a", prot_a), ("prot_b", prot_b)):
        if x is not None and (len(x.shape) != 4 or tuple(x.shape[2:]) not in ((37, 3), (5, 3))):
            raise ValueError(f"{name} should be [S, N, 37, 3] or [S, N, 5, 3], got {tuple(x.shape)}")
    s_a, n_a = int(prot_a.shape[0]), int(prot_a.shape[1])
    if s_a < 1 or n_a < 1:
        raise ValueError(f"prot_a {tuple(prot_a.shape)}: no structures or no residues")
    s_b, n_b = (s_a, n_a) if prot_b is None else (int(prot_b.shape[0]), int(prot_b.shape[1]))
    if s_b < 1 or n_b < 1:
        raise ValueError(f"prot_b {tuple(prot_b.shape)}: no structures or no residues")
    if prot_b is None and mask_b is not None:
        raise ValueError("mask_b without prot_b: the structures of prot_a carry mask_a")
    square = prot_b is None and pairs is None and ref_index is None
    if pairs is not None:
        pair_list = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    elif prot_b is None and ref_index is None:
        pair_list = all_pairs(s_a)
    else:
        if ref_index is None:
            if s_b not in (1, s_a):
                raise ValueError(f"prot_b holds {s_b} structures for {s_a} samples: give ref_index or pairs")
            ref_index = np.arange(s_a) if s_b == s_a and s_b > 1 else np.zeros(s_a)
        pair_list = np.stack([np.arange(s_a), np.asarray(ref_index).reshape(s_a)], axis=1).astype(np.int32)
    n_pairs = len(pair_list)
    shapes = {"rotation": (3, 3), "translation": (3,), "alignment": (n_b,), "init_tm": (3,), "init_dp": (3,)}

    import torch
    lib = _lib.load()
    tensors = [x for x in (prot_a, prot_b) if torch.is_tensor(x)]
    for x in tensors:
        _lib.require_cuda(x, "tm_align")
        if x.dtype != torch.float32:
            raise ValueError(f"prot should be float32, got {x.dtype}")
    dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())

    def structures(x):
        return x.contiguous() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)

    def mask_of(m, s, n, what):
        if m is None:
            return torch.ones((s, n), dtype=torch.float32, device=dev)
        m = m.to(dev) if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m)).to(dev)
        if tuple(m.shape) != (s, n):
            raise ValueError(f"{what} {tuple(m.shape)} should be {(s, n)}")
        return (m != 0).to(torch.float32).contiguous()

    if n_pairs == 0:  # (one structure, all-against-all)
        out = {k: np.zeros((0,) + shapes.get(k, ()), dtype=np.int64 if k in _INTS else np.float64) for k in OUTPUTS}
    else:
        with torch.cuda.device(dev):
            xa = structures(prot_a)
            xb = None if prot_b is None else structures(prot_b)
            ma = mask_of(mask_a, s_a, n_a, "mask_a")
            mb = None if prot_b is None else mask_of(mask_b, s_b, n_b, "mask_b")
            out = {k: torch.zeros((n_pairs,) + shapes.get(k, ()), dtype=torch.int32 if k in _INTS else torch.float64, device=dev) for k in OUTPUTS}
            d_pairs = torch.from_numpy(pair_list).to(dev)
            p = _lib.ptr
            args = _lib.TmAlignArgs(S=s_a, N_a=n_a, atoms=int(prot_a.shape[2]), ca=CA, S_b=s_b, N_b=n_b,
                                    atoms_b=int(prot_a.shape[2] if prot_b is None else prot_b.shape[2]), P=n_pairs, prot=p(xa), mask=p(ma),
                                    prot_b=p(xb), mask_b=p(mb), pairs=p(d_pairs), workspace=None, workspace_bytes=0, **{k: p(v) for k, v in out.items()})
            _lib.check(lib.fdipt_sample_tm_align(C.byref(args), _lib.stream_ptr()), "fdipt_sample_tm_align")
            out = {k: v.cpu().numpy() for k, v in out.items()}
        for k in _INTS:
            out[k] = out[k].astype(np.int64)
    out["pairs"] = pair_list.astype(np.int64)
    if square:
        matrix = np.ones((s_a, s_a), dtype=np.float64)
        matrix[pair_list[:, 0], pair_list[:, 1]] = matrix[pair_list[:, 1], pair_list[:, 0]] = out["tm_b"]
        out["matrix"] = matrix
    return out


def tm_metrics(result: dict, p: int) -> dict:
    """The reference's ``{"tm_score": ...}`` entry of pair ``p`` of a ``tm_align`` result: ``calc_tm_score``'s second value, the score
    normalised by the second structure."""
    return {"tm_score": float(result["tm_b"][p])}
