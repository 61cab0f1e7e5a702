"""TM-score of samples on the device, and the diversity the reference derives from it: the ``tm_score`` key of
framedipt/analysis/metrics.py:protein_metrics (sample against ground truth over the diffused rows) and of the self-consistency table of
experiments/inference.py (sample against its refold), and evaluation/eval_denovo.py:hierarchy_diversity (all-against-all TM-scores of the
samples of one length, Ward linkage on ``1 - TM``, a cut at ``1 - tm_score_th``, ``diversity = clusters / samples``).

``tm_scores`` is one call of ``fdipt_sample_tm_score`` (csrc/tmscore.hip, ABI in include/fdipt.h) for any number of pairs, all in
float64.  What is computed is the TM-score of a GIVEN residue correspondence, row i with row i - Zhang & Skolnick's TMscore search over
seed superpositions - not TM-align's search over alignments; DESIGN.md section 7.8 is the contract.  The reference goes through
``tmtools.tm_align``, which was not at hand: no parity with it is claimed.  Where the two structures are the same chain at the same
length (ground truth, refold) the identity alignment is the one TM-align looks for and this is the quantity the reference means; in the
all-against-all matrix it is a lower bound of TM-align's score, so the diversity from it can only come out equal or higher.

``ward_clusters`` and ``diversity`` run on the host in NumPy (no SciPy).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

CA = 1  # the CA column of atom37 and of the five-atom layout N, CA, C, CB, O
MAX_ROWS = _lib.TM_MAX_ROWS
OUTPUTS = ("tm", "rotation", "translation", "n_aligned", "d0", "best_seed", "passes", "status")


def all_pairs(b: int) -> np.ndarray:
    """[b (b - 1) / 2, 2] int32: every i < j, i-major."""
    i, j = np.triu_indices(b, 1)
    return np.stack([i, j], axis=1).astype(np.int32)


def tm_scores(prot_a, prot_b=None, mask_a=None, mask_b=None, pairs=None, norm_length=None, ref_index=None) -> dict:
    """prot_a [S,N,37,3] or [S,N,5,3] float32, a device tensor (used in place: ``inference_fn(..., return_device=True)["prot_traj"][0]``)
    or a NumPy array (uploaded); prot_b [S_b,N,37 or 5,3] likewise or None.  mask_a [S,N], mask_b [S_b,N] (default: ones): a pair is
    scored over the rows where both of its structures' masks are set - ``protein_metrics`` passes ``diffuse_mask * bb_mask``.

    * ``prot_b`` None, ``pairs`` None: all i < j of prot_a; the result carries ``matrix`` [S,S] with a unit diagonal, entry (i, j)
      mirrored to (j, i) as the reference mirrors it.
    * ``prot_b`` given: sample i against structure ``ref_index[i]`` of prot_b (default: row i where S_b = S, row 0 where S_b = 1).
    * ``pairs`` [P,2]: first index into prot_a, second into prot_b (prot_a without it).
    ``norm_length`` [P] (or one number): the normalisation length L of a pair where > 0, else the number of rows scored.

    Returns NumPy arrays per pair: ``tm`` float64 (NaN with a status bit), ``rotation`` [P,3,3] and ``translation`` [P,3] (R x + t ~ y,
    x the first structure), ``n_aligned``, ``best_seed``, ``passes``, ``status`` int64, ``d0`` float64, and ``pairs`` [P,2].  The
    host does not wait for the device before the read-back."""
    for name, x in (("prot_a", prot_a), ("prot_b", prot_b)):
        if x is not None and (len(x.shape) != 4 or tuple(x.shape[2:]) not in ((37, 3), (5, 3))):
            raise ValueError(f"{name} should be [S, N, 37, 3] or [S, N, 5, 3], got {tuple(x.shape)}")
    s_a, n = int(prot_a.shape[0]), int(prot_a.shape[1])
    if s_a < 1 or n < 1:
        raise ValueError(f"prot_a {tuple(prot_a.shape)}: no structures or no residues")
    if prot_b is not None and int(prot_b.shape[1]) != n:
        raise ValueError(f"prot_b {tuple(prot_b.shape)} does not have the {n} rows of prot_a")
    s_b = s_a if prot_b is None else int(prot_b.shape[0])
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
    if norm_length is not None:
        norm_length = np.broadcast_to(np.asarray(norm_length, dtype=np.int32), (n_pairs,)).copy()
    empty = {"tm": np.zeros(0), "rotation": np.zeros((0, 3, 3)), "translation": np.zeros((0, 3)), "d0": np.zeros(0),
             **{k: np.zeros(0, dtype=np.int64) for k in ("n_aligned", "best_seed", "passes", "status")}}

    import torch
    lib = _lib.load()
    tensors = [x for x in (prot_a, prot_b) if torch.is_tensor(x)]
    for x in tensors:
        _lib.require_cuda(x, "tm_scores")
        if x.dtype != torch.float32:
            raise ValueError(f"prot should be float32, got {x.dtype}")
    dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())

    def structures(x):
        return x.contiguous() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)

    def mask_of(m, s, what):
        if m is None:
            return torch.ones((s, n), dtype=torch.float32, device=dev)
        m = m.to(dev) if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m)).to(dev)
        if tuple(m.shape) != (s, n):
            raise ValueError(f"{what} {tuple(m.shape)} should be {(s, n)}")
        return (m != 0).to(torch.float32).contiguous()

    if n_pairs == 0:  # (one structure, all-against-all)
        out = empty
    else:
        with torch.cuda.device(dev):
            xa = structures(prot_a)
            xb = None if prot_b is None else structures(prot_b)
            ma = mask_of(mask_a, s_a, "mask_a")
            mb = None if prot_b is None else mask_of(mask_b, s_b, "mask_b")
            if prot_b is None and mask_b is not None:
                raise ValueError("mask_b without prot_b: the structures of prot_a carry mask_a")
            zeros = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
            out = dict(tm=zeros(torch.float64, n_pairs), rotation=zeros(torch.float64, n_pairs, 3, 3), translation=zeros(torch.float64, n_pairs, 3),
                       n_aligned=zeros(torch.int32, n_pairs), d0=zeros(torch.float64, n_pairs), best_seed=zeros(torch.int32, n_pairs),
                       passes=zeros(torch.int32, n_pairs), status=zeros(torch.int32, n_pairs))
            d_pairs = torch.from_numpy(pair_list).to(dev)
            d_norm = None if norm_length is None else torch.from_numpy(norm_length).to(dev)
            p = _lib.ptr
            args = _lib.TmArgs(S=s_a, N=n, atoms=int(prot_a.shape[2]), ca=CA, S_b=s_b, atoms_b=int(prot_a.shape[2] if prot_b is None else prot_b.shape[2]),
                               P=n_pairs, prot=p(xa), mask=p(ma), prot_b=p(xb), mask_b=p(mb), pairs=p(d_pairs), norm_length=p(d_norm),
                               workspace=None, workspace_bytes=0, **{k: p(v) for k, v in out.items()})
            _lib.check(lib.fdipt_sample_tm_score(C.byref(args), _lib.stream_ptr()), "fdipt_sample_tm_score")
            out = {k: v.cpu().numpy() for k, v in out.items()}
        for k in ("n_aligned", "best_seed", "passes", "status"):
            out[k] = out[k].astype(np.int64)
    out["pairs"] = pair_list.astype(np.int64)
    if square:
        matrix = np.ones((s_a, s_a), dtype=np.float64)
        matrix[pair_list[:, 0], pair_list[:, 1]] = matrix[pair_list[:, 1], pair_list[:, 0]] = out["tm"]
        out["matrix"] = matrix
    return out


def tm_metrics(result: dict, p: int) -> dict:
    """The reference's ``{"tm_score": ...}`` entry (protein_metrics, the self-consistency table) of pair ``p`` of a ``tm_scores`` result."""
    return {"tm_score": float(result["tm"][p])}


def ward_linkage(distance) -> np.ndarray:
    """[S - 1, 4] float64, the rows (cluster a, cluster b, height, size) of ``scipy.cluster.hierarchy.linkage(squareform(distance),
    method="ward")``: the closest two clusters merge (the lowest pair of indices among equals), distances to the merged cluster follow
    Lance & Williams' update for Ward's criterion, d(k, i + j)^2 = ((n_i + n_k) d_ik^2 + (n_j + n_k) d_jk^2 - n_k d_ij^2) / (n_i + n_j + n_k)."""
    d = np.array(distance, dtype=np.float64)
    s = d.shape[0]
    if d.shape != (s, s) or s < 1:
        raise ValueError(f"distance should be a square matrix, got {d.shape}")
    np.fill_diagonal(d, np.inf)
    size, label, alive = np.ones(s), np.arange(s), np.ones(s, dtype=bool)
    out = np.zeros((s - 1, 4))
    for step in range(s - 1):
        masked = np.where(alive[:, None] & alive[None, :], d, np.inf)
        i, j = divmod(int(np.argmin(masked)), s)
        if i > j:
            i, j = j, i
        dij = d[i, j]
        out[step] = min(label[i], label[j]), max(label[i], label[j]), dij, size[i] + size[j]
        rest = alive.copy()
        rest[[i, j]] = False
        total = size[i] + size[j] + size[rest]
        merged = np.sqrt(np.maximum(((size[i] + size[rest]) * d[i, rest] ** 2 + (size[j] + size[rest]) * d[j, rest] ** 2 - size[rest] * dij ** 2) / total, 0.0))
        d[i, rest] = d[rest, i] = merged
        alive[j] = False
        size[i] += size[j]
        label[i] = s + step
    return out


def ward_clusters(matrix, tm_score_th: float = 0.5) -> np.ndarray:
    """[S] int64 labels 1 .. clusters of ``fcluster(linkage(1 - matrix, "ward"), t=1 - tm_score_th, criterion="distance")``, numbered in the
    order in which the samples first appear: the samples that merges of height <= 1 - tm_score_th join share a label."""
    matrix = np.asarray(matrix, dtype=np.float64)
    if matrix.ndim != 2 or matrix.shape[0] != matrix.shape[1] or matrix.shape[0] < 1:
        raise ValueError(f"matrix should be square, got {matrix.shape}")
    if not np.all(np.isfinite(matrix)):
        raise ValueError("matrix holds TM-scores that are not finite (pairs with a status bit): no clustering")
    s = matrix.shape[0]
    tree = ward_linkage(1.0 - matrix)
    members = [[k] for k in range(s)] + [None] * (s - 1)
    root = list(range(s))  # sample -> the cluster it has been merged into below the cut
    for step, (a, b, height, _) in enumerate(tree):
        members[s + step] = members[int(a)] + members[int(b)]
        if height <= 1.0 - tm_score_th:  # (Ward heights ascend: a merge above the cut has only merges above it over it)
            for k in members[s + step]:
                root[k] = s + step
    names, labels = {}, np.zeros(s, dtype=np.int64)
    for k in range(s):
        labels[k] = names.setdefault(root[k], len(names) + 1)
    return labels


def diversity(matrix, tm_score_th: float = 0.5) -> dict:
    """``hierarchy_diversity`` of a TM-score matrix: {"labels", "clusters", "samples", "diversity" = clusters / samples}."""
    labels = ward_clusters(matrix, tm_score_th)
    return {"labels": labels, "clusters": int(labels.max()), "samples": int(len(labels)), "diversity": float(labels.max()) / len(labels)}
