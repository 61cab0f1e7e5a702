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

import numpy as np

from . import _call, _lib
from ._call import all_pairs  # noqa: F401  (part of this module's interface)

CA = 1  # the CA column of atom37 and of the five-atom layout N, CA, C, CB, O
MAX_ROWS = _lib.TM_MAX_ROWS
OUTPUTS = ("tm", "rotation", "translation", "n_aligned", "d0", "best_seed", "passes", "status")
_INTS = ("n_aligned", "best_seed", "passes", "status")


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
    shapes = {"rotation": (3, 3), "translation": (3,)}
    outputs = {k: ("int32" if k in _INTS else "float64", (n_pairs,) + shapes.get(k, ())) for k in OUTPUTS}
    if n_pairs == 0:  # (one structure, all-against-all)
        out = _call.empty_outputs(outputs, _INTS)
    else:
        import torch
        dev, (xa, xb) = _call.upload("tm_scores", prot_a=prot_a, prot_b=prot_b)
        out = _call.run("fdipt_sample_tm_score", _lib.TmArgs, dev, dict(S=s_a, N=n, atoms=atoms_a, ca=CA, S_b=s_b, atoms_b=atoms_b, P=n_pairs),
                        dict(prot=xa, mask=_call.per_row(mask_a, (s_a, n), "mask_a", "mask", default=1, dev=dev), prot_b=xb,
                             mask_b=None if prot_b is None else _call.per_row(mask_b, (s_b, n), "mask_b", "mask", default=1, dev=dev),
                             pairs=torch.from_numpy(pair_list).to(dev), norm_length=None if norm_length is None else torch.from_numpy(norm_length).to(dev)),
                        outputs, widen=_INTS)
    out["pairs"] = pair_list.astype(np.int64)
    if square:
        out["matrix"] = _call.square_matrix(s_a, pair_list, out["tm"])
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
