"""NumPy restatement of sample selection (framedipt_amd/csrc/select.hip; contract in include/fdipt.h) — test infrastructure.

Two forms of the geometric median: ``plain_median`` is the reference's Weiszfeld loop on the flattened ``(S, M)`` coordinates
(evaluation/utils/sample_selection.py:82-106), ``weight_median`` the iteration on the weights of the affine combination
``mu + sum_s w_s (x_s - mu)`` that the kernel runs.  Everything is float64; atoms are in the reference's BACKBONE_ATOMS order C, N, CA, O.
"""
import numpy as np

BACKBONE_COLUMNS = (2, 0, 1, 4)
ZERO_DISTANCE = 1


def gather(prot, residues, members=None):
    """[S,L,4,3] float64: the backbone atoms of the diffused residues of the group's members."""
    prot = np.asarray(prot)
    if members is not None:
        prot = prot[np.asarray(members)]
    return prot[:, np.asarray(residues)][:, :, list(BACKBONE_COLUMNS)].astype(np.float64)


def plain_median(x, max_iterations=10000):
    """The reference's loop on x [S,L,4,3]: no convergence test; a zero distance gives NaN there (S = 1 always does)."""
    flat = x.reshape(x.shape[0], -1)
    out = flat.mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(max_iterations):
            dist = np.linalg.norm(flat - out[None], ord=2, axis=-1)
            out = (flat / dist[:, None]).sum(axis=0) / (1 / dist).sum()
    return out.reshape(x.shape[1:])


def pair_statistics(x):
    """(D, G): squared distances summed directly, Gram matrix of the mean-centred samples."""
    flat = x.reshape(x.shape[0], -1)
    c = flat - flat.mean(axis=0)[None]
    return ((flat[:, None, :] - flat[None, :, :]) ** 2).sum(axis=-1), c @ c.T


def weight_median(x, max_iterations=10000):
    """(median [L,4,3], w [S], status): the iteration in weight space with the kernel's zero-distance rule."""
    s = x.shape[0]
    mu = x.mean(axis=0)
    _, g = pair_statistics(x)
    diag = np.diag(g).copy()
    w = np.full(s, 1.0 / s)
    for _ in range(max_iterations):
        gw = g @ w
        d = np.sqrt(np.maximum(diag - 2.0 * gw + w @ gw, 0.0))
        if (d == 0).any():
            hit = int(np.argmax(d == 0))
            return x[hit].copy(), np.eye(s)[hit], ZERO_DISTANCE
        inv = 1.0 / d
        w = inv / inv.sum()
    return mu + np.tensordot(w, x - mu[None], axes=1), w, 0


def closest_distances(x, ref):
    """get_closest_index's criterion: per sample the sum over atoms of the Euclidean distance to ref [L,4,3]."""
    return np.linalg.norm(x - ref[None], axis=-1).sum(axis=(-2, -1))


def select(x, sigma=30.0, max_iterations=10000, median="weights"):
    """All outputs of the kernel for one group x [S,L,4,3]."""
    d2, _ = pair_statistics(x)
    density = np.exp(-d2 / sigma ** 2).sum(axis=1)
    mean = x.mean(axis=0)
    if median == "weights":
        med, w, status = weight_median(x, max_iterations)
    else:
        med, w, status = plain_median(x, max_iterations), None, 0
    dm, dd = closest_distances(x, mean), closest_distances(x, med)
    return {"mean": mean, "median": med, "weights": w, "density": density, "dist_to_mean": dm, "dist_to_median": dd,
            "mode": int(density.argmax()), "mean_closest": int(dm.argmin()), "median_closest": int(dd.argmin()), "status": status}


# ---------------------------------------------------------------------------------------------------------------------
# The fixture tests/golden/selection_cases.npz (made by tests/golden/make_goldens_selection.py): per case the backbone block of every
# sample, atom37 columns 0 .. 4 (N, CA, C, CB, O) as float32 [S,N,5,3], its diffuse mask [N] and what the reference returned.
CASES = ("s5_two_chains", "s7_l40", "s64_l21", "s33_l9", "s3_l1", "s1_l4", "s5_outlier")


def case_inputs(fix, name):
    """(prot [S,N,37,3] float32, diffuse_mask [S,N] float32) of a fixture case; the columns the fixture does not hold are zero."""
    bb = fix[f"{name}.bb"]
    prot = np.zeros(bb.shape[:2] + (37, 3), dtype=np.float32)
    prot[:, :, :5] = bb
    return prot, np.tile(fix[f"{name}.mask"].astype(np.float32)[None], (bb.shape[0], 1))


def coordinate_bound(fix, name, factor=32.0):
    """Bound on |coordinate - reference|: ``factor`` x the reference's own spread under a permutation of its samples (``perm_diff``);
    cases whose perm_diff is 0 take the largest of the fixture."""
    own = float(fix[f"{name}.perm_diff"])
    return factor * (own if own > 0 else max(float(fix[f"{c}.perm_diff"]) for c in CASES))


def joint_batch(fix, names=CASES):
    """All cases in one batch: (prot [B,N,37,3], mask [B,N], groups [B]) padded to the longest case plus one row (N odd or not, the
    padded rows are zero with diffuse_mask = 0) — mixed S and L in one launch."""
    parts = [case_inputs(fix, n) for n in names]
    n_max = max(p.shape[1] for p, _ in parts) + 1
    if n_max % 4 == 0:
        n_max += 1
    prot = np.zeros((sum(p.shape[0] for p, _ in parts), n_max, 37, 3), dtype=np.float32)
    mask = np.zeros(prot.shape[:2], dtype=np.float32)
    groups = np.zeros(prot.shape[0], dtype=np.int64)
    b = 0
    for g, (p, m) in enumerate(parts):
        prot[b:b + p.shape[0], :p.shape[1]] = p
        mask[b:b + p.shape[0], :p.shape[1]] = m
        groups[b:b + p.shape[0]] = 100 + g
        b += p.shape[0]
    return prot, mask, groups
