"""NumPy float64 restatement of the structural-violation block (openfold/utils/loss.py: between_residue_bond_loss,
between_residue_clash_loss, within_residue_violations, find_structural_violations, extreme_ca_ca_distance_violations,
compute_violation_metrics) as framedipt/analysis/metrics.py:protein_metrics calls it: every residue ALA, tolerance factor 12, overlap
tolerance 1.5.  Dense and obvious ((n, n, 5, 5) arrays), for the tests only.  Atom columns are atom37's N, CA, C, CB, O."""
import numpy as np

CASES = ("n1", "n2", "n65", "masked", "gaps", "clashy", "clean", "n260")
SCALARS = ("bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "angles_c_n_ca_loss_mean", "clashes_mean_loss",
           "violations_extreme_ca_ca_distance", "violations_between_residue_bond", "violations_between_residue_clash",
           "violations_within_residue", "violations_per_residue")
FLOAT_OUTPUTS = SCALARS + ("connections_per_residue_loss_sum", "clashes_per_atom_loss_sum", "within_per_atom_loss_sum")
EXACT_OUTPUTS = ("num_residue_violations", "n_clash_pairs", "connections_per_residue_violation_mask", "total_per_residue_violations_mask",
                 "clashes_per_atom_clash_mask", "within_per_atom_violations")
MASK_KINDS = ("extreme_ca_ca", "bond", "angle_ca_c_n", "angle_c_n_ca", "clash", "within_low", "within_high")

RADIUS = np.array([1.55, 1.7, 1.7, 1.7, 1.52])  # van der Waals radii of N, CA, C, CB, O
# the C-N length, its stddev and 12 x the stddev reach the reference's arithmetic as float32 values
C_N_LENGTH, C_N_TOLERANCE = float(np.float32(1.329)), float(np.float32(12.0) * np.float32(0.014))
COS_CA_C_N, CA_C_N_TOLERANCE = -0.4473, 12 * 0.014  # (the C-N bond's stddev, as the reference has it)
COS_C_N_CA, C_N_CA_TOLERANCE = -0.5203, 12 * 0.0353
CA_CA = 3.80209737096
# make_atom14_dists_bounds(1.5, 12) of ALA (float32 values) in the order N, CA, C, CB, O
LOWER = np.array([[0.0, 1.21899998, 1.88165307, 2.06256866, 1.57000005], [1.21899998, 0.0, 1.21300006, 1.26800001, 1.9400022],
                  [1.88165307, 1.21300006, 0.0, 2.06785154, 1.00100005], [2.06256866, 1.26800001, 2.06785154, 0.0, 1.72000003],
                  [1.57000005, 1.9400022, 1.00100005, 1.72000003, 0.0]], dtype=np.float32).astype(np.float64)
UPPER = np.array([[0.0, 1.699, 3.03730035, 2.82141972, 1e10], [1.699, 0.0, 1.83700001, 1.77199996, 2.84160995],
                  [3.03730035, 1.83700001, 0.0, 2.92383409, 1.45700002], [2.82141972, 1.77199996, 2.92383409, 0.0, 1e10],
                  [1e10, 2.84160995, 1.45700002, 1e10, 0.0]], dtype=np.float32).astype(np.float64)


def relu(x):
    return np.maximum(x, 0.0)


def violations(atoms, res_mask=None, keep_mask=None, residue_index=None):
    """atoms [N,>=5,3] (columns 0..4 = N, CA, C, CB, O), res_mask / keep_mask [N] (default ones), residue_index [N] (default arange).  Rows
    with res_mask = 0 are removed first; rows with keep_mask = 0 sit at the origin.  Returns the outputs of ``structural_violations``
    for one sample, per-row arrays scattered back to N rows."""
    n_all = atoms.shape[0]
    res = np.ones(n_all, dtype=bool) if res_mask is None else np.asarray(res_mask) != 0
    keep = np.ones(n_all, dtype=bool) if keep_mask is None else np.asarray(keep_mask) != 0
    index = np.arange(n_all) if residue_index is None else np.asarray(residue_index)
    rows = np.nonzero(res)[0]
    x = np.asarray(atoms, dtype=np.float64)[rows, :5] * keep[rows, None, None]
    idx = index[rows].astype(np.int64)
    n = len(rows)

    # bonds and angles between consecutive rows
    ca, c, nn, ca2 = x[:-1, 1], x[:-1, 2], x[1:, 0], x[1:, 1]
    no_gap = (idx[1:] - idx[:-1] == 1).astype(np.float64)
    c_n_len = np.sqrt(1e-6 + ((c - nn) ** 2).sum(-1))
    ca_c_len = np.sqrt(1e-6 + ((ca - c) ** 2).sum(-1))
    n_ca_len = np.sqrt(1e-6 + ((nn - ca2) ** 2).sum(-1))
    len_err = np.sqrt(1e-6 + (c_n_len - C_N_LENGTH) ** 2)
    c_ca_u, c_n_u, n_ca_u = (ca - c) / ca_c_len[:, None], (nn - c) / c_n_len[:, None], (ca2 - nn) / n_ca_len[:, None]
    err1 = np.sqrt(1e-6 + ((c_ca_u * c_n_u).sum(-1) - COS_CA_C_N) ** 2)
    err2 = np.sqrt(1e-6 + (((-c_n_u) * n_ca_u).sum(-1) - COS_C_N_CA) ** 2)
    l0, l1, l2 = relu(len_err - C_N_TOLERANCE), relu(err1 - CA_C_N_TOLERANCE), relu(err2 - C_N_CA_TOLERANCE)
    bonds = no_gap.sum()
    per_bond = l0 + l1 + l2
    conn_loss = 0.5 * (np.pad(per_bond, (0, 1)) + np.pad(per_bond, (1, 0))) if n else np.zeros(0)
    kinds = {"bond": no_gap * (len_err > C_N_TOLERANCE), "angle_ca_c_n": no_gap * (err1 > CA_C_N_TOLERANCE), "angle_c_n_ca": no_gap * (err2 > C_N_CA_TOLERANCE)}
    bad_bond = np.maximum(np.maximum(kinds["bond"], kinds["angle_ca_c_n"]), kinds["angle_c_n_ca"])
    conn_mask = np.maximum(np.pad(bad_bond, (0, 1)), np.pad(bad_bond, (1, 0))) if n else np.zeros(0)
    ca_far = (np.sqrt(1e-6 + ((ca - ca2) ** 2).sum(-1)) - CA_CA > 1.5) * no_gap
    kinds["extreme_ca_ca"] = ca_far

    # clashes between residues
    d = np.sqrt(1e-10 + ((x[:, None, :, None, :] - x[None, :, None, :, :]) ** 2).sum(-1))  # [n,n,5,5]
    pair = (idx[:, None] < idx[None, :]).astype(np.float64)[:, :, None, None] * np.ones((1, 1, 5, 5))
    bonded = idx[:, None] + 1 == idx[None, :]
    pair[:, :, 2, 0] *= 1.0 - bonded
    bound = pair * (RADIUS[None, None, :, None] + RADIUS[None, None, None, :])
    err = pair * relu(bound - 1.5 - d)
    clash = pair * (d < bound - 1.5)
    clash_loss = err.sum(axis=(0, 2)) + err.sum(axis=(1, 3))
    clash_mask = np.maximum(clash.max(axis=(0, 2)), clash.max(axis=(1, 3))) if n else np.zeros((0, 5))
    kinds["clash"] = clash

    # within residues
    dw = np.sqrt(1e-10 + ((x[:, :, None, :] - x[:, None, :, :]) ** 2).sum(-1))  # [n,5,5]
    off = 1.0 - np.eye(5)
    lw = off * (relu(LOWER - dw) + relu(dw - UPPER))
    within_loss = lw.sum(axis=-2) + lw.sum(axis=-1)
    kinds["within_low"], kinds["within_high"] = off * (dw < LOWER), off * (dw > UPPER)
    within = np.maximum(kinds["within_low"], kinds["within_high"])
    within_mask = np.maximum(within.max(axis=-2), within.max(axis=-1)) if n else np.zeros((0, 5))

    total = np.maximum(np.maximum(conn_mask, clash_mask.max(-1)), within_mask.max(-1)) if n else np.zeros(0)
    mean = lambda v: v.sum() / (1e-4 + n)  # noqa: E731  (masked_mean over seq_mask = ones)
    kept = np.asarray(atoms, dtype=np.float64)[res & keep, :5].reshape(-1, 3)
    out = {"bonds_c_n_loss_mean": (no_gap * l0).sum() / (bonds + 1e-6), "angles_ca_c_n_loss_mean": (no_gap * l1).sum() / (bonds + 1e-6),
           "angles_c_n_ca_loss_mean": (no_gap * l2).sum() / (bonds + 1e-6), "clashes_mean_loss": err.sum() / (1e-6 + pair.sum()),
           "violations_extreme_ca_ca_distance": ca_far.sum() / (1e-4 + bonds), "violations_between_residue_bond": mean(conn_mask),
           "violations_between_residue_clash": mean(clash_mask.max(-1)) if n else 0.0, "violations_within_residue": mean(within_mask.max(-1)) if n else 0.0,
           "violations_per_residue": mean(total),
           "radius_of_gyration": np.sqrt(((kept - kept.mean(0)) ** 2).sum(-1).mean()) if len(kept) else np.nan,
           "num_residue_violations": int(total.sum()), "n_clash_pairs": int(pair.sum())}

    def scatter(v, dtype):
        full = np.zeros((n_all,) + v.shape[1:], dtype=dtype)
        full[rows] = v
        return full

    out.update(connections_per_residue_loss_sum=scatter(conn_loss, np.float64), connections_per_residue_violation_mask=scatter(conn_mask, np.uint8),
               total_per_residue_violations_mask=scatter(total, np.uint8), clashes_per_atom_loss_sum=scatter(clash_loss, np.float64),
               clashes_per_atom_clash_mask=scatter(clash_mask, np.uint8), within_per_atom_loss_sum=scatter(within_loss, np.float64),
               within_per_atom_violations=scatter(within_mask, np.uint8))
    out["kinds"] = {k: int(np.asarray(v).sum()) for k, v in kinds.items()}
    # the smallest relative distance of a thresholded quantity from its threshold (the fixture generator asserts it)
    rel = lambda v, t, m: np.min(np.abs(v - t)[m] / np.abs(t * np.ones_like(v))[m], initial=np.inf)  # noqa: E731
    gapless, paired, offdiag = no_gap > 0, pair > 0, np.broadcast_to(off > 0, dw.shape)
    out["margin"] = float(min(rel(len_err, C_N_TOLERANCE, gapless), rel(err1, CA_C_N_TOLERANCE, gapless), rel(err2, C_N_CA_TOLERANCE, gapless),
                              rel(np.sqrt(1e-6 + ((ca - ca2) ** 2).sum(-1)), CA_CA + 1.5, gapless), rel(d, bound - 1.5, paired),
                              rel(dw, LOWER[None], offdiag), rel(dw, UPPER[None], offdiag)))
    return {k: (np.float64(v) if k in SCALARS + ("radius_of_gyration",) else v) for k, v in out.items()}


def case_inputs(fix, name):
    """prot [B,N,37,3] float32 (atoms 5.. zero), diffuse_mask [B,N], residue_index [B,N] of a fixture case."""
    bb = fix[f"{name}.bb"]
    prot = np.zeros(bb.shape[:2] + (37, 3), dtype=np.float32)
    prot[:, :, :5] = bb
    return {"prot": prot, "diffuse_mask": fix[f"{name}.diffuse_mask"], "residue_index": fix[f"{name}.residue_index"]}


def keep_mask(prot, diffuse_mask=None):
    """protein_metrics :149-150 per row: a non-zero coordinate among the five atoms, and diffused."""
    nonzero = np.any(prot[..., :5, :] != 0, axis=(-2, -1))
    return nonzero if diffuse_mask is None else nonzero & (np.asarray(diffuse_mask) != 0)


def bound(fix, name, key):
    """32 x the case's yardstick for the output, the fixture's largest yardstick for it where the case's own is 0."""
    own = float(fix[f"{name}.{key}.yard"])
    return 32.0 * (own if own > 0 else max(float(fix[f"{c}.{key}.yard"]) for c in CASES))


def widest_bound(fix, key):
    """32 x the fixture's largest yardstick for the output: the bound of inputs that have no yardstick of their own."""
    return 32.0 * max(float(fix[f"{c}.{key}.yard"]) for c in CASES)


def check_outputs(want, got, limit, show=None):
    """One sample's outputs ``got`` against ``want`` (dicts of per-sample arrays): floats within ``limit(key)``, masks and counts exactly.
    ``show(key, error, bound)`` receives every figure before its assertion."""
    for key in FLOAT_OUTPUTS:
        err, lim = float(np.max(np.abs(np.asarray(got[key], dtype=np.float64) - np.asarray(want[key], dtype=np.float64)))), limit(key)
        if show is not None:
            show(key, err, lim)
        assert err <= lim, (key, err, lim)
    for key in EXACT_OUTPUTS:
        assert np.array_equal(np.asarray(got[key]).astype(np.int64), np.asarray(want[key]).astype(np.int64)), key


def check_sample(fix, name, s, got, show=None):
    """Sample ``s`` of a case against the fixture's float64 run, within ``bound``."""
    check_outputs({k: fix[f"{name}.{k}"][s] for k in FLOAT_OUTPUTS + EXACT_OUTPUTS}, got, lambda key: bound(fix, name, key), show)


def sample_of(result, s):
    """Sample ``s`` of what ``structural_violations`` returns."""
    return {k: v[s] for k, v in result.items()}


def joint_batch(fix, n_pad=261):
    """Every sample of every case in one batch padded to ``n_pad`` rows with res_mask = 0 (garbage coordinates and indices behind a
    sample): inputs of ``structural_violations`` and the first batch row of every case."""
    prot, diffuse, res, index, first = [], [], [], [], []
    rng = np.random.default_rng(5)
    for name in CASES:
        inp = case_inputs(fix, name)
        b, n = inp["prot"].shape[:2]
        first.append(len(prot))
        for s in range(b):
            x = rng.normal(size=(n_pad, 37, 3)).astype(np.float32) * 30
            x[:n] = inp["prot"][s]
            prot.append(x)
            diffuse.append(np.concatenate([inp["diffuse_mask"][s], np.ones(n_pad - n, dtype=np.float32)]))
            res.append(np.concatenate([np.ones(n, dtype=np.float32), np.zeros(n_pad - n, dtype=np.float32)]))
            index.append(np.concatenate([inp["residue_index"][s], rng.integers(0, 300, size=n_pad - n).astype(np.int32)]))
    return {"prot": np.stack(prot), "diffuse_mask": np.stack(diffuse), "res_mask": np.stack(res), "residue_index": np.stack(index)}, first
