"""NumPy float64 restatement of sample evaluation (framedipt_amd/csrc/evaluate.hip, framedipt_amd/evaluation.py; contract in
include/fdipt.h) and the access to its fixture — test infrastructure.

``evaluate`` computes for one sample what the kernel writes: (a) backbone deviations without superposition, (b) dihedrals per chain
and ``angle_error_with_sign(ground truth, sample)``, (c) the CA geometry checks, (d) the superposition by SVD as ``rigid_transform_3D``
does it (the kernel solves Horn's quaternion eigenproblem instead: the two are independent routes to the same rotation).

The fixture tests/golden/evaluation_cases.npz (made by tests/golden/make_goldens_evaluation.py) holds per case the backbone block of
samples and ground truth, atom37 columns 0 .. 4 (N, CA, C, CB, O) as float32, the masks, what the reference returned under
``<case>.<output>`` and next to it ``<case>.<output>.yard``: the largest change of the reference's own result under permutations of
its sums and a rigid motion of its inputs.
"""
import numpy as np

BACKBONE_COLUMNS = (2, 0, 1, 4)
ANGLES = ("phi", "psi", "omega")
CA_CA = 3.80209737096
CASES = ("two_chains", "region_at_chain_ends", "l4", "wrap", "clashy", "mirror", "n260")
# per-sample float outputs the fixture records with a yardstick (``padded`` is two_chains again: it has no entries of its own)
FLOAT_OUTPUTS = ("res_bb_rmsd", "region_bb_rmsd", "bb_rmsd", "dihedral", "gt_dihedral", "angle_error", "ca_ca_bond_dev", "ca_ca_valid_percent",
                 "ca_steric_clash_percent", "aligned_mean_dev", "aligned_rmsd", "rotation", "translation")
EXACT_OUTPUTS = ("num_ca_steric_clashes", "reflection")
BOUND_FACTOR = 32.0


def dihedrals(a, b, c, d):
    """metrics.py:880-923 (radians); NaN where b and c coincide."""
    b0, b1, b2 = a - b, c - b, d - c
    with np.errstate(divide="ignore", invalid="ignore"):
        b1 = b1 / np.linalg.norm(b1, axis=-1, keepdims=True)
    v = b0 - np.sum(b0 * b1, axis=-1, keepdims=True) * b1
    w = b2 - np.sum(b2 * b1, axis=-1, keepdims=True) * b1
    return np.arctan2(np.sum(np.cross(b1, v) * w, axis=-1), np.sum(v * w, axis=-1))


def chain_dihedrals(n, ca, c):
    """[3,L] degrees in ANGLES order for one chain (calc_dihedrals :926-956)."""
    psi = np.append(dihedrals(n[:-1], ca[:-1], c[:-1], n[1:]), [0.0])
    omega = np.append(dihedrals(ca[:-1], c[:-1], n[1:], ca[1:]), [0.0])
    phi = np.append([0.0], dihedrals(c[:-1], n[1:], ca[1:], c[1:]))
    return np.rad2deg(np.stack([phi, psi, omega]))


def structure_dihedrals(x, chain_idx, res_mask):
    """[3,N] degrees: every chain (the rows of res_mask with one chain id) on its own; rows outside res_mask are 0."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((3, x.shape[0]))
    keep = np.asarray(res_mask) != 0
    for cid in np.unique(np.asarray(chain_idx)[keep]):
        rows = np.nonzero(keep & (np.asarray(chain_idx) == cid))[0]
        out[:, rows] = chain_dihedrals(x[rows, 0], x[rows, 1], x[rows, 2])
    return out


def signed_error(deg1, deg2):
    """angle_error_with_sign (:308-331)."""
    cand = np.stack([deg1 - deg2, deg1 + 360 - deg2, deg1 - 360 - deg2], axis=0)
    return np.take_along_axis(cand, np.argmin(np.abs(cand), axis=0)[None], axis=0)[0]


def regions_of(diffuse_mask, chain_idx, res_mask):
    """(regions, rows): (chain, first, last) chain-local in np.unique order of the chains, and the absolute rows."""
    keep = np.asarray(res_mask) != 0
    diffuse = (np.asarray(diffuse_mask) != 0) & keep
    chain_idx = np.asarray(chain_idx)
    regions, rows = [], []
    for number, cid in enumerate(np.unique(chain_idx[keep])):
        crow = np.nonzero(keep & (chain_idx == cid))[0]
        flags = np.concatenate([[False], diffuse[crow], [False]])
        first, last = np.nonzero(flags[1:-1] & ~flags[:-2])[0], np.nonzero(flags[1:-1] & ~flags[2:])[0]
        for s, e in zip(first, last):
            regions.append((number, int(s), int(e)))
            rows.append((int(crow[s]), int(crow[e])))
    return regions, rows


def rigid_transform(a, b):
    """(R, t, reflection) of rigid_transform_3D (data/transforms.py:77-128): R a + t is a superposed on b."""
    ca, cb = a.mean(axis=0), b.mean(axis=0)
    u, _, vt = np.linalg.svd((a - ca).T @ (b - cb))
    rot, reflection = vt.T @ u.T, False
    if np.linalg.det(rot) < 0:
        vt[2] *= -1
        rot, reflection = vt.T @ u.T, True
    return rot, cb - rot @ ca, reflection


def evaluate(prot, ref, diffuse_mask, chain_idx=None, res_mask=None, align_mask=None):
    """All outputs of the kernel for one sample: prot, ref [N,37,3] (or [N,>=5,3]: only columns 0 .. 4 are read, except by bb_mask)."""
    x, y = np.asarray(prot, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    n = x.shape[0]
    chain_idx = np.zeros(n, dtype=np.int64) if chain_idx is None else np.asarray(chain_idx)
    res_mask = np.ones(n) if res_mask is None else np.asarray(res_mask)
    align = (np.asarray(res_mask if align_mask is None else align_mask) != 0)
    regions, rows = regions_of(diffuse_mask, chain_idx, res_mask)
    cols = list(BACKBONE_COLUMNS)
    d2 = ((x[:, cols] - y[:, cols]) ** 2).sum(axis=-1)  # [N,4]
    res_bb = np.zeros(n)
    sums = []
    for first, last in rows:
        res_bb[first:last + 1] = np.sqrt(d2[first:last + 1].mean(axis=-1))
        sums.append(d2[first:last + 1].sum())
    lengths = [last - first + 1 for first, last in rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"res_bb_rmsd": res_bb, "region_bb_rmsd": np.array([np.sqrt(s / (4 * ln)) for s, ln in zip(sums, lengths)]),
               "bb_rmsd": np.sqrt(np.float64(sum(sums)) / (4 * np.float64(sum(lengths)))), "regions": regions, "region_rows": rows}
        out["dihedral"] = structure_dihedrals(x, chain_idx, res_mask)
        out["gt_dihedral"] = structure_dihedrals(y, chain_idx, res_mask)
        out["angle_error"] = signed_error(out["gt_dihedral"], out["dihedral"])
        ca = x[np.any(x != 0, axis=(-2, -1)), 1]
        bonds = np.linalg.norm(ca[1:] - ca[:-1], axis=-1)
        dist = np.linalg.norm(ca[:, None] - ca[None], axis=-1)
        inter = dist[np.triu(dist) > 0]
        out.update(ca_ca_bond_dev=np.float64(np.abs(bonds - CA_CA).sum()) / len(bonds), ca_ca_valid_percent=np.float64((bonds < CA_CA + 0.1).sum()) / len(bonds),
                   num_ca_steric_clashes=int((inter < 1.5).sum()), ca_steric_clash_percent=np.float64((inter < 1.5).sum()) / len(inter))
    a, b = x[align, 1], y[align, 1]
    if len(a):
        rot, t, reflection = rigid_transform(a, b)
        dev = np.linalg.norm(a @ rot.T + t - b, axis=-1)
        out.update(aligned_mean_dev=dev.mean(), aligned_rmsd=np.sqrt((dev ** 2).mean()), rotation=rot, translation=t, reflection=int(reflection))
    else:
        out.update(aligned_mean_dev=0.0, aligned_rmsd=0.0, rotation=np.eye(3), translation=np.zeros(3), reflection=0)
    return out


def convert_to_eval_idx(vals):
    """metrics.py:1245-1261."""
    out = {idx: vals[idx] for idx in (-4, -3, -2, -1)}
    out.update({i + 1: v for i, v in enumerate(vals[:-4])})
    return out


# ---------------------------------------------------------------------------------------------------------------------
def case_inputs(fix, name):
    """dict(prot [B,N,37,3] f32, ref [R,N,37,3] f32, diffuse_mask, res_mask [B,N] f32, chain_idx [B,N] i32, ref_index [B]) of a case; the
    atom37 columns the fixture does not hold are zero."""
    def atom37(bb):
        out = np.zeros(bb.shape[:2] + (37, 3), dtype=np.float32)
        out[:, :, :5] = bb
        return out
    bb = fix[f"{name}.bb"]
    b = bb.shape[0]
    tile = lambda k, dt: np.tile(fix[f"{name}.{k}"].astype(dt)[None], (b, 1))  # noqa: E731
    return {"prot": atom37(bb), "ref": atom37(fix[f"{name}.gt"]), "diffuse_mask": tile("diffuse_mask", np.float32),
            "res_mask": tile("res_mask", np.float32), "chain_idx": tile("chain_idx", np.int32), "ref_index": np.zeros(b, dtype=np.int32)}


def case_regions(fix, name):
    return [tuple(int(v) for v in row) for row in fix[f"{name}.regions"]]


def bound(fix, name, output, factor=BOUND_FACTOR):
    """Bound on |value - reference| for an output of a case: ``factor`` x the reference's own change under the recorded perturbations;
    where that is 0 for the case, the fixture's largest for that output."""
    own = float(fix[f"{name}.{output}.yard"])
    return factor * (own if own > 0 else max(float(fix[f"{c}.{output}.yard"]) for c in CASES))


def check_sample(fix, name, s, got, report=None):
    """Assert one sample's outputs (a dict of per-sample values, as ``evaluate`` returns) against the fixture: floats within the
    yardstick bound with NaN positions equal, integers and regions exactly.  ``report`` collects {output: (worst error, bound)}."""
    for k in FLOAT_OUTPUTS:
        want = fix[f"{name}.{k}"] if k == "gt_dihedral" else fix[f"{name}.{k}"][s]
        have = np.asarray(got[k], dtype=np.float64)
        assert have.shape == want.shape, (name, s, k, have.shape, want.shape)
        assert np.array_equal(np.isnan(have), np.isnan(want)), (name, s, k)
        err = float(np.nanmax(np.abs(have - want))) if np.isfinite(want).any() else 0.0
        lim = bound(fix, name, k)
        if report is not None:
            worst = report.get(k, (0.0, 0.0))
            report[k] = (err, lim) if err >= worst[0] else worst
        assert err <= lim, (name, s, k, err, lim)
    for k in EXACT_OUTPUTS:
        assert int(got[k]) == int(fix[f"{name}.{k}"][s]), (name, s, k)
    assert [tuple(r) for r in got["regions"]] == case_regions(fix, name), (name, s)


def sample_of(result, s):
    """Sample ``s`` of an ``evaluate_samples`` result in the form ``evaluate`` returns."""
    out = {k: result[k][s] for k in FLOAT_OUTPUTS + EXACT_OUTPUTS if k != "gt_dihedral"}
    out["gt_dihedral"] = result["gt_dihedral"][int(result["ref_index"][s])]
    out["regions"], out["region_rows"] = result["regions"][s], result["region_rows"][s]
    return out


def joint_batch(fix, names=CASES, extra=1):
    """All cases in one launch: every sample padded with zero rows (res_mask = 0) to the longest case plus ``extra`` rows, each case's
    ground truth a row of the reference array.  Returns the keyword arguments of ``evaluate_samples`` and per case its first sample."""
    parts = [case_inputs(fix, nm) for nm in names]
    n_max = max(p["prot"].shape[1] for p in parts) + extra
    total = sum(p["prot"].shape[0] for p in parts)
    out = {"prot": np.zeros((total, n_max, 37, 3), dtype=np.float32), "reference": np.zeros((len(parts), n_max, 37, 3), dtype=np.float32),
           "diffuse_mask": np.zeros((total, n_max), dtype=np.float32), "res_mask": np.zeros((total, n_max), dtype=np.float32),
           "chain_idx": np.zeros((total, n_max), dtype=np.int32), "ref_index": np.zeros(total, dtype=np.int32)}
    first, b = [], 0
    for r, p in enumerate(parts):
        s, n = p["prot"].shape[:2]
        out["prot"][b:b + s, :n], out["reference"][r, :n] = p["prot"], p["ref"][0]
        for k in ("diffuse_mask", "res_mask", "chain_idx"):
            out[k][b:b + s, :n] = p[k]
        out["ref_index"][b:b + s] = r
        first.append(b)
        b += s
    return out, first
