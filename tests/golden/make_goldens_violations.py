"""Fixture of the structural-violation tests, captured from the reference (this container only):

    python tests/golden/make_goldens_violations.py      # -> tests/golden/violation_cases.npz

Per case (SPEC below; tests/violations_ref.py: CASES) synthetic float32 backbones at realistic magnitudes - a chain built from ideal
bond lengths, angles and helix / strand torsions tens of Angstrom from the origin, perturbed so that some bonds and angles violate and
some do not, with segments folded back onto the chain so that real clashes occur - go through the reference's own functions, as
framedipt/analysis/metrics.py:protein_metrics and openfold/np/relax/amber_minimize.py:find_violations chain them:

    framedipt.analysis.utils.create_full_prot -> amber_minimize.make_atom14_positions -> loss.find_structural_violations_np ->
    loss.compute_violation_metrics_np          (config: violation_tolerance_factor = 12, clash_overlap_tolerance = 1.5)

twice: on float64 arrays (``<case>.<output>``, the expected values) and as shipped in float32 (find_violations' casts;
``<case>.<output>.f32``).  residue_index is set on the batch (create_full_prot builds 0 .. N - 1 without a chain index).  Per-atom
outputs are stored for the five atoms that exist, in atom37 order N, CA, C, CB, O (the reference's atom14 order is N, CA, C, O, CB;
its columns 5..13 are asserted zero).  ``constants.*`` records the reference's constants as its arithmetic sees them.

Next to every expected float array the yardstick ``<case>.<output>.yard``: the largest change of the reference's own float64 result
under
* three permutations (seeds ``perm_seeds``) of the rows together with residue_index - the functions use the index, not the position, for
  every pair term, so the clash and within-residue outputs only change by the order of their sums; the bond terms follow the row order
  and are taken from the unpermuted run;
* one rigid motion (``motion.rot``, ``motion.shift`` = 100 Angstrom) of the kept rows, in the cases without undiffused rows (the pile of
  undiffused rows at the origin is not invariant).

Decidability is asserted here, not measured by the tests: every thresholded quantity (bond and cosine errors against 12 stddev, clash
distances against r_i + r_j - 1.5, within-residue distances against their bounds, CA-CA distances against ca_ca + 1.5) is at least 1e-3
relative away from its threshold (the seed of a case is the first from its base that gives this), the float32 and float64 masks and
counts agree, every one of the seven mask kinds occurs in some case and none in ``clean``.
"""
from __future__ import annotations

import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import refharness as rh  # noqa: E402

rh.install_stubs()
for _name in ("pdbfixer", "simtk", "simtk.openmm", "simtk.openmm.app", "openmm", "openmm.app", "openmm.app.internal",
              "openmm.app.internal.pdbstructure"):
    sys.modules.setdefault(_name, mock.MagicMock())
from framedipt.analysis import utils as analysis_utils  # noqa: E402
from openfold.np import residue_constants as rc  # noqa: E402
from openfold.np.relax import amber_minimize  # noqa: E402
from openfold.utils import loss  # noqa: E402

import violations_ref as vr  # noqa: E402

# name: (B, N, base seed)
SPEC = {"n1": (1, 1, 100), "n2": (1, 2, 200), "n65": (1, 65, 300), "masked": (1, 48, 400), "gaps": (1, 40, 500), "clashy": (1, 30, 600),
        "clean": (1, 24, 700), "n260": (2, 260, 800)}
PERM_SEEDS = (2000, 2001, 2002)
CONFIG = dict(violation_tolerance_factor=12, clash_overlap_tolerance=1.5)
ATOM14_TO_37 = [0, 1, 2, 4, 3]  # atom14 column of the atoms N, CA, C, CB, O
MARGIN = 1e-3


def place(a, b, c, bond, angle, torsion):
    """The point at ``bond`` from c with the angle b-c-d and the dihedral a-b-c-d (degrees)."""
    angle, torsion = np.deg2rad(angle), np.deg2rad(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    nrm = np.cross(b - a, bc)
    nrm /= np.linalg.norm(nrm)
    frame = np.stack([bc, np.cross(nrm, bc), nrm], axis=1)
    return c + frame @ (bond * np.array([-np.cos(angle), np.sin(angle) * np.cos(torsion), np.sin(angle) * np.sin(torsion)]))


def ideal_chain(n, torsions):
    """[n,5,3] float64 (N, CA, C, CB, O) from ideal bond lengths and angles and per-residue (phi, psi); omega = 180."""
    x = np.zeros((n, 5, 3))
    x[0, 0], x[0, 1] = [0.0, 0.0, 0.0], [1.458, 0.0, 0.0]
    x[0, 2] = x[0, 1] + 1.525 * np.array([-np.cos(np.deg2rad(111.0)), np.sin(np.deg2rad(111.0)), 0.0])
    for i in range(n):
        phi, psi = torsions[i]
        if i > 0:
            x[i, 0] = place(x[i - 1, 0], x[i - 1, 1], x[i - 1, 2], 1.329, 116.568, torsions[i - 1][1])
            x[i, 1] = place(x[i - 1, 1], x[i - 1, 2], x[i, 0], 1.458, 121.352, 180.0)
            x[i, 2] = place(x[i - 1, 2], x[i, 0], x[i, 1], 1.525, 111.0, phi)
        x[i, 4] = place(x[i, 0], x[i, 1], x[i, 2], 1.231, 120.5, psi + 180.0)
        x[i, 3] = place(x[i, 2], x[i, 0], x[i, 1], 1.53, 110.5, -122.6)
    return x


def backbone(name, n, rng):
    """One sample [n,5,3] float32."""
    helix, strand = (-60.0, -45.0), (-120.0, 130.0)
    if name == "clean":
        x = ideal_chain(n, [helix] * n)
    else:
        kinds = rng.integers(0, 2, size=n // 6 + 1).repeat(6)[:n]
        x = ideal_chain(n, [helix if k else strand for k in kinds])
        x += rng.normal(size=x.shape) * rng.choice([0.02, 0.08, 0.25], size=(n, 1, 1), p=[0.85, 0.1, 0.05] if n > 100 else [0.5, 0.3, 0.2])
        for i in rng.choice(n - 1, size=max(1, min(n // 20, 4)), replace=False) if n > 2 else []:
            x[i + 1:] += 2.5 * rng.normal(size=3)  # a broken chain: an extreme CA-CA distance
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    x = x @ q.T + np.array([31.0, -47.0, 58.0])
    if name in ("clashy", "n260", "n65", "masked"):  # fold the last third back onto the first, a little more than a bond away
        k = min(n // 3, 20)  # (few enough thresholded quantities that a decidable seed exists)
        x[n - k:] = x[:k][::-1] + 2.2 * rng.normal(size=3) / np.sqrt(3) + 0.6 * rng.normal(size=(k, 5, 3))
    return x.astype(np.float32)


def case_inputs(name, b, n, seed):
    rng = np.random.default_rng(seed)
    bb = np.stack([backbone(name, n, rng) for _ in range(b)])
    diffuse = np.ones((b, n), dtype=np.float32)
    index = np.tile(np.arange(n, dtype=np.int32), (b, 1))
    if name == "masked":
        diffuse[:, rng.choice(n, size=13, replace=False)] = 0
    if name == "gaps":  # a gap of 2, a gap of 200, one repeated index
        index[:, 9:] += 1
        index[:, 21:] += 199
        index[:, 30:] -= 1
        assert np.diff(index[0]).tolist().count(2) == 1 and np.diff(index[0]).tolist().count(200) == 1 and np.diff(index[0]).tolist().count(0) == 1
    return bb, diffuse, index


def reference_outputs(bb, diffuse, index, dtype):
    """The reference's outputs for one sample: bb [N,5,3] in ``dtype`` (np.float32: as find_violations casts; np.float64)."""
    n = bb.shape[0]
    atom37 = np.zeros((n, 37, 3), dtype=np.float64)
    atom37[:, :5] = bb
    atom37_mask = np.any(atom37, axis=-1)                                    # protein_metrics :149-151
    prot = analysis_utils.create_full_prot(atom37, diffuse[..., None] * atom37_mask)
    batch = {"aatype": np.asarray(prot.aatype), "all_atom_positions": np.asarray(prot.atom_positions).astype(dtype),
             "all_atom_mask": np.asarray(prot.atom_mask).astype(dtype), "residue_index": np.asarray(index, dtype=np.int64)}
    assert not batch["aatype"].any() and np.array_equal(prot.residue_index, np.arange(n))
    batch["seq_mask"] = np.ones_like(batch["aatype"], dtype)
    batch = amber_minimize.make_atom14_positions(batch)
    for k in ("atom14_atom_exists", "atom14_gt_positions"):
        batch[k] = batch[k].astype(dtype)
    assert (batch["atom14_atom_exists"][:, :5] == 1).all() and not batch["atom14_atom_exists"][:, 5:].any()
    found = loss.find_structural_violations_np(batch=batch, atom14_pred_positions=batch["atom14_gt_positions"], config=CONFIG)
    metrics = loss.compute_violation_metrics_np(batch=batch, atom14_pred_positions=batch["atom14_gt_positions"], violations=found)
    between, within = found["between_residues"], found["within_residues"]

    def atoms(v):
        v = np.asarray(v)
        assert v.shape == (n, 14) and not v[:, 5:].any()
        return v[:, ATOM14_TO_37]

    out = {k: np.float64(between[k]) for k in ("bonds_c_n_loss_mean", "angles_ca_c_n_loss_mean", "angles_c_n_ca_loss_mean", "clashes_mean_loss")}
    out.update({k: np.float64(metrics[k]) for k in vr.SCALARS[4:]})
    total = np.asarray(found["total_per_residue_violations_mask"])
    out.update(connections_per_residue_loss_sum=np.asarray(between["connections_per_residue_loss_sum"], dtype=np.float64),
               connections_per_residue_violation_mask=np.asarray(between["connections_per_residue_violation_mask"]).astype(np.uint8),
               total_per_residue_violations_mask=total.astype(np.uint8), num_residue_violations=len(np.flatnonzero(total)),
               clashes_per_atom_loss_sum=atoms(between["clashes_per_atom_loss_sum"]).astype(np.float64),
               clashes_per_atom_clash_mask=atoms(between["clashes_per_atom_clash_mask"]).astype(np.uint8),
               within_per_atom_loss_sum=atoms(within["per_atom_loss_sum"]).astype(np.float64),
               within_per_atom_violations=atoms(within["per_atom_violations"]).astype(np.uint8))
    return out


def constants():
    """The reference's constants as its arithmetic sees them, in the layout of fdipt_violation_constants."""
    bounds = rc.make_atom14_dists_bounds(overlap_tolerance=1.5, bond_length_tolerance_factor=12)
    ala = rc.restype_order["A"]
    assert rc.restype_name_to_atom14_names["ALA"][:5] == ["N", "CA", "C", "O", "CB"] and bounds["lower_bound"].dtype == np.float32
    pick = np.ix_(ATOM14_TO_37, ATOM14_TO_37)
    f32 = np.float32
    head = [rc.van_der_waals_radius["C"], rc.van_der_waals_radius["N"], rc.van_der_waals_radius["O"],
            f32(rc.between_res_bond_length_c_n[0]), f32(rc.between_res_bond_length_stddev_c_n[0]),
            f32(12) * f32(rc.between_res_bond_length_stddev_c_n[0]),       # (a float32 tensor times the int 12)
            rc.between_res_cos_angles_ca_c_n[0], rc.between_res_bond_length_stddev_c_n[0],  # (the stddev :807 takes)
            rc.between_res_cos_angles_c_n_ca[0], rc.between_res_cos_angles_c_n_ca[1], rc.ca_ca]
    return {"constants.head": np.array([float(v) for v in head]), "constants.lower": bounds["lower_bound"][ala][pick].astype(np.float64),
            "constants.upper": bounds["upper_bound"][ala][pick].astype(np.float64)}


def change(base, other, keys):
    return {k: float(np.max(np.abs(np.asarray(base[k], dtype=np.float64) - np.asarray(other[k], dtype=np.float64)), initial=0.0)) for k in keys}


PAIR_KEYS = ("clashes_mean_loss", "violations_between_residue_clash", "violations_within_residue", "clashes_per_atom_loss_sum",
             "within_per_atom_loss_sum")


def decidable_inputs(name, b, n, base_seed):
    for seed in range(base_seed, base_seed + 200):
        bb, diffuse, index = case_inputs(name, b, n, seed)
        stated = [vr.violations(bb[s].astype(np.float64), None, vr.keep_mask(bb[s], diffuse[s]), index[s]) for s in range(b)]
        if all(st["margin"] >= MARGIN for st in stated):
            return seed, bb, diffuse, index, stated
    raise AssertionError(f"{name}: no decidable seed")


def main():
    q, _ = np.linalg.qr(np.random.default_rng(77).normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    shift = 100.0 * np.array([2.0, -1.0, 2.0]) / 3.0
    fix = {"perm_seeds": np.array(PERM_SEEDS), "motion.rot": q, "motion.shift": shift, **constants()}
    seen = {k: 0 for k in vr.MASK_KINDS}
    for name, (b, n, base_seed) in SPEC.items():
        seed, bb, diffuse, index, stated = decidable_inputs(name, b, n, base_seed)
        per64, per32, yard = [], [], {k: 0.0 for k in vr.FLOAT_OUTPUTS}
        for s in range(b):
            x = bb[s].astype(np.float64)
            base = reference_outputs(x, diffuse[s], index[s], np.float64)
            shipped = reference_outputs(bb[s], diffuse[s], index[s], np.float32)
            per64.append(base)
            per32.append(shipped)
            for k in vr.EXACT_OUTPUTS:
                if k != "n_clash_pairs":
                    assert np.array_equal(base[k], shipped[k]), (name, s, k)
            for k, v in stated[s]["kinds"].items():
                seen[k] += v
                assert name != "clean" or v == 0, (name, k)
            if name == "clean":
                assert all(not np.any(base[k]) for k in vr.FLOAT_OUTPUTS + vr.EXACT_OUTPUTS if k != "n_clash_pairs"), name
            for seed_k in PERM_SEEDS:
                p = np.random.default_rng(seed_k).permutation(n)
                other = reference_outputs(x[p], diffuse[s][p], index[s][p], np.float64)
                for k in ("clashes_per_atom_loss_sum", "within_per_atom_loss_sum", "clashes_per_atom_clash_mask", "within_per_atom_violations"):
                    back = np.empty_like(other[k])
                    back[p] = other[k]
                    other[k] = back
                assert all(np.array_equal(base[k], other[k]) for k in ("clashes_per_atom_clash_mask", "within_per_atom_violations"))
                for k, v in change(base, other, PAIR_KEYS).items():
                    yard[k] = max(yard[k], v)
            if diffuse[s].all():
                moved = reference_outputs(x @ q.T + shift, diffuse[s], index[s], np.float64)
                assert all(np.array_equal(base[k], moved[k]) for k in vr.EXACT_OUTPUTS if k != "n_clash_pairs")
                for k, v in change(base, moved, vr.FLOAT_OUTPUTS).items():
                    yard[k] = max(yard[k], v)
            # (the reference keeps the mean only: the count is the restatement's, checked against the reference's mean and sums below)
            base["n_clash_pairs"] = shipped["n_clash_pairs"] = stated[s]["n_clash_pairs"]
            denominator = 1e-6 + base["n_clash_pairs"]
            assert abs(base["clashes_per_atom_loss_sum"].sum() / 2 / denominator - base["clashes_mean_loss"]) <= 1e-12 * max(1.0, base["clashes_mean_loss"])
        fix.update({f"{name}.bb": bb, f"{name}.diffuse_mask": diffuse, f"{name}.residue_index": index, f"{name}.seed": np.int64(seed)})
        for k in vr.FLOAT_OUTPUTS:
            fix[f"{name}.{k}"] = np.stack([np.asarray(p[k], dtype=np.float64) for p in per64])
            fix[f"{name}.{k}.f32"] = np.stack([np.asarray(p[k], dtype=np.float64) for p in per32])
            fix[f"{name}.{k}.yard"] = np.float64(yard[k])
        for k in vr.EXACT_OUTPUTS:
            fix[f"{name}.{k}"] = np.stack([np.asarray(p[k]) for p in per64]).astype(np.int64 if k in ("num_residue_violations", "n_clash_pairs") else np.uint8)
        print(f"{name}: B = {b}, N = {n}, seed {seed}, kinds {stated[0]['kinds']}, violating residues {[int(p['num_residue_violations']) for p in per64]}, "
              f"margin {min(st['margin'] for st in stated):.1e}, yardsticks " + ", ".join(f"{k} {v:.1e}" for k, v in yard.items()), flush=True)
    assert all(v > 0 for v in seen.values()), seen
    assert set(SPEC) == set(vr.CASES)
    path = os.path.join(HERE, "violation_cases.npz")
    np.savez_compressed(path, **fix)
    print(f"{os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
