"""Fixture of the sample-evaluation tests, captured from the reference (this container only):

    python tests/golden/make_goldens_evaluation.py      # -> tests/golden/evaluation_cases.npz

Per case (SPEC below; tests/evaluation_ref.py: CASES) synthetic float32 backbones at realistic magnitudes - a chain walk tens of
Angstrom from the origin, samples scattered around a ground truth inside the diffused regions and equal to it outside, as an inpainting
run leaves them - widened to float64 and passed through the reference's own functions:

* evaluation.utils.metrics: ``backbone_rmsd``, ``chain_backbone_rmsd``, ``residue_backbone_rmsd``, ``residue_signed_angle_error`` (with
  ``residue_angle_error``, ``residue_sample_angle``, ``residue_groundtruth_angle``) on array-backed stand-ins for the Bio models -
  ``parsers.process_chain`` is replaced in the imported module, everything else runs as it is -, ``calc_dihedrals`` and
  ``angle_error_with_sign`` on whole chains, ``flatten`` for the column names;
* framedipt.analysis.metrics: ``ca_ca_distance``, ``ca_ca_clashes``, ``calc_aligned_rmsd``; framedipt.data.transforms:
  ``rigid_transform_3D``.  ``bb_mask`` restates protein_metrics :149,157-158 (rows with any non-zero coordinate).  ``aligned_rmsd`` has no
  reference function: it is the root mean square of ``rigid_transform_3D``'s own superposed coordinates against the target, pinned by
  this restatement only.

Next to every expected array ``<case>.<output>`` the yardstick ``<case>.<output>.yard``: the largest change of the reference's own
float64 result under
* three permutations (seeds ``perm_seeds``) of what its sums run over: the rows inside every region and the backbone atoms for the
  deviations, the aligned rows for the superposition, the CA rows for the clash fraction, and the reversed chain for the bonds;
* one rigid motion (``motion.rot``, ``motion.shift`` = 100 Angstrom) of sample and ground truth alike - every output except
  ``rotation`` and ``translation`` is invariant to it in exact arithmetic.

Decidability is asserted here, not measured by the tests: all three branches of the signed-error argmin occur, no two of its
candidates are closer than 1e-9 degrees, every CA distance is at least 1e-5 Angstrom away from 1.5 and from ca_ca + 0.1, ``reflection``
is 1 in ``mirror`` only.
"""
from __future__ import annotations

import dataclasses
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
from evaluation.utils import metrics as em  # noqa: E402
from framedipt.analysis import metrics as am  # noqa: E402
from framedipt.data import transforms  # noqa: E402

import evaluation_ref as er  # noqa: E402

# name: (B, N, chain lengths, regions as (first row, length), seed)
SPEC = {
    "two_chains": (3, 19, (10, 9), ((3, 5), (11, 7)), 21),
    "region_at_chain_ends": (2, 14, (7, 7), ((0, 4), (9, 5)), 22),
    "l4": (1, 9, (9,), ((3, 4),), 23),
    "wrap": (4, 45, (45,), ((2, 40),), 24),
    "clashy": (2, 30, (17, 1, 12), ((5, 8),), 25),
    "mirror": (2, 16, (16,), ((4, 8),), 26),
    "n260": (2, 260, (260,), ((120, 21),), 27),
}
PERM_SEEDS = (1000, 1001, 1002)
ANGLE_KEYS = ("phi", "psi", "omega")


@dataclasses.dataclass
class ChainArrays:
    """What metrics.py reads of parsers.process_chain's result."""
    atom_positions: np.ndarray


class ArrayModel:
    """Stand-in for a Bio model: chain id -> [L,37,3] float64 (hashable by identity, as get_dihedral_angles' cache needs)."""

    def __init__(self, atoms, chain_idx):
        self.chains = {}
        for number, cid in enumerate(np.unique(chain_idx)):
            rows = np.nonzero(chain_idx == cid)[0]
            pos = np.zeros((len(rows), 37, 3))
            pos[:, :5] = atoms[rows]
            self.chains[chr(ord("A") + number)] = pos

    @property
    def child_dict(self):
        return self.chains

    def __getitem__(self, chain_id):
        return self.chains[chain_id]


em.parsers.process_chain = lambda chain, chain_id: ChainArrays(atom_positions=np.array(chain))


def walk(rng, n, step=3.8, jitter=0.0):
    steps = rng.normal(size=(n, 3))
    lengths = step + jitter * rng.uniform(-1.0, 1.0, size=(n, 1))
    return np.array([31.0, -47.0, 58.0]) + np.cumsum(lengths * steps / np.linalg.norm(steps, axis=-1, keepdims=True), axis=0)


def backbones(name, b, n, regions, seed):
    """(samples [B,N,5,3], ground truth [N,5,3]) float32: atom37 columns N, CA, C, CB, O."""
    rng = np.random.default_rng(seed)
    ca = walk(rng, n, 2.6, 1.9) if name == "clashy" else walk(rng, n)
    offsets = np.concatenate([1.46 * rng.normal(size=(n, 1, 3)) / np.sqrt(3), np.zeros((n, 1, 3)), 1.52 * rng.normal(size=(n, 1, 3)) / np.sqrt(3),
                              1.53 * rng.normal(size=(n, 1, 3)) / np.sqrt(3), 2.4 * rng.normal(size=(n, 1, 3)) / np.sqrt(3)], axis=1)
    gt = (ca[:, None, :] + offsets).astype(np.float32)
    x = np.tile(gt[None], (b, 1, 1, 1)).astype(np.float64)
    for first, length in regions:
        rows = slice(first, first + length)
        x[:, rows] += 1.5 * rng.normal(size=(b, length, 1, 3)) + 0.3 * rng.normal(size=(b, length, 5, 3))
    if name == "mirror":  # the mirror image of the ground truth in the plane z = 58, a little noise on top
        x = np.tile(gt[None], (b, 1, 1, 1)).astype(np.float64)
        x[..., 2] = 116.0 - x[..., 2]
        x += 0.2 * rng.normal(size=x.shape)
    x = x.astype(np.float32)
    if name == "clashy":
        x[:, 24, 1] = x[:, 20, 1]     # two exactly coincident CA atoms
        x[:, 17], gt[17] = 0.0, 0.0   # an all-zero row (a chain of its own): outside bb_mask
    return x, gt


def masks(n, chain_lengths, regions):
    chain_idx = np.repeat(np.arange(len(chain_lengths)), chain_lengths).astype(np.int32)
    diffuse = np.zeros(n, dtype=np.float32)
    for first, length in regions:
        diffuse[first:first + length] = 1
    assert len(chain_idx) == n
    return chain_idx, diffuse


def from_eval_idx(d):
    """Inverse of convert_to_eval_idx: the values in residue order."""
    return [d[k] for k in sorted(k for k in d if k > 0)] + [d[k] for k in (-4, -3, -2, -1)]


def reference_outputs(x, y, chain_idx, diffuse, spec_regions, *, region_perm=None, atom_perm=None, row_perm=None, reverse=False, bb_mask=None):
    """The reference's numbers for one sample x against y ([N,5,3] float64).  The keyword arguments reorder what its sums run over."""
    n = x.shape[0]
    regions, rows = er.regions_of(diffuse, chain_idx, np.ones(n))
    assert rows == [(f, f + ln - 1) for f, ln in spec_regions]
    xs, ys = x.copy(), y.copy()
    if region_perm is not None:
        for (first, last), p in zip(rows, region_perm):
            xs[first:last + 1], ys[first:last + 1] = xs[first:last + 1][p], ys[first:last + 1][p]
    if atom_perm is not None:  # the contents of atom37 columns 0, 1, 2, 4 change places in both structures
        cols = np.array([0, 1, 2, 4])
        xs[:, cols], ys[:, cols] = xs[:, cols[atom_perm]], ys[:, cols[atom_perm]]
    sample, gt = ArrayModel(xs, chain_idx), ArrayModel(ys, chain_idx)
    chains = [chr(ord("A") + c) for c, _, _ in regions]
    local = [(s, e) for _, s, e in regions]
    call = lambda fn: fn(gt, sample, chains, local, local)  # noqa: E731  (model_1 = ground truth, as evaluate_tcr.py :412-418)
    out = {"bb_rmsd": call(em.backbone_rmsd), "region_bb_rmsd": np.array(list(call(em.chain_backbone_rmsd).values())), "regions": regions}
    per_res = call(em.residue_backbone_rmsd)
    res_bb = np.zeros(n)
    for (first, last), d in zip(rows, per_res.values()):
        res_bb[first:last + 1] = from_eval_idx(d)
    out["res_bb_rmsd"] = res_bb
    if region_perm is None and atom_perm is None:
        dih = {}
        for key, atoms in (("dihedral", x), ("gt_dihedral", y)):
            full = np.zeros((3, n))
            for cid in np.unique(chain_idx):
                r = np.nonzero(chain_idx == cid)[0]
                got = em.calc_dihedrals(n_coords=atoms[r, 0], ca_coords=atoms[r, 1], c_coords=atoms[r, 2])
                full[:, r] = np.stack([np.rad2deg(got[k]) for k in ANGLE_KEYS])
            dih[key] = full
        out.update(dih)
        out["angle_error"] = np.stack([em.angle_error_with_sign(dih["gt_dihedral"][k], dih["dihedral"][k]) for k in range(3)])
        # the pipeline's own per-region dicts say the same (orientation ground truth - sample, region slices, index convention)
        signed = call(em.residue_signed_angle_error)
        for k, key in enumerate(ANGLE_KEYS):
            for (first, last), d in zip(rows, signed[key].values()):
                assert np.array_equal(from_eval_idx(d), out["angle_error"][k, first:last + 1])
        groups = {"model_metrics": {"bb_rmsd": out["bb_rmsd"]}, "chain_metrics": {"bb_rmsd": call(em.chain_backbone_rmsd)},
                  "residue_metrics": {"bb_rmsd": per_res},
                  "residue_group_metrics": {"angle_error": call(em.residue_angle_error), "signed_angle_error": signed,
                                            "sample": call(em.residue_sample_angle), "gt": call(em.residue_groundtruth_angle)}}
        out["columns"] = {}
        for group in groups.values():
            out["columns"].update(em.flatten(group))
    # geometry (protein_metrics :149,157-160): rows with any non-zero coordinate
    if bb_mask is None:
        bb_mask = np.any(np.any(x != 0, axis=-1), axis=-1)
    ca = x[bb_mask, 1]
    if reverse:
        ca = ca[::-1]
    if row_perm is not None:
        ca_clash = ca[np.random.default_rng(row_perm).permutation(len(ca))]
    else:
        ca_clash = ca
    out["ca_ca_bond_dev"], out["ca_ca_valid_percent"] = am.ca_ca_distance(ca)
    out["num_ca_steric_clashes"], out["ca_steric_clash_percent"] = am.ca_ca_clashes(ca_clash)
    a, b = x[:, 1], y[:, 1]
    if row_perm is not None:
        p = np.random.default_rng(row_perm).permutation(n)
        a, b = a[p], b[p]
    out["aligned_mean_dev"] = am.calc_aligned_rmsd(a, b)
    moved, rot, t, reflection = transforms.rigid_transform_3D(a, b)
    out.update(aligned_rmsd=np.sqrt(np.mean(np.sum((moved - b) ** 2, axis=-1))), rotation=rot, translation=t.reshape(3), reflection=int(reflection),
               ca=ca)
    return out


def change(base, other, keys):
    out = {}
    for k in keys:
        a, b = np.asarray(base[k], dtype=np.float64), np.asarray(other[k], dtype=np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        out[k] = float(np.nanmax(np.abs(a - b))) if np.isfinite(a).any() else 0.0
    return out


def main():
    q, _ = np.linalg.qr(np.random.default_rng(77).normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    shift = 100.0 * np.array([2.0, -1.0, 2.0]) / 3.0
    fix = {"perm_seeds": np.array(PERM_SEEDS), "motion.rot": q, "motion.shift": shift}
    branches = set()
    for name, (b, n, chain_lengths, regions, seed) in SPEC.items():
        xs, gt = backbones(name, b, n, regions, seed)
        chain_idx, diffuse = masks(n, chain_lengths, regions)
        y = gt.astype(np.float64)
        per_sample, yard = [], {k: 0.0 for k in er.FLOAT_OUTPUTS}
        for s in range(b):
            x = xs[s].astype(np.float64)
            base = reference_outputs(x, y, chain_idx, diffuse, regions)
            per_sample.append(base)

            def grow(other, keys):
                for k, v in change(base, other, keys).items():
                    yard[k] = max(yard[k], v)

            for seed_k in PERM_SEEDS:
                rng = np.random.default_rng(seed_k)
                grow(reference_outputs(x, y, chain_idx, diffuse, regions, region_perm=[rng.permutation(ln) for _, ln in regions]),
                     ("bb_rmsd", "region_bb_rmsd"))
                grow(reference_outputs(x, y, chain_idx, diffuse, regions, atom_perm=rng.permutation(4)), ("bb_rmsd", "region_bb_rmsd", "res_bb_rmsd"))
                grow(reference_outputs(x, y, chain_idx, diffuse, regions, row_perm=seed_k),
                     ("ca_steric_clash_percent", "aligned_mean_dev", "aligned_rmsd", "rotation", "translation"))
            grow(reference_outputs(x, y, chain_idx, diffuse, regions, reverse=True), ("ca_ca_bond_dev", "ca_ca_valid_percent"))
            # (an all-zero row moves with the rest - it is a point of the superposition - but stays outside bb_mask)
            moved = reference_outputs(x @ q.T + shift, y @ q.T + shift, chain_idx, diffuse, regions, bb_mask=np.any(x != 0, axis=(-2, -1)))
            grow(moved, [k for k in er.FLOAT_OUTPUTS if k not in ("rotation", "translation")])
            assert moved["num_ca_steric_clashes"] == base["num_ca_steric_clashes"] and moved["reflection"] == base["reflection"]
            # decidability
            for k in range(3):
                g, smp = base["gt_dihedral"][k], base["dihedral"][k]
                cand = np.abs(np.stack([g - smp, g + 360 - smp, g - 360 - smp]))
                order = np.sort(cand, axis=0)
                assert (order[1] - order[0] >= 1e-9).all(), (name, s, k)
                branches |= set(np.argmin(cand, axis=0)[diffuse != 0].tolist())
            ca = base["ca"]
            dist = np.linalg.norm(ca[:, None] - ca[None], axis=-1)
            assert (np.abs(dist - 1.5) >= 1e-5).all() and (np.abs(dist - (er.CA_CA + 0.1)) >= 1e-5).all(), name
            assert base["reflection"] == (1 if name == "mirror" else 0), (name, s)
        if name == "clashy":
            bonds = np.linalg.norm(np.diff(per_sample[0]["ca"], axis=0), axis=-1)
            assert per_sample[0]["num_ca_steric_clashes"] >= 3 and (bonds > er.CA_CA + 0.1).any() and (bonds < er.CA_CA + 0.1).any()
            assert (np.linalg.norm(per_sample[0]["ca"][:, None] - per_sample[0]["ca"][None], axis=-1)[np.triu_indices(len(bonds) + 1, 1)] == 0).sum() == 1
        fix.update({f"{name}.bb": xs, f"{name}.gt": gt[None], f"{name}.diffuse_mask": diffuse, f"{name}.res_mask": np.ones(n, dtype=np.float32),
                    f"{name}.chain_idx": chain_idx, f"{name}.regions": np.array(per_sample[0]["regions"], dtype=np.int64).reshape(-1, 3)})
        for k in er.FLOAT_OUTPUTS:
            fix[f"{name}.{k}"] = np.asarray(per_sample[0][k]) if k == "gt_dihedral" else np.stack([np.asarray(p[k], dtype=np.float64) for p in per_sample])
            fix[f"{name}.{k}.yard"] = np.float64(yard[k])
        for k in er.EXACT_OUTPUTS:
            fix[f"{name}.{k}"] = np.array([int(p[k]) for p in per_sample], dtype=np.int64)
        cols = per_sample[0]["columns"]
        fix[f"{name}.columns"], fix[f"{name}.column_values"] = np.array(list(cols)), np.array([float(v) for v in cols.values()])
        print(f"{name}: B = {b}, N = {n}, regions {per_sample[0]['regions']}, clashes {[p['num_ca_steric_clashes'] for p in per_sample]}, "
              f"yardsticks " + ", ".join(f"{k} {v:.1e}" for k, v in yard.items()))
    assert branches == {0, 1, 2}, branches
    assert set(SPEC) == set(er.CASES)
    np.savez_compressed(os.path.join(HERE, "evaluation_cases.npz"), **fix)
    print(f"{os.path.getsize(os.path.join(HERE, 'evaluation_cases.npz')) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
