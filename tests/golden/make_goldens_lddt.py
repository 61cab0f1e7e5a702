"""Fixture of the superposition-free accuracy tests, captured from the reference (this container only):

    python tests/golden/make_goldens_lddt.py      # -> tests/golden/lddt_cases.npz

Per case (tests/lddt_ref.py: CASES) synthetic float32 structures at realistic magnitudes - chains built from ideal bond lengths and
angles with helix, strand and turn torsions, tens of Angstrom from the origin with |coordinate| <= 100, the model a perturbed copy of
the reference (per-residue shifts of 0.05 .. 2 Angstrom and a hinged tail, so that every lDDT threshold is crossed) - go through the
reference's own functions in openfold/utils/loss.py:

* ``lddt_ca`` (the ``ca`` set) and ``lddt`` on the flattened atom list (the multi-atom sets: what ``same_residue=True`` computes), per
  residue / atom (``<case>.<mode>.ref_atom`` [P,N,A]) and with ``per_residue=False`` (``<case>.<mode>.ref_lddt`` [P]), on float64 tensors;
  their float32 run beside them as ``.f32``;
* ``compute_drmsd`` on float64 tensors of the kept rows (``<case>.drmsd``, ``.f32``);
* ``compute_fape`` as ``backbone_loss`` calls it, on frames built as data_transforms.atom37_to_frames builds group 0.  The reference's
  ``Rigid`` forces float32, so the expected values (``<case>.fape``, ``res_fape``, ``region_fape``) are the float64 restatement in
  tests/lddt_ref.py and the reference's float32 number is recorded beside them (``<case>.fape.f32``); the relative distance of the two is
  asserted <= 1e-5 and recorded (``<case>.fape.ref_distance``).

The tile sizes of the kernel come from include/fdipt.h (FDIPT_LDDT_TILE, FDIPT_LDDT_TILE_ALL): ``tile`` and ``tile_all`` have one row more.

Next to every expected float array the yardstick ``<case>.<output>.yard``: the largest change of the reference's (dRMSD) or the
restatement's (FAPE) own float64 result under three recorded row permutations (seeds ``perm_seeds``).

Decidability is asserted here, not measured by the tests: every thresholded quantity - each reference distance against the cutoff, each
|d_b - d_a| of a scored pair against 0.5, 1, 2, 4 - is at least 1e-9 Angstrom from its threshold in every atom set the case runs in,
with and without the pairs inside a residue (10^5 times the float64 rounding of a distance below 300 Angstrom); the seed of a case is
the first from its base that gives this.  ``motion.rot`` and ``motion.shift`` (100 Angstrom) are a recorded rigid motion: for the cases
lddt_ref.MOTION_CASES the moved model, rounded to float32 again as the device takes it, is asserted as decidable and to keep every
integer of the unmoved one.  The restatement is asserted equal to the reference's lDDT bit for bit where the reference
applies.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_goldens_violations as mv  # noqa: E402  (installs the import harness of the reference; ideal_chain)
from openfold.utils import loss  # noqa: E402
from openfold.utils.rigid_utils import Rigid, Rotation  # noqa: E402

import lddt_ref as lr  # noqa: E402
from framedipt_amd import _lib  # noqa: E402  (the header's macros; no library is loaded)

MARGIN = 1e-9
TILE, TILE_ALL = _lib.LDDT_TILE, _lib.LDDT_TILE_ALL
# name: (rows, base seed)
SPEC = {"n1": (1, 100), "n2": (2, 200), "n63": (63, 300), "n64": (64, 400), "n65": (65, 500), "tile": (TILE + 1, 600), "tile_all": (TILE_ALL + 1, 700),
        "masked": (48, 800), "loop": (48, 900), "sidechain": (24, 1000), "all48": (48, 1100), "cutoff": (10, 1200), "no_n": (12, 1300), "b2": (20, 1400),
        "s3": (20, 1500)}
HELIX, STRAND = (-60.0, -45.0), (-120.0, 130.0)


def chain(n, rng, centre=(12.0, -9.0, 15.0)):
    """[n,5,3] float64 (N, CA, C, CB, O): helices, strands and turns of 4 .. 8 residues, rotated at random, its centroid at ``centre``."""
    torsions = []
    while len(torsions) < n:
        kind, length = rng.choice(3, p=[0.5, 0.2, 0.3]), int(rng.integers(4, 9))
        torsions += [HELIX if kind == 0 else STRAND if kind == 1 else tuple(rng.uniform(-180, 180, size=2)) for _ in range(length)]
    x = mv.ideal_chain(n, torsions[:n])
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    x = x @ q.T
    return x - x.reshape(-1, 3).mean(0) + np.asarray(centre)


def perturbed(x, rng, rows=None):
    """A model of the reference x [n,A,3]: per-residue shifts, atom noise and a hinged tail; ``rows``: only these rows move."""
    n = x.shape[0]
    y = x.copy()
    present = np.any(x != 0, axis=-1, keepdims=True)
    scale = rng.choice([0.05, 0.3, 0.8, 2.0], size=(n, 1, 1), p=[0.4, 0.3, 0.2, 0.1])
    y = y + scale * rng.normal(size=(n, 1, 3)) + 0.05 * rng.normal(size=x.shape)
    if n >= 6:
        h = int(rng.integers(n // 2, n - 2))
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        angle = np.deg2rad(rng.uniform(10, 30))
        kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        rot = np.eye(3) + np.sin(angle) * kx + (1 - np.cos(angle)) * kx @ kx
        y[h:] = (y[h:] - y[h, 1]) @ rot.T + y[h, 1]
    if rows is not None:
        keep = np.ones(n, dtype=bool)
        keep[rows] = False
        y[keep] = x[keep]
    return np.where(present, y, 0.0)


def with_side_chains(bb, rng, most):
    """[n,37,3]: the five backbone atoms and 0 .. ``most`` side-chain atoms per residue in columns 5 .., within 4 Angstrom of CB."""
    n = bb.shape[0]
    x = np.zeros((n, 37, 3))
    x[:, :5] = bb
    for i in range(n):
        for col in rng.choice(np.arange(5, 37), size=int(rng.integers(0, most + 1)), replace=False):
            step = rng.normal(size=3)
            x[i, col] = bb[i, 3] + step / np.linalg.norm(step) * rng.uniform(1.4, 4.0)
    return x


def case_inputs(name, n, seed):
    """(xa [S,n,A,3] float32, xb or None, res_mask, score_mask [S,n], pairs [P,2], extras)."""
    rng = np.random.default_rng(seed)
    ref = chain(n, rng)
    res_mask, score_mask, extras, xb = np.ones((1, n), dtype=np.float32), np.ones((1, n), dtype=np.float32), {}, None
    pairs = np.array([[0, 0]], dtype=np.int32)
    if name == "masked":
        res_mask[0, rng.choice(np.arange(1, n - 1), size=13, replace=False)] = 0
        xa, xb = perturbed(ref, rng)[None], ref[None]
    elif name == "loop":  # chain A of 30 rows with a 12-row loop, chain B of 18 rows beside it; the context keeps its coordinates
        second = chain(18, rng, centre=ref[:30].reshape(-1, 3).mean(0) + np.array([9.0, -6.0, 5.0]))
        ref = np.concatenate([ref[:30], second])
        score_mask[:] = 0
        score_mask[0, 10:22] = 1
        extras["chain_index"] = np.repeat([0, 1], [30, 18]).astype(np.int32)
        xa, xb = perturbed(ref, rng, rows=np.arange(10, 22))[None], ref[None]
    elif name in ("sidechain", "all48", "tile_all"):
        full = with_side_chains(ref, rng, 4 if name == "tile_all" else 8)
        model = perturbed(full, rng)
        if name == "sidechain":
            model[:, 5:] = 0  # a backbone-only model
        elif name == "all48":
            drop = rng.random(size=(n, 37)) < 0.1  # side-chain atoms the model lacks
            drop[:, :5] = False
            model[drop] = 0
        xa, xb = model[None], full[None]
    elif name == "cutoff":  # rows 1 and 8 just inside the cutoff, rows 2 and 9 just outside (CA atoms, the reference's distances)
        for (i, j), d in (((1, 8), 15.0 - 1e-3), ((2, 9), 15.0 + 1e-3)):
            line = ref[j, 1] - ref[i, 1]
            ref[j] += line / np.linalg.norm(line) * (d - np.linalg.norm(line))
        ref = ref.astype(np.float32).astype(np.float64)
        for (i, j), (lo, hi) in (((1, 8), (15.0 - 1.5e-3, 15.0 - 0.5e-3)), ((2, 9), (15.0 + 0.5e-3, 15.0 + 1.5e-3))):
            assert lo < np.linalg.norm(ref[i, 1] - ref[j, 1]) < hi, (name, seed)
        extras["planted"] = np.array([[1, 8], [2, 9]], dtype=np.int32)
        xa, xb = perturbed(ref, rng)[None], ref[None]
    elif name == "no_n":
        model = perturbed(ref, rng)
        model[5, 0] = 0  # row 5 of the model has no N: no frame there, still a point
        xa, xb = model[None], ref[None]
    elif name == "b2":  # two models, two references, crossed by ref_index
        xa, xb = np.stack([perturbed(ref, rng), perturbed(ref, rng)]), np.stack([ref, perturbed(ref, rng)])
        res_mask, score_mask = np.ones((2, n), dtype=np.float32), np.ones((2, n), dtype=np.float32)
        extras["ref_index"] = np.array([1, 0], dtype=np.int32)
        pairs = np.array([[0, 1], [1, 0]], dtype=np.int32)
    elif name == "s3":  # three samples, every ordered pair
        xa = np.stack([perturbed(ref, rng) for _ in range(3)])
        res_mask, score_mask = np.ones((3, n), dtype=np.float32), np.ones((3, n), dtype=np.float32)
        pairs = np.array([[i, j] for i in range(3) for j in range(3) if i != j], dtype=np.int32)
    else:
        xa, xb = perturbed(ref, rng)[None], ref[None]
    xa = xa.astype(np.float32)
    xb = None if xb is None else xb.astype(np.float32)
    assert max(np.abs(xa).max(), 0 if xb is None else np.abs(xb).max()) <= 100.0, (name, seed)
    return xa, xb, res_mask, score_mask, pairs, extras


def tensor(x, dtype):
    return torch.tensor(np.asarray(x), dtype=dtype)


def reference_lddt(xa, xb, mode, row, dtype):
    """(per atom [N,A], global) of the reference's functions for one pair; the multi-atom sets go through ``lddt`` on the flattened atoms."""
    cols_a, cols_b = lr.columns(mode, xa.shape[1]), lr.columns(mode, xb.shape[1])
    part = lr.exists(xa)[:, cols_a] & lr.exists(xb)[:, cols_b] & row[:, None]
    n, k = part.shape
    if mode == "ca":
        mask = np.zeros((n, 2))
        mask[:, 1] = part[:, 0]
        args = (tensor(xa[:, :2], dtype), tensor(xb[:, :2], dtype), tensor(mask, dtype))  # (lddt_ca reads column 1 of each)
        per, whole = loss.lddt_ca(*args, cutoff=15.0), loss.lddt_ca(*args, cutoff=15.0, per_residue=False)
    else:
        args = (tensor(xa[:, cols_a].reshape(n * k, 3), dtype), tensor(xb[:, cols_b].reshape(n * k, 3), dtype), tensor(part.reshape(n * k, 1), dtype))
        per, whole = loss.lddt(*args, cutoff=15.0), loss.lddt(*args, cutoff=15.0, per_residue=False)
    return per.double().numpy().reshape(n, k), float(whole)


def kept_rows(xa, xb, row, scored):
    ca_a, ca_b = (0 if xa.shape[1] == 1 else 1), (0 if xb.shape[1] == 1 else 1)
    return np.flatnonzero(row & scored & lr.exists(xa)[:, ca_a] & lr.exists(xb)[:, ca_b])


def reference_drmsd(xa, xb, row, scored, dtype, order=None):
    kept = kept_rows(xa, xb, row, scored)
    if order is not None:
        kept = np.array([r for r in order if r in set(kept.tolist())], dtype=np.int64)
    if len(kept) == 0:
        return 0.0
    return float(loss.compute_drmsd(tensor(xa[kept, 1], dtype), tensor(xb[kept, 1], dtype)))


def reference_fape(xa, xb, row, dtype=torch.float32):
    """compute_fape as backbone_loss calls it, on the frames of atom37_to_frames' group 0, over the rows that exist."""
    ex_a, ex_b = lr.exists(xa), lr.exists(xb)
    point = row & ex_a[:, 1] & ex_b[:, 1]
    framed = point & ex_a[:, 0] & ex_b[:, 0] & ex_a[:, 2] & ex_b[:, 2]

    def frames(x):
        r = Rigid.from_3_points(tensor(x[:, 2], dtype), tensor(x[:, 1], dtype), tensor(x[:, 0], dtype), eps=1e-8)
        return Rigid(Rotation(rot_mats=r.get_rots().get_rot_mats() * torch.tensor([-1.0, 1.0, -1.0], dtype=dtype)), r.get_trans())

    return float(loss.compute_fape(frames(xa), frames(xb), tensor(framed, dtype), tensor(xa[:, 1], dtype), tensor(xb[:, 1], dtype), tensor(point, dtype),
                                   length_scale=10.0, l1_clamp_distance=10.0, eps=1e-4))


def variants(name):
    """(mode, same_residue) of every run of a case."""
    return [(mode, same) for mode in lr.CASES[name] for same in ((False,) if mode == "ca" else (False, True))]


def decidable_inputs(name, n, base_seed):
    for seed in range(base_seed, base_seed + 200):
        try:
            xa, xb, res_mask, score_mask, pairs, extras = case_inputs(name, n, seed)
        except AssertionError:
            continue
        refs = xa if xb is None else xb
        margin = min(lr.local_accuracy(xa[ia], refs[ib], mode, res_mask[ia], score_mask[ia], same_residue=same)["margin"]
                     for ia, ib in pairs for mode, same in variants(name))
        if name in lr.MOTION_CASES:  # the moved model (float32 again) is as decidable and keeps every integer
            moved = lr.move(xa, *motion())
            for ia, ib in pairs:
                for mode, same in variants(name):
                    a = lr.local_accuracy(xa[ia], refs[ib], mode, res_mask[ia], score_mask[ia], same_residue=same)
                    b = lr.local_accuracy(moved[ia], refs[ib], mode, res_mask[ia], score_mask[ia], same_residue=same)
                    margin = min(margin, b["margin"] if all(np.array_equal(a[k], b[k]) for k in ("n_scored", "n_passed", "atom_lddt")) else 0.0)
        if margin >= MARGIN:
            return seed, margin, xa, xb, res_mask, score_mask, pairs, extras
    raise AssertionError(f"{name}: no decidable seed")


def motion():
    """(rotation [3,3], shift [3]): a proper rotation drawn once (seed 77) and a shift of 100 Angstrom."""
    q, _ = np.linalg.qr(np.random.default_rng(77).normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q, 100.0 * np.array([2.0, -1.0, 2.0]) / 3.0


def main():
    fix = {"perm_seeds": np.array(lr.PERM_SEEDS), "motion.rot": motion()[0], "motion.shift": motion()[1], "tile": np.int64(TILE), "tile_all": np.int64(TILE_ALL)}
    assert set(SPEC) == set(lr.CASES)
    for name, (n, base_seed) in SPEC.items():
        seed, margin, xa, xb, res_mask, score_mask, pairs, extras = decidable_inputs(name, n, base_seed)
        refs = xa if xb is None else xb
        fix.update({f"{name}.xa": xa, f"{name}.res_mask": res_mask, f"{name}.score_mask": score_mask, f"{name}.pairs": pairs, f"{name}.seed": np.int64(seed),
                    f"{name}.margin": np.float64(margin)})
        if xb is not None:
            fix[f"{name}.xb"] = xb
        fix.update({f"{name}.{k}": v for k, v in extras.items()})
        applies_global = lr.reference_applies_globally({f"{name}.score_mask": score_mask, f"{name}.res_mask": res_mask}, name)
        for mode in lr.CASES[name]:
            per64, per32, whole64, whole32 = [], [], [], []
            for ia, ib in pairs:
                row, scored = res_mask[ia] != 0, score_mask[ia] != 0
                a64, w64 = reference_lddt(xa[ia], refs[ib], mode, row, torch.float64)
                a32, w32 = reference_lddt(xa[ia], refs[ib], mode, row, torch.float32)
                mine = lr.local_accuracy(xa[ia], refs[ib], mode, res_mask[ia], score_mask[ia], same_residue=True)
                keep = row & scored
                assert np.array_equal(mine["atom_lddt"][keep], a64[keep]), (name, mode, "per atom")
                if mode == "ca":
                    assert np.array_equal(mine["res_lddt"][keep], a64[keep, 0]), (name, mode, "per residue")
                if applies_global:
                    assert mine["lddt"] == w64, (name, mode, "global")
                per64.append(a64), per32.append(a32), whole64.append(w64), whole32.append(w32)
            fix.update({f"{name}.{mode}.ref_atom": np.stack(per64), f"{name}.{mode}.ref_atom.f32": np.stack(per32).astype(np.float32),
                        f"{name}.{mode}.ref_lddt": np.array(whole64), f"{name}.{mode}.ref_lddt.f32": np.array(whole32)})
        # the float outputs: the same in every atom set (CA atoms, frames from N, CA, C)
        outs = {k: [] for k in lr.FLOAT_OUTPUTS}
        drmsd32, fape32, distance, yard = [], [], [], {k: 0.0 for k in lr.FLOAT_OUTPUTS}
        for ia, ib in pairs:
            a, b, row, scored = xa[ia], refs[ib], res_mask[ia] != 0, score_mask[ia] != 0
            mine = lr.local_accuracy(a, b, "ca", res_mask[ia], score_mask[ia])
            base = {"drmsd": reference_drmsd(a, b, row, scored, torch.float64), "fape": mine["fape"], "res_fape": mine["res_fape"],
                    "region_fape": mine["region_fape"]}
            assert abs(mine["drmsd"] - base["drmsd"]) <= 1e-12 * max(1.0, base["drmsd"]), (name, mine["drmsd"], base["drmsd"])
            drmsd32.append(reference_drmsd(a, b, row, scored, torch.float32))
            if not mine["status"] & lr.NO_FRAME:
                shipped = reference_fape(a, b, row)
                distance.append(abs(shipped - mine["fape"]) / mine["fape"])
                assert distance[-1] <= 1e-5, (name, shipped, mine["fape"])
                fape32.append(shipped)
            else:
                fape32.append(0.0)
            for seed_k in lr.PERM_SEEDS:
                perm = np.random.default_rng(seed_k).permutation(n)
                other = lr.local_accuracy(a[perm], b[perm], "ca", res_mask[ia][perm], score_mask[ia][perm])
                back = np.empty_like(other["res_fape"])
                back[perm] = other["res_fape"]
                moved = {"drmsd": reference_drmsd(a, b, row, scored, torch.float64, order=perm), "fape": other["fape"], "res_fape": back,
                         "region_fape": other["region_fape"]}
                for k in lr.FLOAT_OUTPUTS:
                    yard[k] = max(yard[k], float(np.max(np.abs(np.asarray(moved[k]) - np.asarray(base[k])))))
            for k in lr.FLOAT_OUTPUTS:
                outs[k].append(base[k])
        for k in lr.FLOAT_OUTPUTS:
            fix[f"{name}.{k}"] = np.stack([np.asarray(v, dtype=np.float64) for v in outs[k]])
            fix[f"{name}.{k}.yard"] = np.float64(yard[k])
        fix[f"{name}.drmsd.f32"], fix[f"{name}.fape.f32"] = np.array(drmsd32), np.array(fape32)
        fix[f"{name}.fape.ref_distance"] = np.float64(max(distance, default=0.0))
        print(f"{name}: N = {n}, seed {seed}, margin {margin:.1e}, lddt " + ", ".join(f"{m} {fix[f'{name}.{m}.ref_lddt'][0]:.3f}" for m in lr.CASES[name]) +
              f", drmsd {outs['drmsd'][0]:.3f}, fape {outs['fape'][0]:.4f} (float32 run at {fix[f'{name}.fape.ref_distance']:.1e}), yardsticks " +
              ", ".join(f"{k} {v:.1e}" for k, v in yard.items()), flush=True)
    path = os.path.join(HERE, "lddt_cases.npz")
    np.savez_compressed(path, **fix)
    print(f"{os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
