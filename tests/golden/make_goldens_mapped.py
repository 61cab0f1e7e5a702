"""Fixture of the mapped accuracy tests, captured from the reference (the container with the reference sources only):

    python tests/golden/make_goldens_mapped.py      # -> tests/golden/mapped_cases.npz   (arrays only)

Per case (mapped_cases.GOLDEN_CASES: one per atom set) the inputs - model, reference, row map, masks - and the reference's own numbers on
the GATHERED model G (model row map[j] at reference row j):

* lDDT, the penalise oracle: openfold/utils/loss.py ``lddt_ca`` (the ``ca`` set) / ``lddt`` on the flattened atom list (the multi-atom
  sets: ``same_residue=True``) on float64 tensors, predicted positions = G with every absent atom at a far, distinct point
  (mapped_ref.far_points), true positions = the reference structure, mask = the atoms that exist in the reference - the call a user of
  the reference makes when only the true mask is known.  Per atom (``<case>.ref_atom`` [N_b,A]) and with ``per_residue=False``
  (``<case>.ref_lddt``).  Asserted here: the restatement's penalise rule gives the same bits.
* GDT: openfold/utils/validation_metrics.py ``gdt_ts``, ``gdt_ha`` and the five single-cutoff counts on the gathered CA rows, raw
  (``<case>.none.ref_*``) and after a NumPy SVD superposition (``<case>.global.ref_*``; make_goldens_gdt.py says why not ``superimpose``).
  Asserted here: the restatement's counts are the reference's integers, and every distance is 1e-3 Angstrom from every cutoff.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_goldens_gdt as mg  # noqa: E402  (installs the import harness of the reference)
import torch  # noqa: E402
from openfold.utils import loss  # noqa: E402

import lddt_ref as lr  # noqa: E402
import mapped_cases as mc  # noqa: E402
import mapped_ref as mr  # noqa: E402

# name: (N_a, N_b, atoms per row, base seed)
SPEC = {"g_ca": (40, 50, 5, 2100), "g_bb": (44, 38, 5, 2200), "g_all": (20, 24, 37, 2300)}


def inputs(n_a, n_b, atoms, seed):
    rng = np.random.default_rng(seed)
    xb = mc.structure(n_b, rng, atoms)
    m = mc.row_map_of("scatter", n_a, n_b, rng)
    xa = mc.model_of(xb, m, n_a, rng)
    res_mask, res_mask_b = np.ones((1, n_a), dtype=np.float32), np.ones((1, n_b), dtype=np.float32)
    covered = np.flatnonzero(m >= 0)
    res_mask_b[0, covered[1]] = 0
    res_mask[0, m[covered[3]]] = 0
    if atoms == 37:
        xa[m[covered[::4]], 5:] = 0.0
        xb[covered[7], 0] = 0.0
    return {"prot_a": xa[None].astype(np.float32), "prot_b": xb[None].astype(np.float32), "alignment": m, "res_mask": res_mask, "res_mask_b": res_mask_b,
            "score_mask": np.ones((1, n_b), dtype=np.float32)}


def reference_penalise(case, mode):
    """(per atom [N_b,A] float64, global) of the reference on the far-point gathered model, under the reference's mask alone."""
    xa, xb, m = case["prot_a"][0], case["prot_b"][0], case["alignment"]
    exists_b = case["res_mask_b"][0] != 0
    g, present = mr.gathered(xa, m, mr.covered_rows(m, len(xa), case["res_mask"][0], case["res_mask_b"][0]))
    far = mr.far_points(g, present)
    cols = lr.columns(mode, xb.shape[1])
    in_ref = lr.exists(xb)[:, cols] & exists_b[:, None]
    n, k = in_ref.shape
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)  # noqa: E731
    if mode == "ca":
        mask = np.zeros((n, 2))
        mask[:, 1] = in_ref[:, 0]
        args = (t(far[:, :2]), t(xb[:, :2]), t(mask))
        per, whole = loss.lddt_ca(*args, cutoff=15.0), loss.lddt_ca(*args, cutoff=15.0, per_residue=False)
    else:
        args = (t(far[:, cols].reshape(n * k, 3)), t(xb[:, cols].reshape(n * k, 3)), t(in_ref.reshape(n * k, 1)))
        per, whole = loss.lddt(*args, cutoff=15.0), loss.lddt(*args, cutoff=15.0, per_residue=False)
    return per.double().numpy().reshape(n, k), float(whole)


def one_case(name, n_a, n_b, atoms, seed):
    case, mode = inputs(n_a, n_b, atoms, seed), mc.GOLDEN_CASES[name]
    xa, xb, m = case["prot_a"][0], case["prot_b"][0], case["alignment"]
    fix = {f"{name}.{k}": v for k, v in case.items()}
    per, whole = reference_penalise(case, mode)
    own = mr.local_accuracy(xa, xb, m, mode, "penalise", case["res_mask"][0], case["res_mask_b"][0], case["score_mask"][0], same_residue=mode != "ca")
    exists_b = case["res_mask_b"][0] != 0
    assert np.array_equal(own["atom_lddt"][exists_b], per[exists_b]) and own["lddt"] == whole, (name, "the penalise rule is not the reference's lddt")
    fix.update({f"{name}.ref_atom": per, f"{name}.ref_lddt": np.float64(whole)})
    # GDT on the gathered CA rows
    rows = mr.gdt_rows(m, n_a, case["res_mask"][0], case["res_mask_b"][0])
    x32, y32 = xa[m[rows], 1], xb[rows, 1]
    x, y = x32.astype(np.float64), y32.astype(np.float64)
    for gmode in ("none", "global"):
        out = mr.gdt(xa[:, 1], xb[:, 1], m, gmode, case["res_mask"][0], case["res_mask_b"][0])
        if gmode == "none":
            moved, gaps = x32, [mg.cutoff_gap(np.sqrt(((x - y) ** 2).sum(1)))]
        else:
            r, t = mg.kabsch(x, y)
            moved = (x @ r.T + t).astype(np.float32)
            own_moved = x @ out["rotation"][0].T + out["translation"][0]
            gaps = [mg.cutoff_gap(np.sqrt(((x @ r.T + t - y) ** 2).sum(1))), mg.cutoff_gap(np.sqrt(((own_moved - y) ** 2).sum(1)))]
        if min(gaps) < mg.MARGIN_B:
            return f"gdt {gmode}: a distance {min(gaps):.1e} from a cutoff"
        ref_ts, ref_ha, ref_counts = mg.reference_numbers(moved, y32, np.ones(len(rows), dtype=np.float32))
        assert np.array_equal(ref_counts, out["counts"]), (name, gmode, ref_counts, out["counts"])
        assert abs(out["gdt_ts"] - float(ref_ts)) <= 1e-6 and abs(out["gdt_ha"] - float(ref_ha)) <= 1e-6, (name, gmode)
        fix.update({f"{name}.{gmode}.ref_ts": ref_ts, f"{name}.{gmode}.ref_ha": ref_ha, f"{name}.{gmode}.ref_counts": ref_counts})
    print(f"{name}: seed {seed}, {len(rows)} of {n_b} reference rows covered, lddt {whole:.4f}, counts {ref_counts}", flush=True)
    return fix


def main():
    assert tuple(SPEC) == tuple(mc.GOLDEN_CASES)
    fix = {}
    for name, (n_a, n_b, atoms, base) in SPEC.items():
        for seed in range(base, base + 50):
            got = one_case(name, n_a, n_b, atoms, seed)
            if isinstance(got, dict):
                fix.update(got)
                break
            print(f"{name}: seed {seed} does not pass ({got})", flush=True)
        else:
            raise SystemExit(f"{name}: no seed of 50 passes")
    path = os.path.join(HERE, "mapped_cases.npz")
    np.savez_compressed(path, **fix)
    print(f"{os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
