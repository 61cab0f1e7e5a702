"""Fixture of the TM-score tests:

    python tests/golden/make_goldens_tm.py      # -> tests/golden/tm_cases.npz

No tmtools exists to capture from: the expected numbers are those of the NumPy restatement of the contract (tests/tm_ref.py; DESIGN.md
section 7.8).  Per case (SPEC below; tm_ref.CASES) the float32 CA traces of the two structures, their masks, the normalisation length
(0: the number of rows scored) and the restatement's outputs ``<case>.<output>``.  Next to every float output the yardstick
``<case>.<output>.yard``: the restatement's own change between its two evaluation orders (rows ascending, rows descending - every sum
runs the other way round).  A pair whose yardstick exceeds 1e-9 took another path through the selection steps in the second order; the
bound of the GPU tests would mean nothing for it, and this script refuses to record it.  ``<case>.lead`` is the lead of the best seed's
score over every other seed's, over L: where it exceeds the bound the GPU tests compare ``best_seed``.

The backbones: persistent random walks with 3.8 Angstrom steps tens of Angstrom from the origin, and CA excerpts of the three complexes
of tests/golden/sasa_cases.npz (coordinates only).  Structure ``a`` is ``b`` moved rigidly with noise on top (a sample against its
ground truth) unless the case says otherwise.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import sasa_ref as sr  # noqa: E402
import tm_ref as tr  # noqa: E402

# name: (rows N of the arrays, source, kind, seed); kind: "noise" (1 Angstrom), "unrelated", "hinge", "masked"
SPEC = {
    "n3": (3, "walk", "noise", 1), "n4": (4, "walk", "noise", 2), "n5": (5, "walk", "noise", 3), "n9": (9, "walk", "noise", 4),
    "n19": (19, "walk", "noise", 5), "n37": (37, "7t2d:40", "noise", 6), "n64": (64, "walk", "noise", 7), "n65": (65, "walk", "noise", 8),
    "n80": (80, "1fyt:100", "noise", 9), "n130": (130, "5ksa:200", "noise", 10), "hinge": (60, "walk", "hinge", 11),
    "masked": (90, "1fyt:300", "masked", 12), "unrelated": (50, "walk", "unrelated", 13), "n1024": (1024, "walk", "noise", 14),
}
YARD_LIMIT = 1e-9


def walk(rng, n, persist=0.7):
    d, out = rng.normal(size=3), [np.zeros(3)]
    for _ in range(n - 1):
        d = persist * d + (1.0 - persist) * 1.5 * rng.normal(size=3)
        d /= np.linalg.norm(d)
        out.append(out[-1] + 3.8 * d)
    return np.array(out) + np.array([31.0, -47.0, 58.0])


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def traces(fix_sasa, n, source, kind, seed):
    """(ca_a, ca_b [N,3] float32, mask_a, mask_b [N] float32, norm_length)."""
    rng = np.random.default_rng(seed)
    if source == "walk":
        b = walk(rng, n)
    else:
        name, first = source.split(":")
        prot, mask, _ = sr.case_prot(fix_sasa, name, 5)
        b = prot[int(first):int(first) + n, 1].astype(np.float64)
        assert mask[int(first):int(first) + n, 1].all() and len(b) == n
    q, shift = rotation(rng), rng.normal(size=3) * 20.0
    mask_a, mask_b, norm = np.ones(n, dtype=np.float32), np.ones(n, dtype=np.float32), 0
    if kind == "unrelated":
        a = walk(rng, n)
    elif kind == "hinge":  # rows from 25 on turn about row 25
        a, k, q2 = b.copy(), 25, rotation(rng)
        a[k:] = (a[k:] - a[k]) @ q2.T + a[k]
        a = a @ q.T + shift
    else:
        a = (b + rng.normal(size=b.shape) / np.sqrt(3.0)) @ q.T + shift
    if kind == "masked":  # rows dropped at both ends and in the middle, not the same rows in the two masks; L = the unmasked length
        mask_a[:3], mask_a[40:47], mask_a[-2:] = 0, 0, 0
        mask_b[:1], mask_b[44:52], mask_b[70], mask_b[-5:] = 0, 0, 0, 0
        norm = n
    return a.astype(np.float32), b.astype(np.float32), mask_a, mask_b, norm


def main():
    fix_sasa = dict(np.load(os.path.join(HERE, "sasa_cases.npz")))
    fix = {"cases": np.array(list(SPEC))}
    assert tuple(SPEC) == tr.CASES
    for name, (n, source, kind, seed) in SPEC.items():
        ca_a, ca_b, mask_a, mask_b, norm = traces(fix_sasa, n, source, kind, seed)
        fix.update({f"{name}.ca_a": ca_a, f"{name}.ca_b": ca_b, f"{name}.mask_a": mask_a, f"{name}.mask_b": mask_b, f"{name}.norm_length": np.int64(norm)})
        a, b, ma, mb, nl = tr.case_inputs(fix, name)
        x, y = tr.compact(a, b, ma, mb)
        up, down = tr.tm_score(x, y, nl), tr.tm_score(x, y, nl, descending=True)
        yard = abs(up["tm"] - down["tm"])
        if not yard <= YARD_LIMIT:
            raise SystemExit(f"{name}: the two evaluation orders differ by {yard:.3e} > {YARD_LIMIT}: a path flip inside the restatement; not recorded")
        others = np.delete(up["seed_score"], up["best_seed"])
        lead = (up["seed_score"][up["best_seed"]] - others.max()) / up["length"] if len(others) else 1.0
        for k in ("tm", "d0", "rotation", "translation"):
            fix[f"{name}.{k}"] = np.asarray(up[k], dtype=np.float64)
        for k in ("n_aligned", "best_seed", "passes", "status", "widened"):
            fix[f"{name}.{k}"] = np.int64(up[k])
        fix[f"{name}.tm.yard"], fix[f"{name}.d0.yard"], fix[f"{name}.lead"] = np.float64(yard), np.float64(0.0), np.float64(lead)
        fix[f"{name}.passes_down"], fix[f"{name}.best_seed_down"] = np.int64(down["passes"]), np.int64(down["best_seed"])
        print(f"{name}: n = {up['n_aligned']} of N = {n}, L = {up['length']}, d0 = {up['d0']:.4f}, tm = {up['tm']:.6f}, yard {yard:.1e}, seeds "
              f"{len(up['seed_score'])}, best {up['best_seed']} (lead {lead:.1e}), passes {up['passes']} (most {up['seed_passes'].max()}), widened {up['widened']}")
    assert int(fix["unrelated.widened"]) > 0
    np.savez_compressed(os.path.join(HERE, "tm_cases.npz"), **fix)
    print(f"{os.path.getsize(os.path.join(HERE, 'tm_cases.npz')) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
