"""Fixture of the GDT tests, captured from the restatement and the reference (the container with the reference sources only):

    python tests/golden/make_goldens_gdt.py      # -> tests/golden/gdt_cases.npz

Per case (SPEC below; gdt_ref.CASES) the float32 CA traces of the model and the reference structure, their masks, the normalisation
length (0: the number of rows scored) and, per mode ``none``, ``global`` and ``search``, the outputs of the NumPy restatement of the
contract (tests/gdt_ref.py) as ``<case>.<mode>.<output>`` - ``res_within`` spread to the N rows as the device
reports it.  No LGA program exists to capture ``search`` from: it is this project's contract, pinned by the restatement.

For ``none`` the reference's own numbers are recorded beside them: openfold/utils/validation_metrics.py ``gdt_ts`` and ``gdt_ha`` on the
raw float32 coordinates with the product of the masks (``<case>.none.ref_ts``, ``ref_ha``, float32) and the five single-cutoff counts
``round(gdt(p1, p2, mask, [c]) * n)`` (``ref_counts``).  For ``global`` the same calls on coordinates superposed by a NumPy SVD
(Kabsch, float64, proper rotation): openfold/utils/superimposition.py ``superimpose`` goes through Biopython's SVDSuperimposer, which
this container does not have, so ``superimpose`` itself cannot run.

Asserted here, not measured by the tests; the seed of a case is the first from its base that passes:
 (a) every distance compared with a cutoff or a selection cut, in every pass of every item of the search and under the ``global``
     transform, is at least 1e-9 Angstrom from the threshold (``<case>.<mode>.margin``); in ``none`` the arithmetic is exact and a
     distance that EQUALS a cutoff (case ``exact``) is decided by ``<=`` itself;
 (b) under the transforms compared with the reference (the identity; the restatement's and the SVD's global superposition) every
     distance is at least 1e-3 Angstrom from every cutoff - float32 rounding at |coordinate| <= 100 Angstrom is ~1e-5 - the equal
     distance of ``exact`` aside, which float32 holds exactly too;
 (c) the restatement's counts equal the reference's integers in ``none`` and ``global``;
 (d) the closed forms: every searched count of ``planted`` is m and every ``global`` count is smaller; the ``search`` counts are never
     below the ``global`` ones; the cut widens in ``unrelated``; ``exact`` counts its 2.0 Angstrom row at cutoff 2.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_goldens_violations as mv  # noqa: E402,F401  (installs the import harness of the reference)
from openfold.utils import validation_metrics as vm  # noqa: E402

import gdt_ref as gr  # noqa: E402
from make_goldens_tm import rotation, walk  # noqa: E402

# name: (rows N of the arrays, kind, base seed)
SPEC = {"n1": (1, "noise", 100), "n2": (2, "noise", 200), "n3": (3, "noise", 300), "n4": (4, "noise", 400), "n5": (5, "noise", 500), "n9": (9, "noise", 600),
        "n37": (37, "noise", 700), "n64": (64, "noise", 800), "n65": (65, "noise", 900), "n130": (130, "noise", 1000), "masked": (90, "masked", 1100),
        "planted": (40, "planted", 1200), "hinge": (60, "hinge", 1300), "exact": (8, "exact", 1400), "unrelated": (50, "unrelated", 1500),
        "n1024": (1024, "noise", 1600), "nan": (9, "nan", 1700)}
PLANTED_M, HINGE_ROW, EXACT_ROW = 22, 25, 2
MARGIN_A, MARGIN_B = 1e-9, 1e-3


def traces(n, kind, seed):
    """(ca_a, ca_b [N,3] float32, mask_a, mask_b [N] float32, norm_length): the model a and the reference b."""
    rng = np.random.default_rng(seed)
    b = walk(rng, n)
    mask_a, mask_b, norm = np.ones(n, dtype=np.float32), np.ones(n, dtype=np.float32), 0
    # a sample against its ground truth in the frame of a fixed context: a small rigid error and per-row errors of 0.2 .. 3 Angstrom
    tilt = rotation(rng)
    angle = np.deg2rad(4.0)
    axis = tilt[:, 0]
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    small = np.eye(3) + np.sin(angle) * kx + (1 - np.cos(angle)) * kx @ kx
    centre = b.mean(0)
    if kind == "unrelated":
        a = walk(rng, n)
    elif kind == "hinge":  # two rigid halves: rows from HINGE_ROW on turn about that row
        a, q2 = b.copy(), rotation(rng)
        a[HINGE_ROW:] = (a[HINGE_ROW:] - a[HINGE_ROW]) @ q2.T + a[HINGE_ROW]
        a = (a - centre) @ small.T + centre + rng.normal(size=3)
    elif kind == "planted":  # rows 0 .. m - 1 an exact rigid image, every other row 20 Angstrom off in one direction: the least-squares
        off = np.tile(rng.normal(size=(1, 3)), (n, 1))  # superposition of all rows lands between the two parts
        off = 20.0 * off / np.linalg.norm(off, axis=1, keepdims=True)
        off[:PLANTED_M] = 0.0
        a = (b + off) @ rotation(rng).T + rng.normal(size=3) * 10.0
    elif kind == "exact":  # on a grid of 1/8 Angstrom: float32 and float64 hold every coordinate and difference exactly
        b = np.round(b * 8.0) / 8.0
        a = b + np.round(rng.uniform(-1.2, 1.2, size=b.shape) * 8.0) / 8.0 + np.array([0.0625, 0.0, 0.0])
        a[EXACT_ROW] = b[EXACT_ROW] + np.array([2.0, 0.0, 0.0])
    else:
        scale = rng.choice([0.2, 0.6, 1.5, 3.0], size=(n, 1), p=[0.35, 0.3, 0.2, 0.15])
        a = (b + scale * rng.normal(size=b.shape) / np.sqrt(3.0) - centre) @ small.T + centre + 0.3 * rng.normal(size=3)
    if kind == "masked":  # rows dropped at both ends and in the middle, not the same rows in the two masks; L = the unmasked length
        mask_a[:3], mask_a[40:47], mask_a[-2:] = 0, 0, 0
        mask_b[:1], mask_b[44:52], mask_b[70], mask_b[-5:] = 0, 0, 0, 0
        norm = n
    a, b = a.astype(np.float32), b.astype(np.float32)
    if kind == "nan":
        a[4, 1] = np.nan
    return a, b, mask_a, mask_b, norm


def kabsch(x, y):
    """(R [3,3], t [3]) with R x + t ~ y, least squares, a proper rotation: NumPy's SVD."""
    cx, cy = x.mean(0), y.mean(0)
    u, _, vt = np.linalg.svd((x - cx).T @ (y - cy))
    d = np.sign(np.linalg.det(vt.T @ u.T))
    r = vt.T @ np.diag([1.0, 1.0, d]) @ u.T
    return r, cy - r @ cx


def reference_numbers(p1, p2, mask):
    """The reference's float32 gdt_ts, gdt_ha and the five single-cutoff counts of model p1, reference p2 [N,3] and mask [N]."""
    t1, t2, m = torch.from_numpy(np.asarray(p1)), torch.from_numpy(np.asarray(p2)), torch.from_numpy(np.asarray(mask, dtype=np.float32))
    n = float(m.sum())
    counts = [int(round(float(vm.gdt(t1, t2, m, [c])) * n)) for c in gr.CUTOFFS]
    return np.float32(vm.gdt_ts(t1, t2, m).numpy()), np.float32(vm.gdt_ha(t1, t2, m).numpy()), np.array(counts, dtype=np.int64)


def cutoff_gap(d, skip_exact=False):
    gap = np.abs(d[:, None] - np.array(gr.CUTOFFS)[None, :])
    if skip_exact:
        gap = np.where(d[:, None] == np.array(gr.CUTOFFS)[None, :], np.inf, gap)
    return float(gap.min())


def one_case(name, n, kind, seed):
    """The fixture entries of a case, or a string: why this seed does not pass."""
    ca_a, ca_b, mask_a, mask_b, norm = traces(n, kind, seed)
    fix = {f"{name}.ca_a": ca_a, f"{name}.ca_b": ca_b, f"{name}.mask_a": mask_a, f"{name}.mask_b": mask_b, f"{name}.norm_length": np.int64(norm),
           f"{name}.seed": np.int64(seed)}
    rows = gr.scored_rows(mask_a, mask_b)
    x, y = ca_a[rows].astype(np.float64), ca_b[rows].astype(np.float64)
    both = mask_a * mask_b
    res = {}
    for mode in gr.MODES:
        res[mode] = out = gr.gdt(x, y, mode, norm or None)
        if out["status"] == 0 and not out["margin"] >= MARGIN_A:
            return f"{mode}: a distance {out['margin']:.1e} from a threshold"
        for k in gr.RECORDED:
            v = gr.spread(out[k], rows, n) if k == "res_within" else out[k]
            fix[f"{name}.{mode}.{k}"] = np.asarray(v, dtype=np.float64 if k in ("gdt_ts", "gdt_ha", "rotation", "translation") else np.int32 if k == "res_within" else np.int64)
        fix[f"{name}.{mode}.margin"] = np.float64(out["margin"])
        if out["status"] or mode == "search":
            continue
        # the reference on the raw coordinates (none) and on coordinates superposed by NumPy's SVD (global)
        if mode == "none":
            moved, gaps = ca_a, [cutoff_gap(np.sqrt(((x - y) ** 2).sum(1)), skip_exact=True)]
        else:
            r, t = kabsch(x, y)
            moved = (ca_a.astype(np.float64) @ r.T + t).astype(np.float32)
            own = x @ out["rotation"][0].T + out["translation"][0]
            gaps = [cutoff_gap(np.sqrt(((x @ r.T + t - y) ** 2).sum(1))), cutoff_gap(np.sqrt(((own - y) ** 2).sum(1)))]
        if min(gaps) < MARGIN_B:
            return f"{mode}: a distance {min(gaps):.1e} from a cutoff"
        ref_ts, ref_ha, ref_counts = reference_numbers(moved, ca_b, both)
        if not np.array_equal(ref_counts, out["counts"]):
            raise SystemExit(f"{name} {mode}: the restatement counts {out['counts']}, the reference {ref_counts}")
        plain = gr.gdt(x, y, mode)  # (the reference divides by the rows scored)
        assert abs(plain["gdt_ts"] - float(ref_ts)) <= 1e-6 and abs(plain["gdt_ha"] - float(ref_ha)) <= 1e-6, (name, mode)
        fix.update({f"{name}.{mode}.ref_ts": ref_ts, f"{name}.{mode}.ref_ha": ref_ha, f"{name}.{mode}.ref_counts": ref_counts})
    glob, search = res["global"], res["search"]
    if search["status"] == 0:
        assert (search["counts"] >= glob["counts"]).all(), (name, search["counts"], glob["counts"])
    if kind == "planted" and not ((search["counts"] == PLANTED_M).all() and (glob["counts"] < PLANTED_M).all()):
        return f"planted: search {search['counts']}, global {glob['counts']}"
    if kind == "unrelated" and not search["widened"] > 0:
        return "unrelated: the cut never widened"
    if kind == "exact":
        d2 = ((x - y) ** 2).sum(1)
        assert d2[EXACT_ROW] == 4.0 and res["none"]["res_within"][EXACT_ROW] & 4 and not res["none"]["res_within"][EXACT_ROW] & 2
    fix[f"{name}.search.widened"] = np.int64(search.get("widened", 0))
    print(f"{name}: seed {seed}, n = {len(rows)} of N = {n}, counts none {res['none']['counts']}, global {glob['counts']}, search {search['counts']}; "
          f"items {search['best_item']}, passes {search['best_pass']} of {search['passes']}, widened {search.get('widened', 0)}, margins "
          f"{res['none']['margin']:.1e} {glob['margin']:.1e} {search['margin']:.1e}", flush=True)
    return fix


def main():
    assert tuple(SPEC) == gr.CASES
    fix = {"cases": np.array(list(SPEC))}
    for name, (n, kind, base) in SPEC.items():
        for seed in range(base, base + 50):
            got = one_case(name, n, kind, seed)
            if isinstance(got, dict):
                fix.update(got)
                break
            print(f"{name}: seed {seed} does not pass ({got})", flush=True)
        else:
            raise SystemExit(f"{name}: no seed of 50 passes")
    np.savez_compressed(os.path.join(HERE, "gdt_cases.npz"), **fix)
    print(f"{os.path.getsize(os.path.join(HERE, 'gdt_cases.npz')) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
