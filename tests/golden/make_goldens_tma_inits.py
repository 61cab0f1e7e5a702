"""Fixture of the five-start mode of the structural alignment search (``inits="all"``; DESIGN.md section 7.9, "The two fragment starts"):

    python tests/golden/make_goldens_tma_inits.py      # -> tests/golden/tma_inits_cases.npz

As tma_cases.npz (make_goldens_tma.py): per case (SPEC below; tma_inits_ref.CASES) the float32 CA traces, their masks and the outputs
of the NumPy restatement tests/tma_inits_ref.py, the alignment in original rows, and next to every float output ``<case>.<output>.yard``,
the restatement's change between its two evaluation orders.  A case whose ``tm`` yard exceeds 1e-9 or whose exact outputs differ between
the orders is refused.  The cases are the smallest shapes at which the two new starts can go wrong: no candidate of I4 (5 x 5), one
fragment length (6 x 9), both ``d0`` branches, every threshold of I4's jump (151, 201, 251 rows), the second row per thread (300), the
row limit (512); for Frag a 12 Angstrom gap with the longer run behind it, two equal runs, a trace spaced 4.5 Angstrom (one widening
round), equal runs in both traces with the shorter trace first and second (the donor); the masked case of tma_cases.npz; and two planted
pairs (tma_inits_ref.planted_motif: a rigid 40-row motif at rows 5 .. 44 of 120 and 80 .. 119 of 125, 0.3 and 0.05 Angstrom of noise).
A planted pair is recorded with the first seed at which ``best_init >= 3`` and ``tm_b`` lies at least 0.1 above the default search's
(tests/tma_ref.py) on the same pair, which is stored as ``<case>.default_tm_b``.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import tma_inits_ref as ti  # noqa: E402
import tma_ref as ta  # noqa: E402
import make_goldens_tma as mt  # noqa: E402
from make_goldens_tm import rotation, walk  # noqa: E402

YARD_LIMIT = 1e-9
PLANTED_GAIN = 0.1
# name: (kind, seed, parameters)
SPEC = {
    "n5": ("window", 1, dict(na=5, nb=5, first=0, sigma=0.3)),
    "n6x9": ("window", 2, dict(na=6, nb=9, first=2, sigma=0.3)),
    "n19x22": ("window", 3, dict(na=19, nb=22, first=1, sigma=0.5)),
    "n64x65": ("window", 4, dict(na=64, nb=65, first=1, sigma=1.0)),
    "n151x150": ("window", 5, dict(na=151, nb=150, first=2, sigma=1.0)),
    "n201x200": ("window", 6, dict(na=201, nb=200, first=2, sigma=1.0)),
    "n251x250": ("window", 7, dict(na=251, nb=250, first=2, sigma=1.0)),
    "n300": ("window", 8, dict(na=300, nb=300, first=3, sigma=1.0)),
    "n512": ("window", 9, dict(na=512, nb=512, first=0, sigma=1.0)),
    "gap12": ("gaps", 10, dict(n=40, gaps_a=(), gaps_b=(15,), sigma=0.1)),
    "equal_runs": ("gaps", 11, dict(n=41, gaps_a=(), gaps_b=(14, 28), sigma=0.1)),
    "wide45": ("wide", 12, dict(n=36, step=4.5, sigma=0.02)),
    "donor_x": ("donor", 13, dict(first=True)),
    "donor_y": ("donor", 13, dict(first=False)),
    "masked": ("masked", 12, dict(n=90, source="1fyt:300")),
    "motif03": ("planted", 0, dict(sigma=0.3)),
    "motif005": ("planted", 0, dict(sigma=0.05)),
}


def with_gaps(w, gaps, length=12.0):
    """The walk with the step into each row of ``gaps`` stretched to ``length`` Angstrom."""
    w = w.copy()
    for g in gaps:
        step = w[g] - w[g - 1]
        w[g:] += step / np.linalg.norm(step) * (length - np.linalg.norm(step))
    return w


def traces(fix_sasa, kind, seed, par):
    """(ca_a [N_a,3], ca_b [N_b,3] float32, mask_a [N_a], mask_b [N_b] float32)."""
    if kind == "masked":  # the traces of tma_cases.npz's case
        return mt.traces(fix_sasa, kind, seed, par)
    rng = np.random.default_rng(seed)
    q, shift = rotation(rng), rng.normal(size=3) * 20.0
    move = lambda a: a @ q.T + shift  # noqa: E731
    noisy = lambda a, sigma: a + sigma * rng.normal(size=a.shape) / np.sqrt(3.0)  # noqa: E731
    if kind == "window":  # a: a noisy window of the walk b is cut from, `first` rows on
        w = walk(rng, max(par["first"] + par["na"], par["nb"]))
        a, b = move(noisy(w[par["first"]:par["first"] + par["na"]], par["sigma"])), w[:par["nb"]]
    elif kind == "gaps":
        w = walk(rng, par["n"])
        a, b = move(noisy(with_gaps(w, par["gaps_a"]), par["sigma"])), with_gaps(w, par["gaps_b"])
    elif kind == "wide":
        w = walk(rng, par["n"])
        b = w[0] + (w - w[0]) * (par["step"] / 3.8)
        a = move(noisy(b[2:], par["sigma"]))
    elif kind == "donor":  # runs of 20 rows in both traces: rows 10 .. 29 of 30, rows 0 .. 19 of 36
        w = walk(rng, 36)
        short, long_ = with_gaps(w[:30], (10,)), move(noisy(with_gaps(w, (20,)), 0.1))
        a, b = (short, long_) if par["first"] else (long_, short)
    elif kind == "planted":
        a, b = ti.planted_motif(seed, par["sigma"], walk)
        a = move(a)
    else:
        raise ValueError(kind)
    return a.astype(np.float32), b.astype(np.float32), np.ones(len(a), dtype=np.float32), np.ones(len(b), dtype=np.float32)


def both_orders(name, prot_a, prot_b, mask_a=None, mask_b=None):
    """The restatement in its two evaluation orders; (outputs of the ascending one, yard per float output)."""
    up = ti.align_structures(prot_a, prot_b, mask_a, mask_b)
    down = ti.align_structures(prot_a, prot_b, mask_a, mask_b, descending=True)
    yard = {k: np.abs(np.asarray(up[k], dtype=np.float64) - np.asarray(down[k], dtype=np.float64)) for k in ti.FLOAT_OUTPUTS}
    yard = {k: np.where(np.isnan(v), 0.0, v) for k, v in yard.items()}
    flips = [k for k in ti.EXACT_OUTPUTS if not np.array_equal(up[k], down[k])]
    if not yard["tm"] <= YARD_LIMIT or flips:
        raise SystemExit(f"{name}: the two evaluation orders differ (tm by {float(yard['tm']):.3e}; {flips}): a path flip inside the restatement; "
                         "not recorded - change the case's seed")
    return up, yard


def main():
    fix_sasa = dict(np.load(os.path.join(HERE, "sasa_cases.npz")))
    fix = {"cases": np.array(list(SPEC))}
    assert tuple(SPEC) == ti.CASES
    winners = []
    for name, (kind, seed, par) in SPEC.items():
        while True:
            ca_a, ca_b, mask_a, mask_b = traces(fix_sasa, kind, seed, par)
            fix.update({f"{name}.ca_a": ca_a, f"{name}.ca_b": ca_b, f"{name}.mask_a": mask_a, f"{name}.mask_b": mask_b})
            up, yard = both_orders(name, *ti.case_inputs(fix, name))
            if kind != "planted":
                break
            default = ta.align_structures(*ti.case_inputs(fix, name))["tm_b"]
            if up["best_init"] >= 3 and up["tm_b"] >= default + PLANTED_GAIN:
                fix[f"{name}.default_tm_b"], fix[f"{name}.seed"] = np.float64(default), np.int64(seed)
                break
            print(f"{name}: seed {seed} refused (best_init {up['best_init']}, tm_b {up['tm_b']:.4f} against the default's {default:.4f})", flush=True)
            seed += 1
        mt.record(fix, name, up, yard)
        winners.append(int(up["best_init"]))
        print(f"{name}: n1 = {int(mask_a.sum())}, n2 = {int(mask_b.sum())}, tm_a = {up['tm_a']:.6f}, tm_b = {up['tm_b']:.6f} (yard {float(yard['tm']):.1e}), "
              f"aligned {up['n_aligned']}, init_tm {np.round(up['init_tm'], 4)}, init_dp {up['init_dp']}, best {up['best_init']}, status {up['status']}, "
              f"I4 candidate {up.get('i4_candidate')} of {up.get('i4_candidates')}, I5 offset {up.get('i5_offset')}"
              + (f", default tm_b {float(fix[f'{name}.default_tm_b']):.6f} (seed {seed})" if kind == "planted" else ""), flush=True)
    print("best_init over the cases:", dict(zip(SPEC, winners)))
    np.savez_compressed(os.path.join(HERE, "tma_inits_cases.npz"), **fix)
    print(f"{os.path.getsize(os.path.join(HERE, 'tma_inits_cases.npz')) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
