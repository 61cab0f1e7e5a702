"""Fixture of the structural-alignment tests:

    python tests/golden/make_goldens_tma.py      # -> tests/golden/tma_cases.npz

No tmtools exists to capture from: the expected numbers are those of the NumPy restatement of the contract (tests/tma_ref.py; DESIGN.md
section 7.9).  Per case (SPEC below; tma_ref.CASES) the float32 CA traces of the two structures, their masks and the restatement's
outputs ``<case>.<output>``, the alignment in original rows.  Next to every float output the yardstick ``<case>.<output>.yard``: the
restatement's own change between its two evaluation orders (pairs ascending, pairs descending - every sum over pairs runs the other way
round).  A case whose ``tm`` yardstick exceeds 1e-9, or whose ``alignment``, ``best_init`` or ``init_dp`` differ between the two orders,
took another path in the second order: the bound of the GPU tests would mean nothing for it, and this script refuses to record it (a
named case is not dropped for that: its seed changes).  ``far`` ends with fewer than three pairs within d8 (a status, NaN scores; the cut of the fast score widens there).  ``all8`` holds eight structures of 40 rows and the outputs of their 28 pairs.

The backbones: persistent random walks with 3.8 Angstrom steps tens of Angstrom from the origin, and CA excerpts of the three complexes
of tests/golden/sasa_cases.npz (coordinates only): the windows of ``tcr80`` and ``tcr130`` are TCR beta-chain variable domains of
different complexes, which share the immunoglobulin fold but not their rows.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import sasa_ref as sr  # noqa: E402
import tma_ref as ta  # noqa: E402
from make_goldens_tm import rotation, walk  # noqa: E402

YARD_LIMIT = 1e-9
# name: (kind, seed, parameters)
SPEC = {
    "n5": ("noise", 1, dict(n=5, rows_a=(0, 5), sigma=0.3)),
    "n5x9": ("noise", 2, dict(n=9, rows_a=(2, 7), sigma=0.3)),
    "n19x22": ("noise", 3, dict(n=22, rows_a=(1, 20), sigma=0.5)),
    "n64x65": ("noise", 4, dict(n=65, rows_a=(1, 65), sigma=1.0)),
    "n61x80": ("noise", 5, dict(n=80, rows_a=(12, 73), sigma=1.0)),
    "copy80": ("noise", 6, dict(n=80, rows_a=(0, 80), sigma=0.0)),
    "shift6": ("shift", 7, dict(n=80, shift=6)),
    "deletion": ("deletion", 8, dict(n=80, deleted=(30, 37))),
    "partial": ("noise", 9, dict(n=64, rows_a=(11, 56), sigma=0.5)),
    "hinge": ("hinge", 10, dict(n=60, at=25)),
    "unrelated": ("unrelated", 11, dict(n=50)),
    "masked": ("masked", 12, dict(n=90, source="1fyt:300")),
    "tcr80": ("excerpts", 13, dict(a="1fyt:575:80", b="5ksa:570:80")),
    "tcr130": ("excerpts", 14, dict(a="7t2d:566:130", b="5ksa:569:130")),
    "shift4_300": ("excerpts", 15, dict(a="5ksa:204:300", b="5ksa:200:300")),
    "n512": ("noise", 16, dict(n=512, rows_a=(0, 512), sigma=1.0)),
    "far": ("far", 17, dict(n=5, spacing=100.0)),
}


def excerpt(fix_sasa, spec):
    name, first, n = spec.split(":")
    prot, mask, _ = sr.case_prot(fix_sasa, name, 5)
    ca = prot[int(first):int(first) + int(n), 1].astype(np.float64)
    assert mask[int(first):int(first) + int(n), 1].all() and len(ca) == int(n)
    return ca


def traces(fix_sasa, kind, seed, par):
    """(ca_a [N_a,3], ca_b [N_b,3] float32, mask_a [N_a], mask_b [N_b] float32)."""
    rng = np.random.default_rng(seed)
    q, shift = rotation(rng), rng.normal(size=3) * 20.0
    move = lambda a: a @ q.T + shift  # noqa: E731
    mask_a = mask_b = None
    if kind == "noise":
        b = walk(rng, par["n"])
        a = b[par["rows_a"][0]:par["rows_a"][1]]
        a = move(a + par["sigma"] * rng.normal(size=a.shape) / np.sqrt(3.0))
    elif kind == "shift":
        w = walk(rng, par["n"] + par["shift"])
        a, b = move(w[par["shift"]:]), w[:par["n"]]
    elif kind == "deletion":  # a: all rows, b: the same rows with a stretch deleted
        a = walk(rng, par["n"])
        b = move(np.delete(a, np.arange(*par["deleted"]), axis=0))
    elif kind == "hinge":
        b = walk(rng, par["n"])
        a, k, q2 = b.copy(), par["at"], rotation(rng)
        a[k:] = (a[k:] - a[k]) @ q2.T + a[k]
        a = move(a)
    elif kind == "unrelated":
        a, b = walk(rng, par["n"]), walk(rng, par["n"])
    elif kind == "masked":  # rows dropped at both ends and in the middle, not the same rows in the two masks: 69 and 75 rows set
        b = excerpt(fix_sasa, par["source"] + f":{par['n']}")
        a = move(b + rng.normal(size=b.shape) / np.sqrt(3.0))
        mask_a, mask_b = np.ones(par["n"], dtype=np.float32), np.ones(par["n"], dtype=np.float32)
        mask_a[:3], mask_a[40:56], mask_a[-2:] = 0, 0, 0
        mask_b[:1], mask_b[44:52], mask_b[70], mask_b[-5:] = 0, 0, 0, 0
        assert mask_a.sum() == 69 and mask_b.sum() == 75
    elif kind == "excerpts":
        a, b = move(excerpt(fix_sasa, par["a"])), excerpt(fix_sasa, par["b"])
    elif kind == "far":  # a chain against points no chain connects: no three pairs within d8 of each other, FDIPT_TMA_NO_ALIGNMENT
        k = np.arange(par["n"], dtype=np.float64)
        a = move(walk(rng, par["n"]))
        b = np.stack([np.zeros(par["n"]), par["spacing"] * k, 0.3 * k * k], axis=1)
    else:
        raise ValueError(kind)
    mask_a = np.ones(len(a), dtype=np.float32) if mask_a is None else mask_a
    mask_b = np.ones(len(b), dtype=np.float32) if mask_b is None else mask_b
    return a.astype(np.float32), b.astype(np.float32), mask_a, mask_b


def both_orders(name, prot_a, prot_b, mask_a=None, mask_b=None):
    """The restatement in its two evaluation orders; (outputs of the ascending one, yard per float output)."""
    up = ta.align_structures(prot_a, prot_b, mask_a, mask_b)
    down = ta.align_structures(prot_a, prot_b, mask_a, mask_b, descending=True)
    yard = {k: np.abs(np.asarray(up[k], dtype=np.float64) - np.asarray(down[k], dtype=np.float64)) for k in ta.FLOAT_OUTPUTS}
    yard = {k: np.where(np.isnan(v), 0.0, v) for k, v in yard.items()}  # (NaN in both orders: a status)
    flips = [k for k in ("alignment", "best_init", "init_dp", "status") if not np.array_equal(up[k], down[k])]
    if not yard["tm"] <= YARD_LIMIT or flips:
        raise SystemExit(f"{name}: the two evaluation orders differ (tm by {float(yard['tm']):.3e}; {flips}): a path flip inside the restatement; "
                         "not recorded - change the case's seed")
    return up, yard


def record(fix, name, up, yard):
    for k in ("tm", "tm_a", "tm_b", "rmsd", "d0_a", "d0_b", "init_tm", "rotation", "translation"):
        fix[f"{name}.{k}"] = np.asarray(up[k], dtype=np.float64)
    for k in ta.EXACT_OUTPUTS:
        fix[f"{name}.{k}"] = np.asarray(up[k], dtype=np.int64)
    for k in ta.FLOAT_OUTPUTS:
        fix[f"{name}.{k}.yard"] = np.asarray(yard[k], dtype=np.float64)


def all8(fix_sasa):
    """Eight structures of 40 rows: windows of one excerpt 0 .. 5 rows apart with growing noise, each moved rigidly."""
    rng = np.random.default_rng(17)
    base = excerpt(fix_sasa, "1fyt:100:48")
    out = []
    for s, off in enumerate((0, 0, 2, 0, 5, 1, 3, 0)):
        w = base[off:off + 40] + rng.normal(size=(40, 3)) * (0.3 + 0.2 * s) / np.sqrt(3.0)
        out.append((w @ rotation(rng).T + rng.normal(size=3) * 10.0).astype(np.float32))
    return np.stack(out)


def main():
    fix_sasa = dict(np.load(os.path.join(HERE, "sasa_cases.npz")))
    fix = {"cases": np.array(list(SPEC))}
    assert tuple(SPEC) == ta.CASES
    for name, (kind, seed, par) in SPEC.items():
        ca_a, ca_b, mask_a, mask_b = traces(fix_sasa, kind, seed, par)
        fix.update({f"{name}.ca_a": ca_a, f"{name}.ca_b": ca_b, f"{name}.mask_a": mask_a, f"{name}.mask_b": mask_b})
        up, yard = both_orders(name, *ta.case_inputs(fix, name))
        record(fix, name, up, yard)
        if kind == "excerpts" and name.startswith("tcr"):  # I2 and I3 have something to work with
            for s in (up["sec_a"], up["sec_b"]):
                assert np.isin(s, (ta.SEC_H, ta.SEC_E)).any(), name
            assert up["init_tm"][1] > 0, name
        assert (up["status"] == ta.NO_ALIGNMENT) == (kind == "far"), name
        print(f"{name}: n1 = {int(mask_a.sum())}, n2 = {int(mask_b.sum())}, tm_a = {up['tm_a']:.6f}, tm_b = {up['tm_b']:.6f} (yard {float(yard['tm']):.1e}), "
              f"aligned {up['n_aligned']}, rmsd {up['rmsd']:.3f}, init_tm {np.round(up['init_tm'], 4)}, init_dp {up['init_dp']}, best {up['best_init']}, "
              f"status {up['status']}", flush=True)
    prot = all8(fix_sasa)
    fix["all8.ca"] = prot
    rows = []
    for i in range(8):
        for j in range(i + 1, 8):
            rows.append(both_orders(f"all8 ({i}, {j})", ta.five_atoms(prot[i]), ta.five_atoms(prot[j])))
    stacked = {k: np.stack([np.asarray(up[k]) for up, _ in rows]) for k in ("tm", "tm_a", "tm_b", "rmsd", "d0_a", "d0_b", "init_tm", "rotation", "translation")
               + ta.EXACT_OUTPUTS}
    record(fix, "all8", stacked, {k: np.stack([np.asarray(y[k]) for _, y in rows]) for k in ta.FLOAT_OUTPUTS})
    print(f"all8: tm {stacked['tm'].min():.4f} .. {stacked['tm'].max():.4f}, yard {fix['all8.tm.yard'].max():.1e}, init_dp {stacked['init_dp'].sum(1).min()} .. "
          f"{stacked['init_dp'].sum(1).max()}")
    np.savez_compressed(os.path.join(HERE, "tma_cases.npz"), **fix)
    print(f"{os.path.getsize(os.path.join(HERE, 'tma_cases.npz')) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
