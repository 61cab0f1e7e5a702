"""Fixture of the secondary-structure tests, read from the reference's three test complexes (this container only):

    python tests/golden/make_goldens_dssp.py      # -> tests/golden/dssp_cases.npz

The complexes are ``tests/data/inference_data/structures/cifs/{1fyt,5ksa,7t2d}-assembly1.cif`` of the reference.  Of each the file
keeps data only: N, CA, C, O of the ATOM rows that have all four (float32, as ``framedipt_amd/data/mmcif.py`` reads them), a chain
index per author chain, the proline flag, and the deposited three-class label per row: ``_struct_conf`` helix records -> H,
``_struct_sheet_range`` ranges -> E, helix wins, everything else C.  The cif text itself is not kept.

Excerpts of 1fyt give launches of a few dozen rows: ``anti`` (a two-strand antiparallel piece of at most 40 rows whose strands stay
bridged when cut out), ``bulge`` (two antiparallel ladders the bulge pass joins: its classes change when the pass is switched off),
``parallel`` (the two windows of a parallel ladder, if a complex holds one), ``helix`` (a helix with its flanks), ``boundary`` (the
rows on both sides of a chain boundary).  An excerpt is kept only if no class changes under the rigid motion below.

Per case the yardsticks of the restatement (tests/dssp_ref.py), in float64:
* ``<case>.energy_yard``: the largest change of any evaluated hydrogen-bond energy, before rounding, under one rigid motion of all atoms
  (``motion.rot``, ``motion.shift`` = 100 Angstrom);
* ``<case>.class_changes``: the number of rows whose class changes under that motion (0 for every excerpt, asserted);
* ``<case>.half_margin``: the smallest distance of 1000 E from a half-integer over the evaluated pairs, asserted above 1e-6: the
  rounding to three decimals cannot split two float64 evaluations that differ in their last bits.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import refharness as rh  # noqa: E402

import dssp_ref as dr  # noqa: E402
from framedipt_amd.data import features as F  # noqa: E402
from framedipt_amd.data import mmcif  # noqa: E402

CIFS = rh.REF + "/tests/data/inference_data/structures/cifs/{}-assembly1.cif"
PRO = 14
MARGIN = 1e-6


def read_loop(path, prefix):
    """The rows of the loop whose tags start with ``prefix`` as dicts of strings."""
    rows, cols, state = [], [], 0  # 0 outside, 1 a loop's tags, 2 the wanted loop's rows
    with open(path, encoding="utf-8") as f:
        for line in f:
            s = line.strip()
            if s == "loop_":
                state, cols = 1, []
            elif not s or s.startswith("#"):
                state = 0
            elif s.startswith("_"):
                if state == 1 and s.startswith(prefix):
                    cols.append(s[len(prefix):].split()[0])
                elif state:
                    state = 1 if not cols else 0
            elif state and cols:
                state = 2
                t = mmcif._tokens(s)
                if len(t) == len(cols):
                    rows.append(dict(zip(cols, t)))
    return rows


def read_complex(name):
    """-> bb [n,4,3] float32, chain_idx [n] int32, is_proline [n] uint8, label [n] uint8 (dssp_ref class codes)."""
    path = CIFS.format(name)
    atoms, _ = mmcif.read_atom_site(path)
    atoms = [r for r in atoms if r["group_PDB"] == "ATOM"]
    chains = mmcif.chain_features(atoms)
    keys = {}  # chain -> [(author sequence number, insertion code)] in the order chain_features keeps
    for r in atoms:
        icode = r.get("pdbx_PDB_ins_code", "?")
        key = (int(r["auth_seq_id"]), " " if icode in ("?", ".") else icode)
        seen = keys.setdefault(r["auth_asym_id"].upper(), {})
        seen.setdefault(key, None)
    label = {c: np.zeros(len(keys[c]), dtype=np.uint8) for c in chains}

    def mark(rows, code):
        for r in rows:
            c = r["beg_auth_asym_id"].upper()
            assert c == r["end_auth_asym_id"].upper() and c in chains, r
            order = list(keys[c])
            icode = lambda v: " " if v in ("?", ".") else v  # noqa: E731
            lo = order.index((int(r["beg_auth_seq_id"]), icode(r.get("pdbx_beg_PDB_ins_code", "?"))))
            hi = order.index((int(r["end_auth_seq_id"]), icode(r.get("pdbx_end_PDB_ins_code", "?"))))
            assert lo <= hi, r
            label[c][lo:hi + 1] = code

    mark(read_loop(path, "_struct_sheet_range."), dr.STRAND)
    mark([r for r in read_loop(path, "_struct_conf.") if r["conf_type_id"].startswith("HELX")], dr.HELIX)  # (helix wins)
    bb, chain_idx, pro, lab = [], [], [], []
    for k, (c, d) in enumerate(chains.items()):
        assert len(d["aatype"]) == len(keys[c])
        whole = d["atom_mask"][:, [0, 1, 2, 4]].all(axis=1)
        bb.append(d["atom_positions"][whole][:, [0, 1, 2, 4]].astype(np.float32))
        chain_idx.append(np.full(int(whole.sum()), k, dtype=np.int32))
        pro.append((d["aatype"][whole] == PRO).astype(np.uint8))
        lab.append(label[c][whole])
    assert F.RESTYPE_3_TO_INDEX["PRO"] == PRO
    return np.concatenate(bb), np.concatenate(chain_idx), np.concatenate(pro), np.concatenate(lab)


def yardsticks(case, rot, shift):
    base = dr.dssp(case["bb"], None, case["chain_idx"], case["is_proline"])
    moved = dr.dssp(case["bb"].astype(np.float64) @ rot.T + shift, None, case["chain_idx"], case["is_proline"])
    both = base["valid"] & moved["valid"]
    yard = float(np.max(np.abs(base["raw_energy"][both] - moved["raw_energy"][both]), initial=0.0))
    return base, yard, int((base["ss"] != moved["ss"]).sum())


def cut(case, rows):
    return {k: np.ascontiguousarray(v[rows]) for k, v in case.items() if k != "label"}


def windows(ladder, n, flank=2):
    """The rows of a ladder's two strands with ``flank`` rows on every side, ascending."""
    _, ib, ie, jb, je = ladder
    rows = set(range(max(ib - flank, 0), min(ie + flank, n - 1) + 1)) | set(range(max(jb - flank, 0), min(je + flank, n - 1) + 1))
    return np.array(sorted(rows))


def excerpts(case, rot, shift):
    """Named excerpts of one complex; each keeps its classes under the motion."""
    n = len(case["bb"])
    with_pass = dr.dssp(case["bb"], None, case["chain_idx"], case["is_proline"])
    without = dr.dssp(case["bb"], None, case["chain_idx"], case["is_proline"], bulges=False)
    chain = case["chain_idx"]
    out = {}

    def stable(ex):
        return yardsticks(ex, rot, shift)[2] == 0

    def one_chain(ladder):
        return chain[ladder[1]] == chain[ladder[4]]

    for lad in with_pass["ladders"]:  # a hairpin-like piece as one contiguous window
        if "anti" not in out and lad[0] == dr.ANTIPARALLEL and one_chain(lad) and lad[2] - lad[1] >= 3 and lad[4] - lad[1] + 5 <= 40:
            ex = cut(case, np.arange(max(lad[1] - 2, 0), min(lad[4] + 2, n - 1) + 1))
            got = dr.dssp(ex["bb"], None, ex["chain_idx"], ex["is_proline"])
            if got["n_bridges"] >= 4 and stable(ex):
                out["anti"] = ex
    for lad in with_pass["ladders"]:
        if lad in without["ladders"]:
            continue  # (a merged ladder is none of the unmerged ones)
        rows = windows(lad, n)
        if "bulge" in out or len(rows) > 60:
            continue
        ex = cut(case, rows)
        a = dr.dssp(ex["bb"], None, ex["chain_idx"], ex["is_proline"])
        b = dr.dssp(ex["bb"], None, ex["chain_idx"], ex["is_proline"], bulges=False)
        if (a["ss"] != b["ss"]).any() and stable(ex):
            out["bulge"] = ex
    for lad in with_pass["ladders"]:
        if "parallel" not in out and lad[0] == dr.PARALLEL and lad[2] - lad[1] >= 1:
            ex = cut(case, windows(lad, n, flank=3))
            got = dr.dssp(ex["bb"], None, ex["chain_idx"], ex["is_proline"])
            if len(ex["bb"]) <= 60 and any(l[0] == dr.PARALLEL for l in got["ladders"]) and stable(ex):
                out["parallel"] = ex
    cls = with_pass["ss"]
    for start in range(4, n - 16):
        if "helix" not in out and cls[start - 1] != dr.HELIX and (cls[start:start + 8] == dr.HELIX).all():
            stop = start + int(np.argmax(np.append(cls[start:] != dr.HELIX, True)))
            ex = cut(case, np.arange(start - 4, min(stop + 4, n)))
            if len(ex["bb"]) <= 40 and len(set(ex["chain_idx"])) == 1 and stable(ex):
                out["helix"] = ex
    edge = int(np.flatnonzero(np.diff(chain))[0]) + 1
    ex = cut(case, np.arange(edge - 14, edge + 14))
    if stable(ex):
        out["boundary"] = ex
    return out


def agreement(ss, label):
    ss, label = np.asarray(ss), np.asarray(label)
    confusions = int(((ss == dr.HELIX) & (label == dr.STRAND)).sum() + ((ss == dr.STRAND) & (label == dr.HELIX)).sum())
    return float((ss == label).mean()), confusions


def main():
    q, _ = np.linalg.qr(np.random.default_rng(77).normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    shift = 100.0 * np.array([2.0, -1.0, 2.0]) / 3.0
    fix = {"motion.rot": q, "motion.shift": shift}
    cases = {}
    for name in dr.COMPLEXES:
        bb, chain_idx, pro, label = read_complex(name)
        cases[name] = {"bb": bb, "chain_idx": chain_idx, "is_proline": pro, "label": label}
    for name, ex in excerpts(cases["1fyt"], q, shift).items():
        cases[name] = ex
    if "parallel" not in cases:
        for other in dr.COMPLEXES[1:]:
            found = excerpts(cases[other], q, shift)
            if "parallel" in found:
                cases["parallel"] = found["parallel"]
                break
    for name, case in cases.items():
        base, yard, changes = yardsticks(case, q, shift)
        assert base["half_margin"] > MARGIN, (name, base["half_margin"])
        assert name in dr.COMPLEXES or changes == 0, (name, changes)
        for k, v in case.items():
            fix[f"{name}.{k}"] = v
        fix[f"{name}.energy_yard"], fix[f"{name}.class_changes"] = np.float64(yard), np.int64(changes)
        fix[f"{name}.half_margin"] = np.float64(base["half_margin"])
        line = f"{name}: n = {base['n_rows']}, chains {len(set(case['chain_idx'].tolist()))}, {dr.ss_string(base['ss']) if base['n_rows'] <= 60 else ''} " \
               f"hbonds {base['n_hbonds']}, bridges {base['n_bridges']}, ladders {base['n_ladders']}, energy yardstick {yard:.1e}, " \
               f"class changes under the motion {changes}, half-integer margin {base['half_margin']:.1e}"
        if "label" in case:
            agree, confusions = agreement(base["ss"], case["label"])
            no_pass = dr.dssp(case["bb"], None, case["chain_idx"], case["is_proline"], bulges=False)
            line += (f", agreement with the deposited labels {agree:.3f} ({agreement(no_pass['ss'], case['label'])[0]:.3f} without the bulge pass), "
                     f"H<->E confusions {confusions}, helix {base['helix_percent']:.3f} / deposited {(case['label'] == dr.HELIX).mean():.3f}, "
                     f"strand {base['strand_percent']:.3f} / deposited {(case['label'] == dr.STRAND).mean():.3f}")
        print(line, flush=True)
    fix["cases"] = np.array(list(cases))
    path = os.path.join(HERE, "dssp_cases.npz")
    np.savez_compressed(path, **fix)
    print(f"{os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
