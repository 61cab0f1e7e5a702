"""GPU tests (-m gpu) of accuracy through a row map: ``lddt.local_accuracy`` and ``gdt.gdt_scores`` with
``alignment=`` (fdipt_sample_lddt_mapped, fdipt_sample_gdt_mapped; csrc/lddt_mapped.hip, csrc/gdt_mapped.hip) against the un-mapped entries
on the gathered model - bit for bit -, the NumPy restatement (tests/mapped_ref.py), the reference's recorded numbers
(tests/golden/mapped_cases.npz) and closed forms; then the callers: ``compare.aligned_accuracy``, ``structure_search.hit_accuracy`` and
``run_sharded --novelty-accuracy``.  Every case is at most a few hundred rows and a handful of pairs."""
import functools
import gzip
import os

import numpy as np
import pytest
import torch

import gdt_ref as gr
import lddt_ref as lr
import mapped_cases as mc
import mapped_ref as mr
from conftest import GOLDEN, load_golden
from framedipt_amd import _lib, compare, gdt, lddt, row_map, structure_search as ss, tm_align

pytestmark = pytest.mark.gpu

LDDT_OUTPUTS = lr.EXACT_OUTPUTS + lr.FLOAT_OUTPUTS
GDT_OUTPUTS = gdt.OUTPUTS
EDGE_CASES = ("edge257", "edge40", "all65", "tiny5", "one")


@functools.lru_cache(maxsize=None)
def _case(name):
    return mc.build(name)


def _same(got, want, keys, rows=slice(None)):
    for k in keys:
        x, y = np.asarray(got[k])[rows], np.asarray(want[k])[rows]
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k


def _mapped(case, mode, coverage, same=False, **over):
    kw = dict(case, atoms=mode, coverage=coverage, same_residue=same, per_atom=True)
    kw.update(over)
    return lddt.local_accuracy(**kw)


def _gathered(case):
    """(G [1,N_b,A,3], present [1,N_b,A], covered [N_b]) of a case, on the host."""
    m, xa = case["alignment"], case["prot_a"][0]
    covered = mr.covered_rows(m, len(xa), case["res_mask"][0], case["res_mask_b"][0])
    g, present = mr.gathered(xa, m, covered)
    return g[None], present[None], covered


def _unmapped_on_g(case, mode, coverage, same=False):
    """Today's entry on the gathered model: absent atoms masked off (ignore), or at far points and marked present (penalise)."""
    g, present, _ = _gathered(case)
    if coverage == "penalise":
        g, present = mr.far_points(g[0], present[0])[None], np.ones_like(present)
    return lddt.local_accuracy(g, case["prot_b"], atoms=mode, res_mask=case["res_mask_b"], score_mask=case["score_mask"], atom_mask_a=present.astype(np.uint8),
                               same_residue=same, per_atom=True)


def _gdt_mapped(case, superpose, **over):
    kw = dict(prot_a=case["prot_a"], prot_b=case["prot_b"], mask_a=case["res_mask"], mask_b=case["res_mask_b"], alignment=case["alignment"], superpose=superpose)
    kw.update(over)
    return gdt.gdt_scores(**kw)


def _gdt_on_g(case, superpose, **over):
    g, _, covered = _gathered(case)
    return gdt.gdt_scores(g, case["prot_b"], mask_a=covered[None].astype(np.float32), mask_b=case["res_mask_b"], superpose=superpose, **over)


def _check_against_g(case, modes):
    n_cov, n_ref = int(_gathered(case)[2].sum()), int(np.count_nonzero(case["res_mask_b"]))
    for mode in modes:
        for same in ((False,) if mode == "ca" else (False, True)):
            got, want = _mapped(case, mode, "ignore", same), _unmapped_on_g(case, mode, "ignore", same)
            _same(got, want, LDDT_OUTPUTS)
            pen, far = _mapped(case, mode, "penalise", same), _unmapped_on_g(case, mode, "penalise", same)
            _same(pen, far, ("lddt", "res_lddt", "n_scored", "n_passed", "atom_lddt"))
            _same(pen, got, lr.FLOAT_OUTPUTS)  # coverage has no meaning for dRMSD and FAPE
            assert pen["status"][0] & ~_lib.LDDT_NO_PARTNER == got["status"][0] & ~_lib.LDDT_NO_PARTNER
            for res, coverage in ((got, "ignore"), (pen, "penalise")):
                assert res["n_covered"].tolist() == [n_cov] and res["n_reference"].tolist() == [n_ref] and res["coverage"][0] == n_cov / n_ref
                rest = mr.local_accuracy(case["prot_a"][0], case["prot_b"][0], case["alignment"], mode, coverage, case["res_mask"][0], case["res_mask_b"][0],
                                         case["score_mask"][0], same_residue=same)
                lr.check_exact({k: np.asarray(rest[k])[None] for k in lr.EXACT_OUTPUTS}, res)
                assert rest["n_covered"] == n_cov and rest["n_reference"] == n_ref
    for superpose in gr.MODES:
        got, want = _gdt_mapped(case, superpose), _gdt_on_g(case, superpose)
        _same(got, want, GDT_OUTPUTS)
        assert got["n_covered"].tolist() == got["n_scored"].tolist() == [n_cov] and got["n_reference"].tolist() == [n_ref]
        ca_a, ca_b = case["prot_a"][0][:, 1], case["prot_b"][0][:, 1]
        rest = mr.gdt(ca_a, ca_b, case["alignment"], superpose, case["res_mask"][0], case["res_mask_b"][0])
        for k in ("counts", "n_scored", "best_item", "best_pass", "passes", "res_within", "status"):
            assert np.array_equal(np.asarray(got[k])[0], np.asarray(rest[k])), (superpose, k)


def test_identity_map_is_the_unmapped_entry():
    """N_a = N_b = 70 through the identity: every output of both entries equals the un-mapped entry on the same arrays bit for bit, in
    all three atom sets and under both coverage switches (every row is covered: they agree)."""
    case = _case("identity70")
    assert np.array_equal(case["alignment"], row_map.identity(70))
    for mode in lr.MODES:
        want = lddt.local_accuracy(case["prot_a"], case["prot_b"], atoms=mode, per_atom=True)
        for coverage in ("ignore", "penalise"):
            got = _mapped(case, mode, coverage)
            _same(got, want, LDDT_OUTPUTS)
            assert got["n_covered"].tolist() == got["n_reference"].tolist() == [70] and got["coverage"].tolist() == [1.0]
    for superpose in gr.MODES:
        got = _gdt_mapped(case, superpose)
        _same(got, gdt.gdt_scores(case["prot_a"], case["prot_b"], superpose=superpose), GDT_OUTPUTS)
        assert got["n_covered"].tolist() == got["n_reference"].tolist() == [70]


def test_permutation_equals_the_unmapped_entry_on_permuted_arrays():
    """N = 66, a non-monotone map of all rows: the un-mapped entries on the model permuted on the host."""
    case = _case("perm66")
    m = case["alignment"]
    assert sorted(m.tolist()) == list(range(66)) and (np.diff(m) < 0).any()
    permuted = np.ascontiguousarray(case["prot_a"][:, m])
    for mode in ("ca", "backbone"):
        _same(_mapped(case, mode, "ignore"), lddt.local_accuracy(permuted, case["prot_b"], atoms=mode, per_atom=True), LDDT_OUTPUTS)
    for superpose in gr.MODES:
        _same(_gdt_mapped(case, superpose), gdt.gdt_scores(permuted, case["prot_b"], superpose=superpose), GDT_OUTPUTS)


@pytest.mark.parametrize("name", EDGE_CASES)
def test_tile_and_block_edges(name):
    """(N_a, N_b) = (90, 257) with covered reference rows 255 and 256, (257, 40), the ALL set at (50, 65) with atoms missing on both
    sides, (3, 5) and (1, 1): every output of the un-mapped entry on the gathered model under ignore; the lDDT integers and scores of
    the far-point construction under penalise; the restatement's integers; GDT in its three modes."""
    case = _case(name)
    if name == "edge257":
        covered = _gathered(case)[2]
        assert covered[255] and covered[256] and not case["res_mask_b"].all()
    _check_against_g(case, mc.modes_of(case))


@pytest.mark.parametrize("name", list(mc.GOLDEN_CASES))
def test_the_references_recorded_numbers(name):
    """lDDT under penalise is the reference's ``lddt`` / ``lddt_ca`` on the gathered model under the true mask alone, bit for bit per
    atom and per pair; the GDT counts are the integers behind the reference's scores (none, global)."""
    fix, mode = load_golden("mapped_cases.npz"), mc.GOLDEN_CASES[name]
    case = mc.golden_inputs(fix, name)
    got = _mapped(case, mode, "penalise", same=mode != "ca")
    exists_b = case["res_mask_b"][0] != 0
    assert np.array_equal(got["atom_lddt"][0][exists_b], fix[f"{name}.ref_atom"][exists_b]) and got["lddt"][0] == float(fix[f"{name}.ref_lddt"])
    for superpose in ("none", "global"):
        out = _gdt_mapped(case, superpose)
        assert np.array_equal(out["counts"][0], fix[f"{name}.{superpose}.ref_counts"])
        assert abs(out["gdt_ts"][0] - float(fix[f"{name}.{superpose}.ref_ts"])) <= 1e-6 and abs(out["gdt_ha"][0] - float(fix[f"{name}.{superpose}.ref_ha"])) <= 1e-6


def test_closed_form_of_the_straight_trace():
    """60 rows on a line, 3.8 Angstrom apart, the model without rows 20 .. 29 and rigidly moved.  Three neighbours on each side lie
    within 15 Angstrom (11.4 < 15 < 15.2): a run of L rows holds 6 L - 12 ordered pairs.  Ignore: the runs of 20 and 30 covered rows,
    108 + 168 = 276 pairs, all passed, lddt = 1.0 exactly.  Penalise: the whole reference, 6 * 60 - 12 = 348 scored, the same 276
    passed at every threshold.  n_covered = 50; GDT-TS over the reference's rows = 50 / 60."""
    model, ref, m = mc.straight_trace()
    ignore = lddt.local_accuracy(model, ref, alignment=m, coverage="ignore")
    assert ignore["lddt"][0] == 1.0 and ignore["n_scored"].sum() == 276 and (ignore["n_passed"].sum(1) == 276).all() and ignore["status"][0] == _lib.LDDT_NO_PARTNER | _lib.LDDT_NO_FRAME
    pen = lddt.local_accuracy(model, ref, alignment=m, coverage="penalise")
    assert pen["n_scored"].sum() == 348 and (pen["n_passed"].sum(1) == 276).all() and pen["n_covered"][0] == 50 and pen["n_reference"][0] == 60
    assert pen["lddt"][0] == float(lr.score(348, np.full(4, 276))) and pen["status"][0] == _lib.LDDT_NO_FRAME
    assert pen["n_scored"][0, 24] == 6 and pen["res_lddt"][0, 24] == float(lr.score(6, np.zeros(4))) and not pen["n_passed"][0, 20:30].any()
    out = gdt.gdt_scores(model, ref, alignment=m, norm_length="reference", superpose="search")
    assert (out["counts"] == 50).all() and out["gdt_ts"][0] == 50 / 60 and out["gdt_ha"][0] == 50 / 60 and out["n_covered"][0] == 50


def test_nothing_covered():
    """All -1: ignore has no scored pair (NO_PARTNER, the reference's eps / eps), penalise scores eps / (eps + c), GDT is TOO_SHORT; no
    NaN reaches an lDDT output."""
    case = dict(_case("edge40"), alignment=np.full(40, -1, dtype=np.int32))
    ignore, pen = _mapped(case, "backbone", "ignore"), _mapped(case, "backbone", "penalise")
    assert ignore["status"][0] & _lib.LDDT_NO_PARTNER and not ignore["n_scored"].any() and ignore["n_covered"][0] == 0
    c = int(pen["n_scored"].sum())
    assert c > 0 and not pen["n_passed"].any() and pen["lddt"][0] == float(lr.score(c, np.zeros(4))) and not pen["status"][0] & _lib.LDDT_NO_PARTNER
    rows = np.flatnonzero(pen["n_scored"][0])
    assert np.array_equal(pen["res_lddt"][0, rows], lr.score(pen["n_scored"][0, rows], np.zeros((len(rows), 4))))
    for res in (ignore, pen):
        assert all(np.isfinite(res[k]).all() for k in ("lddt", "res_lddt", "atom_lddt", "drmsd", "fape", "res_fape", "region_fape"))
    out = _gdt_mapped(case, "search")
    assert out["status"][0] == _lib.GDT_TOO_SHORT and np.isnan(out["gdt_ts"][0]) and out["n_covered"][0] == 0 and out["n_reference"][0] == 39


def _batch_with_bad_maps(dev):
    """Four pairs of one (model, reference): a good map, one with an entry out of range, one with a duplicate, a good map again."""
    case = _case("edge40")
    good = case["alignment"]
    out_of_range, twice = good.copy(), good.copy()
    out_of_range[np.flatnonzero(good < 0)[0]] = 257
    twice[np.flatnonzero(good < 0)[1]] = good[good >= 0][0]
    maps = torch.from_numpy(np.stack([good, out_of_range, twice, good])).to(dev)
    return case, maps, np.zeros((4, 2), dtype=np.int32)


def test_bad_maps_are_flagged_and_touch_no_other_pair():
    case, maps, pairs = _batch_with_bad_maps("cuda")
    alone = _mapped(case, "backbone", "penalise")
    got = _mapped(dict(case, alignment=maps), "backbone", "penalise", pairs=pairs)
    assert got["status"][1] == _lib.MAP_OUT_OF_RANGE and got["status"][2] == _lib.MAP_DUPLICATE
    for p in (1, 2):
        assert not any(np.asarray(got[k])[p].any() for k in LDDT_OUTPUTS if k != "status") and got["n_covered"][p] == 0 and got["n_reference"][p] == 0
    for p in (0, 3):
        _same({k: got[k][p:p + 1] for k in LDDT_OUTPUTS + ("n_covered", "n_reference")}, alone, LDDT_OUTPUTS + ("n_covered", "n_reference"))
    g_alone = _gdt_mapped(case, "search")
    g = _gdt_mapped(dict(case, alignment=maps), "search", pairs=pairs)
    assert g["status"].tolist() == [0, _lib.MAP_OUT_OF_RANGE, _lib.MAP_DUPLICATE, 0]
    for p in (1, 2):
        assert np.isnan(g["gdt_ts"][p]) and np.isnan(g["gdt_ha"][p]) and not g["counts"][p].any() and not g["res_within"][p].any() and g["n_covered"][p] == 0
    for p in (0, 3):
        _same({k: g[k][p:p + 1] for k in GDT_OUTPUTS}, g_alone, GDT_OUTPUTS)
    # both bits in one map; a NumPy map is refused on the host
    both = maps[1].clone()
    both[np.flatnonzero(case["alignment"] < 0)[1]] = int(case["alignment"][case["alignment"] >= 0][0])
    assert _mapped(dict(case, alignment=both), "ca", "ignore")["status"][0] == _lib.MAP_OUT_OF_RANGE | _lib.MAP_DUPLICATE
    with pytest.raises(ValueError, match="outside"):
        _mapped(dict(case, alignment=maps[1].cpu().numpy()), "ca", "ignore")


def test_batch_mates_appended_rows_and_input_kinds_change_no_bit():
    """A pair's bits do not depend on its batch mates, on rows appended behind either structure (masked off / not mapped to), or on
    whether the inputs are device tensors or NumPy arrays."""
    a, b = _case("edge40"), _case("tiny5")
    alone = _mapped(a, "backbone", "penalise")
    g_alone = _gdt_mapped(a, "search")
    rng = np.random.default_rng(3)
    n_a, n_b = 257 + 7, 40 + 9
    pa, pb = (rng.normal(size=(2, n_a, 5, 3)) * 30).astype(np.float32), (rng.normal(size=(2, n_b, 5, 3)) * 30).astype(np.float32)
    pa[0, :257], pb[0, :40], pa[1, :3], pb[1, :5] = a["prot_a"][0], a["prot_b"][0], b["prot_a"][0], b["prot_b"][0]
    maps = np.full((2, n_b), -1, dtype=np.int32)
    maps[0, :40], maps[1, :5] = a["alignment"], b["alignment"]
    rm, rmb, sm = np.zeros((2, n_a), np.float32), np.zeros((2, n_b), np.float32), np.ones((2, n_b), np.float32)
    rm[0, :257], rm[1, :3], rmb[0, :40], rmb[1, :5], sm[0, :40], sm[1, :5] = a["res_mask"][0], b["res_mask"][0], a["res_mask_b"][0], b["res_mask_b"][0], a["score_mask"][0], b["score_mask"][0]
    joint = dict(prot_a=pa, prot_b=pb, alignment=maps, res_mask=rm, res_mask_b=rmb, score_mask=sm)
    got = _mapped(joint, "backbone", "penalise")
    for k in LDDT_OUTPUTS + ("n_covered", "n_reference"):
        x, y = np.asarray(got[k])[0], np.asarray(alone[k])[0]
        if x.ndim:
            assert not x[40:].any(), k
            x = x[:40]
        assert np.array_equal(x, y), k
    g = gdt.gdt_scores(pa, pb, mask_a=rm, mask_b=rmb, alignment=maps, superpose="search")
    for k in GDT_OUTPUTS:
        x, y = np.asarray(g[k])[0], np.asarray(g_alone[k])[0]
        assert np.array_equal(x[:40] if k == "res_within" else x, y, equal_nan=True), k
    on_device = {k: torch.from_numpy(v).cuda() for k, v in joint.items()}
    _same(_mapped(on_device, "backbone", "penalise"), got, LDDT_OUTPUTS + ("n_covered", "n_reference"))
    _same(gdt.gdt_scores(on_device["prot_a"], on_device["prot_b"], mask_a=on_device["res_mask"], mask_b=on_device["res_mask_b"], alignment=on_device["alignment"],
                         superpose="search"), g, GDT_OUTPUTS + ("n_covered", "n_reference"))


def test_aligned_accuracy_on_the_shifted_window():
    """The 74 / 80 closed form of the alignment search (tma_cases ``shift6``: the model is rows 6 .. 85 of a walk, the reference rows
    0 .. 79, rigidly apart): ``tm`` is ``tm_align``'s, the 74 common rows are found, lDDT under ignore is exactly 1 on them and every
    GDT count is 74."""
    fix = load_golden("tma_cases.npz")
    a, b = gr.five_atoms(fix["shift6.ca_a"])[None], gr.five_atoms(fix["shift6.ca_b"])[None]
    found = tm_align.tm_align(a, b)
    got = compare.aligned_accuracy(a, b, coverage="ignore")
    assert np.array_equal(got["tm"], found["tm"]) and np.array_equal(got["alignment"], found["alignment"]) and got["n_aligned"][0] == 74
    assert got["lddt"][0] == 1.0 and got["n_covered"][0] == 74 and got["n_reference"][0] == 80 and (got["counts"][0] == 74).all()
    assert got["gdt_ts"][0] == got["gdt_ha"][0] == 74 / 80 and got["lddt_status"][0] & _lib.LDDT_NO_PARTNER
    assert not got["n_scored"][0, :6].any() and (got["res_lddt"][0, :6] == 1.0).all()  # (rows without a partner: c = 0, the reference's eps / eps)
    assert np.array_equal(got["n_passed"][0, 6:], np.repeat(got["n_scored"][0, 6:, None], 4, axis=1)) and (got["n_scored"][0, 6:] > 0).all()
    assert np.array_equal(got["res_lddt"][0, 6:], lr.score(got["n_scored"][0, 6:], got["n_passed"][0, 6:]))
    pen = compare.aligned_accuracy(a, b)
    assert pen["lddt"][0] < 1.0 and np.array_equal(pen["n_passed"], got["n_passed"]) and (pen["n_scored"] >= got["n_scored"]).all()
    flat = compare.aligned_metrics(pen, 0)
    assert flat["tm_score"] == float(found["tm_b"][0]) and flat["lddt_ca"] == float(pen["lddt"][0]) and flat["gdt_ts"] == 74 / 80 and flat["n_covered"] == 74


def test_hit_accuracy_is_local_accuracy_through_each_hits_alignment(tmp_path):
    """Two queries against the chains of the three recorded complexes, two hits each: ``hit_accuracy`` equals one mapped call per
    (query, hit) on the hit's own trace."""
    for name in ("1fyt", "5ksa", "7t2d"):
        with gzip.open(os.path.join(GOLDEN, "search_structures", f"{name}-assembly1.cif.gz"), "rb") as f:
            (tmp_path / f"{name}-assembly1.cif").write_bytes(f.read())
    db = ss.StructureSet.from_directory(tmp_path, "*.cif")
    kept = [e for e in range(len(db)) if db.lengths[e] > 0]  # (one chain of the three complexes has no CA atom)
    db = ss.StructureSet.from_arrays([db.entry(e) for e in kept], [db.names[e] for e in kept])
    prot = np.stack([gr.five_atoms(db.entry(0)[40:112]), gr.five_atoms(db.entry(8)[20:92])]).astype(np.float32)
    mask = np.ones((2, 72), dtype=np.float32)
    mask[1, 30:36] = 0
    res = ss.search(prot, db, mask=mask, top_k=2)
    acc = ss.hit_accuracy(res, prot, db, mask=mask)
    assert (res["hit"] >= 0).all() and res["hit"][0, 0] == 0 and res["hit"][1, 0] == 8
    for q in range(2):
        for k in range(2):
            trace = db.entry(int(res["hit"][q, k]))
            m = res["alignment"][q, k, :len(trace)].astype(np.int32)
            one = lddt.local_accuracy(prot[q:q + 1, :, 1], trace[None], res_mask=mask[q:q + 1], alignment=m, coverage="penalise")
            assert acc["lddt"][q, k] == one["lddt"][0] and np.array_equal(acc["res_lddt"][q, k, :len(trace)], one["res_lddt"][0]) and not acc["res_lddt"][q, k, len(trace):].any()
            assert acc["n_covered"][q, k] == one["n_covered"][0] == np.count_nonzero(m >= 0) > 0 and acc["n_reference"][q, k] == len(trace)
            two = gdt.gdt_scores(prot[q:q + 1, :, 1], trace[None], mask_a=mask[q:q + 1], alignment=m, norm_length="reference")
            assert acc["gdt_ts"][q, k] == two["gdt_ts"][0] and acc["gdt_ha"][q, k] == two["gdt_ha"][0]
    assert ss.hit_accuracy_metrics(acc, 1, 0)["lddt_ca"] == float(acc["lddt"][1, 0]) and acc["coverage"][0, 0] == acc["n_covered"][0, 0] / len(db.entry(0))


def test_run_sharded_novelty_accuracy_adds_files_and_changes_none(tmp_path):
    """``run_sharded --novelty SET.npz --novelty-accuracy`` on the smallest de novo configuration of the novelty test: the two new files
    exist, and ``novelty.json`` / ``novelty.csv`` are byte-equal to those of a run without the flag."""
    import json
    import subprocess
    import sys

    import search_ref as sr
    from conftest import ROOT
    _, _, entries, _ = sr.case_a()
    ss.StructureSet.from_arrays([entries[k] for k in (9, 10, 11, 12, sr.SELF)], names=["a", "b", "c", "d", "e"]).save(tmp_path / "set.npz")
    written = {}
    for flag in ((), ("--novelty-accuracy",)):
        out_dir = tmp_path / ("with" if flag else "without")
        cmd = [sys.executable, "-m", "framedipt_amd.run_sharded", "--out-dir", str(out_dir), "--num-t", "2", "--max-batch", "4", "--keep", "last", "--min-length", "48",
               "--max-length", "48", "--length-step", "5", "--samples-per-length", "2", "--precision", "fp32", "--novelty", str(tmp_path / "set.npz"), *flag]
        r = subprocess.run(cmd, env=dict(os.environ, FDIPT_SHARED_GPU="allow"), cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        written[bool(flag)] = {name: (out_dir / name).read_bytes() for name in ("novelty.json", "novelty.csv")}
        assert (out_dir / "novelty_accuracy.json").exists() == (out_dir / "novelty_accuracy.csv").exists() == bool(flag)
    assert written[True] == written[False]
    with open(tmp_path / "with" / "novelty_accuracy.json") as f:
        summary = json.load(f)
    assert [(h["length"], h["sample"], h["rank"]) for h in summary["hits"]] == [(48, 0, 0), (48, 1, 0)] and summary["coverage"] == "penalise"
    lines = (tmp_path / "with" / "novelty_accuracy.csv").read_text().split()
    assert lines[0] == "length,sample,rank,hit,lddt_ca,gdt_ts,gdt_ha,n_covered,n_reference" and len(lines) == 3
    for h in summary["hits"]:
        assert 0.0 <= h["lddt_ca"] <= 1.0 and 0 < h["n_covered"] <= h["n_reference"] and h["hit"] in "abcde"
