"""GPU tests (-m gpu) of GDT-TS / GDT-HA (framedipt_amd/gdt.py -> fdipt_sample_gdt, csrc/gdt.hip) against the NumPy restatement of the
contract (tests/gdt_ref.py) as recorded in tests/golden/gdt_cases.npz.  The generator asserted that every
distance the search compares is at least 1e-9 Angstrom from its threshold, so every integer output - counts, winners, passes, the
per-row bits - is asserted EQUAL, and the two scores, formed from the integers by one division, bit for bit."""
import functools

import numpy as np
import pytest
import torch

import gdt_ref as gr
from conftest import load_golden
from framedipt_amd import _lib, gdt

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("gdt_cases.npz")


@functools.lru_cache(maxsize=None)
def _single(name, mode):
    """One recorded case as a launch of its own (NumPy inputs, uploaded)."""
    a, b, ma, mb, norm = gr.case_inputs(_fix(), name)
    return gdt.gdt_scores(a[None], b[None], ma[None], mb[None], norm_length=norm, superpose=mode)


def _same_pair(got, p, want, q, rows=None):
    for k in gdt.OUTPUTS:
        u, v = np.asarray(got[k][p]), np.asarray(want[k][q])
        if k == "res_within" and rows is not None:  # (another padding: the case's own rows, nothing behind them)
            assert not u[rows:].any() and not v[rows:].any()
            u, v = u[:rows], v[:rows]
        assert np.array_equal(u, v, equal_nan=True), k


@pytest.mark.parametrize("mode", gr.MODES)
@pytest.mark.parametrize("name", gr.CASES)
def test_case_equals_the_restatement(name, mode):
    """n = 1, 2 (none only), 3, 4, 5 (a one-level ladder), 9, 37, 64 / 65 (the wave edge of the compaction), 130 (2 655 items: many times
    the threads), masks with a normalisation length, a planted rigid part, a hinge, a distance that equals a cutoff, an unrelated pair
    (the cut widens), N = 1024 (the LDS limit, 20 810 items) and a coordinate that is not finite."""
    fix, got = _fix(), _single(name, mode)
    for k in gr.INT_OUTPUTS:
        assert np.array_equal(got[k][0], fix[f"{name}.{mode}.{k}"]), (k, got[k][0], fix[f"{name}.{mode}.{k}"])
    for k in ("gdt_ts", "gdt_ha"):
        assert np.array_equal(got[k][0], fix[f"{name}.{mode}.{k}"], equal_nan=True), k
    assert got["res_within"].dtype == np.int32 and got["counts"].dtype == np.int64
    if got["status"][0]:
        assert np.array_equal(got["rotation"][0], np.tile(np.eye(3), (5, 1, 1))) and not got["translation"].any()
        return
    a, b, ma, mb, _ = gr.case_inputs(fix, name)
    x, y = gr.compact(a, b, ma, mb)
    for j in range(5):
        rot, shift = got["rotation"][0, j], got["translation"][0, j]
        assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(rot) - 1.0) <= 1e-12
        assert gr.counts_under(rot, shift, x, y)[j] == got["counts"][0, j]
        assert np.abs(rot - fix[f"{name}.{mode}.rotation"][j]).max() <= 1e-9 and np.abs(shift - fix[f"{name}.{mode}.translation"][j]).max() <= 1e-7
    if mode == "search":
        assert (got["counts"][0] >= _single(name, "global")["counts"][0]).all()


def _batch(names, n_rows, atoms=5):
    """The recorded cases as one padded batch: structures 2 k (a) and 2 k + 1 (b), rows behind a case masked out and filled with junk."""
    fix = _fix()
    prot = np.full((2 * len(names), n_rows, atoms, 3), 7.5, dtype=np.float32)
    mask = np.zeros((2 * len(names), n_rows), dtype=np.float32)
    norm = np.zeros(len(names), dtype=np.int32)
    for k, name in enumerate(names):
        a, b, ma, mb, nl = gr.case_inputs(fix, name)
        n = len(a)
        prot[2 * k, :n, :5], prot[2 * k + 1, :n, :5] = a, b
        mask[2 * k, :n], mask[2 * k + 1, :n] = ma, mb
        norm[k] = nl or 0
    return prot, mask, norm


BATCH = ("n5", "n37", "masked", "n65", "unrelated", "n130", "n3")


@pytest.mark.parametrize("mode", gr.MODES)
def test_padded_masked_batch_equals_the_pairs_alone_in_any_order(mode):
    """Seven cases of n = 3 .. 130 padded to 140 rows in one launch, masks and a normalisation length among them; the pair list in
    order and permuted: every pair's outputs equal its own launch bit for bit."""
    prot, mask, norm = _batch(BATCH, 140)
    pairs = np.array([[2 * k, 2 * k + 1] for k in range(len(BATCH))])
    got = gdt.gdt_scores(prot, mask_a=mask, pairs=pairs, norm_length=norm, superpose=mode)
    order = np.array([4, 0, 6, 2, 5, 1, 3])
    mixed = gdt.gdt_scores(prot, mask_a=mask, pairs=pairs[order], norm_length=norm[order], superpose=mode)
    for k, name in enumerate(BATCH):
        rows = len(_fix()[f"{name}.ca_a"])
        _same_pair(got, k, _single(name, mode), 0, rows)
        _same_pair(mixed, int(np.flatnonzero(order == k)[0]), _single(name, mode), 0, rows)
    assert "matrix_ts" not in got and np.array_equal(mixed["pairs"], pairs[order]) and got["res_within"].shape == (7, 140)


def test_atom37_and_device_tensors_equal_the_five_atom_arrays():
    prot, mask, norm = _batch(BATCH[:4], 90)
    wide, _, _ = _batch(BATCH[:4], 90, atoms=37)
    pairs = np.array([[2 * k, 2 * k + 1] for k in range(4)])
    base = gdt.gdt_scores(prot, mask_a=mask, pairs=pairs, norm_length=norm)
    for other in (gdt.gdt_scores(wide, mask_a=mask, pairs=pairs, norm_length=norm),
                  gdt.gdt_scores(torch.from_numpy(wide).cuda(), mask_a=torch.from_numpy(mask).cuda(), pairs=pairs, norm_length=norm),
                  # the second structures from an array of their own, in the other layout
                  gdt.gdt_scores(torch.from_numpy(wide[0::2]).cuda(), prot[1::2], mask[0::2], mask[1::2], norm_length=norm)):
        for k in range(4):
            _same_pair(other, k, base, k)
    shared = gdt.gdt_scores(prot[[0, 2]], prot[1:2], mask[[0, 2]], mask[1:2], ref_index=[0, 0], superpose="none")
    assert np.array_equal(shared["pairs"], [[0, 0], [1, 0]])
    _same_pair(shared, 0, gdt.gdt_scores(prot, mask_a=mask, pairs=pairs[:1], superpose="none"), 0)


def test_all_against_all_of_eight_samples():
    """Eight noisy copies of a 40-row trace: the matrix form against the pair-list form bit for bit, the matrices symmetric with a unit
    diagonal, every pair equal to the restatement."""
    rng = np.random.default_rng(17)
    base = _fix()["n130.ca_b"][:40].astype(np.float64)
    prot = np.stack([gr.five_atoms((base + rng.normal(size=base.shape) * (0.3 + 0.4 * s) / np.sqrt(3.0)).astype(np.float32)) for s in range(8)])
    got = gdt.gdt_scores(prot)
    listed = gdt.gdt_scores(prot, pairs=gdt.all_pairs(8))
    for key, score in (("matrix_ts", "gdt_ts"), ("matrix_ha", "gdt_ha")):
        m = got[key]
        assert m.shape == (8, 8) and np.array_equal(m, m.T) and np.array_equal(np.diag(m), np.ones(8))
        assert all(m[i, j] == got[score][p] for p, (i, j) in enumerate(got["pairs"]))
    assert len(got["gdt_ts"]) == 28 and np.array_equal(got["pairs"], listed["pairs"]) and "matrix_ts" not in listed
    for p, (i, j) in enumerate(got["pairs"]):
        _same_pair(got, p, listed, p)
        want = gr.gdt(*gr.compact(prot[i], prot[j]))
        assert want["margin"] >= 1e-9  # (decidable as the fixture's cases are: the smallest of the 28 margins is 1.2e-6 Angstrom)
        for k in ("counts", "best_item", "best_pass", "passes", "res_within"):
            assert np.array_equal(got[k][p], want[k]), k
        assert got["gdt_ts"][p] == want["gdt_ts"] and got["gdt_ha"][p] == want["gdt_ha"]
    assert gdt.gdt_metrics(got, 3) == {"gdt_ts": float(got["gdt_ts"][3]), "gdt_ha": float(got["gdt_ha"][3])}


def test_skipped_pairs_and_too_many_rows():
    fix = _fix()
    a, b, _, _, _ = gr.case_inputs(fix, "n9")
    both = np.stack([a, b])
    for mode in gr.MODES:
        got = gdt.gdt_scores(both, pairs=[[0, 1], [0, 2], [-1, 0], [1, 0]], superpose=mode)
        assert got["status"].tolist() == [0, _lib.GDT_SKIPPED, _lib.GDT_SKIPPED, 0] and np.isnan(got["gdt_ts"][1:3]).all() and np.isfinite(got["gdt_ha"][[0, 3]]).all()
        assert not got["counts"][1:3].any() and not got["res_within"][1:3].any() and (got["best_item"][1:3] == -1).all() and got["n_scored"].tolist() == [9, 0, 0, 9]
        _same_pair(got, 0, _single("n9", mode), 0)
        if mode == "none":  # (|x - y| does not depend on which of the two is the model)
            assert np.array_equal(got["counts"][3], got["counts"][0]) and np.array_equal(got["res_within"][3], got["res_within"][0])
    mask = np.zeros((1, 9), dtype=np.float32)
    mask[0, [2, 7]] = 1
    short = gdt.gdt_scores(a[None], b[None], mask)  # n = 2
    assert short["status"].tolist() == [_lib.GDT_TOO_SHORT] and short["n_scored"].tolist() == [2] and np.isnan(short["gdt_ts"][0])
    long = np.zeros((1, gdt.MAX_ROWS + 1, 5, 3), dtype=np.float32)
    with pytest.raises(_lib.FdiptError, match="ESIZE"):
        gdt.gdt_scores(long, long)


def test_run_gdt_on_gathered_entries(tmp_path):
    """``run_sharded.run_gdt`` (what ``--gdt`` runs on rank 0) on gathered entries as an inpainting run leaves them - the hinge case as
    atom37, rows 20 .. 44 diffused, two samples and the ground truth: ``gdt.json`` and ``gdt.csv`` carry the numbers of direct calls
    without a superposition and searched over the diffused rows; without ground truth the structure is skipped; a de novo gather writes
    the searched all-against-all matrix per length."""
    import csv
    import json

    from framedipt_amd import run_sharded
    fix = _fix()
    wide = lambda ca: np.concatenate([gr.five_atoms(ca), np.zeros((len(ca), 32, 3), dtype=np.float32)], axis=1)  # noqa: E731
    truth, samples = wide(fix["hinge.ca_b"]), [wide(fix["hinge.ca_a"]), wide(fix["hinge.ca_b"] + np.float32(0.75))]
    diffused = np.zeros(60, dtype=np.float32)
    diffused[20:45] = 1
    records = [{"item": s, "name": "complex", "sample_i": s, "file": f"complex/sample_{s}/sample_{s}_1.pdb"} for s in range(2)]
    gathered = {s: {"prot": samples[s], "diffused": diffused, "res_mask": np.ones(60, dtype=np.float32), **({"gt": truth} if s == 0 else {})} for s in range(2)}
    summary = run_sharded.run_gdt(str(tmp_path), records, gathered, inpainting=True)
    with open(tmp_path / "gdt.json") as f:
        assert json.load(f) == json.loads(json.dumps(summary))
    with open(tmp_path / "gdt.csv", newline="") as f:
        table = list(csv.DictReader(f))
    entry = summary["structures"]["complex"]
    assert entry["samples"] == ["0", "1"] == [t["sample"] for t in table] and not summary["skipped"] and entry["n_scored"] == [25, 25]
    mask = np.stack([diffused, diffused])
    fixed, search = (gdt.gdt_scores(np.stack(samples), truth[None], mask_a=mask, superpose=m) for m in ("none", "search"))
    for s, row in enumerate(table):
        assert entry["gdt_ts_fixed"][s] == fixed["gdt_ts"][s] == float(row["gdt_ts_fixed"]) and entry["gdt_ha_fixed"][s] == fixed["gdt_ha"][s] == float(row["gdt_ha_fixed"])
        assert entry["gdt_ts"][s] == search["gdt_ts"][s] == float(row["gdt_ts"]) and entry["gdt_ha"][s] == search["gdt_ha"][s] == float(row["gdt_ha"])
        assert entry["counts"][s] == search["counts"][s].tolist() and entry["counts_fixed"][s] == fixed["counts"][s].tolist() and int(row["n_scored"]) == 25
    # sample 1 is the ground truth moved by 0.75 A along every axis (1.3 A): outside 1 A where it stands, inside 0.5 A once superposed
    assert entry["counts_fixed"][1] == [0, 0, 25, 25, 25] and entry["counts"][1] == [25] * 5 and entry["gdt_ts"][1] == 1.0
    bare = {i: {k: v for k, v in it.items() if k != "gt"} for i, it in gathered.items()}
    assert run_sharded.run_gdt(str(tmp_path), records, bare, inpainting=True)["skipped"] == ["complex"]
    done = run_sharded.run_gdt(str(tmp_path), records, bare, inpainting=False)
    matrix = np.load(tmp_path / "pairwise_gdt_ts_length_60.npy")
    assert done == {"lengths": [60]} and np.array_equal(matrix, gdt.gdt_scores(np.stack(samples))["matrix_ts"]) and matrix.shape == (2, 2)
