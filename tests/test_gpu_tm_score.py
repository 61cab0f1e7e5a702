"""GPU tests (-m gpu) of the TM-score (framedipt_amd/tm_score.py -> fdipt_sample_tm_score, csrc/tmscore.hip) against the NumPy
restatement of the contract (tests/tm_ref.py) as recorded in tests/golden/tm_cases.npz.  ``pytest tests/test_gpu_tm_score.py -m gpu -s``
prints the device's error per case next to its bound, max(32 x the restatement's own change between its two evaluation orders, 1e-13).

Measured on one MI355X: |device - restatement| of ``tm`` is 0 in all 14 cases and in the 28 pairs of the all-against-all test, and
``best_seed`` and ``passes`` equal the restatement's everywhere; the bound is what is asserted."""
import functools

import numpy as np
import pytest
import torch

import tm_ref as tr
from conftest import load_golden
from framedipt_amd import _lib, tm_score

pytestmark = pytest.mark.gpu

EXACT = ("n_aligned", "status")


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("tm_cases.npz")


@functools.lru_cache(maxsize=None)
def _single(name):
    """One recorded case as a launch of its own (NumPy inputs, uploaded)."""
    a, b, ma, mb, norm = tr.case_inputs(_fix(), name)
    return tm_score.tm_scores(a[None], b[None], ma[None], mb[None], norm_length=norm)


def _same_pair(got, p, want, q):
    for k in tm_score.OUTPUTS:
        assert np.array_equal(np.asarray(got[k][p]), np.asarray(want[k][q]), equal_nan=True), k


def _check_transform(got, p, x, y, length, lim):
    rot, shift = got["rotation"][p], got["translation"][p]
    assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(rot) - 1.0) <= 1e-12
    again = tr.score_of(rot, shift, x, y, float(got["d0"][p]), length)
    assert abs(again - got["tm"][p]) <= lim, (again, got["tm"][p])


@pytest.mark.parametrize("name", tr.CASES)
def test_case_matches_the_restatement(name):
    """n = 3 (the minimum), 4 and 5 (one level), 9, 19, 37 (the ladder), 64 / 65 (the wave edge of the compaction), 80 and 130 (327 and
    531 seeds: more seeds than threads, the lanes fetch further seeds), a hinge and an unrelated pair (the cut widens), masks that drop
    rows at the ends and in the middle with a normalisation length, N = 1024 (the LDS limit, 4162 seeds)."""
    fix, got = _fix(), _single(name)
    lim = tr.bound(fix, name)
    err = abs(got["tm"][0] - float(fix[f"{name}.tm"]))
    print(f"{name}: tm {got['tm'][0]:.15f}, |device - restatement| = {err:.3e}, bound {lim:.3e}; passes {got['passes'][0]} ({int(fix[f'{name}.passes'])}), "
          f"best seed {got['best_seed'][0]} ({int(fix[f'{name}.best_seed'])}, lead {float(fix[f'{name}.lead']):.1e})")
    assert err <= lim
    assert abs(got["d0"][0] - float(fix[f"{name}.d0"])) <= tr.bound(fix, name, "d0") and (got["d0"][0] == 0.5) == (float(fix[f"{name}.d0"]) == 0.5)
    for k in EXACT:
        assert got[k][0] == int(fix[f"{name}.{k}"]), k
    a, b, ma, mb, norm = tr.case_inputs(fix, name)
    x, y = tr.compact(a, b, ma, mb)
    n = len(x)
    _check_transform(got, 0, x, y, norm or n, lim)
    n_seeds = len(tr.seeds(n)[0])
    assert 0 <= got["best_seed"][0] < n_seeds and n_seeds <= got["passes"][0] <= tr.MAX_PASSES * n_seeds
    if float(fix[f"{name}.lead"]) > lim:
        assert got["best_seed"][0] == int(fix[f"{name}.best_seed"]) and got["passes"][0] == int(fix[f"{name}.passes"])


def test_too_short_skipped_and_too_long():
    fix = _fix()
    a, b, _, _, _ = tr.case_inputs(fix, "n9")
    mask = np.zeros((1, 9), dtype=np.float32)
    mask[0, [2, 7]] = 1
    got = tm_score.tm_scores(a[None], b[None], mask)  # n = 2
    assert got["status"].tolist() == [_lib.TM_TOO_SHORT] and np.isnan(got["tm"][0]) and got["n_aligned"].tolist() == [2] and got["best_seed"].tolist() == [-1]
    assert np.array_equal(got["rotation"][0], np.eye(3)) and not got["translation"].any() and got["d0"][0] == 0.5
    three = mask.copy()
    three[0, 4] = 1
    got = tm_score.tm_scores(a[None], b[None], three)  # n = 3 out of 9 rows
    want = tr.tm_score(*tr.compact(a, b, three[0]))
    assert got["status"].tolist() == [0] and abs(got["tm"][0] - want["tm"]) <= 1e-13 and got["n_aligned"].tolist() == [3]
    both = np.stack([a, b])
    got = tm_score.tm_scores(both, pairs=[[0, 1], [0, 2], [-1, 0], [1, 0]])
    assert got["status"].tolist() == [0, _lib.TM_SKIPPED, _lib.TM_SKIPPED, 0] and np.isnan(got["tm"][1:3]).all() and np.isfinite(got["tm"][[0, 3]]).all()
    _same_pair(got, 0, _single("n9"), 0)
    long = np.zeros((1, tm_score.MAX_ROWS + 1, 5, 3), dtype=np.float32)
    with pytest.raises(_lib.FdiptError, match="ESIZE"):
        tm_score.tm_scores(long, long)


def _batch(names, n_rows, atoms=5):
    """The recorded cases as one padded batch: structures 2 k (a) and 2 k + 1 (b), rows behind a case masked out and filled with junk."""
    fix = _fix()
    prot = np.full((2 * len(names), n_rows, atoms, 3), 7.5, dtype=np.float32)
    mask = np.zeros((2 * len(names), n_rows), dtype=np.float32)
    norm = np.zeros(len(names), dtype=np.int32)
    for k, name in enumerate(names):
        a, b, ma, mb, nl = tr.case_inputs(fix, name)
        n = len(a)
        prot[2 * k, :n, :5], prot[2 * k + 1, :n, :5] = a, b
        mask[2 * k, :n], mask[2 * k + 1, :n] = ma, mb
        norm[k] = nl or 0
    return prot, mask, norm


BATCH = ("n5", "n37", "masked", "n65", "unrelated", "n130", "n3")


def test_padded_masked_batch_equals_the_pairs_alone_in_any_order():
    """Seven cases of n = 3 .. 130 padded to 140 rows in one launch, masks and a normalisation length among them; the pair list in
    order and permuted: every pair's outputs equal its own launch bit for bit."""
    prot, mask, norm = _batch(BATCH, 140)
    pairs = np.array([[2 * k, 2 * k + 1] for k in range(len(BATCH))])
    got = tm_score.tm_scores(prot, mask_a=mask, pairs=pairs, norm_length=norm)
    order = np.array([4, 0, 6, 2, 5, 1, 3])
    mixed = tm_score.tm_scores(prot, mask_a=mask, pairs=pairs[order], norm_length=norm[order])
    for k, name in enumerate(BATCH):
        _same_pair(got, k, _single(name), 0)
        _same_pair(mixed, int(np.flatnonzero(order == k)[0]), _single(name), 0)
    assert "matrix" not in got and np.array_equal(mixed["pairs"], pairs[order])


def test_atom37_and_device_tensors_equal_the_five_atom_arrays():
    prot, mask, norm = _batch(BATCH[:4], 90)
    wide, _, _ = _batch(BATCH[:4], 90, atoms=37)
    pairs = np.array([[2 * k, 2 * k + 1] for k in range(4)])
    base = tm_score.tm_scores(prot, mask_a=mask, pairs=pairs, norm_length=norm)
    for other in (tm_score.tm_scores(wide, mask_a=mask, pairs=pairs, norm_length=norm),
                  tm_score.tm_scores(torch.from_numpy(wide).cuda(), mask_a=torch.from_numpy(mask).cuda(), pairs=pairs, norm_length=norm),
                  # the second structures from an array of their own, in the other layout
                  tm_score.tm_scores(torch.from_numpy(wide[0::2]).cuda(), prot[1::2], mask[0::2], mask[1::2], norm_length=norm)):
        for k in range(4):
            _same_pair(other, k, base, k)
    shared = tm_score.tm_scores(prot[[0, 2]], prot[1:2], mask[[0, 2]], mask[1:2], ref_index=[0, 0])
    assert np.array_equal(shared["pairs"], [[0, 0], [1, 0]])
    _same_pair(shared, 0, base, 0)


def test_all_against_all_of_eight_samples():
    """Eight noisy copies of a 40-row excerpt: the matrix form against the pair-list form bit for bit, the matrix symmetric with a unit
    diagonal, every score against the restatement within the bound of its own two evaluation orders."""
    fix = _fix()
    rng = np.random.default_rng(17)
    base = fix["n80.ca_b"][:40].astype(np.float64)
    prot = np.stack([tr.five_atoms((base + rng.normal(size=base.shape) * (0.3 + 0.4 * s) / np.sqrt(3.0)).astype(np.float32)) for s in range(8)])
    got = tm_score.tm_scores(prot)
    listed = tm_score.tm_scores(prot, pairs=tm_score.all_pairs(8))
    assert got["matrix"].shape == (8, 8) and np.array_equal(got["matrix"], got["matrix"].T) and np.array_equal(np.diag(got["matrix"]), np.ones(8))
    assert len(got["tm"]) == 28 and np.array_equal(got["pairs"], listed["pairs"])
    worst = 0.0
    for p, (i, j) in enumerate(got["pairs"]):
        _same_pair(got, p, listed, p)
        assert got["matrix"][i, j] == got["tm"][p]
        x, y = tr.compact(prot[i], prot[j])
        up, down = tr.tm_score(x, y), tr.tm_score(x, y, descending=True)
        lim = max(32.0 * abs(up["tm"] - down["tm"]), 1e-13)
        worst = max(worst, abs(got["tm"][p] - up["tm"]))
        assert abs(got["tm"][p] - up["tm"]) <= lim
        _check_transform(got, p, x, y, 40, lim)
    print(f"all-against-all of 8: worst |device - restatement| = {worst:.3e}")
    d = tm_score.diversity(got["matrix"], 0.5)
    assert d["samples"] == 8 and 1 <= d["clusters"] <= 8
    assert tm_score.tm_metrics(got, 3) == {"tm_score": float(got["tm"][3])}
