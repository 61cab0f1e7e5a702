"""CPU tests of the TM-score contract as tests/tm_ref.py restates it - closed forms, invariances, the branches
of d0, the fragment ladder, the widening of the cut, the statuses, the recorded fixture - and of the host side of
framedipt_amd/tm_score.py: Ward clusters and diversity against SciPy, the writers of ``run_sharded --tm-score``."""
import csv
import functools
import json

import numpy as np
import pytest

import tm_ref as tr
from conftest import load_golden
from framedipt_amd import run_sharded, tm_score

ORIGIN = np.array([31.0, -47.0, 58.0])


def _walk(rng, n, persist=0.7):
    d, out = rng.normal(size=3), [np.zeros(3)]
    for _ in range(n - 1):
        d = persist * d + (1.0 - persist) * 1.5 * rng.normal(size=3)
        d /= np.linalg.norm(d)
        out.append(out[-1] + 3.8 * d)
    return (np.array(out) + ORIGIN).astype(np.float32).astype(np.float64)


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("tm_cases.npz")


def _yard(x, y, **kw):
    up, down = tr.tm_score(x, y, **kw), tr.tm_score(x, y, descending=True, **kw)
    return up, max(32.0 * abs(up["tm"] - down["tm"]), 1e-13)


@pytest.mark.parametrize("n", [3, 4, 5, 9, 10, 37, 80])
def test_rigid_copy_scores_one(n):
    rng = np.random.default_rng(n)
    x = _walk(rng, n)
    y = x @ _rotation(rng).T + rng.normal(size=3) * 30.0
    got = tr.tm_score(x, y)
    assert abs(got["tm"] - 1.0) <= 1e-12 and got["status"] == 0 and got["n_aligned"] == n
    rot = got["rotation"]
    assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(rot) - 1.0) <= 1e-12
    assert np.abs(x @ rot.T + got["translation"] - y).max() <= 1e-9


@pytest.mark.parametrize("n,k", [(40, 10), (60, 25), (80, 17)])
def test_hinge_keeps_the_longer_arm(n, k):
    """A chain hinged at row k: superposing the arm of n - k rows alone scores n - k there, so TM >= (n - k) / n."""
    rng = np.random.default_rng(100 + n)
    y = _walk(rng, n)
    x = y.copy()
    x[:k] = (x[:k] - x[k]) @ _rotation(rng).T + x[k]
    x = x @ _rotation(rng).T + 7.0
    got = tr.tm_score(x, y)
    assert (n - k) / n - 1e-12 <= got["tm"] <= 1.0


def test_scores_stay_in_range_and_unrelated_chains_score_low():
    rng = np.random.default_rng(5)
    for n in (20, 50, 90):
        got = tr.tm_score(_walk(rng, n), _walk(rng, n))
        assert 0.0 < got["tm"] <= 1.0 and got["tm"] < 0.4
        noisy = _walk(rng, n)
        near = tr.tm_score(noisy + rng.normal(size=noisy.shape) / np.sqrt(3.0), noisy)
        assert got["tm"] < near["tm"] <= 1.0


def test_invariant_under_a_common_motion_and_under_swapping_the_pair():
    rng = np.random.default_rng(6)
    for n in (9, 37, 64):
        y = _walk(rng, n)
        x = (y + rng.normal(size=y.shape) / np.sqrt(3.0)) @ _rotation(rng).T
        base, lim = _yard(x, y)
        q, shift = _rotation(rng), np.array([40.0, -20.0, 10.0])
        moved = tr.tm_score(x @ q.T + shift, y @ q.T + shift)
        swapped = tr.tm_score(y, x)
        print(f"n = {n}: motion {abs(moved['tm'] - base['tm']):.2e}, swap {abs(swapped['tm'] - base['tm']):.2e}, bound {lim:.2e}")
        assert abs(moved["tm"] - base["tm"]) <= lim and abs(swapped["tm"] - base["tm"]) <= lim
        assert swapped["n_aligned"] == base["n_aligned"] == n


def test_d0_branches_at_21_and_22():
    assert tr.d0_of(21) == 0.5 and tr.d0_of(3) == 0.5
    assert tr.d0_of(22) == pytest.approx(1.24 * 7.0 ** (1.0 / 3.0) - 1.8, abs=1e-15) and tr.d0_of(22) < 0.6
    assert tr.d0_of(300) == pytest.approx(1.24 * 285.0 ** (1.0 / 3.0) - 1.8, abs=1e-14)
    rng = np.random.default_rng(7)
    x, y = _walk(rng, 30), _walk(rng, 30)
    assert tr.tm_score(x[:21], y[:21])["d0"] == 0.5 and tr.tm_score(x[:22], y[:22])["d0"] == tr.d0_of(22)


def test_fragment_ladder_and_seed_numbers():
    assert [tr.ladder(n) for n in (3, 4, 5, 9, 10)] == [[3], [4], [5, 4], [9, 4], [10, 5, 4]]
    assert tr.ladder(19) == [19, 9, 4] and tr.ladder(64) == tr.ladder(65)[:0] + [64, 32, 16, 8, 4] and tr.ladder(65) == [65, 32, 16, 8, 4]
    assert tr.ladder(300) == [300, 150, 75, 37, 18, 4] and tr.ladder(1024) == [1024, 512, 256, 128, 64, 4]
    assert [len(tr.seeds(n)[0]) for n in (3, 4, 5, 9, 10, 80, 130)] == [1, 1, 3, 7, 14, 327, 531]
    assert len(tr.seeds(300)[0]) == 1 + 151 + 226 + 264 + 283 + 297 == 1222 and len(tr.seeds(1024)[0]) == 4162
    length, start = tr.seeds(10)
    assert length.tolist() == [10] + [5] * 6 + [4] * 7 and start.tolist() == [0] + list(range(6)) + list(range(7))


def test_cut_widens_where_fewer_than_three_rows_are_inside():
    """Two unrelated chains: after many seeds' first superposition fewer than 3 rows lie inside d_search - 1 and the cut grows by 0.5."""
    rng = np.random.default_rng(8)
    got = tr.tm_score(_walk(rng, 40), _walk(rng, 40))
    assert got["widened"] > 0 and 0.0 < got["tm"] < 0.4
    # n = 3 never widens: whatever is inside is superposed
    assert tr.tm_score(_walk(rng, 3), _walk(rng, 3))["widened"] == 0


def test_norm_length():
    rng = np.random.default_rng(9)
    y = _walk(rng, 40)
    x = y + rng.normal(size=y.shape) / np.sqrt(3.0)
    own, longer = tr.tm_score(x, y), tr.tm_score(x, y, norm_length=120)
    assert own["d0"] == tr.d0_of(40) and longer["d0"] == tr.d0_of(120) and longer["n_aligned"] == 40
    assert longer["tm"] < own["tm"] and longer["tm"] <= 40 / 120
    assert tr.tm_score(x, y, norm_length=0)["tm"] == own["tm"] == tr.tm_score(x, y, norm_length=40)["tm"]
    assert abs(tr.score_of(longer["rotation"], longer["translation"], x, y, longer["d0"], 120) - longer["tm"]) <= 1e-13


def test_statuses():
    rng = np.random.default_rng(10)
    x = _walk(rng, 5)
    for n in (0, 1, 2):
        got = tr.tm_score(x[:n], x[:n])
        assert got["status"] == tr.TOO_SHORT and np.isnan(got["tm"]) and got["n_aligned"] == n and got["best_seed"] == -1
    bad = x.copy()
    bad[2, 1] = np.nan
    got = tr.tm_score(bad, x)
    assert got["status"] == tr.NOT_FINITE and np.isnan(got["tm"])
    assert (tm_score._lib.TM_TOO_SHORT, tm_score._lib.TM_SKIPPED, tm_score._lib.TM_NOT_FINITE) == (tr.TOO_SHORT, tr.SKIPPED, tr.NOT_FINITE) == (1, 2, 4)
    assert tm_score.MAX_ROWS == 1024


@pytest.mark.parametrize("name", [c for c in tr.CASES if c != "n1024"])
def test_fixture_records_the_restatement(name):
    """The recorded outputs are the restatement's (exactly: same code, same order), the yardstick is within its limit, and the returned
    transform reproduces the recorded score."""
    fix = _fix()
    a, b, ma, mb, norm = tr.case_inputs(fix, name)
    x, y = tr.compact(a, b, ma, mb)
    got = tr.tm_score(x, y, norm)
    assert got["tm"] == float(fix[f"{name}.tm"]) and got["best_seed"] == int(fix[f"{name}.best_seed"]) and got["passes"] == int(fix[f"{name}.passes"])
    assert float(fix[f"{name}.tm.yard"]) <= 1e-9 and tr.bound(fix, name) <= 1e-12
    assert abs(tr.score_of(fix[f"{name}.rotation"], fix[f"{name}.translation"], x, y, got["d0"], got["length"]) - got["tm"]) <= tr.bound(fix, name)
    if name == "masked":
        assert got["n_aligned"] == 69 and got["length"] == 90 and len(a) == 90
    if name in ("unrelated", "hinge"):
        assert int(fix[f"{name}.widened"]) > 0


def _scipy_labels(matrix, th):
    from scipy.cluster import hierarchy
    from scipy.spatial import distance
    tree = hierarchy.linkage(distance.squareform(1 - matrix, force="tovector"), method="ward")
    return tree, hierarchy.fcluster(tree, t=1 - th, criterion="distance")


def _same_partition(a, b):
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("seed", range(6))
def test_ward_clusters_agree_with_scipy(seed):
    rng = np.random.default_rng(seed)
    s = int(rng.integers(2, 40))
    if seed % 2:  # block-structured: high scores inside a block, low between
        block = rng.integers(0, 4, size=s)
        m = np.where(block[:, None] == block[None, :], rng.uniform(0.6, 0.95, size=(s, s)), rng.uniform(0.1, 0.3, size=(s, s)))
    else:
        m = rng.uniform(0.1, 0.9, size=(s, s))
    m = np.triu(m, 1)
    m = m + m.T + np.eye(s)
    for th in (0.3, 0.5, 0.7):
        tree, want = _scipy_labels(m, th)
        labels = tm_score.ward_clusters(m, th)
        assert _same_partition(labels, want) and labels.min() == 1
        d = tm_score.diversity(m, th)
        assert d["clusters"] == len(set(want.tolist())) and d["samples"] == s and d["diversity"] == len(set(want.tolist())) / s
    assert np.allclose(tm_score.ward_linkage(1 - m)[:, 2:], tree[:, 2:], rtol=1e-12, atol=1e-12)
    if seed % 2:
        assert _same_partition(tm_score.ward_clusters(m, 0.5), block + 1)


def test_one_sample_is_one_cluster_and_nan_is_refused():
    assert tm_score.diversity(np.ones((1, 1)))["diversity"] == 1.0
    with pytest.raises(ValueError):
        tm_score.ward_clusters(np.array([[1.0, np.nan], [np.nan, 1.0]]))
    assert tm_score.tm_metrics({"tm": np.array([0.25, 0.5])}, 1) == {"tm_score": 0.5}
    assert tm_score.all_pairs(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]


def test_writers_of_run_sharded(tmp_path):
    """``write_diversity`` and ``write_tm_table`` on a recorded result: the files of a de novo and of an inpainting run."""
    rng = np.random.default_rng(3)
    block = np.array([0, 0, 1, 1, 1, 2])
    m = np.where(block[:, None] == block[None, :], 0.8, 0.2) + np.triu(rng.uniform(0, 0.05, size=(6, 6)), 1)
    m = np.triu(m, 1)
    m = m + m.T + np.eye(6)
    done = run_sharded.write_diversity(str(tmp_path), {24: m, 16: np.ones((1, 1))}, tm_score_th=0.5)
    assert [e["length"] for e in done["lengths"]] == [16, 24] and done["lengths"][1]["clusters"] == 3 and done["lengths"][1]["diversity"] == 0.5
    assert np.array_equal(np.load(tmp_path / "pairwise_tm_score_fixed_length_24.npy"), m)
    assert not list(tmp_path.glob("pairwise_tm_score_length_*"))  # (the reference's cache name is not used)
    assert json.load(open(tmp_path / "diversity.json")) == done
    rows = list(csv.DictReader(open(tmp_path / "diversity.csv")))
    assert [r["length"] for r in rows] == ["16", "24"] and rows[1]["samples"] == "6" and rows[1]["clusters"] == "3" and float(rows[1]["diversity"]) == 0.5
    table = run_sharded.write_tm_table(str(tmp_path), {"1abc": {"samples": ["0", "1"], "tm_score": np.array([0.75, np.nan]), "n_aligned": [12, 2],
                                                                "matrix": np.array([[1.0, 0.6], [0.6, 1.0]])}})
    assert table["structures"]["1abc"]["tm_score"] == [0.75, None] and table["structures"]["1abc"]["matrix"][0][1] == 0.6
    assert json.load(open(tmp_path / "tm_score.json")) == table
    rows = list(csv.DictReader(open(tmp_path / "tm_score.csv")))
    assert rows[0] == {"pdb_name": "1abc", "sample": "0", "n_aligned": "12", "tm_score": "0.75"} and rows[1]["tm_score"] == "nan"
