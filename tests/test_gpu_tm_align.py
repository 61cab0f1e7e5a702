"""GPU tests (-m gpu) of the structural-alignment search (framedipt_amd/tm_align.py -> fdipt_sample_tm_align, csrc/tmalign.hip) against
the NumPy restatement of the contract (tests/tma_ref.py) as recorded in tests/golden/tma_cases.npz.  ``pytest tests/test_gpu_tm_align.py
-m gpu -s`` prints the device's error per case next to its bound, max(32 x the restatement's own change between its two evaluation
orders, 1e-13).  The measured worst device error is in DESIGN.md section 7.9; the bound is what is asserted."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import tma_ref as ta
from conftest import load_golden
from framedipt_amd import _lib, run_sharded, tm_align

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("tma_cases.npz")


@functools.lru_cache(maxsize=None)
def _single(name):
    """One recorded case as a launch of its own (NumPy inputs, uploaded)."""
    a, b, ma, mb = ta.case_inputs(_fix(), name)
    return tm_align.tm_align(a[None], b[None], ma[None], mb[None])


def _same_pair(got, p, want, q, rows=None):
    for k in tm_align.OUTPUTS:
        g, w = np.asarray(got[k][p]), np.asarray(want[k][q])
        if k == "alignment" and rows is not None:  # (arrays of different row counts: nothing is aligned behind the shorter)
            assert not (g[rows:] >= 0).any() and not (w[rows:] >= 0).any()
            g, w = g[:rows], w[:rows]
        assert np.array_equal(g, w, equal_nan=True), k


def _ulps(a, b):
    return abs(float(a) - float(b)) / np.spacing(abs(float(b)))


def _check_pair(got, p, fix, name, q=None, prot_a=None, prot_b=None, mask_a=None, mask_b=None):
    """Pair ``p`` of a device result against entry ``q`` (None: a scalar case) of the fixture; returns the worst float error."""
    pick = (lambda v: v) if q is None else (lambda v: v[q])
    worst = 0.0
    for k in ta.FLOAT_OUTPUTS:
        want, yard = pick(fix[f"{name}.{k}"]), pick(fix[f"{name}.{k}.yard"])
        lim = np.maximum(32.0 * yard, 1e-13)
        err = np.abs(got[k][p] - want)
        assert np.array_equal(np.isnan(got[k][p]), np.isnan(want)), k
        err = np.where(np.isnan(want), 0.0, err)
        print(f"{name}{'' if q is None else q}: {k} |device - restatement| = {np.max(err):.3e}, bound {np.min(lim):.3e}")
        assert np.all(err <= lim), (k, err, lim)
        worst = max(worst, float(np.max(err)))
    for k in ("d0_a", "d0_b"):
        assert _ulps(got[k][p], pick(fix[f"{name}.{k}"])) <= 4, k
    for k in ta.EXACT_OUTPUTS:
        assert np.array_equal(got[k][p], pick(fix[f"{name}.{k}"])), k
    if int(got["status"][p]) == 0:
        rot, shift = got["rotation"][p], got["translation"][p]
        assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(rot) - 1.0) <= 1e-12
        (x, rows_a), (y, rows_b) = ta.compact(prot_a, mask_a), ta.compact(prot_b, mask_b)
        inner = np.full(len(y), -1, dtype=np.int64)  # the alignment over the compacted rows
        back = np.full(prot_a.shape[0], -1, dtype=np.int64)
        back[rows_a] = np.arange(len(rows_a))
        full = got["alignment"][p][rows_b]
        inner[full >= 0] = back[full[full >= 0]]
        again = ta.score_of(rot, shift, x, y, inner, float(got["d0_b"][p]), len(y))
        lim = max(32.0 * float(pick(fix[f"{name}.tm.yard"])), 1e-13)
        assert abs(again - got["tm_b"][p]) <= lim, (again, got["tm_b"][p])
        assert got["tm"][p] == got["tm_b"][p] and got["n_aligned"][p] == (full >= 0).sum()
    return worst


@pytest.mark.parametrize("name", ta.CASES)
def test_case_matches_the_restatement(name):
    """5 x 5 and 5 x 9 (the minimum), 19 x 22 (both d0 branches), 64 x 65 (the wave edge of the compactions), 61 x 80 (N_a != N_b), a
    copy, a shifted window, a deletion, a partial match, a hinge and an unrelated pair (long iterations), separate masks, two pairs of
    TCR variable domains of different complexes (I2 and I3 have secondary structure to work with), 300 x 300 (two rows per thread
    in the programme), 512 x 512 (the LDS limit), and a chain against far-apart points (the cut of the fast score widens; fewer than three
    pairs survive the d8 filter: FDIPT_TMA_NO_ALIGNMENT with the filtered alignment written)."""
    fix, got = _fix(), _single(name)
    a, b, ma, mb = ta.case_inputs(fix, name)
    _check_pair(got, 0, fix, name, None, a, b, ma, mb)


def test_all_against_all_of_eight_matches_the_fixture_and_the_pair_list():
    fix = _fix()
    prot = np.stack([ta.five_atoms(c) for c in fix["all8.ca"]])
    got = tm_align.tm_align(prot)
    listed = tm_align.tm_align(prot, pairs=tm_align.all_pairs(8))
    assert got["matrix"].shape == (8, 8) and np.array_equal(got["matrix"], got["matrix"].T) and np.array_equal(np.diag(got["matrix"]), np.ones(8))
    assert len(got["tm"]) == 28 and np.array_equal(got["pairs"], listed["pairs"]) and "matrix" not in listed
    worst = 0.0
    for p, (i, j) in enumerate(got["pairs"]):
        _same_pair(got, p, listed, p)
        assert got["matrix"][i, j] == got["tm_b"][p]
        worst = max(worst, _check_pair(got, p, fix, "all8", p, prot[i], prot[j]))
    print(f"all-against-all of 8: worst |device - restatement| = {worst:.3e}")
    assert tm_align.tm_metrics(got, 3) == {"tm_score": float(got["tm_b"][3])}


BATCH = ("n5", "n19x22", "masked", "n64x65", "unrelated", "tcr130", "deletion")


def _batch(names, n_rows, atoms=5):
    """The recorded cases as one padded batch: structures 2 k (a) and 2 k + 1 (b), rows behind a case masked out and filled with junk."""
    fix = _fix()
    prot = np.full((2 * len(names), n_rows, atoms, 3), 7.5, dtype=np.float32)
    mask = np.zeros((2 * len(names), n_rows), dtype=np.float32)
    for k, name in enumerate(names):
        a, b, ma, mb = ta.case_inputs(fix, name)
        prot[2 * k, :len(a), :5], prot[2 * k + 1, :len(b), :5] = a, b
        mask[2 * k, :len(a)], mask[2 * k + 1, :len(b)] = ma, mb
    return prot, mask


def test_padded_masked_batch_equals_the_pairs_alone_in_any_order():
    """Seven cases of 5 .. 130 rows padded to 140 rows in one launch, masks among them; the pair list in order and permuted: every
    pair's outputs equal its own launch bit for bit (the alignment over the case's own rows, -1 behind them)."""
    fix = _fix()
    prot, mask = _batch(BATCH, 140)
    pairs = np.array([[2 * k, 2 * k + 1] for k in range(len(BATCH))])
    got = tm_align.tm_align(prot, mask_a=mask, pairs=pairs)
    order = np.array([4, 0, 6, 2, 5, 1, 3])
    mixed = tm_align.tm_align(prot, mask_a=mask, pairs=pairs[order])
    for k, name in enumerate(BATCH):
        rows = len(fix[f"{name}.ca_b"])
        _same_pair(got, k, _single(name), 0, rows)
        _same_pair(mixed, int(np.flatnonzero(order == k)[0]), _single(name), 0, rows)
    assert "matrix" not in got and np.array_equal(mixed["pairs"], pairs[order])


def test_atom37_device_tensors_and_a_second_array_of_another_row_count():
    fix = _fix()
    names = BATCH[:4]
    prot, mask = _batch(names, 90)
    wide, _ = _batch(names, 90, atoms=37)
    pairs = np.array([[2 * k, 2 * k + 1] for k in range(4)])
    base = tm_align.tm_align(prot, mask_a=mask, pairs=pairs)
    for other in (tm_align.tm_align(wide, mask_a=mask, pairs=pairs),
                  tm_align.tm_align(torch.from_numpy(wide).cuda(), mask_a=torch.from_numpy(mask).cuda(), pairs=pairs)):
        for k in range(4):
            _same_pair(other, k, base, k)
    # the second structures from an array of their own, in the other layout and with 86 rows instead of 90
    split = tm_align.tm_align(torch.from_numpy(wide[0::2]).cuda(), prot[1::2, :86], mask[0::2], mask[1::2, :86])
    assert split["alignment"].shape == (4, 86) and np.array_equal(split["pairs"], [[k, k] for k in range(4)])
    for k in range(4):
        _same_pair(split, k, base, k, 86)
    shared = tm_align.tm_align(prot[[0, 2]], prot[1:2, :86], mask[[0, 2]], mask[1:2, :86], ref_index=[0, 0])
    assert np.array_equal(shared["pairs"], [[0, 0], [1, 0]])
    _same_pair(shared, 0, base, 0, 86)


def test_statuses_and_limits():
    fix = _fix()
    a, b, _, _ = ta.case_inputs(fix, "n5x9")
    mask_b = np.ones((1, 9), dtype=np.float32)
    mask_b[0, [0, 2, 4, 6, 8]] = 0
    got = tm_align.tm_align(a[None], b[None], None, mask_b)  # n2 = 4
    assert got["status"].tolist() == [_lib.TMA_TOO_SHORT] and np.isnan(got["tm"][0]) and np.isnan(got["tm_a"][0]) and got["n_aligned"].tolist() == [0]
    assert np.array_equal(got["rotation"][0], np.eye(3)) and not got["translation"].any() and (got["alignment"] == -1).all()
    assert got["best_init"].tolist() == [-1] and (got["init_tm"] == -1).all() and not got["init_dp"].any() and got["d0_a"][0] == 0.5 == got["d0_b"][0]
    bad = a.copy()
    bad[2, 1, 0] = np.nan
    got = tm_align.tm_align(np.stack([a, bad]), b[None], ref_index=[0, 0])
    assert got["status"].tolist() == [0, _lib.TMA_NOT_FINITE] and np.isnan(got["tm"][1])
    _same_pair(got, 0, _single("n5x9"), 0)
    both = np.stack([b, b[::-1].copy()])
    got = tm_align.tm_align(both, pairs=[[0, 1], [0, 2], [-1, 0], [1, 0]])  # an index out of range
    assert got["status"].tolist() == [0, _lib.TMA_SKIPPED, _lib.TMA_SKIPPED, 0] and np.isnan(got["tm"][1:3]).all() and np.isfinite(got["tm"][[0, 3]]).all()
    long = np.zeros((1, tm_align.MAX_ROWS + 1, 5, 3), dtype=np.float32)
    with pytest.raises(_lib.FdiptError, match="ESIZE"):
        tm_align.tm_align(long, long)
    with pytest.raises(_lib.FdiptError, match="ESIZE"):
        tm_align.tm_align(b[None], long)


def test_bad_arguments_are_refused_before_any_launch():
    """The entry itself: a second row count without a second array, a missing output, no pairs."""
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    bufs = {k: torch.zeros(64, dtype=torch.float64, device=dev) for k in tm_align.OUTPUTS + ("prot", "mask", "pairs")}

    def call(**change):
        fields = dict(S=1, N_a=9, atoms=5, ca=1, S_b=1, N_b=9, atoms_b=5, P=1, prot_b=None, mask_b=None, workspace=None, workspace_bytes=0,
                      **{k: _lib.ptr(v) for k, v in bufs.items()})
        fields.update(change)
        return lib.fdipt_sample_tm_align(C.byref(_lib.TmAlignArgs(**fields)), _lib.stream_ptr())

    assert call(N_b=8) == _lib.EINVAL and call(rmsd=None) == _lib.EINVAL and call(alignment=None) == _lib.EINVAL and call(P=0) == _lib.EINVAL
    assert call(atoms=4) == _lib.EINVAL and call(ca=5) == _lib.EINVAL and call(prot_b=_lib.ptr(bufs["prot"])) == _lib.EINVAL  # (no mask_b)
    assert call(N_a=513, N_b=513) == _lib.ESIZE
    assert lib.fdipt_sample_tm_align_workspace(8, 300, 200, 28) == 0


def test_run_tm_align_on_a_complex_beyond_the_row_limit(tmp_path):
    """``run_sharded --tm-align`` after an inpainting run on a 600-row complex with 40 diffused rows, and after a de novo run: the
    samples reach the search compacted to their set rows, where handing over the whole complex is refused."""
    rng = np.random.default_rng(21)
    window = _fix()["tcr130.ca_b"][:40]
    prot = np.zeros((3, 600, 5, 3), dtype=np.float32)
    prot[:] = ta.five_atoms(np.cumsum(rng.normal(size=(600, 3)) * 2.2, axis=0).astype(np.float32))
    for s in range(3):
        prot[s, 300:340] = ta.five_atoms((window + rng.normal(size=window.shape) * 0.3 * s).astype(np.float32))
    diffused = np.zeros(600, dtype=np.float32)
    diffused[300:340] = 1
    with pytest.raises(_lib.FdiptError, match="ESIZE"):
        tm_align.tm_align(prot, mask_a=np.tile(diffused, (3, 1)))
    records = [{"item": s, "name": "cplx", "sample_i": s} for s in range(3)]
    gathered = {s: {"prot": prot[s], "diffused": diffused} for s in range(3)}
    done = run_sharded.run_tm_align(str(tmp_path), records, gathered, inpainting=True)
    entry = done["structures"]["cplx"]
    assert entry["samples"] == ["0", "1", "2"] and entry["rows"] == 40 and done["skipped_structures"] == {}
    matrix = np.array(entry["matrix"])
    assert np.array_equal(matrix, tm_align.tm_align(prot[:, 300:340])["matrix"]) and json.load(open(tmp_path / "tm_align.json")) == done
    want = ta.align_structures(prot[0], prot[1], diffused, diffused)
    assert abs(matrix[0, 1] - want["tm_b"]) <= 1e-13 and matrix[0, 1] > 0.8  # (0.5 A of noise at d0 = 1.8: about 0.92)
    wide = np.ones(600, dtype=np.float32)  # every row diffused: beyond the limit, recorded, no error
    done = run_sharded.run_tm_align(str(tmp_path), records, {s: {"prot": prot[s], "diffused": wide} for s in range(3)}, inpainting=True)
    assert done["structures"] == {} and done["skipped_structures"] == {"cplx": 600}
    # de novo: the samples of one length, a res_mask that keeps 40 of the 600 rows
    done = run_sharded.run_tm_align(str(tmp_path), records, {s: {"prot": prot[s], "res_mask": diffused} for s in range(3)}, inpainting=False)
    (e,) = done["lengths"]
    assert (e["length"], e["samples"], e["nan_pairs"], e["fixed_won"]) == (600, 3, 0, 0) and done["skipped_lengths"] == []
    assert np.array_equal(np.load(tmp_path / "pairwise_tm_score_aligned_length_600.npy"), matrix)
