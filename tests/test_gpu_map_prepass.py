"""GPU tests (-m gpu) of the map pre-pass that the mapped lDDT and the mapped interface accuracy share (csrc/rowmap.hpp ``fd_map_judge``
under ``lddt_map_kernel`` and ``ifm_map_kernel``): both entries give a pair the same verdict on its map and the same ``n_covered`` /
``n_reference``.  The expectation is NumPy's - ``row_map.flags`` for the bits, a plain loop for the counts - and comes from neither entry.
The maps are device tensors, so the host judges nothing."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_A, N_B = 4, 5
# case A, one map per pair: valid with one -1 | an entry equal to N_a | an entry of -2 | a model row used twice | valid, onto the model
# row whose res_mask is 0 and with the reference row whose res_mask_b is 0 | valid, for the pair whose reference index is out of range
MAPS = np.array([[0, 1, 2, 3, -1], [0, 1, 2, N_A, -1], [0, 1, -2, 3, -1], [0, 1, 1, 3, -1], [2, 3, 0, -1, 1], [0, 1, 2, 3, -1]], dtype=np.int32)
PAIRS = np.array([[0, 0]] * 5 + [[0, 1]], dtype=np.int32)
ROWS_A, ROWS_B = np.array([[1, 1, 0, 1]], dtype=np.float32), np.array([[1, 0, 1, 1, 1]], dtype=np.float32)
SIDES = np.array([1, 1, 1, 2, 2], dtype=np.int32)
FLAGGED, SKIPPED = [1, 2, 3], [5]


def _expected(maps, pairs, rows_a, rows_b):
    """(map bits, n_covered, n_reference) per pair: the bits and the counts 0 for a skipped pair, the counts 0 for a flagged one."""
    from framedipt_amd import row_map
    n_a, judged = rows_a.shape[1], [0 <= ib < len(rows_b) for _, ib in pairs]
    bits = np.where(judged, row_map.flags(maps, n_a), 0)
    covered, reference = np.zeros(len(pairs), dtype=np.int64), np.zeros(len(pairs), dtype=np.int64)
    for p, (ia, ib) in enumerate(pairs):
        if not judged[p] or bits[p]:
            continue
        for j, r in enumerate(maps[p]):
            if rows_b[ib, j] != 0:
                reference[p] += 1
                covered[p] += bool(0 <= r < n_a and rows_a[ia, r] != 0)
    return bits, covered, reference


def _traces(n_a, n_b, seed):
    rng = np.random.RandomState(seed)
    return (rng.normal(0.0, 5.0, size=(1, n_a, 3)) + 1.0).astype(np.float32), (rng.normal(0.0, 5.0, size=(1, n_b, 3)) + 1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case_a(coverage):
    from framedipt_amd import interface, lddt
    xa, xb = _traces(N_A, N_B, 45)
    common = dict(atoms="ca", res_mask=ROWS_A, res_mask_b=ROWS_B, pairs=PAIRS, alignment=torch.from_numpy(MAPS).cuda(), coverage=coverage)
    return lddt.local_accuracy(xa, xb, **common), interface.interface_accuracy(xa, xb, sides=SIDES, **common)


@functools.lru_cache(maxsize=None)
def _case_b():
    from framedipt_amd import interface, lddt
    n = 257  # one row past the 256-thread stride of the counting loop
    xa, xb = _traces(n, n, 257)
    rows_b = np.ones((1, n), dtype=np.float32)
    rows_b[0, 256] = 0
    common = dict(atoms="ca", res_mask_b=rows_b, alignment=torch.arange(n, dtype=torch.int32, device="cuda"))
    return rows_b, lddt.local_accuracy(xa, xb, **common), interface.interface_accuracy(xa, xb, sides=np.arange(n) % 2 + 1, **common)


@pytest.mark.parametrize("coverage", ["ignore", "penalise"])
def test_both_entries_count_what_numpy_counts(coverage):
    bits, covered, reference = _expected(MAPS, PAIRS, ROWS_A, ROWS_B)
    assert np.flatnonzero(bits).tolist() == FLAGGED and covered.tolist() == [2, 0, 0, 0, 2, 0] and reference.tolist() == [4, 0, 0, 0, 4, 0]
    local, iface = _case_a(coverage)
    for key, want in (("n_covered", covered), ("n_reference", reference)):
        print(coverage, key, "lddt", local[key].tolist(), "interface", iface[key].tolist(), "numpy", want.tolist())
        assert local[key].dtype == iface[key].dtype == np.int64
        assert np.array_equal(local[key], iface[key]) and np.array_equal(local[key], want), key


@pytest.mark.parametrize("coverage", ["ignore", "penalise"])
def test_both_entries_flag_the_same_maps(coverage):
    from framedipt_amd import _lib, row_map
    bits, _, _ = _expected(MAPS, PAIRS, ROWS_A, ROWS_B)
    local, iface = _case_a(coverage)
    assert np.array_equal(local["status"] & (_lib.MAP_OUT_OF_RANGE | _lib.MAP_DUPLICATE), bits)
    translated = np.where(bits & row_map.OUT_OF_RANGE, _lib.IFACE_MAP_OUT_OF_RANGE, 0) | np.where(bits & row_map.DUPLICATE, _lib.IFACE_MAP_DUPLICATE, 0)
    assert iface["status"].shape == (len(PAIRS), 1)
    assert np.array_equal(iface["status"][:, 0] & (_lib.IFACE_MAP_OUT_OF_RANGE | _lib.IFACE_MAP_DUPLICATE), translated)
    assert np.flatnonzero(translated).tolist() == FLAGGED
    assert np.flatnonzero(local["status"] & _lib.LDDT_SKIPPED).tolist() == SKIPPED
    assert np.flatnonzero(iface["status"][:, 0] & _lib.IFACE_SKIPPED).tolist() == SKIPPED


def test_a_row_past_the_counting_stride():
    rows_b, local, iface = _case_b()
    n = rows_b.shape[1]
    _, covered, reference = _expected(np.arange(n, dtype=np.int32)[None], np.zeros((1, 2), dtype=np.int32), np.ones((1, n), dtype=np.float32), rows_b)
    assert covered.tolist() == [256] and reference.tolist() == [256]
    from framedipt_amd import _lib
    for out, bad in ((local, _lib.MAP_OUT_OF_RANGE | _lib.MAP_DUPLICATE | _lib.LDDT_SKIPPED),
                     (iface, _lib.IFACE_MAP_OUT_OF_RANGE | _lib.IFACE_MAP_DUPLICATE | _lib.IFACE_SKIPPED)):
        assert out["n_covered"].tolist() == [256] and out["n_reference"].tolist() == [256] and not np.any(out["status"] & bad)
