"""GPU tests (-m gpu) of the interface accuracy through a row map (framedipt_amd/interface.py ``alignment=`` ->
fdipt_sample_interface_mapped, csrc/interface_mapped.hip) against its two oracles - the un-mapped device call on
the gathered model (coverage "ignore": every bit) and on the far-point model (coverage "penalise": the counts) - and against the fixture
tests/golden/interface_mapped_cases.npz of the NumPy restatement tests/interface_mapped_ref.py.  The cases
(``interface_mapped_ref.cases``) sit at the kernel's edges: 64 receptor rows per block, ligand tiles of 256 rows (64 for "all").
``pytest tests/test_gpu_interface_mapped.py -m gpu -s`` prints the device error of every float output next to its bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import interface_mapped_ref as mr
import interface_ref as ir
from conftest import load_golden

pytestmark = pytest.mark.gpu

OUTPUTS = ir.INT_OUTPUTS + ir.ROW_OUTPUTS + ir.FLOAT_OUTPUTS
MAPPED_OUTPUTS = OUTPUTS + ("n_interface_covered", "n_covered", "n_reference")
CASES = sorted(mr.cases())


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("interface_mapped_cases.npz")


def _masks(c):
    return {} if c["res_mask_a"] is None else dict(res_mask=c["res_mask_a"][None])


@functools.lru_cache(maxsize=None)
def _mapped(name, coverage, prune=True):
    """One case as a call of its own (NumPy inputs, uploaded)."""
    from framedipt_amd import interface
    c = mr.cases()[name]
    return interface.interface_accuracy(c["xa"][None], c["xb"][None], c["sides"], atoms=c["mode"], alignment=c["m"], coverage=coverage, prune=prune, **_masks(c))


def _same_bits(a, pa, b, pb, keys=OUTPUTS):
    for k in keys:
        x, y = np.asarray(a[k])[pa], np.asarray(b[k])[pb]
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k


@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_ignore_is_the_unmapped_call_on_the_gathered_model(name, prune):
    """The first oracle.  The model is gathered with torch on the device - row j is model row m[j], masked off where the map is -1 or
    the model's res_mask drops the row - and the un-mapped entry runs on it: every output equals, bit for bit, with pruning and without.
    The cases cover the four atom sets, an atom37 reference against a five-atom model (n257.*) and CA traces (n2.*)."""
    from framedipt_amd import interface
    c = mr.cases()[name]
    dev = torch.device("cuda", torch.cuda.current_device())
    xa, m = torch.from_numpy(c["xa"]).to(dev), torch.from_numpy(c["m"]).to(dev).long()
    rows_a = torch.ones(len(xa), device=dev) if c["res_mask_a"] is None else torch.from_numpy(c["res_mask_a"]).to(dev)
    rows = ((m >= 0) & (rows_a[m.clamp(min=0)] != 0)).float()
    gathered = xa[m.clamp(min=0)] * rows.reshape((-1,) + (1,) * (xa.dim() - 1))
    want = interface.interface_accuracy(gathered[None], torch.from_numpy(c["xb"][None]).to(dev), c["sides"], atoms=c["mode"], res_mask=rows[None], prune=prune)
    got = _mapped(name, "ignore", prune)
    _same_bits(got, 0, want, 0)
    assert np.array_equal(got["n_interface_covered"], got["n_interface_rows"])
    assert got["n_covered"].tolist() == [int(rows.sum())] and got["n_reference"].tolist() == [len(c["xb"])]
    assert got["coverage"][0] == int(rows.sum()) / len(c["xb"]) and got["coverage_mode"] == "ignore"


@pytest.mark.parametrize("name", CASES)
def test_penalise_matches_the_far_point_model_and_the_restatement(name):
    """The second oracle: the counts and the per-row outputs equal the un-mapped device call on the far-point model (every uncovered
    reference row with the reference's atom pattern at a far, distinct point, marked present).  Every integer - the status and
    n_interface_covered among them - and ``interface_rows`` equal the restatement's; every float output is NaN where the restatement's is
    and within 32 x the restatement's own summation-order change for the case (``interface_ref.bound`` on the fixture's yardsticks).
    Pruning changes no bit."""
    from framedipt_amd import interface
    c, fix, key = mr.cases()[name], _fix(), f"{name}.penalise"
    got = _mapped(name, "penalise")
    xf, rows, mask = mr.far_point_model(c["xa"], c["xb"], c["m"], res_mask_a=c["res_mask_a"])
    far = interface.interface_accuracy(xf[None], c["xb"][None], c["sides"], atoms=c["mode"], res_mask=rows[None], atom_mask_a=mask[None])
    _same_bits(got, 0, far, 0, mr.COUNT_OUTPUTS + ir.ROW_OUTPUTS)
    for k in mr.INT_OUTPUTS + ir.ROW_OUTPUTS:
        assert np.array_equal(np.asarray(got[k])[0], fix[f"{key}.{k}"]), (name, k)
    assert got["n_covered"].tolist() == [int(fix[f"{key}.n_covered"])] and got["n_reference"].tolist() == [int(fix[f"{key}.n_reference"])]
    for k in ir.FLOAT_OUTPUTS:
        want, have = fix[f"{key}.{k}"], np.asarray(got[k])[0]
        assert have.dtype == np.float64 and np.array_equal(np.isnan(want), np.isnan(have)), (name, k)
        err, lim = float(np.max(np.abs(have - want)[~np.isnan(want)], initial=0.0)), ir.bound(fix, key, k, want[~np.isnan(want)])
        print(f"{key}: {k}: |device - restatement| = {err:.3e}, bound {lim:.3e}")
        assert err <= lim, (name, k, err, lim)
    _same_bits(got, 0, _mapped(name, "penalise", False), 0, MAPPED_OUTPUTS)


@pytest.mark.parametrize("name", ["n65.insert", "n257.tile", "all130.window"])
def test_ignore_matches_the_restatement(name):
    """(The recorded "ignore" results, for the integers: the device's gather is the restatement's.)"""
    got, fix = _mapped(name, "ignore"), _fix()
    for k in mr.INT_OUTPUTS + ir.ROW_OUTPUTS:
        assert np.array_equal(np.asarray(got[k])[0], fix[f"{name}.ignore.{k}"]), (name, k)


@pytest.mark.parametrize("coverage", ["ignore", "penalise"])
@pytest.mark.parametrize("name", ["n65.backbone", "all130.swapped", "n2.swapped"])
def test_an_identity_map_is_the_call_without_an_alignment(name, coverage):
    """N_a = N_b and m[j] = j: every output equals ``interface_accuracy`` without ``alignment`` bit for bit under both switches."""
    from framedipt_amd import interface
    c = mr.cases()[name]
    model, _, _ = mr.gathered_model(c["xa"], c["m"])
    model = np.where((c["m"] >= 0).reshape((-1,) + (1,) * (model.ndim - 1)), model, c["xb"][:, :5] if model.shape[1:] == (5, 3) else c["xb"])
    want = interface.interface_accuracy(model[None], c["xb"][None], c["sides"], atoms=c["mode"])
    got = interface.interface_accuracy(model[None], c["xb"][None], c["sides"], atoms=c["mode"], alignment=np.arange(len(model)), coverage=coverage)
    _same_bits(got, 0, want, 0)
    assert np.array_equal(got["n_covered"], got["n_reference"]) and got["n_covered"].tolist() == [len(model)]
    assert np.array_equal(got["n_interface_covered"], got["n_interface_rows"])


def _batch():
    """Three models of 70 rows against the one 65-row reference, each with its own map."""
    names = ("n65.insert", "n65.window", "n65.backbone")
    c = [mr.cases()[n] for n in names]
    return names, np.stack([v["xa"] for v in c]), c[0]["xb"][None], c[0]["sides"], np.stack([v["m"] for v in c])


@pytest.mark.parametrize("coverage", ["ignore", "penalise"])
def test_per_pair_maps_and_map_verdicts(coverage):
    """Maps [P,N_b] in one call equal the P calls of their own, bit for bit.  A batch that holds a map with an entry out of range, a map
    that uses a model row twice and a pair whose reference index is out of range (device-tensor maps: NumPy maps raise) flags exactly
    those pairs on every interface, with the outputs of a skipped pair and n_covered = n_reference = 0; the others keep every bit."""
    from framedipt_amd import _lib, interface
    names, models, ref, sides, maps = _batch()
    sides = np.concatenate([sides, np.where(sides == ir.RECEPTOR, ir.LIGAND, ir.RECEPTOR)])  # (two interfaces: the second with the sides swapped)
    single = [interface.interface_accuracy(models[i:i + 1], ref, sides, atoms="cb", alignment=maps[i], coverage=coverage) for i in range(3)]
    got = interface.interface_accuracy(models, ref, sides, atoms="cb", ref_index=[0, 0, 0], alignment=maps, coverage=coverage)
    for i in range(3):
        _same_bits(got, i, single[i], 0, MAPPED_OUTPUTS)
    dev = torch.device("cuda", torch.cuda.current_device())
    bad = np.stack([maps[0], maps[1], maps[2], maps[0], maps[1]])
    bad[1, 7] = 70  # out of range (N_a = 70)
    bad[2, 64] = bad[2, 0]  # a model row used twice
    pairs = np.array([[0, 0], [1, 0], [2, 0], [0, 5], [1, 0]])
    got = interface.interface_accuracy(models, ref, sides, atoms="cb", pairs=pairs, alignment=torch.from_numpy(bad).to(dev), coverage=coverage)
    _same_bits(got, 0, single[0], 0, MAPPED_OUTPUTS)
    _same_bits(got, 4, single[1], 0, MAPPED_OUTPUTS)
    assert _lib.IFACE_MAP_OUT_OF_RANGE == mr.MAP_OUT_OF_RANGE and _lib.IFACE_MAP_DUPLICATE == mr.MAP_DUPLICATE
    assert not (mr.MAP_OUT_OF_RANGE | mr.MAP_DUPLICATE) & (ir.NO_NATIVE_CONTACT | ir.TOO_FEW_ATOMS | ir.DEGENERATE | ir.EMPTY_SIDE | ir.NOT_FINITE | ir.SKIPPED)
    assert got["status"][1:4].tolist() == [[mr.MAP_OUT_OF_RANGE] * 2, [mr.MAP_DUPLICATE] * 2, [ir.SKIPPED] * 2]
    for p in (1, 2, 3):
        for k in ir.INT_OUTPUTS[:4] + ir.ROW_OUTPUTS + ("fnat", "fnonnat", "n_interface_covered", "n_covered", "n_reference") + tuple(interface.TRANSFORMS):
            assert not np.asarray(got[k])[p].any(), (p, k)
        assert np.isnan(got["irmsd"][p]).all() and np.isnan(got["lrmsd"][p]).all() and np.isnan(got["dockq"][p]).all()
    with pytest.raises(ValueError, match="row map 1 of 5"):
        interface.interface_accuracy(models, ref, sides, atoms="cb", pairs=pairs, alignment=bad, coverage=coverage)


@pytest.mark.parametrize("name", ["n65.masked", "n257.window"])
def test_device_tensors_give_the_same_bits(name):
    from framedipt_amd import interface
    c = mr.cases()[name]
    dev = torch.device("cuda", torch.cuda.current_device())
    on = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    masks = {} if c["res_mask_a"] is None else dict(res_mask=on(c["res_mask_a"][None]))
    got = interface.interface_accuracy(on(c["xa"][None]), on(c["xb"][None]), on(c["sides"]), atoms=c["mode"], alignment=on(c["m"]), coverage="penalise",
                                       res_mask_b=torch.ones(1, len(c["xb"]), device=dev), **masks)
    _same_bits(got, 0, _mapped(name, "penalise"), 0, MAPPED_OUTPUTS)


def _truncated_and_swapped():
    """A 65-row reference (receptor chain 0: rows 0 .. 34, ligand chain 1: rows 35 .. 64) and a model that stores the ligand chain first
    and lacks 5 rows at one end of one chain - the first (chain, end) at which the letters leave the alignment no choice: the diagonal of
    BLOSUM62 dominates its rows strictly, so another placement of the 5-row gap scores the same only where the letter next to the gap
    occurs among the 5 deleted ones."""
    xb, sides, chain, aatype = mr.cut_complex("1fyt", 0, 1, 35, 30)
    for label in (0, 1):
        rows = np.flatnonzero(chain == label)
        for gone, neighbour in ((rows[:5], rows[5]), (rows[-5:], rows[-6])):
            if aatype[neighbour] not in aatype[gone]:
                keep = np.setdiff1d(np.arange(len(chain)), gone)
                src = np.concatenate([keep[chain[keep] == 1], keep[chain[keep] == 0]])  # the ligand chain first
                xa, m = mr.plant(ir.noisy_chain(xb, chain, 1, 11, 1.0), src, xb)
                return xa, aatype[src], chain[src], xb, aatype, chain, sides, m
    raise AssertionError("no unambiguous truncation")


def test_sequence_aligned_interface_on_a_truncated_model_with_swapped_chains():
    """Sequences in, DockQ out: the map the Gotoh aligner finds is the planted one (not monotone across the chains), n_covered = N_b - 5,
    and the counts under "penalise" are the restatement's."""
    from framedipt_amd import compare, interface
    xa, aatype_a, chain_a, xb, aatype_b, chain_b, sides, m = _truncated_and_swapped()
    got = compare.sequence_aligned_interface(xa[None], aatype_a, xb[None], aatype_b, chain_a, chain_b, atoms="cb", coverage="penalise")
    assert np.array_equal(got["alignment"], m) and np.any(np.diff(m[m >= 0]) < 0)
    assert got["n_covered"].tolist() == [len(xb) - 5] and got["n_reference"].tolist() == [len(xb)]
    assert np.array_equal(got["sides"], sides) and got["labels"].tolist() == [[0, 1]]
    want = mr.mapped_all(xa, xb, sides, m, "cb", "penalise")
    for k in mr.INT_OUTPUTS + ir.ROW_OUTPUTS:
        assert np.array_equal(np.asarray(got[k])[0], want[k]), k
    assert got["fnat"][0, 0] == want["fnat"][0] and 0 < want["fnat"][0] < 1
    assert got["global_dockq"].tolist() == [interface.global_dockq(got, 0)] == [got["dockq"][0, 0]]
    ignore = compare.sequence_aligned_interface(xa[None], aatype_a, xb[None], aatype_b, chain_a, chain_b, atoms="cb", coverage="ignore")
    assert ignore["n_native"][0, 0] <= got["n_native"][0, 0] and ignore["fnat"][0, 0] >= got["fnat"][0, 0]


def test_abi_refusals_come_before_any_launch():
    """FDIPT_EINVAL / FDIPT_ESIZE of fdipt_sample_interface_mapped; the workspace holds the un-mapped entry's plus a row and a verdict."""
    from framedipt_amd import _lib
    lib = _lib.load()
    for p, n in ((1, 1), (3, 65), (64, 810)):
        assert lib.fdipt_sample_interface_mapped_workspace(p, n) == lib.fdipt_sample_interface_workspace(p, n) + 4 * p * n + 4 * p
    assert lib.fdipt_sample_interface_mapped_workspace(0, 5) == 0 and lib.fdipt_sample_interface_mapped_workspace(5, 0) == 0
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = _lib.ptr(buf)
    pointers = lambda cls: {name: p for name, t in cls._fields_ if t is C.c_void_p}  # noqa: E731
    good = dict(pointers(_lib.InterfaceArgs), S=1, N=4, atoms=5, S_b=1, atoms_b=5, P=1, I=1, mode=_lib.IFACE_CB, flags=0, contact_cutoff=8.0,
                interface_cutoff=10.0, workspace_bytes=lib.fdipt_sample_interface_mapped_workspace(1, 4))
    good_map = dict(pointers(_lib.RowMap), N_a=6, coverage=_lib.MAP_PENALISE)

    def call(args=None, row_map=None, no_map=False):
        a, m = _lib.InterfaceArgs(**dict(good, **(args or {}))), _lib.RowMap(**dict(good_map, **(row_map or {})))
        return lib.fdipt_sample_interface_mapped(C.byref(a), None if no_map else C.byref(m), _lib.stream_ptr())

    assert lib.fdipt_sample_interface_mapped(None, None, None) == _lib.EINVAL and call(no_map=True) == _lib.EINVAL
    for bad in (dict(map=None), dict(n_covered=None), dict(n_reference=None), dict(N_a=0), dict(coverage=2), dict(coverage=-1)):
        assert call(row_map=bad) == _lib.EINVAL, bad
    for bad in (dict(n_interface_covered=None), dict(prot_b=None), dict(res_mask_b=None), dict(N=0), dict(I=0), dict(mode=4), dict(atoms=14), dict(flags=2),
                dict(contact_cutoff=0.0), dict(status=None), dict(workspace=None)):
        assert call(args=bad) == _lib.EINVAL, bad
    assert call(row_map=dict(N_a=_lib.IFACE_MAX_ROWS + 1)) == _lib.ESIZE
    assert call(args=dict(N=_lib.IFACE_MAX_ROWS + 1, workspace_bytes=1 << 40)) == _lib.ESIZE
    assert call(args=dict(I=_lib.IFACE_MAX_INTERFACES + 1)) == _lib.ESIZE
    assert call(args=dict(workspace_bytes=good["workspace_bytes"] - 1)) == _lib.ESIZE
    assert call(args=dict(workspace_bytes=lib.fdipt_sample_interface_workspace(1, 4))) == _lib.ESIZE  # (the un-mapped entry's is too short)
