"""GPU tests (-m gpu) of the interface accuracy (framedipt_amd/interface.py -> fdipt_sample_interface, csrc/interface.hip) against the
fixture tests/golden/interface_cases.npz of the NumPy restatement tests/interface_ref.py.  ``pytest tests/test_gpu_interface.py -m gpu -s``
prints the device error of every float output next to its bound."""
import functools

import numpy as np
import pytest
import torch

import interface_ref as ir
from conftest import load_golden

pytestmark = pytest.mark.gpu

OUTPUTS = ir.INT_OUTPUTS + ir.ROW_OUTPUTS + ir.FLOAT_OUTPUTS


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("interface_cases.npz")


CASES = [str(c) for c in np.load(ir.os.path.join(ir.GOLDEN, "interface_cases.npz"))["cases"]]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return ir.case_inputs(_fix(), name)


@functools.lru_cache(maxsize=None)
def _single(name, prune=True):
    """One case as a call of its own (NumPy inputs, uploaded)."""
    from framedipt_amd import interface
    xa, xb, sides, mode = _inputs(name)
    return interface.interface_accuracy(xa[None], xb[None], sides, atoms=mode, prune=prune)


def _same_bits(a, pa, b, pb, keys=OUTPUTS):
    for k in keys:
        x, y = np.asarray(a[k])[pa], np.asarray(b[k])[pb]
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k


@pytest.mark.parametrize("name", CASES)
def test_case_matches_the_restatement(name):
    """Every fixture case alone: integers, masks and status exactly; the float outputs within 32 x the restatement's own change between its
    two summation orders (``<case>.<key>.yard``), and where that change is 0 within 32 ulp of the value (fnat and fnonnat are one
    division of integers; an RMSD of a model that equals its reference on the rows in question is exactly 0 on both sides)."""
    got = _single(name)
    assert got["pairs"].tolist() == [[0, 0]] and got["fnat"].shape == (1, len(_inputs(name)[2]))
    ir.check_case(_fix(), name, got, report=lambda k, err, lim: print(f"{name}: {k}: |device - restatement| = {err:.3e}, bound {lim:.3e}"))


@pytest.mark.parametrize("name", CASES)
def test_pruning_changes_no_bit(name):
    """FDIPT_IFACE_NO_PRUNE evaluates every residue pair across the sides: every output is the pruned call's, bit for bit."""
    _same_bits(_single(name, True), 0, _single(name, False), 0)


@pytest.mark.parametrize("name", ["missing_cb", "mixed", "all65"])
def test_device_tensors_give_the_same_bits(name):
    from framedipt_amd import interface
    xa, xb, sides, mode = _inputs(name)
    dev = torch.device("cuda", torch.cuda.current_device())
    got = interface.interface_accuracy(torch.from_numpy(xa[None]).to(dev), torch.from_numpy(xb[None]).to(dev), torch.from_numpy(sides).to(dev), atoms=mode,
                                       res_mask=torch.ones(1, len(xa), device=dev))
    _same_bits(got, 0, _single(name), 0)


def test_smallest_shapes_and_missing_atoms():
    """N = 2 with one row per side: the contact is counted, no superposition has three atoms.  A ligand of exactly three CA atoms is
    superposed.  A row without CB in the model counts through its CA under "cb"; a row without N in the reference loses that atom under
    "backbone" and in the RMSDs.  A full-atom reference against a five-atom model is compared on the common atoms: the same numbers as
    against the reference cut to five columns."""
    from framedipt_amd import _lib, interface
    n2 = _single("n2")
    assert n2["status"].tolist() == [[_lib.IFACE_TOO_FEW_ATOMS]] and n2["n_native"].tolist() == [[1]] and n2["n_model"].tolist() == [[1]]
    assert np.isnan(n2["irmsd"][0, 0]) and np.isnan(n2["lrmsd"][0, 0]) and np.isnan(n2["dockq"][0, 0]) and n2["fnat"][0, 0] == 1.0
    assert not n2["interface_rotation"].any() and not n2["receptor_translation"].any()
    assert _single("lig3")["status"].tolist() == [[0]] and np.isfinite(_single("lig3")["lrmsd"][0, 0])
    xa, xb, sides, _ = _inputs("missing_cb")
    assert not xa[15, 3].any() and xa[15, 1].any() and not xb[4, 0].any()
    moved = xa.copy()
    moved[15, 1] += np.float32(40.0)  # (the CA of the row without CB carries its contacts)
    assert _single("missing_cb")["res_model"][0, 0, 15] > 0
    assert interface.interface_accuracy(moved[None], xb[None], sides, atoms="cb")["res_model"][0, 0, 15] == 0
    xa, xb, sides, mode = _inputs("mixed")
    assert xa.shape[1] == 5 and xb.shape[1] == 37
    _same_bits(_single("mixed"), 0, interface.interface_accuracy(xa[None], xb[None, :, :5].copy(), sides, atoms=mode), 0)


def test_planted_cutoff_pairs_and_the_prune_trap():
    """Ligand CA atoms 1e-3 A inside and outside the contact cutoff (8) and the interface cutoff (10) of one receptor CA: one contact in the
    reference, two in the model (the row outside has moved 2e-3 inside), three ligand rows and the receptor row at the interface.  The
    trap: two rows whose CAs are 14 A apart and whose side-chain atoms are 4 A apart are a contact with pruning on."""
    got = _single("planted")
    assert (got["n_native"][0, 0], got["n_model"][0, 0], got["n_shared"][0, 0], got["n_interface_rows"][0, 0]) == (1, 2, 1, 4)
    assert got["res_native"][0, 0].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0] and got["res_model"][0, 0].tolist() == [2, 0, 0, 0, 0, 1, 1, 0, 0]
    assert got["interface_rows"][0, 0].tolist() == [True, False, False, False, False, True, True, True, False]
    assert got["fnat"][0, 0] == 1.0 and got["fnonnat"][0, 0] == 0.5
    xa, xb, _, _ = _inputs("trap")
    assert np.linalg.norm(xb[2, 1] - xb[8, 1]) == 14.0 and np.linalg.norm(xb[2, 10] - xb[8, 10]) == 4.0
    trap = _single("trap", prune=True)
    assert trap["n_native"][0, 0] == 1 and trap["res_native"][0, 0, 2] == 1 and trap["res_native"][0, 0, 8] == 1 and trap["n_shared"][0, 0] == 1


@pytest.mark.parametrize("name", ir.MOTION_CASES)
def test_rigid_motion_of_the_model(name):
    """The model under the fixture's rotation and 100 A shift, rounded to float32 again: every integer and mask is the unmoved call's;
    irmsd moves by no more than the float32 rounding of the moved coordinates can move it (``interface_ref.MOTION_IRMSD``: the RMSD after the
    best superposition is 1-Lipschitz in the root mean square displacement of its atoms) plus the two calls' own bounds; every float output
    of the moved call is the restatement's on the moved input within its bound (the parametrised parity test holds it, ``<case>_moved``)."""
    fix, still, moved = _fix(), _single(name), _single(f"{name}_moved")
    assert np.abs(_inputs(f"{name}_moved")[0]).max() < 512
    _same_bits(still, 0, moved, 0, ir.INT_OUTPUTS + ir.ROW_OUTPUTS)
    lim = ir.MOTION_IRMSD + ir.bound(fix, name, "irmsd", still["irmsd"][0]) + ir.bound(fix, f"{name}_moved", "irmsd", moved["irmsd"][0])
    err = np.abs(still["irmsd"] - moved["irmsd"]).max()
    print(f"{name}: |irmsd - irmsd of the moved model| = {err:.3e}, bound {lim:.3e}")
    assert err <= lim
    assert np.array_equal(still["fnat"], moved["fnat"]) and np.array_equal(still["fnonnat"], moved["fnonnat"])


def test_swapped_sides_keep_the_counts_and_irmsd():
    """Interface 2 of ``interleaved`` is interface 0 with receptor and ligand swapped: the integers, the per-row counts, the interface
    rows and irmsd (the same atoms in the same order) are the same bits; lrmsd differs."""
    got = _single("interleaved")
    for k in ("n_native", "n_model", "n_shared", "n_interface_rows", "status", "fnat", "fnonnat", "irmsd", "res_native", "res_model", "res_shared", "interface_rows",
              "interface_rotation", "interface_translation"):
        assert np.array_equal(got[k][0, 0], got[k][0, 2]), k
    assert got["lrmsd"][0, 0] != got["lrmsd"][0, 2]


def test_pairs_batches_and_a_skipped_pair():
    """Three pairs of one call, the middle one with a model index out of range: it is SKIPPED (integers and fractions 0, RMSDs and DockQ
    NaN, transforms 0) and its neighbours carry the bits of calls of their own; so do the pairs of a call against ``ref_index``."""
    from framedipt_amd import _lib, interface
    xa, xb, sides, mode = _inputs("interleaved")
    models = np.stack([xa, xb])
    got = interface.interface_accuracy(models, xb[None], sides, atoms=mode, pairs=np.array([[0, 0], [7, 0], [1, 0]]))
    _same_bits(got, 0, _single("interleaved"), 0)
    same = interface.interface_accuracy(xb[None], xb[None], sides, atoms=mode)
    _same_bits(got, 2, same, 0)
    assert same["fnat"].tolist() == [[1.0] * 3] and same["fnonnat"].tolist() == [[0.0] * 3] and same["dockq"].tolist() == [[1.0] * 3]
    assert not same["irmsd"].any() and not same["lrmsd"].any()
    assert got["status"][1].tolist() == [_lib.IFACE_SKIPPED] * 3
    for k in ir.INT_OUTPUTS[:4] + ir.ROW_OUTPUTS + ("fnat", "fnonnat") + tuple(interface.TRANSFORMS):
        assert not np.asarray(got[k])[1].any(), k
    assert np.isnan(got["irmsd"][1]).all() and np.isnan(got["lrmsd"][1]).all() and np.isnan(got["dockq"][1]).all()
    by_index = interface.interface_accuracy(models, models[::-1].copy(), sides, atoms=mode, ref_index=[0, 0])
    _same_bits(by_index, 0, _single("interleaved"), 0)
    _same_bits(by_index, 1, same, 0)


def test_all_against_all_fills_the_matrices():
    """One array: every ordered pair, the reference owning the native contacts; ``matrix_dockq`` and ``matrix_fnat`` [I,S,S] (row = model,
    column = reference) with a unit diagonal."""
    from framedipt_amd import interface
    xa, xb, sides, mode = _inputs("interleaved")
    models = np.stack([xa, xb, ir.move(xa, np.eye(3), [0.3, -0.2, 0.1])])
    got = interface.interface_accuracy(models, sides=sides, atoms=mode)
    assert got["pairs"].tolist() == [[0, 1], [0, 2], [1, 0], [1, 2], [2, 0], [2, 1]]
    assert got["matrix_dockq"].shape == got["matrix_fnat"].shape == (3, 3, 3)
    for k in range(3):
        assert np.array_equal(np.diag(got["matrix_dockq"][k]), np.ones(3)) and np.array_equal(np.diag(got["matrix_fnat"][k]), np.ones(3))
        for p, (i, j) in enumerate(got["pairs"]):
            assert got["matrix_dockq"][k, i, j] == got["dockq"][p, k] and got["matrix_fnat"][k, i, j] == got["fnat"][p, k]
    _same_bits(got, 0, _single("interleaved"), 0)  # (pair (0, 1): the model against the reference)
    assert not np.array_equal(got["n_native"][0], got["n_native"][2])  # (the reference owns the native contacts)
    assert interface.interface_accuracy(models[:1], sides=sides, atoms=mode)["matrix_dockq"].tolist() == [[[1.0]]] * 3


def test_refusals():
    """65 interfaces and 2049 rows are FDIPT_ESIZE, never another path."""
    from framedipt_amd import _lib, interface
    x = np.ones((1, 8, 5, 3), dtype=np.float32)
    sides = np.tile(np.array([1, 1, 1, 1, 2, 2, 2, 2], dtype=np.int32), (interface.MAX_INTERFACES + 1, 1))
    interface.interface_accuracy(x, x, sides[:-1])
    with pytest.raises(_lib.FdiptError, match="ESIZE"):
        interface.interface_accuracy(x, x, sides)
    long = np.ones((1, interface.MAX_ROWS + 1, 5, 3), dtype=np.float32)
    with pytest.raises(_lib.FdiptError, match="ESIZE"):
        interface.interface_accuracy(long, long, np.ones(interface.MAX_ROWS + 1, dtype=np.int32))


def test_run_interface_on_gathered_entries(tmp_path):
    """``run_sharded.run_interface`` (what ``--interface`` runs on rank 0) on gathered entries as an inpainting run leaves them - the 1fyt
    complex with the fixture's 12-row loop diffused, two samples and the ground truth: ``interface.json`` and ``interface.csv`` carry the
    numbers of a direct call on ``loop_sides``; without ground truth the structure is skipped; a de novo gather is refused."""
    import csv
    import json

    from framedipt_amd import interface, run_sharded
    fix = _fix()
    xa, truth, sides, mode = _inputs("1fyt.loop")
    _, chain = ir.complex_atom37("1fyt")
    diffused = fix["1fyt.loop.window"]
    samples = [xa, truth.copy()]
    records = [{"item": s, "name": "1fyt", "sample_i": s, "file": f"1fyt/sample_{s}/sample_{s}_1.pdb"} for s in range(2)]
    gathered = {s: {"prot": samples[s], "diffused": diffused, "res_mask": np.ones(len(xa), dtype=np.float32), "chain_idx": chain.astype(np.float32),
                    **({"gt": truth} if s == 0 else {})} for s in range(2)}
    summary = run_sharded.run_interface(str(tmp_path), records, gathered, inpainting=True, atoms=mode)
    with open(tmp_path / "interface.json") as f:
        assert json.load(f) == json.loads(json.dumps(summary))
    with open(tmp_path / "interface.csv", newline="") as f:
        table = list(csv.DictReader(f))
    assert [e["sample"] for e in summary["samples"]] == ["0", "1"] == [t["sample"] for t in table] and not summary["skipped"] and summary["atoms"] == mode
    assert np.array_equal(interface.loop_sides(diffused, chain)[0], sides)
    direct = interface.interface_accuracy(np.stack(samples), truth[None], sides, atoms=mode)
    for s, (entry, row) in enumerate(zip(summary["samples"], table)):
        want = interface.interface_metrics(direct, s, 0)
        assert entry["chain"] == int(fix["1fyt.loop.label"]) == int(row["chain"]) and entry["ligand_rows"] == np.flatnonzero(diffused).tolist()
        for k, v in want.items():
            assert entry[k] == v and (v is None or float(row[k]) == v), k
        assert entry["res_native"] == direct["res_native"][s, 0][diffused].tolist() and entry["res_shared"] == direct["res_shared"][s, 0][diffused].tolist()
    assert summary["samples"][1]["dockq"] == 1.0 and summary["samples"][1]["capri_class"] == 3
    assert summary["samples"][0]["n_native"] == int(fix["1fyt.loop.n_native"][0])
    bare = {i: {k: v for k, v in it.items() if k != "gt"} for i, it in gathered.items()}
    assert run_sharded.run_interface(str(tmp_path), records, bare, inpainting=True)["skipped"] == ["1fyt"]
    with pytest.raises(SystemExit, match="inpainting"):
        run_sharded.run_interface(str(tmp_path), records, bare, inpainting=False)
