"""CPU tests of the interface accuracy: the NumPy restatement (tests/interface_ref.py) against closed forms, the side helpers of
framedipt_amd/interface.py on the chain labels of the 1fyt complex, the fixture's own records, and the errors ``interface_accuracy``
raises before torch or the library is touched."""
import sys

import numpy as np
import pytest

import interface_ref as ir
from conftest import load_golden
from framedipt_amd import interface

NATIVE_1FYT = [173, 46, 4, 26, 41, 14, 4, 10, 14, 152]  # residue pairs within 5 A on all atoms, chain pairs in label order


def _complex(n_rec=14, n_lig=9, seed=7):
    """A five-atom two-chain complex: two wavy strands 6 A apart."""
    rng = np.random.RandomState(seed)
    t_r, t_l = np.arange(n_rec), np.arange(n_lig)
    ca = np.concatenate([np.stack([3.8 * t_r, 1.5 * np.sin(0.7 * t_r), 0.0 * t_r], axis=1),
                         np.stack([3.8 * t_l + 8.0, 1.5 * np.cos(0.6 * t_l), 6.0 + 0.0 * t_l], axis=1)]) + rng.normal(0, 0.3, size=(n_rec + n_lig, 3)) + 5.0
    x = np.zeros((n_rec + n_lig, 5, 3), dtype=np.float32)
    for col, step in enumerate(((-1.2, 0.6, 0.3), (0.0, 0.0, 0.0), (1.1, 0.9, -0.4), (0.2, -1.1, 1.0), (2.0, 1.6, -0.9))):
        x[:, col] = np.round((ca + np.asarray(step)) * 1024.0) / 1024.0  # (multiples of 2^-10 below 64: a shift by 8.5 or 100 is exact in float32)
    return x, np.concatenate([np.full(n_rec, 1), np.full(n_lig, 2)]).astype(np.int32)


@pytest.mark.parametrize("mode", ir.MODES[:3])
def test_model_equal_to_the_reference(mode):
    x, side = _complex()
    got = ir.interface_one(x, x, side, mode)
    assert got["n_native"] > 0 and got["n_native"] == got["n_model"] == got["n_shared"] and got["status"] == 0
    assert got["fnat"] == 1.0 and got["fnonnat"] == 0.0 and got["irmsd"] == 0.0 and got["lrmsd"] == 0.0 and got["dockq"] == 1.0
    assert np.array_equal(got["interface_rotation"], np.eye(3)) and not got["receptor_translation"].any()
    assert np.array_equal(got["res_native"], got["res_shared"]) and got["res_native"][side == 1].sum() == got["n_native"] == got["res_native"][side == 2].sum()
    assert got["n_interface_rows"] == got["interface_rows"].sum() and got["interface_rows"][got["res_native"] > 0].all()


def test_ligand_moved_rigidly():
    """The ligand moved by t with the receptor fixed: lrmsd = |t|.  At |t| = 8.5 A the third DockQ term is 1/2; the ligand moved 100 A away
    has no contact: n_model 0, fnat 0, fnonnat 0."""
    x, side = _complex()
    moved = x.copy()
    moved[side == 2] += np.array([0.0, 8.5, 0.0], dtype=np.float32)  # (8.5 is a float32)
    got = ir.interface_one(moved, x, side, "backbone")
    # the receptor is the reference's: its superposition is the identity exactly, every ligand atom is 8.5 A off exactly
    assert got["lrmsd"] == 8.5 and np.array_equal(got["receptor_rotation"], np.eye(3)) and not got["receptor_translation"].any()
    third = 1.0 / (1.0 + (got["lrmsd"] / 8.5) ** 2)
    assert third == 0.5 and got["dockq"] == (got["fnat"] + 1.0 / (1.0 + (got["irmsd"] / 1.5) ** 2) + third) / 3.0
    far = x.copy()
    far[side == 2] += np.array([0.0, 0.0, 100.0], dtype=np.float32)
    got = ir.interface_one(far, x, side, "backbone")
    assert got["n_model"] == 0 and got["n_shared"] == 0 and got["fnat"] == 0.0 and got["fnonnat"] == 0.0 and got["n_native"] > 0
    assert got["lrmsd"] == 100.0 and not got["res_model"].any()


def test_status_bits_and_the_two_orders():
    x, side = _complex()
    away = x.copy()
    away[side == 2] += np.float32(60.0)
    got = ir.interface_one(away, away, side, "cb")  # the reference itself has no contact
    assert got["status"] == ir.NO_NATIVE_CONTACT | ir.TOO_FEW_ATOMS and got["fnat"] == 0.0 and np.isnan(got["irmsd"]) and np.isnan(got["dockq"]) and got["lrmsd"] == 0.0
    assert ir.interface_one(x, x, np.where(side == 2, 0, side), "cb")["status"] & ir.EMPTY_SIDE
    masked = ir.interface_one(x, x, side, "cb", res_mask_b=(side == 1).astype(np.float32))  # (no ligand row takes part)
    assert masked["status"] & ir.EMPTY_SIDE and masked["n_native"] == 0 and not masked["interface_rows"].any()
    two = ir.interface_one(x[[0, 20]], x[[0, 20]], side[[0, 20]], "ca")
    assert two["status"] & ir.TOO_FEW_ATOMS and np.isnan(two["lrmsd"])
    rng = np.random.RandomState(3)
    noisy = (x + rng.normal(0, 0.7, size=x.shape) * np.where(side == 2, 1.0, 0.3)[:, None, None]).astype(np.float32)
    up, down = ir.interface_one(noisy, x, side, "backbone"), ir.interface_one(noisy, x, side, "backbone", descending=True)
    for k in ir.INT_OUTPUTS + ir.ROW_OUTPUTS:
        assert np.array_equal(up[k], down[k]), k
    assert 0 < abs(up["lrmsd"] - down["lrmsd"]) + abs(up["irmsd"] - down["irmsd"]) + np.abs(up["receptor_rotation"] - down["receptor_rotation"]).max() < 1e-12
    swapped = ir.interface_one(noisy, x, np.where(side == 1, 2, 1), "backbone")
    for k in ("n_native", "n_model", "n_shared", "n_interface_rows", "irmsd", "res_native", "res_model", "res_shared", "interface_rows"):
        assert np.array_equal(up[k], swapped[k]), k


def test_cb_falls_back_to_ca_and_common_atoms():
    x, side = _complex()
    no_cb = x.copy()
    no_cb[:, 3] = 0
    assert ir.interface_one(no_cb, x, side, "cb")["n_native"] == ir.interface_one(x, x, side, "ca", contact_cutoff=8.0)["n_native"]
    wide = np.concatenate([x, np.zeros((len(x), 32, 3), dtype=np.float32)], axis=1)
    wide[:, 7] = x[:, 3] + np.float32(1.5)  # a side-chain atom the five-atom model does not have
    a, b = ir.interface_one(x, wide, side, "backbone"), ir.interface_one(x, x, side, "backbone")
    assert all(np.array_equal(a[k], b[k]) for k in ir.INT_OUTPUTS + ir.ROW_OUTPUTS + ("irmsd", "lrmsd"))


def test_side_helpers_on_the_chain_labels_of_1fyt():
    """``chain_sides``: ten chain pairs, the larger chain the receptor; its native contact counts on all atoms at 5 A are those of an
    independent loop over residues.  ``loop_sides``: the ligand is the diffused rows of a chain."""
    pos, chain = ir.complex_atom37("1fyt")
    sides, labels = interface.chain_sides(chain)
    sizes = {c: int((chain == c).sum()) for c in range(5)}
    assert sizes == {0: 180, 1: 179, 2: 13, 3: 198, 4: 240} and sides.shape == (10, 810) and sides.dtype == np.int32
    assert labels.tolist() == [[0, 1], [0, 2], [3, 0], [4, 0], [1, 2], [3, 1], [4, 1], [3, 2], [4, 2], [4, 3]]
    for k, (r, l) in enumerate(labels):
        assert np.array_equal(sides[k] == 1, chain == r) and np.array_equal(sides[k] == 2, chain == l) and sizes[r] >= sizes[l]
    counted = ir.chain_contacts(pos, chain, 5.0)
    assert [counted[tuple(sorted(pair))] for pair in labels.tolist()] == NATIVE_1FYT
    assert [ir.interface_one(pos, pos, s, "all")["n_native"] for s in sides] == NATIVE_1FYT
    few, few_labels = interface.chain_sides(chain, [(2, 4), (1, 0)])
    assert few_labels.tolist() == [[4, 2], [0, 1]] and np.array_equal(few[0], sides[8]) and np.array_equal(few[1], sides[0])
    with pytest.raises(ValueError, match="chain pair"):
        interface.chain_sides(chain, [(1, 1)])
    with pytest.raises(ValueError, match="chain pair"):
        interface.chain_sides(chain, [(1, 9)])
    diffused = ir.loop_window(chain, 4, 25) | ir.loop_window(chain, 3, 90, 7)
    loop, chains = interface.loop_sides(diffused, chain)
    assert chains.tolist() == [3, 4] and loop.shape == (2, 810)
    assert np.array_equal(loop[0] == 2, diffused & (chain == 3)) and np.array_equal(loop[0] == 1, chain != 3)
    assert np.array_equal(loop[1] == 2, diffused & (chain == 4)) and np.array_equal(loop[1] == 1, chain != 4)
    rest, _ = interface.loop_sides(diffused, chain, partner="rest")
    assert np.array_equal(rest[1] == 1, ~diffused) and np.array_equal(rest[1] == 2, loop[1] == 2)
    assert interface.loop_sides(np.zeros(810), chain)[0].shape == (0, 810)
    with pytest.raises(ValueError, match="partner"):
        interface.loop_sides(diffused, chain, partner="all")


def test_capri_class_and_metrics():
    assert interface.capri_class([0.0, 0.229, 0.23, 0.48, 0.49, 0.79, 0.80, 1.0, np.nan]).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 0]
    result = {"n_native": np.array([[4]]), "n_model": np.array([[5]]), "n_shared": np.array([[3]]), "n_interface_rows": np.array([[9]]), "status": np.array([[0]]),
              "fnat": np.array([[0.75]]), "fnonnat": np.array([[0.4]]), "irmsd": np.array([[1.5]]), "lrmsd": np.array([[8.5]]), "dockq": np.array([[(0.75 + 0.5 + 0.5) / 3]])}
    flat = interface.interface_metrics(result, 0, 0)
    assert flat == {"n_native": 4, "n_model": 5, "n_shared": 3, "n_interface_rows": 9, "fnat": 0.75, "fnonnat": 0.4, "irmsd": 1.5, "lrmsd": 8.5,
                    "dockq": (0.75 + 0.5 + 0.5) / 3, "capri_class": 2, "status": 0}
    result["dockq"][0, 0] = result["irmsd"][0, 0] = np.nan
    flat = interface.interface_metrics(result, 0, 0)
    assert flat["dockq"] is None and flat["irmsd"] is None and flat["capri_class"] is None


def test_fixture_records():
    """What the generator promises: every margin above 1e-9, the real cases with 0 < fnat < 1 on an interface, the 1fyt counts, a moved
    model with the integers of the unmoved one, sizes around the tiles."""
    fix = load_golden("interface_cases.npz")
    names = [str(c) for c in fix["cases"]]
    assert all(float(fix[f"{n}.margin"]) > 1e-9 for n in names) and len(names) == 26
    for n in names:
        if n.split(".")[0] in ir.COMPLEXES:
            assert np.any((fix[f"{n}.fnat"] > 0) & (fix[f"{n}.fnat"] < 1)) and f"{n}.xa" not in fix, n
    assert fix["1fyt.all.n_native"].tolist() == NATIVE_1FYT
    for n in ir.MOTION_CASES:
        assert all(np.array_equal(fix[f"{n}.{k}"], fix[f"{n}_moved.{k}"]) for k in ir.INT_OUTPUTS + ir.ROW_OUTPUTS)
    from framedipt_amd import _lib
    assert [int((fix[f"tile{n}.sides"] == 2).sum()) for n in (255, 256, 257)] == [_lib.IFACE_TILE - 1, _lib.IFACE_TILE, _lib.IFACE_TILE + 1]
    assert [int((fix[f"all{n}.sides"] == 2).sum()) for n in (63, 64, 65)] == [_lib.IFACE_TILE_ALL - 1, _lib.IFACE_TILE_ALL, _lib.IFACE_TILE_ALL + 1]
    assert [int((fix[f"rec{n}.sides"] == 1).sum()) for n in (63, 64, 65)] == [_lib.IFACE_ROWS - 1, _lib.IFACE_ROWS, _lib.IFACE_ROWS + 1]
    assert fix["degenerate.status"].tolist() == [_lib.IFACE_DEGENERATE] and (ir.NO_NATIVE_CONTACT, ir.TOO_FEW_ATOMS, ir.DEGENERATE, ir.EMPTY_SIDE, ir.NOT_FINITE, ir.SKIPPED) == (
        _lib.IFACE_NO_NATIVE_CONTACT, _lib.IFACE_TOO_FEW_ATOMS, _lib.IFACE_DEGENERATE, _lib.IFACE_EMPTY_SIDE, _lib.IFACE_NOT_FINITE, _lib.IFACE_SKIPPED)
    xa, xb, sides, mode = ir.case_inputs(fix, "interleaved")
    again = ir.interface_all(xa, xb, sides, mode)
    assert all(np.array_equal(again[k], fix[f"interleaved.{k}"], equal_nan=True) for k in ir.INT_OUTPUTS + ir.ROW_OUTPUTS + ir.FLOAT_OUTPUTS)


def test_errors_before_torch_or_the_library(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", None)  # (an import of torch would raise)
    x, side = _complex()
    x = x[None]
    for kw, text in ((dict(atoms="heavy"), "atoms should be"), (dict(sides=None), "sides is required"), (dict(sides=side[:-1]), "sides should be"),
                     (dict(prot_b=x[:, :-1]), "rows of prot_a"), (dict(atoms="all"), "needs atom37"), (dict(contact_cutoff=0.0), "cutoffs should be positive"),
                     (dict(interface_cutoff=-1.0), "cutoffs should be positive"), (dict(res_mask=np.ones((1, 5))), "res_mask"),
                     (dict(atom_mask_a=np.ones((1, 23, 4))), "atom_mask_a"), (dict(prot_b=None, res_mask_b=np.ones((1, 23))), "without prot_b"),
                     (dict(prot_b=np.concatenate([x, x, x])), "give ref_index or pairs")):
        with pytest.raises(ValueError, match=text):
            interface.interface_accuracy(**{**dict(prot_a=np.concatenate([x, x]), prot_b=x, sides=side), **kw})
    with pytest.raises(ValueError, match="needs the backbone atoms"):
        interface.interface_accuracy(x[:, :, 1], x[:, :, 1], side, atoms="cb")
    with pytest.raises(ValueError, match="should be"):
        interface.interface_accuracy(x[0, :, 1], x, side)  # ([N,3]: no leading structure axis)
    empty = interface.interface_accuracy(x, sides=side)  # one structure, all against all: no pair, no call
    assert empty["dockq"].shape == (0, 1) and empty["matrix_dockq"].tolist() == [[[1.0]]] and empty["res_native"].shape == (0, 1, 23)


def test_run_sharded_names_the_flag(monkeypatch, capsys):
    from framedipt_amd import run_sharded
    monkeypatch.setattr(sys, "argv", ["run_sharded", "--help"])
    with pytest.raises(SystemExit) as done:
        run_sharded.main()
    text = " ".join(capsys.readouterr().out.split())
    assert done.value.code == 0 and "--interface" in text and "--interface-atoms" in text and "interface.json and interface.csv" in text
    monkeypatch.setattr(sys, "argv", ["run_sharded", "--out-dir", "x", "--interface"])  # a de novo run: refused before anything is loaded
    with pytest.raises(SystemExit) as done:
        run_sharded.main()
    assert done.value.code == 2 and "de novo run has none" in " ".join(capsys.readouterr().err.split())
    a = run_sharded.parse_args(["--out-dir", "x", "--download-dir", "d", "--interface"])
    for inp in (False, True):  # the samples are gathered, the stage alone runs, the ground truth is built in inpainting runs only
        plan = run_sharded.stage_plan(a, inp)
        assert plan.collect and [s.flag for s in plan.stages] == ["interface"] and plan.ground_truth == inp and not plan.keep_selection
    with pytest.raises(SystemExit, match="inpainting"):
        run_sharded.run_interface("x", [], {}, inpainting=False)
