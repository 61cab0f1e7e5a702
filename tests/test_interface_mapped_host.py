"""Host tests (no device) of the mapped interface-accuracy contract: the NumPy restatement
tests/interface_mapped_ref.py against its two oracles - ``interface_ref.interface_all`` on the gathered model (coverage "ignore") and on
the far-point model (coverage "penalise") -, closed forms, ``interface.global_dockq`` and the errors ``interface_accuracy`` raises before
the library is loaded."""
import numpy as np
import pytest

import interface_mapped_ref as mr
import interface_ref as ir

ALL_OUTPUTS = ir.INT_OUTPUTS + ir.ROW_OUTPUTS + ir.FLOAT_OUTPUTS
CASES = sorted(mr.cases())


def _equal(a, b, keys):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k


@pytest.mark.parametrize("name", CASES)
def test_ignore_is_the_unmapped_restatement_on_the_gathered_model(name):
    c = mr.cases()[name]
    got = mr.mapped_all(c["xa"], c["xb"], c["sides"], c["m"], coverage="ignore", **mr.case_kw(c))
    xg, rows, _ = mr.gathered_model(c["xa"], c["m"], res_mask_a=c["res_mask_a"])
    want = ir.interface_all(xg, c["xb"], c["sides"], c["mode"], res_mask_a=rows)
    _equal(got, want, ALL_OUTPUTS)
    assert np.array_equal(got["n_interface_covered"], got["n_interface_rows"])
    assert got["n_covered"] == int(rows.sum()) and got["n_reference"] == len(c["xb"])


@pytest.mark.parametrize("name", CASES)
def test_penalise_counts_are_the_unmapped_restatement_on_the_far_point_model(name):
    c = mr.cases()[name]
    got = mr.mapped_all(c["xa"], c["xb"], c["sides"], c["m"], coverage="penalise", **mr.case_kw(c))
    xf, rows, mask = mr.far_point_model(c["xa"], c["xb"], c["m"], res_mask_a=c["res_mask_a"])
    want = ir.interface_all(xf, c["xb"], c["sides"], c["mode"], res_mask_a=rows, mask_a=mask)
    _equal(got, want, mr.COUNT_OUTPUTS + ir.ROW_OUTPUTS)
    ignore = mr.mapped_all(c["xa"], c["xb"], c["sides"], c["m"], coverage="ignore", **mr.case_kw(c))
    assert np.all(got["n_native"] >= ignore["n_native"]) and np.array_equal(got["n_model"], ignore["n_model"])
    assert np.array_equal(got["n_interface_covered"], (got["interface_rows"] & (mr.resolve(c["m"], c["res_mask_a"], None, len(c["xa"]))[0] >= 0)).sum(-1))


def test_the_cases_reach_the_edges_they_are_built_for():
    c = mr.cases()
    assert {(len(v["xb"]), len(v["xa"])) for v in c.values()} >= {(65, 70), (257, 200), (130, 130), (2, 2)}
    assert {v["mode"] for v in c.values()} == set(ir.MODES)
    m = c["n65.window"]["m"]
    assert np.all(m[62:65] == -1) and np.all(m[:62] >= 0) and c["n65.window"]["sides"][0, 64] == ir.RECEPTOR  # the only receptor row of block 1
    m = c["n257.window"]["m"]
    assert np.all(m[196:] == -1) and np.all(c["n257.window"]["sides"][0, 255:] == ir.LIGAND)  # rows 255, 256; the whole second ligand tile
    assert c["n257.window"]["xa"].shape[1] == 5 and c["n257.window"]["xb"].shape[1] == 37
    m = c["all130.tile"]["m"]
    assert np.all(m[70:128] == -1) and np.all(c["all130.tile"]["sides"][0, 70:] == ir.LIGAND)
    assert np.any(np.diff(c["all130.swapped"]["m"]) < 0) and np.all(c["all130.swapped"]["m"] >= 0)  # not monotone, every row covered
    assert c["n65.masked"]["res_mask_a"][3] == 0 and c["n65.masked"]["m"][3] == 3
    assert np.all(c["n65.insert"]["m"] >= 0) and len(c["n65.insert"]["xa"]) == 70
    for name in ("n65.window", "n257.window", "all130.window"):  # a deleted window costs native contacts: 0 < fnat(penalise) < fnat(ignore)
        v = c[name]
        pen = mr.mapped_all(v["xa"], v["xb"], v["sides"], v["m"], coverage="penalise", **mr.case_kw(v))
        ign = mr.mapped_all(v["xa"], v["xb"], v["sides"], v["m"], coverage="ignore", **mr.case_kw(v))
        assert pen["n_native"][0] > ign["n_native"][0] > 0 and 0 < pen["fnat"][0] < ign["fnat"][0], name


@pytest.mark.parametrize("coverage", ["ignore", "penalise"])
def test_an_identity_map_reproduces_the_unmapped_restatement(coverage):
    c = mr.cases()["n65.backbone"]
    xg, rows, _ = mr.gathered_model(c["xa"], c["m"])
    xg = np.where(rows[:, None, None] != 0, xg, c["xb"])  # a model in the reference's rows, every row present
    got = mr.mapped_all(xg, c["xb"], c["sides"], np.arange(65), c["mode"], coverage)
    _equal(got, ir.interface_all(xg, c["xb"], c["sides"], c["mode"]), ALL_OUTPUTS)
    assert got["n_covered"] == got["n_reference"] == 65 and np.array_equal(got["n_interface_covered"], got["n_interface_rows"])


def _two_chains():
    """Two 6-row CA chains with 4 native contacts at the 8 A cutoff: ligand row 6 touches receptor rows 0 and 1, row 7 touches row 3, row
    8 touches row 5; ligand rows 9 .. 11 are far away."""
    receptor = np.array([[10.0 * i, 0.0, 0.0] for i in range(6)])
    ligand = np.array([[5.0, 5.0, 0.0], [30.0, 5.0, 0.0], [50.0, 5.0, 0.0], [0.0, 100.0, 0.0], [20.0, 100.0, 0.0], [40.0, 100.0, 0.0]])
    x = np.concatenate([receptor, ligand]).astype(np.float32)
    x[0] += np.float32(0.5)  # (no atom at the origin: a zero coordinate triple means "absent")
    return x, np.array([1] * 6 + [2] * 6, dtype=np.int32)


def test_a_deleted_ligand_row_costs_its_native_contacts_under_penalise():
    x, side = _two_chains()
    assert ir.interface_one(x, x, side, "ca")["n_native"] == 4
    xa = np.delete(x, 6, axis=0)  # the model lacks ligand row 6, which carries 2 of the 4 contacts
    m = np.array([0, 1, 2, 3, 4, 5, -1, 6, 7, 8, 9, 10])
    ign, pen = mr.mapped_one(xa, x, side, m, "ca", "ignore"), mr.mapped_one(xa, x, side, m, "ca", "penalise")
    assert (ign["n_native"], ign["n_shared"], ign["fnat"]) == (2, 2, 1.0)
    assert (pen["n_native"], pen["n_model"], pen["n_shared"], pen["fnat"]) == (4, 2, 2, 0.5)
    assert pen["res_native"].tolist() == [1, 1, 0, 1, 0, 1, 2, 1, 1, 0, 0, 0] and pen["res_shared"][6] == 0
    assert pen["interface_rows"][6] and pen["n_interface_covered"] == pen["n_interface_rows"] - 1
    assert ign["n_covered"] == pen["n_covered"] == 11 and pen["n_reference"] == 12


@pytest.mark.parametrize("coverage", ["ignore", "penalise"])
def test_a_model_with_its_chains_in_the_opposite_order_scores_as_the_ordered_one(coverage):
    x, side = _two_chains()
    rng = np.random.RandomState(3)
    xa = (x + rng.normal(0, 0.7, x.shape)).astype(np.float32)
    ordered = mr.mapped_one(xa, x, side, np.arange(12), "ca", coverage)
    swapped = mr.mapped_one(np.concatenate([xa[6:], xa[:6]]), x, side, np.concatenate([np.arange(6, 12), np.arange(6)]), "ca", coverage)
    for k in mr.INT_OUTPUTS + ir.ROW_OUTPUTS + ir.FLOAT_OUTPUTS:
        assert np.array_equal(np.asarray(ordered[k]), np.asarray(swapped[k]), equal_nan=True), k
    assert 0 < ordered["n_native"] and ordered["irmsd"] > 0


def test_global_dockq_on_hand_made_results():
    from framedipt_amd import interface
    nan = np.nan
    result = dict(dockq=np.array([[0.9, 0.5, nan], [nan, nan, nan], [0.2, nan, 0.4]]), n_native=np.array([[3, 1, 0], [0, 0, 0], [2, 5, 1]]))
    assert interface.global_dockq(result, 0) == pytest.approx(0.7)  # the interface without a native contact is left out
    assert np.isnan(interface.global_dockq(result, 1))  # no interface has a native contact
    assert interface.global_dockq(result, 2) == pytest.approx(0.3)  # no alignment: a NaN is left out
    assert interface.global_dockq(dict(result, coverage_mode="ignore"), 2) == pytest.approx(0.3)
    assert interface.global_dockq(dict(result, coverage_mode="penalise"), 2) == pytest.approx(0.2)  # ... and counts as 0 under penalise
    assert interface.global_dockq(dict(result, coverage_mode="penalise"), 0) == pytest.approx(0.7)
    only_nan = dict(dockq=np.array([[nan]]), n_native=np.array([[2]]))
    assert np.isnan(interface.global_dockq(only_nan, 0)) and interface.global_dockq(dict(only_nan, coverage_mode="penalise"), 0) == 0.0


def test_errors_raised_before_the_library_is_loaded():
    from framedipt_amd import interface
    xa, xb = np.ones((1, 7, 5, 3), dtype=np.float32), np.ones((1, 9, 5, 3), dtype=np.float32)
    sides, m = np.array([1] * 4 + [2] * 5), np.array([0, 1, 2, 3, 4, 5, 6, -1, -1])
    with pytest.raises(ValueError, match="alignment.*prot_b is required"):
        interface.interface_accuracy(xa, None, sides[:7], alignment=m[:7])
    with pytest.raises(ValueError, match="coverage.*alignment"):
        interface.interface_accuracy(xa, xa, sides[:7], coverage="penalise")
    with pytest.raises(ValueError, match="coverage should be"):
        interface.interface_accuracy(xa, xb, sides, alignment=m, coverage="strict")
    with pytest.raises(ValueError, match=r"sides should be \[I, 9\]"):
        interface.interface_accuracy(xa, xb, sides[:7], alignment=m)
    for bad in (m[:7], np.stack([m, m]), m.astype(np.float32)):
        with pytest.raises(ValueError, match="alignment should be integers"):
            interface.interface_accuracy(xa, xb, sides, alignment=bad)
    with pytest.raises(ValueError, match="row map 0 of 1: an entry outside -1 .. 6"):
        interface.interface_accuracy(xa, xb, sides, alignment=np.where(m == 6, 7, m))
    with pytest.raises(ValueError, match="a model row used twice"):
        interface.interface_accuracy(xa, xb, sides, alignment=np.where(m == 6, 5, m))
    with pytest.raises(ValueError, match="res_mask_b .* expected \\(1, 9\\)"):
        interface.interface_accuracy(xa, xb, sides, alignment=m, res_mask_b=np.ones((1, 7)))
    with pytest.raises(ValueError, match="prot_b .* does not have the 7 rows"):  # (without an alignment the rows must correspond, as before)
        interface.interface_accuracy(xa, xb, sides[:7])
