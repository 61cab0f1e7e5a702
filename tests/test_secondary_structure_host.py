"""CPU tests of the secondary-structure contract through its NumPy restatement tests/dssp_ref.py: ideal
backbones whose classes follow from the definitions, the annotation deposited with the reference's three test complexes
(tests/golden/dssp_cases.npz), and the corner rules one by one.  ``pytest tests/test_secondary_structure_host.py -s`` prints the
measured agreement figures next to their floors."""
import functools

import numpy as np
import pytest

import dssp_ref as dr
from conftest import load_golden


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("dssp_cases.npz")


@functools.lru_cache(maxsize=None)
def _stated(name, bulges=True):
    return dr.dssp(**dr.case_inputs(_fix(), name), bulges=bulges)


@pytest.mark.parametrize("name", list(dr.IDEAL))
def test_ideal_backbone(name):
    phi, psi, want = dr.IDEAL[name]
    got = dr.dssp(dr.ideal_backbone(20, phi, psi))
    assert dr.ss_string(got["ss"]) == want
    evaluated = got["raw_energy"][got["valid"]]
    print(f"{name}: nearest energy to the -0.5 threshold at {np.abs(evaluated - dr.E_BOND).min():.3f} kcal/mol")
    assert np.abs(evaluated - dr.E_BOND).min() > 0.05  # not knife-edge


@pytest.mark.parametrize("name", dr.COMPLEXES)
def test_complex_agrees_with_its_deposited_annotation(name):
    """Floors of the specification: three-class agreement >= 0.94, no helix <-> strand confusion, helix and strand fractions within 0.04 of the
    deposited ones."""
    got, label = _stated(name), _fix()[f"{name}.label"]
    ss = got["ss"]
    assert len(ss) == len(label) == got["n_rows"]
    agree = float((ss == label).mean())
    confusions = int(((ss == dr.HELIX) & (label == dr.STRAND)).sum() + ((ss == dr.STRAND) & (label == dr.HELIX)).sum())
    helix, strand = float((label == dr.HELIX).mean()), float((label == dr.STRAND).mean())
    print(f"{name}: n = {got['n_rows']}, agreement {agree:.3f} (floor 0.94), H<->E confusions {confusions}, helix {got['helix_percent']:.3f} "
          f"against {helix:.3f} deposited, strand {got['strand_percent']:.3f} against {strand:.3f} deposited")
    assert agree >= 0.94 and confusions == 0
    assert abs(got["helix_percent"] - helix) <= 0.04 and abs(got["strand_percent"] - strand) <= 0.04
    without = float((_stated(name, False)["ss"] == label).mean())
    print(f"{name}: agreement without the bulge pass {without:.3f}")
    assert without < agree  # the yardstick sees the bulge rule


def test_fixture_cases_are_decidable_and_within_the_bridge_slots():
    """What the generator asserted, on the committed file: 1000 E at least 1e-6 from a half-integer in every case, no excerpt changes a
    class under the recorded motion; and the capacity the kernel relies on: no row holds more bridges than the header's slots."""
    from framedipt_amd import _lib
    fix = _fix()
    assert _lib.DSSP_BRIDGES_PER_ROW == dr.SLOTS_PER_ROW == 8
    assert (_lib.DSSP_COIL, _lib.DSSP_HELIX, _lib.DSSP_STRAND, _lib.DSSP_ABSENT) == (dr.COIL, dr.HELIX, dr.STRAND, dr.ABSENT) == (0, 1, 2, 255)
    assert (_lib.DSSP_BRIDGE_OVERFLOW, _lib.DSSP_LADDER_OVERFLOW) == (1, 2)
    names = dr.case_names(fix)
    assert set(dr.COMPLEXES) <= set(names) and {"anti", "bulge", "helix", "boundary"} <= set(names)
    for name in names:
        got = _stated(name)
        assert got["half_margin"] > 1e-6 and got["half_margin"] == fix[f"{name}.half_margin"], name
        assert name in dr.COMPLEXES or fix[f"{name}.class_changes"] == 0, name
        assert got["bridges_per_row"].max(initial=0) <= dr.SLOTS_PER_ROW and got["n_ladders"] <= got["n_bridges"], name
        moved = dr.dssp(fix[f"{name}.bb"].astype(np.float64) @ fix["motion.rot"].T + fix["motion.shift"], None, fix[f"{name}.chain_idx"],
                        fix[f"{name}.is_proline"])
        assert int((moved["ss"] != got["ss"]).sum()) == fix[f"{name}.class_changes"], name
    assert len(fix["anti.bb"]) <= 40 and _stated("anti")["n_bridges"] >= 4 and len(set(fix["boundary.chain_idx"].tolist())) == 2


def test_bulge_pass_changes_classes():
    with_pass, without = _stated("bulge"), _stated("bulge", False)
    changed = with_pass["ss"] != without["ss"]
    assert changed.any() and (with_pass["ss"][changed] == dr.STRAND).all() and (without["ss"][changed] == dr.COIL).all()
    assert with_pass["n_ladders"] < without["n_ladders"] and with_pass["n_bridges"] == without["n_bridges"]


def test_rounding_is_half_away_from_zero():
    """-0.0625 and -0.5625 kcal/mol are 62.5 and 562.5 thousandths exactly: C ``round`` gives 63 and 563, NumPy's half-to-even 62."""
    assert np.round(-62.5) == -62 and np.round(-562.5) == -562
    assert dr.round_energy([-0.0625, -0.5625, 0.0625, -0.0624, -20.0]).tolist() == [-0.063, -0.563, 0.063, -0.062, -9.9]
    assert dr.round_half_away([0.5, -0.5, 1.5, 2.5, -2.5, 2.4999]).tolist() == [1, -1, 2, 3, -3, 2]


def test_third_acceptor_does_not_bond():
    bb, chain = dr.three_acceptor_case()
    got = dr.dssp(bb, None, chain)
    raw = got["raw_energy"][1]
    assert (raw[2:] < dr.E_BOND).all() and raw[2] < raw[3] < raw[4]  # three acceptors below -0.5
    assert got["acceptor"][1].tolist() == [2, 3] and got["acceptor_energy"][1].tolist() == [-2.053, -1.832]
    assert got["hb"][1].tolist() == [False, False, True, True, False] and got["n_hbonds"] == 2


def test_proline_donates_nothing():
    phi, psi, _ = dr.IDEAL["alpha"]
    bb = dr.ideal_backbone(20, phi, psi)
    pro = np.zeros(20, dtype=np.uint8)
    pro[10] = 1
    plain, got = dr.dssp(bb), dr.dssp(bb, is_proline=pro)
    assert plain["acceptor"][10, 0] == 6 and plain["acceptor_energy"][10, 0] < dr.E_BOND <= plain["acceptor_energy"][10, 1]
    assert got["acceptor"][10].tolist() == [-1, -1] and not got["acceptor_energy"][10].any()
    assert got["n_hbonds"] == plain["n_hbonds"] - 1 and np.array_equal(np.delete(got["acceptor"], 10, 0), np.delete(plain["acceptor"], 10, 0))
    assert not got["turns"][4][6] and plain["turns"][4][6]


def test_masked_and_origin_rows_are_as_if_removed():
    inp = dr.case_inputs(_fix(), "anti")
    n = len(inp["bb"])
    keep = np.sort(np.random.default_rng(5).choice(n + 6, size=n, replace=False))  # the rows of the case among n + 6
    bb = np.random.default_rng(6).normal(size=(n + 6, 4, 3)).astype(np.float32) * 30
    chain, pro, mask = np.full(n + 6, 9, dtype=np.int32), np.ones(n + 6, dtype=np.uint8), np.ones(n + 6, dtype=np.float32)
    bb[keep], chain[keep], pro[keep] = inp["bb"], inp["chain_idx"], inp["is_proline"]
    holes = np.setdiff1d(np.arange(n + 6), keep)
    mask[holes[:3]] = 0        # masked rows that hold garbage
    bb[holes[3:5]] = 0         # rows at the origin
    bb[holes[5], 2] = 0        # one atom (C) at the origin: the row is absent too
    got, want = dr.dssp(bb, mask, chain, pro), _stated("anti")
    assert (got["ss"][holes] == dr.ABSENT).all() and np.array_equal(got["ss"][keep], want["ss"])
    assert np.array_equal(got["acceptor_energy"][keep], want["acceptor_energy"]) and not got["acceptor_energy"][holes].any()
    assert np.array_equal(got["acceptor"][keep], np.where(want["acceptor"] >= 0, keep[np.maximum(want["acceptor"], 0)], -1))
    for k in ("n_rows", "n_hbonds", "n_bridges", "n_ladders") + dr.FRACTIONS:
        assert got[k] == want[k], k


def test_no_row_gives_nan():
    got = dr.dssp(np.zeros((7, 4, 3), dtype=np.float32))
    assert got["n_rows"] == 0 and (got["ss"] == dr.ABSENT).all() and all(np.isnan(got[k]) for k in dr.FRACTIONS)


def test_python_helpers():
    """``shape_metrics`` and ``region_counts`` of framedipt_amd/secondary_structure.py on a result dict."""
    from framedipt_amd import secondary_structure as sec
    ss = np.array([[0, 1, 1, 2, 255, 2, 0, 0]], dtype=np.uint8)
    result = {"ss": ss, "non_coil_percent": np.array([4 / 7]), "coil_percent": np.array([3 / 7]), "helix_percent": np.array([2 / 7]),
              "strand_percent": np.array([2 / 7])}
    assert list(sec.shape_metrics(result, 0)) == ["non_coil_percent", "coil_percent", "helix_percent", "strand_percent"]
    assert sec.shape_metrics(result, 0)["helix_percent"] == 2 / 7
    assert sec.region_counts(result, 0, [(0, 2), (5, 7)]) == (3, 2, 1) and sec.region_counts(result, 0, [(3, 4)]) == (0, 0, 1)
    assert sec.region_counts(result, 0, []) == (0, 0, 0) and sec.PRO == 14
