"""CPU tests of DESIGN.md section 7.11 (per-row controls, tied positions, the probability modes): the float64 restatement
(tests/mpnn_controls_ref.py) against the reference's recorded outputs (tests/golden/mpnn_ctl_<case>.npz) and the host side of
framedipt_amd/inverse_folding.py (order flattening, the refused groups, the log-odds mask, the homo-oligomer helper)."""
import functools

import numpy as np
import pytest
import torch

import mpnn_controls_ref as cr
import mpnn_ref as mr
from conftest import load_golden
from framedipt_amd import inverse_folding as inv


@functools.lru_cache(maxsize=None)
def fixture_and_restatement(name):
    fix = dict(load_golden(f"mpnn_ctl_{name}.npz"))
    fix["groups"] = cr.unpack_groups(fix["groups"])
    return fix, cr.run_case(inv.synthetic_state_dict(mr.WEIGHT_SEED, cr.CASES[name][2]), name, fix)


@pytest.mark.parametrize("name", ["p", "q", "r"])
def test_restatement_of_design_matches_the_reference(name):
    """Letters exactly on every row with res_mask, probs within four times the recorded deviation on the designed rows (tied_sample
    stores the distribution of a fixed untied row, this project zeros: asserted), and the fixture conditions hold on the recorded inputs."""
    fix, res = fixture_and_restatement(name)
    b, n, k = cr.CASES[name]
    valid = np.broadcast_to((fix["res_mask"] != 0)[:, None], (b, mr.M, n))
    designed = np.broadcast_to((fix["res_mask"] * fix["chain_mask"] != 0)[:, None], (b, mr.M, n))
    assert res["gap"][fix["res_mask"] != 0].min() >= 1e-3
    for t, d in res["design"].items():
        assert d["margin"] >= 1e-4 and not d["no_letter"]
        assert np.array_equal(fix[f"S_T{t}"][valid], d["S"][valid])
        dev = np.abs(fix[f"probs_T{t}"] - d["probs"])[designed].max()
        print(f"case {name} T={t}: probs deviation {dev:.3e} (bound {cr.bound('probs'):.3e})")
        assert dev <= cr.bound("probs")
        assert not d["probs"][~designed].any()
    # the recorded flattened order is the host's, and the host's tie ids are the fixture's
    tie, groups = inv.tie_groups(fix["groups"], b, n, fix["res_mask"], fix["chain_mask"])
    assert np.array_equal(tie, fix["tie_group"]) and groups == fix["groups"]
    for i in range(b):
        for m in range(mr.M):
            assert np.array_equal(inv.flatten_decoding_order(fix["drawn_order"][i, m], groups[i]), fix["decoding_order"][i, m])
            assert np.array_equal(cr.flatten(fix["drawn_order"][i, m], groups[i]), fix["decoding_order"][i, m])
            assert sorted(fix["decoding_order"][i, m]) == list(range(n))


def test_restatement_of_the_probability_modes_matches_the_reference():
    fix, res = fixture_and_restatement("s")
    valid, rows = fix["res_mask"] != 0, fix["chain_mask"] * fix["res_mask"] != 0
    assert rows.sum() == 9
    for key, what in (("unconditional", "unconditional"), ("conditional", "conditional"), ("conditional_backbone", "conditional")):
        dev = np.abs(fix[key] - res[key])[valid].max()
        print(f"case s {key}: deviation {dev:.3e} (bound {cr.bound(what):.3e})")
        assert dev <= cr.bound(what)
    for key in ("conditional", "conditional_backbone"):
        assert not fix[key][~rows].any() and not res[key][~rows].any() and fix[key][rows].all()
    # backbone_only: row i is decoded first, so nothing counts as decoded for it - the unconditional row
    assert np.abs(res["conditional_backbone"] - res["unconditional"])[rows].max() <= 1e-12
    assert np.abs(res["conditional"] - res["unconditional"])[rows].max() > 1e-3
    # native_scores: the mean negative log-probability of the letters over the mask
    want = -np.mean([res["conditional"][0, r, fix["S"][0, r]] for r in np.flatnonzero(rows[0])])
    assert np.allclose(inv.native_scores(res["conditional"], fix["S"], rows), [want], rtol=1e-6)


def test_the_cases_hold_what_they_are_for():
    p, q, r = (fixture_and_restatement(name)[0] for name in "pqr")
    assert set(p["chain_idx"][0]) == {1, 2} and all(key in p for key in cr.CONTROL_KEYS) and not p["groups"][0]
    assert sorted(len(g) for g in q["groups"][0]) == [2, 2, 3] and sorted(q["tied_beta"][0, [10, 11]]) == [0.5, 1.5]
    assert cr.mutual_pair(fixture_and_restatement("q")[1]["E_idx"][0], q["groups"][0]) == (10, 11)
    assert q["groups"][0][1] == [33, 5, 20]                                             # a listed order that is not ascending
    assert (1 - q["omit_mask"][0, 25]).nonzero()[0].tolist() == [7]                     # one letter left at row 25 ...
    assert (q["S_T1.0"][0, :, 25] == 7).all() and (fixture_and_restatement("q")[1]["design"][1.0]["S"][0, :, 25] == 7).all()   # ... and drawn
    assert (q["S_T1.0"][0, :, [33, 5, 20]] >= 10).all()                                 # the last member's omit mask binds its group
    assert r["groups"][0] == [g for g in inv.tied_positions_from_chains(r["chain_idx"][0], r["res_mask"][0]) if r["chain_mask"][0, g].all()]
    assert all(r["chain_idx"][0, g[0]] != r["chain_idx"][0, g[1]] for g in r["groups"][0]) and len(r["groups"][0]) == 28   # groups span the chains
    assert r["groups"][0] != r["groups"][1] and (r["res_mask"] == 0).sum(-1).tolist() == [4, 2] and (r["chain_mask"] == 0).sum(-1).tolist() == [10, 5]
    for name, fix in (("q", q), ("r", r)):
        for t in cr.TEMPERATURES[name]:
            for i, groups in enumerate(fix["groups"]):
                for g in groups:
                    assert (fix[f"S_T{t}"][i][:, g] == fix[f"S_T{t}"][i][:, g[:1]]).all()                 # one letter per group
                    assert np.array_equal(fix[f"probs_T{t}"][i][:, g[0]], fix[f"probs_T{t}"][i][:, g[-1]])  # and one distribution


def test_order_flattening_on_hand_made_examples():
    # a group hit through its second member is emitted whole, in its listed order, where that member stood
    assert inv.flatten_decoding_order([4, 2, 0, 1, 3, 5], [[0, 2]]).tolist() == [4, 0, 2, 1, 3, 5]
    assert inv.flatten_decoding_order([4, 2, 0, 1, 3, 5], [[2, 0]]).tolist() == [4, 2, 0, 1, 3, 5]
    # two groups interleaved in the drawn order: each comes out whole at its first drawn member
    assert inv.flatten_decoding_order([1, 6, 3, 0, 4, 2, 5], [[0, 1, 2], [3, 4]]).tolist() == [0, 1, 2, 6, 3, 4, 5]
    assert inv.flatten_decoding_order([5, 4, 3, 2, 1, 0], []).tolist() == [5, 4, 3, 2, 1, 0]
    for order, groups in (([4, 2, 0, 1, 3, 5], [[0, 2]]), ([1, 6, 3, 0, 4, 2, 5], [[0, 1, 2], [3, 4]])):
        assert np.array_equal(cr.flatten(order, groups), inv.flatten_decoding_order(order, groups))


def test_groups_that_are_refused_name_their_row():
    ones = np.ones((2, 8), np.float32)
    tie, groups = inv.tie_groups([[0, 3], [5, 1, 2]], 2, 8, ones, ones)                 # one list serves both backbones
    assert tie.tolist() == [[0, 1, 1, 0, -1, 1, -1, -1]] * 2 and groups == [[[0, 3], [5, 1, 2]]] * 2 and tie.dtype == np.int32
    tie, groups = inv.tie_groups([[[0, 3]], []], 2, 8, ones, ones)                      # or one list per backbone
    assert tie.tolist() == [[0, -1, -1, 0, -1, -1, -1, -1], [-1] * 8] and groups == [[[0, 3]], []]
    assert (inv.tie_groups(None, 2, 8, ones, ones)[0] == -1).all()
    masked, fixed = ones.copy(), ones.copy()
    masked[1, 3], fixed[0, 5] = 0, 0
    with pytest.raises(ValueError, match="backbone 1, group 0: row 3 has no res_mask"):
        inv.tie_groups([[0, 3]], 2, 8, masked, ones)
    with pytest.raises(ValueError, match="row 5 is fixed"):
        inv.tie_groups([[0, 3], [5, 1]], 2, 8, ones, fixed)
    with pytest.raises(ValueError, match="row 3 is in two groups"):
        inv.tie_groups([[0, 3], [3, 4]], 2, 8, ones, ones)
    with pytest.raises(ValueError, match="row 2 is in two groups"):
        inv.tie_groups([[2, 2]], 2, 8, ones, ones)
    with pytest.raises(ValueError, match=r"a group of one \(row 6\)"):
        inv.tie_groups([[0, 3], [6]], 2, 8, ones, ones)
    with pytest.raises(ValueError, match="row 8 outside 0 .. 7"):
        inv.tie_groups([[0, 8]], 2, 8, ones, ones)
    with pytest.raises(ValueError, match="row -1 outside"):
        inv.tie_groups([[[0, 1]], [[-1, 2]]], 2, 8, ones, ones)
    with pytest.raises(ValueError, match="one such list for each of the 2 backbones"):
        inv.tie_groups([[[0, 1]], [[1, 2]], [[3, 4]]], 2, 8, ones, ones)


def test_log_odds_mask_and_threshold():
    odds = np.array([[-1.0, 0.0, 0.5, 2.0]])
    assert inv.log_odds_mask(odds).tolist() == [[0.0, 0.0, 1.0, 1.0]] and inv.log_odds_mask(odds).dtype == np.float32
    assert inv.log_odds_mask(odds, 0.5).tolist() == [[0.0, 0.0, 0.0, 1.0]] and inv.log_odds_mask(odds, -2.0).tolist() == [[1.0] * 4]


def test_tied_positions_from_chains():
    assert inv.tied_positions_from_chains([1, 1, 1, 2, 2, 2, 7, 7, 7]) == [[0, 3, 6], [1, 4, 7], [2, 5, 8]]
    assert inv.tied_positions_from_chains([1, 1, 1, 2, 2, 2], [1, 1, 0, 1, 0, 1]) == [[0, 3], [1, 5]]       # rows without res_mask drop out
    assert inv.tied_positions_from_chains(np.array([[1, 1, 2, 2], [3, 3, 3, 3]])) == [[[0, 2], [1, 3]], []]  # per backbone; one chain: no ties
    with pytest.raises(ValueError, match=r"chains of lengths \[2, 3\]"):
        inv.tied_positions_from_chains([1, 1, 1, 2, 2])
    tie, _ = inv.tie_groups(inv.tied_positions_from_chains([1] * 3 + [2] * 3), 1, 6, np.ones((1, 6)), np.ones((1, 6)))
    assert tie.tolist() == [[0, 1, 2, 0, 1, 2]]


def test_an_omit_mask_that_leaves_one_letter_yields_it_and_none_leaves_the_input():
    """The epilogue of the restatement alone: whatever the logits and the uniform, one letter left is the letter drawn; no letter left
    is reported and gives zeros."""
    model = mr.Model(inv.synthetic_state_dict(mr.WEIGHT_SEED, 48), 48, torch.float64)
    omit, bias = mr.omit_bias()
    z = torch.linspace(-3.0, 3.0, 21, dtype=torch.float64)
    om = np.ones((2, 21), np.float32)
    om[0, 13] = 0.0
    ctl = {"omit": omit, "bias": bias, "temperature": 0.7, "omit_mask": om}
    p, left = cr.epilogue(model, z, 0, ctl)
    assert left and p[13] == 1.0 and p.sum() == 1.0 and all(mr.pick(p, u)[0] == 13 for u in (0.0, 0.5, 0.999999))
    p, left = cr.epilogue(model, z, 1, ctl)
    assert not left and not p.any()
    # the log-odds stage keeps a thousandth of the letters it masks: [p0 1.001, p1 0.001] / sum
    ctl = {"omit": np.zeros(21, np.float32), "bias": np.zeros(21, np.float32), "temperature": 1.0, "pssm_coef": np.ones(1), "pssm_multi": 0.0,
           "pssm_log_odds_mask": np.array([[1.0] + [0.0] * 20], np.float32)}
    p, left = cr.epilogue(model, torch.zeros(21, dtype=torch.float64), 0, ctl)
    assert left and np.isclose(float(p[0]), 1.001 / (1.001 + 20 * 0.001)) and np.isclose(float(p[1]), 0.001 / (1.001 + 20 * 0.001))
