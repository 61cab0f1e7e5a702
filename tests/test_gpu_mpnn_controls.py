"""GPU tests (-m gpu) of DESIGN.md section 7.11: the per-row controls of the sampling epilogue, tied positions and the two probability
modes (framedipt_amd/inverse_folding.py -> fdipt_mpnn_design / fdipt_mpnn_score, csrc/mpnn.hip) against the reference's recorded outputs
(tests/golden/mpnn_ctl_<case>.npz) and the float64 restatement (tests/mpnn_controls_ref.py).  The tolerance is four times the deviation
of the reference's float32 outputs from the restatement (mpnn_controls_ref.DEVIATION); letters, orders, tie ids and status compare
exactly.  ``-s`` prints the device's figures next to the bounds."""
import functools

import numpy as np
import pytest
import torch

import mpnn_controls_ref as cr
import mpnn_ref as mr
from conftest import load_golden
from framedipt_amd import _lib
from framedipt_amd import inverse_folding as inv

pytestmark = pytest.mark.gpu
ROWS = ("res_mask", "chain_mask", "residue_index", "chain_idx")


@functools.lru_cache(maxsize=None)
def _model(k):
    return inv.ProteinMPNN(k).load_synthetic(mr.WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def _fix(name):
    fix = load_golden(f"mpnn_ctl_{name}.npz")
    fix["groups"] = cr.unpack_groups(fix["groups"])
    return fix


def _design_kw(fix, b=slice(None)):
    """design's keyword arguments for the backbones ``b`` of a fixture: its rows, controls, ties, drawn orders and uniforms."""
    _, bias = mr.omit_bias()
    kw = {k: fix[k][b] for k in ROWS}
    kw.update({k: fix[k][b] for k in cr.CONTROL_KEYS + ("tied_beta",) if k in fix})
    if "pssm_bias" in fix:
        kw.update(pssm_multi=cr.PSSM_MULTI, pssm_threshold=cr.PSSM_THRESHOLD)
    if any(fix["groups"]):
        kw["tied_positions"] = fix["groups"][b]
    return dict(kw, num_seq=mr.M, aatype=inv.mpnn_to_aatype(fix["S"][b]), omit="X", bias=bias, decoding_order=fix["drawn_order"][b], u=fix["u"][b])


@functools.lru_cache(maxsize=None)
def _design(name, t):
    fix = _fix(name)
    return _model(cr.CASES[name][2]).design(fix["prot"], temperature=t, **_design_kw(fix))


@pytest.mark.parametrize("name,t", [(name, t) for name in cr.TEMPERATURES for t in cr.TEMPERATURES[name]])
def test_design_matches_the_reference(name, t):
    fix, got = _fix(name), _design(name, t)
    b, n, _ = cr.CASES[name]
    designed = np.broadcast_to((fix["res_mask"] * fix["chain_mask"] != 0)[:, None], (b, mr.M, n))
    assert np.array_equal(got["decoding_order"], fix["decoding_order"]) and np.array_equal(got["tie_group"], fix["tie_group"])
    differ = int((got["S"] != fix[f"S_T{t}"]).sum())
    err = np.abs(got["probs"] - fix[f"probs_T{t}"])[designed].max()
    print(f"case {name} T={t}: {differ} letters differ, probs error {err:.3e} (bound {cr.bound('probs'):.3e})")
    assert differ == 0
    assert err <= cr.bound("probs")
    S_in = np.repeat(fix["S"][:, None], mr.M, axis=1)
    assert np.array_equal(got["S"][~designed], S_in[~designed]) and not got["probs"][~designed].any()   # fixed and masked rows, tied run or not
    assert got["status"].tolist() == [0] * b and np.isfinite(got["score"]).all()
    for i, groups in enumerate(fix["groups"]):                                          # one letter and one distribution per group
        for g in groups:
            assert (got["S"][i][:, g] == got["S"][i][:, g[:1]]).all()
            assert all(np.array_equal(got["probs"][i][:, r], got["probs"][i][:, g[0]]) for r in g)
    # the rescoring is the score entry on the flattened order
    sc = _model(cr.CASES[name][2]).score(fix["prot"], got["S"], decoding_order=got["decoding_order"], **{k: fix[k] for k in ROWS})
    assert np.array_equal(sc["log_probs"], got["log_probs"])


def test_probability_modes_match_the_reference():
    fix, model = _fix("s"), _model(48)
    rows = {k: fix[k] for k in ROWS}
    valid, chosen = fix["res_mask"] != 0, fix["chain_mask"] * fix["res_mask"] != 0
    unc = model.unconditional_probs(fix["prot"], **{k: v for k, v in rows.items() if k != "chain_mask"})
    err = np.abs(unc["log_probs"] - fix["unconditional"])[valid].max()
    print(f"unconditional: error {err:.3e} (bound {cr.bound('unconditional'):.3e})")
    assert unc["log_probs"].shape == (1, 24, 21) and err <= cr.bound("unconditional") and unc["status"].tolist() == [0]
    got = {}
    for key, flag in (("conditional", False), ("conditional_backbone", True)):
        got[key] = model.conditional_probs(fix["prot"], fix["S"], backbone_only=flag, randn=fix["cond_randn"], **rows)
        err = np.abs(got[key]["log_probs"] - fix[key])[valid].max()
        print(f"{key}: error {err:.3e} (bound {cr.bound('conditional'):.3e})")
        assert err <= cr.bound("conditional") and not got[key]["log_probs"][~chosen].any() and np.array_equal(got[key]["randn"], fix["cond_randn"])
    # row i decoded first sees nothing decoded: the unconditional row
    err = np.abs(got["conditional_backbone"]["log_probs"] - unc["log_probs"])[chosen].max()
    print(f"conditional(backbone_only) against unconditional on the device: {err:.3e}")
    assert err <= cr.bound("conditional")
    seeded = model.conditional_probs(fix["prot"], fix["S"], seed=4, **rows)
    again = model.conditional_probs(fix["prot"], fix["S"], randn=seeded["randn"], **rows)
    assert np.array_equal(seeded["log_probs"], again["log_probs"]) and not np.array_equal(seeded["randn"], fix["cond_randn"])
    score = inv.native_scores(got["conditional"]["log_probs"], fix["S"], chosen)
    assert score.shape == (1,) and np.isclose(score[0], -np.mean([got["conditional"]["log_probs"][0, r, fix["S"][0, r]] for r in np.flatnonzero(chosen[0])]))


def test_more_rows_with_chain_mask_than_one_call_takes():
    """70 chosen rows: conditional_probs goes through the score entry in two chunks (64 orders at most per call); each row is the row of
    its own order, whichever chunk it falls in."""
    fix, model = _fix("r"), _model(48)
    rows = {k: fix[k][:1] for k in ROWS}
    rows["chain_mask"] = np.ones((1, 70), np.float32)
    randn = np.random.default_rng(3).standard_normal((1, 70)).astype(np.float32)
    got = model.conditional_probs(fix["prot"][:1], fix["S"][:1], randn=randn, **rows)
    chosen = np.flatnonzero(fix["res_mask"][0])
    assert len(chosen) == 66 > inv.MAX_SEQ
    orders = cr.conditional_orders(randn[0], chosen[[0, 65]], 70, False)
    sc = model.score(fix["prot"][:1], np.repeat(fix["S"][:1, None], 2, axis=1), decoding_order=orders[None], **rows)
    assert np.array_equal(got["log_probs"][0, chosen[0]], sc["log_probs"][0, 0, chosen[0]])
    assert np.array_equal(got["log_probs"][0, chosen[65]], sc["log_probs"][0, 1, chosen[65]])
    assert got["log_probs"][0, chosen].all() and not got["log_probs"][0, fix["res_mask"][0] == 0].any()


def test_neutral_controls_keep_every_bit():
    """bias_by_res of zeros, an empty list of ties (tie_group all -1 on the device), no PSSM and no omit mask: S, probs and log_probs are
    those of the call without them, bit for bit."""
    fix, model = load_golden("mpnn_b.npz"), _model(48)
    _, bias = mr.omit_bias()
    kw = dict(num_seq=mr.M, temperature=0.1, aatype=inv.mpnn_to_aatype(fix["S"]), omit="X", bias=bias, decoding_order=fix["decoding_order"], u=fix["u"],
              **{k: fix[k] for k in ROWS})
    plain = model.design(fix["prot"], **kw)
    neutral = model.design(fix["prot"], bias_by_res=np.zeros((2, 70, 21), np.float32), tied_positions=[], tied_beta=np.ones((2, 70), np.float32), **kw)
    assert np.array_equal(plain["S"], fix["S_T0.1"])
    for key in ("S", "probs", "log_probs", "decoding_order", "status"):
        assert np.array_equal(plain[key], neutral[key]), key
    assert (neutral["tie_group"] == -1).all() and (plain["tie_group"] == -1).all()


def test_results_do_not_depend_on_the_batch():
    """Case r's two backbones (different ties, masks and fixed rows) together against each alone."""
    fix, model, pair = _fix("r"), _model(48), _design("r", 1.0)
    for i in range(2):
        alone = model.design(fix["prot"][i:i + 1], temperature=1.0, **_design_kw(fix, slice(i, i + 1)))
        for key in ("S", "probs", "log_probs", "decoding_order", "tie_group"):
            assert np.array_equal(alone[key][0], pair[key][i]), (i, key)


def _restated(prot, S_in, residue_index, chain_idx, groups, drawn, u, t, tied_beta=None):
    """The float64 restatement of a tied design of one backbone with every row designed: per sequence S, probs, margin."""
    n = len(S_in)
    ones = np.ones(n, np.float32)
    omit, bias = mr.omit_bias()
    ref = mr.Model(inv.synthetic_state_dict(mr.WEIGHT_SEED, 48), 48, torch.float64)
    enc = mr.encode(ref, prot, ones, residue_index, chain_idx)
    ctl = {"omit": omit, "bias": bias, "temperature": t}
    tie = cr.tie_group_of(groups, n)
    return enc, [cr.design(ref, enc, ones, ones, S_in, cr.flatten(drawn[m], groups), u[m], ctl, tie, tied_beta) for m in range(len(drawn))]


def _check_against_restatement(got, runs, groups, u):
    for m, (S, probs, margin, none) in enumerate(runs):
        assert margin >= 1e-4 and not none
        err = np.abs(got["probs"][0, m] - probs.numpy()).max()
        print(f"sequence {m}: probs error {err:.3e} (bound {cr.bound('probs'):.3e}), margin {margin:.2e}")
        assert err <= cr.bound("probs")
        assert np.array_equal(got["S"][0, m], S.numpy())
        for g in groups:  # the group's letter is an inverse-CDF choice for the uniform of its LAST member
            assert mr.valid_choice(got["probs"][0, m, g[-1]], float(u[m, g[-1]]), int(got["S"][0, m, g[0]]), 1e-6), (m, g)


def test_homo_trimer_of_300_rows_matches_the_restatement():
    """N = 300 as 3 x 100 (K_eff = 48 of 300, more rows than a block has threads), every row tied to its two copies through the helper,
    M = 2.  The backbone is the one of the untied N = 300 test (1.19e-3 A between the 48th and 49th distance)."""
    rng = np.random.default_rng(0)
    prot, S_in = mr.backbone(rng, 300), rng.integers(0, 20, size=300)
    chain_idx, residue_index = np.repeat([1, 2, 3], 100), np.tile(np.arange(100), 3)
    groups = inv.tied_positions_from_chains(chain_idx)
    assert len(groups) == 100 and groups[7] == [7, 107, 207]
    gen = torch.Generator().manual_seed(TRIMER_SEED)
    drawn = inv.decoding_order_from(torch.randn((2, 300), generator=gen), torch.ones(300)).numpy()
    u = torch.rand((2, 300), generator=gen, dtype=torch.float32).numpy()
    enc, runs = _restated(prot, S_in, residue_index, chain_idx, groups, drawn, u, 1.0)
    assert enc[3].min() >= 1e-3
    _, bias = mr.omit_bias()
    got = _model(48).design(prot[None], num_seq=2, temperature=1.0, aatype=inv.mpnn_to_aatype(S_in)[None], omit="X", bias=bias, decoding_order=drawn[None],
                            u=u[None], residue_index=residue_index, chain_idx=chain_idx, tied_positions=groups)
    assert all(set(got["E_idx"][0, r]) == set(enc[2][r].tolist()) for r in range(300)) and got["status"].tolist() == [0]
    assert all(np.array_equal(got["decoding_order"][0, m], cr.flatten(drawn[m], groups)) for m in range(2))
    _check_against_restatement(got, runs, groups, u)


def test_tied_beta_of_ones_on_rows_with_identical_environments():
    """A C2 dimer of 2 x 16 rows (chain B is chain A turned by 180 degrees about z), row r of both chains tied: the two members see
    the same environment.  tied_beta of ones is the default, bit for bit, and the device equals the restatement."""
    rng = np.random.default_rng(12)
    a = mr.backbone(rng, 16)
    a = a - a[:, 1].mean(0) + np.array([9.0, 0.0, 0.0], np.float32)
    prot = np.concatenate([a, a * np.array([-1.0, -1.0, 1.0], np.float32)]).astype(np.float32)
    S_in = rng.integers(0, 20, size=32)
    chain_idx, residue_index = np.repeat([1, 2], 16), np.tile(np.arange(16), 2)
    groups = inv.tied_positions_from_chains(chain_idx)
    gen = torch.Generator().manual_seed(DIMER_SEED)
    drawn = inv.decoding_order_from(torch.randn((2, 32), generator=gen), torch.ones(32)).numpy()
    u = torch.rand((2, 32), generator=gen, dtype=torch.float32).numpy()
    _, runs = _restated(prot, S_in, residue_index, chain_idx, groups, drawn, u, 1.0, np.ones(32))
    _, bias = mr.omit_bias()
    kw = dict(num_seq=2, temperature=1.0, aatype=inv.mpnn_to_aatype(S_in)[None], omit="X", bias=bias, decoding_order=drawn[None], u=u[None],
              residue_index=residue_index, chain_idx=chain_idx, tied_positions=groups)
    model = _model(48)
    got = model.design(prot[None], tied_beta=np.ones(32, np.float32), **kw)
    default = model.design(prot[None], **kw)
    assert np.array_equal(got["S"], default["S"]) and np.array_equal(got["probs"], default["probs"])
    _check_against_restatement(got, runs, groups, u)
    beta = np.where(chain_idx == 1, 0.5, 1.5).astype(np.float32)
    assert not np.array_equal(model.design(prot[None], tied_beta=beta, **kw)["probs"], got["probs"])   # (the weights are read)


def test_a_row_left_without_a_letter_keeps_its_input():
    rng = np.random.default_rng(21)
    prot = np.stack([mr.backbone(rng, 24), mr.backbone(rng, 24)])
    aatype = rng.integers(0, 20, size=(2, 24))
    omit_mask = np.zeros((2, 24, 21), np.float32)
    omit_mask[0, 7] = 1.0
    omit_mask[1, 9, 1:] = 1.0
    model = _model(48)
    des = model.design(prot, num_seq=2, temperature=1.0, seed=3, aatype=aatype, omit_mask=omit_mask)
    S_in = inv.aatype_to_mpnn(aatype)
    assert des["status"].tolist() == [inv.NO_LETTER, 0] and inv.NO_LETTER == _lib.MPNN_NO_LETTER == 2
    assert (des["S"][0, :, 7] == S_in[0, 7]).all() and not des["probs"][0, :, 7].any()
    others = np.ones((2, 2, 24), bool)
    others[0, :, 7] = False
    assert np.allclose(des["probs"][others].sum(-1), 1.0, atol=1e-5) and np.isfinite(des["probs"]).all() and np.isfinite(des["log_probs"]).all()
    assert (des["S"][1, :, 9] == 0).all() and (des["probs"][1, :, 9, 0] == 1.0).all()   # one letter left: that letter
    plain = model.design(prot, num_seq=2, temperature=1.0, seed=3, aatype=aatype)
    assert plain["status"].tolist() == [0, 0]


def test_entries_refuse_what_the_header_says():
    fix, model = _fix("p"), _model(48)
    dev, x, b, n, res_mask, chain_mask, residue_index, chain_idx = model._inputs(fix["prot"], *(fix[k] for k in ROWS))
    S, order = np.repeat(fix["S"][:, None], 2, axis=1), fix["decoding_order"]
    omit, bias = mr.omit_bias()
    common = (dev, x, b, n, 2, res_mask, chain_mask, residue_index, chain_idx)
    design = dict(u=fix["u"], omit=omit, bias=bias, temperature=1.0)
    zeros, coef = np.zeros((b, n, 21), np.float32), np.zeros((b, n), np.float32)
    for controls in ({"pssm_bias": zeros}, {"pssm_log_odds_mask": zeros}, {"tie_group": np.full((b, n), -1, np.int32)}):
        with pytest.raises(_lib.FdiptError, match="FDIPT_EINVAL"):
            model._run(True, *common, S, order, controls=controls, **design)
    model._run(True, *common, S, order, controls={"pssm_bias": zeros, "pssm_log_odds_mask": zeros, "pssm_coef": coef,
                                                  "tie_group": np.full((b, n), -1, np.int32), "tied_beta": coef}, **design)
    with pytest.raises(_lib.FdiptError, match="FDIPT_EINVAL"):                          # the conditional score needs S and an order
        model._run(False, *common, None, None)
    with pytest.raises(_lib.FdiptError, match="FDIPT_EINVAL"):                          # design always does
        model._run(True, *common, None, None, unconditional=True, **design)
    model._run(False, *common, None, None, unconditional=True)
    # the Python layer says the same earlier, and names the row of a group it refuses
    kw = dict(num_seq=2, **{k: fix[k] for k in ROWS})
    with pytest.raises(ValueError, match="need pssm_coef"):
        model.design(fix["prot"], pssm_bias=zeros, **kw)
    with pytest.raises(ValueError, match="need pssm_coef"):
        model.design(fix["prot"], pssm_log_odds=zeros, **kw)
    with pytest.raises(ValueError, match="tied_beta without tied_positions"):
        model.design(fix["prot"], tied_beta=coef, **kw)
    with pytest.raises(ValueError, match="row 20 outside 0 .. 19"):
        model.design(fix["prot"], tied_positions=[[3, 20]], **kw)
    with pytest.raises(ValueError, match="bias_by_res"):
        model.design(fix["prot"], bias_by_res=np.zeros((1, 20, 20), np.float32), **kw)


def test_run_sharded_design_omits_letters_and_scores_the_native_loop(tmp_path):
    """``run_sharded --design --omit-aas CX`` on a small inpainting run: no C or X among the designed rows, and design.json carries the
    conditional score of the true letters of the diffused rows."""
    import json

    from framedipt_amd import run_sharded
    rng = np.random.default_rng(9)
    x = np.zeros((24, 37, 3), np.float32)
    x[:, :5] = mr.backbone(rng, 24)
    diffused = (np.arange(24) >= 6) & (np.arange(24) < 14)
    gathered = {0: {"prot": x, "diffused": diffused, "res_mask": np.ones(24, np.float32), "aatype": np.arange(24) % 20,
                    "residue_index": np.arange(24), "chain_idx": np.ones(24, np.int64)}}
    records = [{"item": 0, "name": "7abc", "sample_i": 0, "n_res": 24, "file": "7abc/sample_0/sample_0_1.pdb"}]
    done = run_sharded.run_design(str(tmp_path), records, gathered, inpainting=True, seq_per_sample=4, omit_aas="CX")
    entry = done["samples"]["7abc_sample_0_sample_0_1"]
    assert done["omit"] == "CX" and entry["designed_rows"] == 8
    designed = ["".join(c for i, c in enumerate(s) if diffused[i]) for s in entry["sequences"]]
    assert all(len(s) == 8 and "C" not in s and "X" not in s for s in designed)
    assert np.isfinite(entry["native_conditional_score"]) and entry["native_conditional_score"] > 0
    assert json.load(open(tmp_path / "design.json"))["samples"]["7abc_sample_0_sample_0_1"]["native_conditional_score"] == entry["native_conditional_score"]
    assert run_sharded.run_design(str(tmp_path / "x"), records, gathered, inpainting=True, seq_per_sample=1)["omit"] == "X"   # the default
    # a de novo run has no true letters: no such number
    assert "native_conditional_score" not in run_sharded.run_design(str(tmp_path / "d"), records, gathered, seq_per_sample=1)["samples"]["7abc_sample_0_sample_0_1"]


# the seeds of the two restated runs: the first from 0 whose every draw keeps a margin of 1e-4 in the restatement (asserted there)
TRIMER_SEED, DIMER_SEED = 2, 1
