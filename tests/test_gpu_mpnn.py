"""GPU tests (-m gpu) of inverse folding (framedipt_amd/inverse_folding.py -> fdipt_mpnn_score / fdipt_mpnn_design, csrc/mpnn.hip) against
the reference's recorded outputs (tests/golden/mpnn_<case>.npz; weights come back from the seed).  The tolerance on log-probabilities
and probs is four times the deviation of the reference's float32 outputs from the float64 restatement (tests/mpnn_ref.py: DEVIATION,
DESIGN.md section 7.10); letters and neighbour sets are compared exactly.  ``-s`` prints the device's figures next to the bounds."""
import functools

import numpy as np
import pytest

import mpnn_ref as mr
from conftest import load_golden
from framedipt_amd import inverse_folding as inv

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _model(k):
    return inv.ProteinMPNN(k).load_synthetic(mr.WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def _fix(name):
    return load_golden(f"mpnn_{name}.npz")


def _rows(fix, keys=("res_mask", "chain_mask", "residue_index", "chain_idx"), b=slice(None)):
    return {k: fix[k][b] for k in keys}


@functools.lru_cache(maxsize=None)
def _score(name):
    fix = _fix(name)
    return _model(mr.CASES[name][2]).score(fix["prot"], fix["S"], decoding_order=fix["decoding_order"], **_rows(fix))


@functools.lru_cache(maxsize=None)
def _design(name, t):
    fix = _fix(name)
    omit, bias = mr.omit_bias()
    assert omit.tolist() == [0.0] * 20 + [1.0]
    return _model(mr.CASES[name][2]).design(fix["prot"], num_seq=mr.M, temperature=t, aatype=inv.mpnn_to_aatype(fix["S"]), omit="X", bias=bias,
                                            decoding_order=fix["decoding_order"], u=fix["u"], **_rows(fix))


@pytest.mark.parametrize("name", list(mr.CASES))
def test_score_matches_the_reference(name):
    fix, got = _fix(name), _score(name)
    b, n, k = mr.CASES[name]
    valid = fix["res_mask"] != 0
    assert got["log_probs"].shape == (b, mr.M, n, 21) and got["E_idx"].shape == (b, n, min(k, n)) and got["status"].tolist() == [0] * b
    for i in range(b):
        for r in np.nonzero(valid[i])[0]:
            assert set(got["E_idx"][i, r]) == set(fix["E_idx"][i, r]), (i, r)
    rows = np.broadcast_to(valid[:, None], (b, mr.M, n))
    err = np.abs(got["log_probs"] - fix["log_probs"])[rows].max()
    print(f"case {name}: log_probs error {err:.3e} (bound {mr.bound('log_probs'):.3e})")
    assert err <= mr.bound("log_probs")
    assert not got["log_probs"][~rows].any()                                            # rows without res_mask: 0
    want = inv.scores_of(fix["log_probs"], np.repeat(fix["S"][:, None], mr.M, axis=1), (fix["res_mask"] * fix["chain_mask"])[:, None])
    assert np.abs(got["score"] - want).max() <= mr.bound("log_probs")


@pytest.mark.parametrize("name,t", [(name, t) for name in mr.CASES for t in mr.TEMPERATURES[name]])
def test_design_matches_the_reference(name, t):
    fix, got = _fix(name), _design(name, t)
    b, n, _ = mr.CASES[name]
    valid = fix["res_mask"] != 0
    rows = np.broadcast_to(valid[:, None], (b, mr.M, n))
    differ = int((got["S"] != fix[f"S_T{t}"]).sum())
    err = np.abs(got["probs"] - fix[f"probs_T{t}"])[rows].max()
    print(f"case {name} T={t}: {differ} letters differ, probs error {err:.3e} (bound {mr.bound('probs'):.3e})")
    assert differ == 0
    assert err <= mr.bound("probs")
    S_in = np.repeat(fix["S"][:, None], mr.M, axis=1)
    fixed = np.broadcast_to(((fix["chain_mask"] == 0) | ~valid)[:, None], (b, mr.M, n))
    assert np.array_equal(got["S"][fixed], S_in[fixed]) and not got["probs"][fixed].any()      # fixed and masked rows keep the input letter
    assert np.array_equal(got["aatype"], inv.mpnn_to_aatype(got["S"])) and (got["S"][~fixed] != 20).all()   # X is omitted
    assert got["status"].tolist() == [0] * b and np.isfinite(got["score"]).all() and np.isfinite(got["global_score"]).all()
    assert got["sequences"][0][0] == inv.mpnn_to_seq(got["S"][0, 0], fix["res_mask"][0])
    designed = (fix["chain_mask"] * fix["res_mask"])[:, None]
    assert np.allclose(got["seq_recovery"], ((got["S"] == S_in) * designed).sum(-1) / designed.sum(-1))


def test_case_c_exercises_fixed_and_masked_rows():
    fix = _fix("c")
    assert (fix["res_mask"] == 0).sum() == 7 and (fix["chain_mask"] == 0).sum() == 20 and len(set(fix["chain_idx"][0])) == 2


@functools.lru_cache(maxsize=None)
def _own_input():
    rng = np.random.default_rng(2024)
    return mr.backbone(rng, 64)[None], rng.integers(0, 20, size=(1, 64))


def test_design_and_score_agree():
    """An input with no fixture (N = 64, M = 3): design's letters and orders fed to score give back design's distribution, and every letter
    is an inverse-CDF choice for its uniform."""
    prot, aatype = _own_input()
    t, bias = 0.5, {"A": 0.4, "W": -0.3}
    model = _model(48)
    des = model.design(prot, num_seq=3, temperature=t, seed=11, aatype=aatype, omit="XC", bias=bias)
    sc = model.score(prot, des["S"], decoding_order=des["decoding_order"])
    assert np.array_equal(sc["log_probs"], des["log_probs"]) and np.array_equal(sc["score"], des["score"])   # design's own rescoring
    omit = np.array([1.0 if c in "XC" else 0.0 for c in inv.ALPHABET])
    bias_v = np.array([bias.get(c, 0.0) for c in inv.ALPHABET])
    z = sc["log_probs"].astype(np.float64) / t - omit * 1e8 + bias_v / t
    p = np.exp(z - z.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    err = np.abs(p - des["probs"]).max()
    print(f"design probs against score's log_probs: {err:.3e} (bound {mr.bound('probs'):.3e})")
    assert err <= mr.bound("probs")
    assert len(np.unique(des["S"])) > 3 and not np.isin(des["S"], [1, 20]).any()        # C and X never drawn
    assert len({tuple(o) for o in des["decoding_order"][0]}) == 3                       # each sequence has its own order
    for m in range(3):
        for r in range(64):
            assert mr.valid_choice(des["probs"][0, m, r], float(des["u"][0, m, r]), int(des["S"][0, m, r]), 1e-6), (m, r)
    again = model.design(prot, num_seq=3, temperature=t, seed=11, aatype=aatype, omit="XC", bias=bias)
    assert np.array_equal(again["S"], des["S"]) and np.array_equal(again["probs"], des["probs"])


def test_results_do_not_depend_on_the_batch():
    fix = _fix("b")
    model = _model(48)
    one = slice(1, 2)
    alone = model.score(fix["prot"][one], fix["S"][one], decoding_order=fix["decoding_order"][one], **_rows(fix, b=one))
    assert np.array_equal(alone["log_probs"][0], _score("b")["log_probs"][1]) and np.array_equal(alone["E_idx"][0], _score("b")["E_idx"][1])
    omit, bias = mr.omit_bias()
    kw = dict(temperature=1.0, aatype=inv.mpnn_to_aatype(fix["S"]), omit="X", bias=bias, **_rows(fix))
    alone = model.design(fix["prot"][one], num_seq=mr.M, decoding_order=fix["decoding_order"][one], u=fix["u"][one],
                         **dict(kw, aatype=kw["aatype"][one], **_rows(fix, b=one)))
    pair = _design("b", 1.0)
    assert np.array_equal(alone["S"][0], pair["S"][1]) and np.array_equal(alone["probs"][0], pair["probs"][1])
    # M = 2 gives the first two sequences of M = 4
    rng = np.random.default_rng(5)
    order4 = np.concatenate([fix["decoding_order"], np.stack([[rng.permutation(70) for _ in range(2)] for _ in range(2)])], axis=1)
    u4 = np.concatenate([fix["u"], rng.random((2, 2, 70), dtype=np.float32)], axis=1)
    four = model.design(fix["prot"], num_seq=4, decoding_order=order4, u=u4, **kw)
    assert np.array_equal(four["S"][:, :2], pair["S"]) and np.array_equal(four["probs"][:, :2], pair["probs"])
    assert np.array_equal(four["log_probs"][:, :2], pair["log_probs"]) and not np.array_equal(four["S"][:, 2], four["S"][:, 0])


def test_status_flags_a_masked_neighbour_and_masked_rows_come_back_as_stated():
    """N = 30 with 5 rows masked under K = 48: every row's neighbour set is all 30 columns, so valid rows have masked neighbours."""
    rng = np.random.default_rng(77)
    prot = np.stack([mr.backbone(rng, 30), mr.backbone(rng, 30)])
    res_mask = np.ones((2, 30), np.float32)
    res_mask[0, [3, 4, 17, 28, 29]] = 0
    aatype = rng.integers(0, 20, size=(2, 30))
    chain_mask = np.ones((2, 30), np.float32)
    chain_mask[:, 10:14] = 0
    model = _model(48)
    des = model.design(prot, num_seq=2, temperature=1.0, seed=3, res_mask=res_mask, chain_mask=chain_mask, aatype=aatype)
    assert des["status"].tolist() == [inv.MASKED_NEIGHBOR, 0]
    S_in = inv.aatype_to_mpnn(aatype)
    keep = (res_mask == 0) | (chain_mask == 0)
    for m in range(2):
        assert np.array_equal(des["S"][:, m][keep], S_in[keep]) and not des["probs"][:, m][keep].any()
        assert not des["log_probs"][:, m][res_mask == 0].any() and des["log_probs"][:, m][res_mask != 0].all()
    assert np.isfinite(des["probs"]).all() and np.isfinite(des["score"]).all()
    assert des["sequences"][0][0] == inv.mpnn_to_seq(des["S"][0, 0], res_mask[0]) and len(des["sequences"][0][0]) == 25
    sc = model.score(prot, des["S"], res_mask=res_mask, chain_mask=chain_mask, decoding_order=des["decoding_order"])
    assert sc["status"].tolist() == [inv.MASKED_NEIGHBOR, 0]


def test_run_sharded_design_writes_fasta_and_summary(tmp_path):
    """``run_sharded --design`` after the gather: de novo samples design every row, inpainting samples the diffused rows with the context
    fixed to its true residue types; the FASTA files are in the reference's layout and the summary says that the weights are synthetic."""
    import json

    from framedipt_amd import run_sharded
    rng = np.random.default_rng(9)

    def atom37(n):
        x = np.zeros((n, 37, 3), np.float32)
        x[:, :5] = mr.backbone(rng, n)
        return x

    records = [{"item": i, "name": "length_24", "sample_i": i, "n_res": 24, "file": f"sample_{i:06d}.npz"} for i in range(2)]
    gathered = {i: {"prot": atom37(24), "diffused": np.ones(24, bool), "res_mask": np.ones(24, np.float32), "aatype": np.zeros(24, np.int64),
                    "residue_index": np.arange(24), "chain_idx": np.ones(24, np.int64)} for i in range(2)}
    done = run_sharded.run_design(str(tmp_path), records, gathered, seq_per_sample=3)
    assert done["synthetic"] and done["weights"] == "synthetic(0)" and sorted(done["samples"]) == ["sample_000000", "sample_000001"]
    assert json.load(open(tmp_path / "design.json"))["samples"]["sample_000001"]["sequences"] == done["samples"]["sample_000001"]["sequences"]
    lines = open(tmp_path / "seqs" / "sample_000000.fa").read().splitlines()
    entry = done["samples"]["sample_000000"]
    assert len(lines) == 8 and lines[0].startswith(">sample_000000, score=") and lines[1] == "X" * 24 and lines[3::2] == entry["sequences"]
    assert lines[2].startswith(">T=0.1, sample=1, score=") and lines[2].endswith("seq_recovery=nan") and entry["designed_rows"] == 24
    assert all(len(s) == 24 and "X" not in s for s in entry["sequences"]) and entry["seq_recovery"] == [None] * 3
    # inpainting: rows 5 .. 11 are diffused, the context keeps its residue types (restype order: 0 = A, 1 = R)
    gathered[0]["diffused"] = np.arange(24) // 6 == 1
    gathered[0]["diffused"][5] = True
    gathered[0]["aatype"] = np.arange(24) % 2
    inp = run_sharded.run_design(str(tmp_path / "inp"), [dict(records[0], file="7abc/sample_0/sample_0_1.pdb")], gathered, inpainting=True, seq_per_sample=2)
    entry = inp["samples"]["7abc_sample_0_sample_0_1"]
    assert entry["designed_rows"] == 7 and all(0 <= v <= 1 for v in entry["seq_recovery"])
    lines = open(tmp_path / "inp" / "seqs" / "7abc_sample_0_sample_0_1.fa").read().splitlines()
    assert lines[1] == "RARARAR" and all(len(s) == 7 for s in lines[3::2])          # the FASTA holds the designed rows, as the reference's
    context = "".join("AR"[i % 2] for i in range(24) if not gathered[0]["diffused"][i])
    assert all("".join(c for i, c in enumerate(s) if not gathered[0]["diffused"][i]) == context for s in entry["sequences"])


def test_more_rows_than_threads_match_the_restatement():
    """N = 300: every per-row loop of the kernels takes a second pass (a block has 256 threads), K_eff = 48 of 300.  Against the float64
    restatement: neighbour sets exactly (the input seed leaves 1.19e-3 A between the 48th and 49th distance), log-probabilities and probs
    within the bound, letters exactly (every draw keeps a margin of 1e-4 in the restatement: asserted)."""
    import torch
    rng = np.random.default_rng(0)
    prot = mr.backbone(rng, 300)
    S_in = rng.integers(0, 20, size=300)
    ones, index = np.ones(300, np.float32), np.arange(300)
    omit, bias = mr.omit_bias()
    ref = mr.Model(inv.synthetic_state_dict(mr.WEIGHT_SEED, 48), 48, torch.float64)
    enc = mr.encode(ref, prot, ones, index, ones)
    assert enc[3].min() >= 1e-3
    model = _model(48)
    gen = torch.Generator().manual_seed(0)
    order = inv.decoding_order_from(torch.randn(300, generator=gen), torch.ones(300)).numpy()
    u = torch.rand(300, generator=gen, dtype=torch.float32).numpy()
    S, probs, margin = mr.design(ref, enc, ones, ones, S_in, order, u, 1.0, omit, bias)
    assert margin >= 1e-4
    got = model.design(prot[None], num_seq=1, temperature=1.0, aatype=inv.mpnn_to_aatype(S_in)[None], omit="X", bias=bias, decoding_order=order[None, None],
                       u=u[None, None])
    assert all(set(got["E_idx"][0, r]) == set(enc[2][r].tolist()) for r in range(300))
    err = np.abs(got["probs"][0, 0] - probs.numpy()).max()
    lp = mr.score(ref, enc, ones, S, order).numpy()
    err_lp = np.abs(got["log_probs"][0, 0] - lp).max()
    print(f"N = 300: probs error {err:.3e} (bound {mr.bound('probs'):.3e}), log_probs error {err_lp:.3e} (bound {mr.bound('log_probs'):.3e})")
    assert np.array_equal(got["S"][0, 0], S.numpy()) and err <= mr.bound("probs") and err_lp <= mr.bound("log_probs")


def test_the_longest_chain_runs_and_agrees_with_itself():
    """N = 2048, the limit (the distances, the letters and the decoding steps of a whole chain live in LDS), M = 1.  No restatement at this
    size: neighbour sets against a float64 evaluation of the contract's distances (the input seed leaves 2.3e-4 A between the 48th and
    49th distance, the float32 error of a distance at this extent is 2e-5), design against score, every letter an inverse-CDF choice."""
    rng = np.random.default_rng(9)
    prot = mr.backbone(rng, 2048)[None]
    ca = prot[0, :, 1].astype(np.float64)
    d = np.sqrt(((ca[:, None] - ca[None]) ** 2).sum(-1) + 1e-6)
    srt = np.sort(d, axis=1)
    assert (srt[:, 48] - srt[:, 47]).min() >= 2e-4
    model = _model(48)
    des = model.design(prot, num_seq=1, temperature=1.0, seed=5)
    want = np.argsort(d, axis=1, kind="stable")[:, :48]
    assert all(set(des["E_idx"][0, r]) == set(want[r]) for r in range(2048)) and des["status"].tolist() == [0]
    assert sorted(des["decoding_order"][0, 0]) == list(range(2048)) and (des["S"] != 20).all() and len(np.unique(des["S"])) > 10
    omit = np.array([0.0] * 20 + [1.0])
    z = des["log_probs"].astype(np.float64) - omit * 1e8
    p = np.exp(z - z.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    assert np.abs(p - des["probs"]).max() <= mr.bound("probs")
    assert all(mr.valid_choice(des["probs"][0, 0, r], float(des["u"][0, 0, r]), int(des["S"][0, 0, r]), 1e-6) for r in range(2048))
    with pytest.raises(ValueError, match="at most"):
        model.design(np.zeros((1, 2049, 5, 3), np.float32))
