"""CPU tests of inverse folding: the torch restatement (tests/mpnn_ref.py) in float64 against the reference's recorded outputs
(tests/golden/mpnn_<case>.npz), the host side of framedipt_amd/inverse_folding.py and the C entries' argument checks."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest
import torch

import mpnn_ref as mr
from conftest import load_golden
from framedipt_amd import _lib
from framedipt_amd import inverse_folding as inv


@functools.lru_cache(maxsize=None)
def fixture_and_restatement(name):
    fix = load_golden(f"mpnn_{name}.npz")
    return fix, mr.run_case(inv.synthetic_state_dict(mr.WEIGHT_SEED, mr.CASES[name][2]), name, fix)


@pytest.mark.parametrize("name", list(mr.CASES))
def test_restatement_matches_the_reference(name):
    """Neighbour sets per row, letters exactly, log-probabilities and probs within four times the recorded deviation, on every row with
    res_mask; the fixture conditions (distance gap, draw margin) hold on the recorded inputs."""
    fix, res = fixture_and_restatement(name)
    b, n, k = mr.CASES[name]
    valid = fix["res_mask"] != 0
    assert fix["E_idx"].shape == (b, n, min(k, n)) == res["E_idx"].shape
    for i in range(b):
        for r in np.nonzero(valid[i])[0]:
            assert set(fix["E_idx"][i, r]) == set(res["E_idx"][i, r]), (i, r)
    assert res["gap"][valid].min() >= 1e-3
    rows = np.broadcast_to(valid[:, None], (b, mr.M, n))
    dev = np.abs(fix["log_probs"] - res["log_probs"])[rows].max()
    print(f"case {name}: log_probs deviation {dev:.3e} (bound {mr.bound('log_probs'):.3e})")
    assert dev <= mr.bound("log_probs")
    for t, d in res["design"].items():
        assert d["margin"] >= 1e-4
        assert np.array_equal(fix[f"S_T{t}"], d["S"])
        dev = np.abs(fix[f"probs_T{t}"] - d["probs"])[rows].max()
        print(f"case {name} T={t}: probs deviation {dev:.3e} (bound {mr.bound('probs'):.3e})")
        assert dev <= mr.bound("probs")


def test_fixture_c_has_its_special_rows():
    fix, res = fixture_and_restatement("c")
    assert (fix["res_mask"][0, -7:] == 0).all() and fix["res_mask"].sum() == 123 and (fix["chain_mask"][0, 30:50] == 0).all()
    assert set(fix["chain_idx"][0]) == {1, 2} and fix["residue_index"][0, 60] - fix["residue_index"][0, 59] == 101
    for t, d in res["design"].items():
        assert np.array_equal(d["S"][0, :, 30:50], np.repeat(fix["S"][:, 30:50], mr.M, axis=0))   # fixed rows keep the input
        assert np.array_equal(d["S"][0, :, -7:], np.repeat(fix["S"][:, -7:], mr.M, axis=0))       # so do masked rows
        assert not d["probs"][0, :, 30:50].any() and not d["probs"][0, :, -7:].any()
    assert not res["log_probs"][0, :, -7:].any()
    # fixed rows are decoded first
    assert all(set(fix["decoding_order"][0, m, :27]) == set(range(30, 50)) | set(range(123, 130)) for m in range(mr.M))


def test_synthetic_parameters_are_stable_and_pack_as_the_header_says():
    sd = inv.synthetic_state_dict(7, 48)
    assert list(sd) == list(inv.param_shapes()) and all(v.dtype == np.float32 for v in sd.values())
    image = inv.pack_image(sd)
    dims = inv.ProteinMPNN(48).dims()
    assert image.dtype == np.float32 and image.size == 1660485 == sum(v.size for v in sd.values()) == _lib.load().fdipt_mpnn_weights_floats(C.byref(dims))
    assert hashlib.sha256(image.tobytes()).hexdigest()[:16] == IMAGE_SHA
    assert np.array_equal(image, inv.pack_image(inv.synthetic_state_dict(7, 48)))
    assert not np.array_equal(image, inv.pack_image(inv.synthetic_state_dict(8, 48))) and not np.array_equal(image, inv.pack_image(inv.synthetic_state_dict(7, 30)))
    # gains around 1, shifts around 0, nothing exactly 0 or 1
    g, s = sd["encoder_layers.1.norm2.weight"], sd["encoder_layers.1.norm2.bias"]
    assert abs(g.mean() - 1) < 0.05 and abs(s.mean()) < 0.05 and g.std() > 0.05 and s.std() > 0.05 and (sd["W_out.bias"] != 0).all()
    # the table in include/fdipt.h: transposed matrices, in order
    assert np.array_equal(image[:66 * 16].reshape(66, 16), sd["features.embeddings.linear.weight"].T)
    o = 66 * 16 + 16
    assert np.array_equal(image[o:o + 416 * 128].reshape(416, 128), sd["features.edge_embedding.weight"].T)
    o += 416 * 128
    assert np.array_equal(image[o:o + 128], sd["features.norm_edges.weight"]) and np.array_equal(image[o + 128:o + 256], sd["features.norm_edges.bias"])
    assert np.array_equal(image[-21:], sd["W_out.bias"]) and np.array_equal(image[-21 - 128 * 21:-21].reshape(128, 21), sd["W_out.weight"].T)
    enc0 = 66 * 16 + 16 + 416 * 128 + 256 + 128 * 128 + 128 + 21 * 128
    assert np.array_equal(image[enc0:enc0 + 384 * 128].reshape(384, 128), sd["encoder_layers.0.W1.weight"].T)
    with pytest.raises(ValueError, match="lacks"):
        inv.pack_image({k: v for k, v in sd.items() if k != "W_s.weight"})
    with pytest.raises(ValueError, match="W_out.weight"):
        inv.pack_image(dict(sd, **{"W_out.weight": np.zeros((20, 128), np.float32)}))


IMAGE_SHA = "2e7b7a0c1096e126"


def test_checkpoint_round_trip(tmp_path):
    sd = inv.synthetic_state_dict(3, 30)
    path = tmp_path / "v_30_020.pt"
    torch.save({"num_edges": 30, "noise_level": 0.2, "model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}}, path)
    model = inv.ProteinMPNN().load_checkpoint(path)
    assert model.k_neighbors == 30 and model.noise_level == 0.2 and model.source == str(path)
    assert np.array_equal(model.image, inv.pack_image(sd))
    torch.save({"num_edges": 65, "noise_level": 0.2, "model_state_dict": {}}, path)
    with pytest.raises(ValueError, match="num_edges"):
        inv.ProteinMPNN().load_checkpoint(path)
    with pytest.raises(ValueError):
        inv.ProteinMPNN(0)


def test_alphabet_conversion_round_trips():
    aatype = np.arange(21)
    S = inv.aatype_to_mpnn(aatype)
    assert sorted(S) == list(range(21)) and np.array_equal(inv.mpnn_to_aatype(S), aatype) and S[20] == 20
    assert "".join(inv.ALPHABET[s] for s in S[:20]) == "ARNDCQEGHILKMFPSTWYV"
    assert np.array_equal(inv.aatype_to_mpnn(inv.mpnn_to_aatype(np.arange(21))), np.arange(21))
    assert inv.mpnn_to_seq(inv.seq_to_mpnn("MKVLAXB")) == "MKVLAXX" and inv.mpnn_to_seq([0, 1, 2], [1, 0, 1]) == "AD"
    with pytest.raises(ValueError):
        inv.aatype_to_mpnn([21])


def test_fasta_records_follow_the_reference_format():
    S = np.array([[[0, 1, 2, 3], [4, 5, 6, 7]]])
    result = {"S": S, "S_input": np.array([[9, 9, 9, 9]]), "res_mask": np.array([[1, 1, 1, 0]], np.float32), "chain_mask": np.ones((1, 4), np.float32),
              "score": np.array([[1.23456, 0.5]], np.float32), "global_score": np.array([[2.0, 0.98768]], np.float32),
              "seq_recovery": np.array([[0.25, np.nan]], np.float32), "temperature": 0.1, "seed": 38}
    text = inv.fasta_records(result, 0, "sample_1")
    lines = text.splitlines()
    assert lines[0] == ">sample_1, score=nan, global_score=nan, fixed_chains=[], designed_chains=['A'], model_name=synthetic, git_hash=unknown, seed=38"
    assert lines[1] == "LLL"
    # protein_mpnn_run.py:363-367
    want = '>T={}, sample={}, score={}, global_score={}, seq_recovery={}\n{}\n'.format(
        0.1, 1, np.format_float_positional(np.float32(1.23456), unique=False, precision=4), np.format_float_positional(np.float32(2.0), unique=False, precision=4),
        np.format_float_positional(np.float32(0.25), unique=False, precision=4), "ACD")
    assert "\n".join(lines[2:4]) + "\n" == want == ">T=0.1, sample=1, score=1.2346, global_score=2.0000, seq_recovery=0.2500\nACD\n"
    assert lines[4] == ">T=0.1, sample=2, score=0.5000, global_score=0.9877, seq_recovery=nan" and lines[5] == "FGH" and text.endswith("\n") and len(lines) == 6


def test_scores_follow_the_reference():
    lp = np.log(np.full((1, 2, 3, 21), 1 / 21.0))
    lp[0, 1, 2, 5] = -2.0
    S = np.array([[[0, 1, 2], [3, 4, 5]]])
    assert np.allclose(inv.scores_of(lp, S, np.ones((1, 1, 3))), [[np.log(21), (2 * np.log(21) + 2) / 3]])
    assert np.allclose(inv.scores_of(lp, S, np.array([[[0, 0, 1.0]]])), [[np.log(21), 2.0]])
    order = inv.decoding_order_from(torch.tensor([[0.5, -0.1, 2.0, -0.3]]), torch.tensor([[1.0, 1.0, 0.0, 1.0]]))
    assert order.tolist() == [[2, 1, 3, 0]]   # the fixed row first, then by |randn|


def test_entries_refuse_bad_arguments_before_any_launch():
    """FDIPT_EINVAL / FDIPT_ESIZE decided on the host values, before the device is touched (the pointers are never dereferenced)."""
    lib = _lib.load()

    def dims(**kw):
        return _lib.MpnnDims(**dict(dict(hidden=128, enc_layers=3, dec_layers=3, vocab=21, k_neighbors=48), **kw))

    good = dims()
    assert lib.fdipt_mpnn_weights_floats(C.byref(good)) == 1660485 == lib.fdipt_mpnn_weights_floats(C.byref(dims(k_neighbors=1)))
    for bad in (dims(hidden=64), dims(enc_layers=2), dims(dec_layers=4), dims(vocab=20), dims(k_neighbors=0), dims(k_neighbors=65)):
        assert lib.fdipt_mpnn_weights_floats(C.byref(bad)) == _lib.EINVAL and lib.fdipt_mpnn_workspace(C.byref(bad), 1, 10, 1) == 0
    # h_E [B,N,K_eff,128] + two h_V + three decoder outputs per sequence, then the decoding steps
    assert lib.fdipt_mpnn_workspace(C.byref(good), 2, 70, 3) == 4 * (2 * 70 * 48 * 128 + 2 * 2 * 70 * 128 + 3 * 2 * 70 * 3 * 128 + 2 * 70 * 3)
    assert lib.fdipt_mpnn_workspace(C.byref(good), 1, 20, 1) == 4 * (20 * 20 * 128 + 2 * 20 * 128 + 3 * 20 * 128 + 20)
    names = ("weights", "prot", "res_mask", "chain_mask", "residue_index", "chain_idx", "S", "decoding_order", "u", "omit", "bias", "E_idx", "log_probs",
             "S_out", "probs", "status", "workspace")

    def call(fn, d=good, b=1, n=10, m=1, atoms=37, temperature=0.1, workspace_bytes=1 << 40, **null):
        fake = {k: (None if null.get(k) else 64) for k in names}
        args = _lib.MpnnArgs(B=b, N=n, M=m, atoms=atoms, temperature=temperature, workspace_bytes=workspace_bytes, **fake)
        return fn(C.byref(d), C.byref(args), None)

    for fn in (lib.fdipt_mpnn_score, lib.fdipt_mpnn_design):
        assert call(fn, d=dims(hidden=256)) == _lib.EINVAL and call(fn, d=dims(k_neighbors=65)) == _lib.EINVAL
        assert call(fn, b=0) == call(fn, n=0) == call(fn, m=0) == call(fn, atoms=14) == _lib.EINVAL
        assert call(fn, weights=True) == call(fn, prot=True) == call(fn, decoding_order=True) == call(fn, E_idx=True) == call(fn, status=True) == _lib.EINVAL
        assert call(fn, n=2049) == call(fn, m=65) == call(fn, workspace_bytes=1000) == call(fn, workspace=True) == _lib.ESIZE
    assert call(lib.fdipt_mpnn_score, log_probs=True) == _lib.EINVAL
    assert call(lib.fdipt_mpnn_design, temperature=0.0) == call(lib.fdipt_mpnn_design, u=True) == call(lib.fdipt_mpnn_design, probs=True) == _lib.EINVAL
    assert call(lib.fdipt_mpnn_design, omit=True) == call(lib.fdipt_mpnn_design, S_out=True) == call(lib.fdipt_mpnn_design, chain_mask=True) == _lib.EINVAL


def test_python_layer_refuses_bad_inputs_without_a_device():
    model = inv.ProteinMPNN()
    with pytest.raises(ValueError, match="37, 3"):
        model.score(np.zeros((1, 8, 4, 3), np.float32), np.zeros((1, 8), int))
    with pytest.raises(ValueError, match="at most"):
        model.score(np.zeros((1, 2049, 5, 3), np.float32), np.zeros((1, 2049), int))
    with pytest.raises(ValueError, match="temperature"):
        model.design(np.zeros((1, 8, 5, 3), np.float32), temperature=0.0)
