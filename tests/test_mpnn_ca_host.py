"""CPU tests of the CA-only inverse folding: the torch restatement (tests/mpnn_ca_ref.py) in float64 against the
reference's recorded outputs (tests/golden/mpnn_ca_<case>.npz), the host side of framedipt_amd/inverse_folding.py for ``ca_only`` and the
C entries' argument checks."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import mpnn_ca_ref as mc
import mpnn_ref as mr
from conftest import ROOT, load_golden
from framedipt_amd import _lib
from framedipt_amd import inverse_folding as inv

CA_FLOATS = 1628613


@functools.lru_cache(maxsize=None)
def fixture_and_restatement(name):
    fix = load_golden(f"mpnn_{name}.npz")
    return fix, mc.run_case(inv.synthetic_state_dict(mr.WEIGHT_SEED, mc.CASES[name][2], ca_only=True), name, fix)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_restatement_matches_the_reference(name):
    """Neighbour sets per row, letters exactly, log-probabilities and probs within four times the recorded deviation, on every row with
    res_mask; the four fixture conditions (distance gap, draw margin, step margin, antisymmetric margin) hold on the recorded inputs and
    Q on the self edges is the identity."""
    fix, res = fixture_and_restatement(name)
    b, n, k = mc.CASES[name]
    valid = fix["res_mask"] != 0
    assert fix["ca"].shape == (b, n, 3) and fix["E_idx"].shape == (b, n, min(k, n)) == res["E_idx"].shape
    for i in range(b):
        for r in np.nonzero(valid[i])[0]:
            assert set(fix["E_idx"][i, r]) == set(res["E_idx"][i, r]), (i, r)
    assert res["gap"][valid].min() >= 1e-3 and res["step_margin"] >= 1e-3 and res["min_anti"] >= 1e-5
    assert (res["self_q"] == np.array([0.0, 0.0, 0.0, 1.0])).all()
    rows = np.broadcast_to(valid[:, None], (b, mc.M, n))
    dev = np.abs(fix["log_probs"] - res["log_probs"])[rows].max()
    print(f"case {name}: log_probs deviation {dev:.3e} (bound {mc.bound('log_probs'):.3e})")
    assert dev <= mc.bound("log_probs")
    for t, d in res["design"].items():
        assert d["margin"] >= 1e-4
        assert np.array_equal(fix[f"S_T{t}"], d["S"])
        dev = np.abs(fix[f"probs_T{t}"] - d["probs"])[rows].max()
        print(f"case {name} T={t}: probs deviation {dev:.3e} (bound {mc.bound('probs'):.3e})")
        assert dev <= mc.bound("probs")


def test_fixtures_hold_what_the_table_says():
    fix, res = fixture_and_restatement("ca_c")
    assert (fix["res_mask"][0, -7:] == 0).all() and fix["res_mask"].sum() == 123 and (fix["chain_mask"][0, 30:50] == 0).all() and fix["chain_mask"].sum() == 110
    assert set(fix["chain_idx"][0]) == {1, 2} and fix["residue_index"][0, 60] - fix["residue_index"][0, 59] == 101
    step = np.linalg.norm(np.diff(fix["ca"][0].astype(np.float64), axis=0), axis=-1)
    assert step[59] > 100                                                          # the second chain is displaced
    for row, length in mc.STEPS_C.items():                                         # 3.3 and 4.3 are zeroed, 3.65 and 3.95 kept
        assert abs(step[row - 1] - length) < 1e-3 and row < 60
    assert sorted(np.round(step[(np.abs(step - 3.8) > 1e-3) & (step < 100)], 2)) == [3.3, 3.65, 3.95, 4.3]
    o = mc.frames(torch.from_numpy(fix["ca"][0].astype(np.float64)))
    rank = np.linalg.matrix_rank(o.numpy(), tol=1e-9)
    assert rank[19] == rank[20] == rank[24] == rank[25] == 1 and rank[51] == rank[52] == rank[55] == rank[56] == 3   # rows around a zeroed step
    assert rank[0] == rank[128] == rank[129] == 0 and rank[59] == rank[60] == 1
    # the shortest length: every O is zero, so dU is zero and every Q the identity
    fix_e, _ = fixture_and_restatement("ca_e")
    e = mc.edge_inputs(mr.Model(inv.synthetic_state_dict(mr.WEIGHT_SEED, 48, ca_only=True), 48), fix_e["ca"][0], fix_e["res_mask"][0],
                       fix_e["residue_index"][0], fix_e["chain_idx"][0])[0]
    assert e.shape == (3, 3, 167) and not e[..., 160:163].any() and (e[..., 163:] == torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)).all()
    assert not mc.frames(torch.zeros((3, 3))).any() and mc.frames(torch.from_numpy(fixture_and_restatement("ca_f")[0]["ca"][0]))[1:5].abs().sum() > 0


def test_the_shifted_traces_ignore_chains_and_use_the_origin():
    fix, _ = fixture_and_restatement("ca_a")
    ca = torch.from_numpy(fix["ca"][0].astype(np.float64))
    tr = mc.shifted(ca)
    assert not tr[0, 0].any() and not tr[2, -1].any() and torch.equal(tr[0, 1:], ca[:-1]) and torch.equal(tr[2, :-1], ca[1:]) and torch.equal(tr[1], ca)
    sd = inv.synthetic_state_dict(mr.WEIGHT_SEED, 48, ca_only=True)
    model = mr.Model(sd, 48)
    args = (fix["res_mask"][0], fix["residue_index"][0], fix["chain_idx"][0])
    here = mc.edge_inputs(model, fix["ca"][0], *args)[0]
    moved = mc.edge_inputs(model, fix["ca"][0].astype(np.float64) + 50.0, *args)[0]
    # block (1,1) does not see the translation, block (0,0) of row 0 (the origin against the neighbours' predecessors) does
    assert torch.allclose(here[:, :, 16:32], moved[:, :, 16:32], rtol=0, atol=1e-9) and not torch.allclose(here[0, :, 32:48], moved[0, :, 32:48], rtol=0, atol=1e-3)


def test_parameter_names_and_shapes_are_the_reference_s():
    want = {n: tuple(s) for n, s in json.load(open(os.path.join(ROOT, "tests", "golden", "mpnn_ca_state_dict.json")))}
    got = inv.param_shapes(ca_only=True)
    assert dict(got) == want and len(got) == len(want) == len(inv.param_shapes()) + 5
    assert set(got) - set(inv.param_shapes()) == set(inv.CA_UNREAD) and got["features.edge_embedding.weight"] == (128, 167)
    assert got["features.node_embedding.weight"] == (128, 3) and got["W_v.weight"] == (128, 128)
    assert inv.param_shapes(ca_only=False) == inv.param_shapes()
    sd = inv.synthetic_state_dict(7, 48, ca_only=True)
    assert list(sd) == list(got) and all(v.dtype == np.float32 and v.shape == got[n] for n, v in sd.items())
    rng = np.random.default_rng((7, 48, 1))                                         # the stream and the order of the draws
    first = rng.uniform(-np.sqrt(6.0 / (16 + 66)), np.sqrt(6.0 / (16 + 66)), size=(16, 66)).astype(np.float32)
    assert np.array_equal(sd["features.embeddings.linear.weight"], first)
    assert not np.array_equal(sd["W_e.weight"], inv.synthetic_state_dict(7, 48)["W_e.weight"])


def test_image_of_the_ca_model():
    sd = inv.synthetic_state_dict(7, 48, ca_only=True)
    image = inv.pack_image(sd)
    assert image.dtype == np.float32 and image.size == CA_FLOATS == 1660485 - 249 * 128 == sum(v.size for n, v in sd.items() if n not in inv.CA_UNREAD)
    assert np.array_equal(image, inv.pack_image(sd, ca_only=True)) and inv.is_ca_state_dict(sd) and not inv.is_ca_state_dict(inv.synthetic_state_dict(7, 48))
    o = 66 * 16 + 16
    assert np.array_equal(image[:66 * 16].reshape(66, 16), sd["features.embeddings.linear.weight"].T)
    assert np.array_equal(image[o:o + 167 * 128].reshape(167, 128), sd["features.edge_embedding.weight"].T)
    o += 167 * 128
    assert np.array_equal(image[o:o + 128], sd["features.norm_edges.weight"]) and np.array_equal(image[o + 128:o + 256], sd["features.norm_edges.bias"])
    assert np.array_equal(image[o + 256:o + 256 + 128 * 128].reshape(128, 128), sd["W_e.weight"].T)
    assert np.array_equal(image[-21:], sd["W_out.bias"])
    # the five unread parameters are accepted and dropped
    lean = {k: v for k, v in sd.items() if k not in inv.CA_UNREAD}
    assert np.array_equal(inv.pack_image(lean), image)
    with pytest.raises(ValueError, match="CA-only"):
        inv.pack_image(inv.synthetic_state_dict(7, 48), ca_only=True)
    with pytest.raises(ValueError, match="vanilla"):
        inv.pack_image(sd, ca_only=False)


def test_defaults_are_unchanged():
    """The vanilla synthetic parameters and their image hash as before ``ca_only`` existed (tests/test_mpnn_host.py:IMAGE_SHA)."""
    assert hashlib.sha256(inv.pack_image(inv.synthetic_state_dict(7, 48)).tobytes()).hexdigest()[:16] == "2e7b7a0c1096e126"
    assert hashlib.sha256(inv.pack_image(inv.synthetic_state_dict(7, 48, ca_only=False), ca_only=None).tobytes()).hexdigest()[:16] == "2e7b7a0c1096e126"
    model = inv.ProteinMPNN()
    assert model.ca_only is False and model.k_neighbors == 48 and model.dims().ca_only == 0 and inv.ProteinMPNN(30, ca_only=True).dims().ca_only == 1


def test_a_state_dict_of_the_other_model_is_refused_by_name(tmp_path):
    vanilla, ca = inv.synthetic_state_dict(3, 30), inv.synthetic_state_dict(3, 30, ca_only=True)
    with pytest.raises(ValueError, match=r"vanilla full-backbone model .*416 columns.* ProteinMPNN\(ca_only=True\)"):
        inv.ProteinMPNN(30, ca_only=True).load_state_dict(vanilla)
    with pytest.raises(ValueError, match=r"CA-only model .*167 columns.* ProteinMPNN\(ca_only=False\)"):
        inv.ProteinMPNN(30).load_state_dict(ca)
    path = tmp_path / "v_30_020.pt"
    torch.save({"num_edges": 30, "noise_level": 0.2, "model_state_dict": {k: torch.from_numpy(v) for k, v in ca.items()}}, path)
    with pytest.raises(ValueError, match="CA-only"):
        inv.ProteinMPNN().load_checkpoint(path)
    model = inv.ProteinMPNN(ca_only=True).load_checkpoint(path)
    assert model.k_neighbors == 30 and model.ca_only and model.image.size == CA_FLOATS and np.array_equal(model.image, inv.pack_image(ca))
    assert np.array_equal(inv.ProteinMPNN(30, ca_only=True).load_synthetic(3).image, model.image)


def test_entries_decide_the_ca_refusals_before_any_launch():
    """FDIPT_EINVAL decided on the host values (the pointers are never dereferenced); a call that passes these checks is stopped by the
    next one, the workspace size (FDIPT_ESIZE), before the device is touched."""
    lib = _lib.load()

    def dims(**kw):
        return _lib.MpnnDims(**dict(dict(hidden=128, enc_layers=3, dec_layers=3, vocab=21, k_neighbors=48), **kw))

    assert lib.fdipt_mpnn_weights_floats(C.byref(dims())) == 1660485 == lib.fdipt_mpnn_weights_floats(C.byref(dims(ca_only=0)))
    assert lib.fdipt_mpnn_weights_floats(C.byref(dims(ca_only=1))) == CA_FLOATS == lib.fdipt_mpnn_weights_floats(C.byref(dims(ca_only=1, k_neighbors=30)))
    for bad in (2, -1):
        assert lib.fdipt_mpnn_weights_floats(C.byref(dims(ca_only=bad))) == _lib.EINVAL and lib.fdipt_mpnn_workspace(C.byref(dims(ca_only=bad)), 1, 10, 1) == 0
    # the workspace formula does not change
    assert lib.fdipt_mpnn_workspace(C.byref(dims(ca_only=1)), 2, 70, 3) == lib.fdipt_mpnn_workspace(C.byref(dims()), 2, 70, 3) > 0
    names = ("weights", "prot", "res_mask", "chain_mask", "residue_index", "chain_idx", "S", "decoding_order", "u", "omit", "bias", "E_idx", "log_probs",
             "S_out", "probs", "status", "workspace")

    def call(fn, d, n=10, atoms=37, workspace_bytes=1000):
        args = _lib.MpnnArgs(B=1, N=n, M=1, atoms=atoms, temperature=0.1, workspace_bytes=workspace_bytes, **{k: 64 for k in names})
        return fn(C.byref(d), C.byref(args), None)

    for fn in (lib.fdipt_mpnn_score, lib.fdipt_mpnn_design):
        assert call(fn, dims(ca_only=2)) == _lib.EINVAL
        assert call(fn, dims(ca_only=1), n=2) == call(fn, dims(ca_only=1), n=2, atoms=1) == call(fn, dims(ca_only=1), n=1) == _lib.EINVAL
        assert call(fn, dims(), atoms=1) == call(fn, dims(ca_only=1), atoms=14) == call(fn, dims(ca_only=1), atoms=3) == _lib.EINVAL
        # these pass every argument check and stop at the workspace size
        assert call(fn, dims(ca_only=1), atoms=1) == call(fn, dims(ca_only=1), atoms=5) == call(fn, dims(ca_only=1), atoms=37) == _lib.ESIZE
        assert call(fn, dims(ca_only=1), n=3, atoms=1) == call(fn, dims(), n=2) == _lib.ESIZE


def test_python_layer_reads_the_three_input_layouts_and_refuses_short_traces():
    model = inv.ProteinMPNN(ca_only=True)
    with pytest.raises(ValueError, match="at least 3"):
        model.score(np.zeros((1, 2, 3), np.float32), np.zeros((1, 2), int))
    with pytest.raises(ValueError, match="at least 3"):
        model.unconditional_probs(np.zeros((2, 5, 3), np.float32))               # [N,5,3]: ONE backbone of two rows
    with pytest.raises(ValueError, match="37, 3"):
        model.score(np.zeros((1, 8, 4, 3), np.float32), np.zeros((1, 8), int))
    with pytest.raises(ValueError, match="37, 3"):
        inv.ProteinMPNN().score(np.zeros((1, 8, 3), np.float32), np.zeros((1, 8), int))   # the vanilla model takes no trace


def test_fasta_header_names_a_ca_model():
    S = np.array([[[0, 1, 2, 3]]])
    result = {"S": S, "S_input": np.array([[9, 9, 9, 9]]), "res_mask": np.ones((1, 4), np.float32), "chain_mask": np.ones((1, 4), np.float32),
              "score": np.array([[1.0]], np.float32), "global_score": np.array([[2.0]], np.float32), "seq_recovery": np.array([[0.25]], np.float32),
              "temperature": 0.1, "seed": 38, "ca_only": True}
    head = inv.fasta_records(result, 0, "sample_1", model_name="v_48_020").splitlines()[0]
    assert head == ">sample_1, score=nan, global_score=nan, fixed_chains=[], designed_chains=['A'], CA_model_name=v_48_020, git_hash=unknown, seed=38"
    assert ", model_name=v_48_020," in inv.fasta_records(dict(result, ca_only=False), 0, "sample_1", model_name="v_48_020").splitlines()[0]
