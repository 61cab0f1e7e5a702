"""FDIPT_PREC_F16X on the host side (no GPU): the fp16 mode's parameter inventory, a derived blob that grows by the lo images of the
split terms, the size queries and the Python surfaces that name the mode."""
import ctypes as C

import torch


def _dims(precision, size="full"):
    from framedipt_amd import config
    from framedipt_amd.model.score_network import dims_from_conf
    conf = config.base_config() if size == "full" else config.small_config()
    return dims_from_conf(conf.model, conf.diffuser, False, precision)


def test_header_and_python_agree_on_the_mode():
    from framedipt_amd import _lib
    from framedipt_amd.model.score_network import PRECISIONS
    assert PRECISIONS["fp16x"] == _lib.PREC_F16X == 3  # (_lib reads the value from FDIPT_PREC_F16X of include/fdipt.h)


def test_same_parameters_as_fp16_and_a_larger_blob():
    from framedipt_amd import _lib
    lib = _lib.load()
    d16, dx = _dims(_lib.PREC_F16), _dims(_lib.PREC_F16X)
    n = lib.fdipt_param_count(C.byref(d16))
    assert n > 0 and lib.fdipt_param_count(C.byref(dx)) == n
    assert all(lib.fdipt_param_offset(C.byref(dx), i) == lib.fdipt_param_offset(C.byref(d16), i) for i in range(n + 1))
    b16, bx = lib.fdipt_derived_bytes(C.byref(d16)), lib.fdipt_derived_bytes(C.byref(dx))
    # per EdgeTransition (num_blocks - 1 of them) the 640 KB fp16x stream (the final layer's lo fragments beside the hi ones) takes the place
    # of the 512 KB fp16 stream and of edge_transition3's 640 KB stream, which fp16x never runs; the edge embedder's 64 KB of layer-2/3 images
    # gain their 64 KB of lo images; everything else is the fp16 blob
    assert b16 > 0 and bx == b16 + (dx.num_blocks - 1) * (640 - 512 - 640) * 1024 + 64 * 1024
    for B, N in ((1, 64), (8, 300), (1, 1024)):
        w16, wx = lib.fdipt_forward_workspace_bytes(C.byref(d16), B, N), lib.fdipt_forward_workspace_bytes(C.byref(dx), B, N)
        assert 0 < w16 <= wx
    # the small widths pass the size queries (the forward refuses them: no split kernel at those widths)
    assert lib.fdipt_derived_bytes(C.byref(_dims(_lib.PREC_F16X, "small"))) > 0
    # precision 7 stays invalid, and the mode takes kernel_flags like the others (the refusals are the forward's)
    assert lib.fdipt_param_count(C.byref(_dims(7))) == -1
    dx.kernel_flags = _lib.KF_ET3
    assert lib.fdipt_param_count(C.byref(dx)) == n


def test_score_network_and_checkpoint_take_fp16x(tmp_path, monkeypatch):
    from framedipt_amd import _lib, checkpoint, config
    from framedipt_amd import weights as W
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    conf = config.small_config()
    net = ScoreNetwork(conf.model, SE3Diffuser(conf.diffuser, device="cpu"), precision="fp16x")
    assert net.precision == _lib.PREC_F16X and net.dims.precision == _lib.PREC_F16X
    sd = W.synth_state_dict(W.param_shapes(conf.model), 3)
    ckpt_conf = {"model": {"node_embed_size": 64, "edge_embed_size": 32,
                           "embed": {"index_embed_size": 32, "num_bins": 22, "min_bin": 1e-5, "max_bin": 20.0},
                           "ipa": {"c_s": 64, "c_z": 32, "c_hidden": 16, "c_skip": 16, "no_heads": 4, "no_qk_points": 4,
                                   "no_v_points": 6, "seq_tfmr_num_heads": 2, "seq_tfmr_num_layers": 1, "num_blocks": 2}},
                 "diffuser": {"r3": {"min_b": 0.1, "max_b": 20.0, "coordinate_scaling": 0.1}}}
    torch.save({"model": {k: torch.tensor(v) for k, v in sd.items()}, "conf": ckpt_conf}, tmp_path / "m.pth")
    monkeypatch.setattr(ScoreNetwork, "to", lambda self, device: self)  # (the upload needs a GPU)
    _, _, model = checkpoint.load_model(tmp_path / "m.pth", precision="fp16x", device="cpu")
    assert model.precision == _lib.PREC_F16X
    lib = _lib.load()
    assert lib.fdipt_param_count(C.byref(model.dims)) == len(sd)

