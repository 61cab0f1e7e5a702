"""FDIPT_KF_STREAM_ATTN on the host side (no GPU): the flag is a valid kernel_flags bit and the workspace query covers N <= 2048."""
import ctypes as C


def test_stream_attn_flag_is_accepted_and_sizes_the_workspace():
    from framedipt_amd import _lib, config
    from framedipt_amd.model.score_network import dims_from_conf
    lib = _lib.load()
    conf = config.base_config()
    d = dims_from_conf(conf.model, conf.diffuser, False, _lib.PREC_F16)
    d.kernel_flags = _lib.KF_STREAM_ATTN
    assert lib.fdipt_param_count(C.byref(d)) > 0
    w1024, w2048 = lib.fdipt_forward_workspace_bytes(C.byref(d), 1, 1024), lib.fdipt_forward_workspace_bytes(C.byref(d), 1, 2048)
    assert 0 < w1024 < w2048 < 1 << 40
    # every bit up to this one but the retired 32 is a flag; the next one is not
    d.kernel_flags = 2 * _lib.KF_STREAM_ATTN - 1 - 32
    assert lib.fdipt_param_count(C.byref(d)) > 0
    d.kernel_flags = 2 * _lib.KF_STREAM_ATTN - 1
    assert lib.fdipt_param_count(C.byref(d)) == -1
    d.kernel_flags = 2 * _lib.KF_STREAM_ATTN
    assert lib.fdipt_param_count(C.byref(d)) == -1
