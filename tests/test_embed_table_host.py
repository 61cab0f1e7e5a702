"""The predicate of the edge embedder's row table on the host side (no GPU): fdipt_embed_table_rows answers with the plan a whole forward
makes (csrc/model.hip: plan_forward, ForwardPlan.ee_table) — rows per sample and class pair where the table path runs, 0 where every pair
is evaluated."""
import ctypes as C

import pytest


def _dims(prec="fp16", **over):
    from framedipt_amd import _lib, config
    from framedipt_amd.model.score_network import dims_from_conf
    conf = config.base_config()
    d = dims_from_conf(conf.model, conf.diffuser, False, {"fp16": _lib.PREC_F16, "fp16x": _lib.PREC_F16X, "fp32": _lib.PREC_F32}[prec])
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _rows(d, b, n, n_rel):
    from framedipt_amd import _lib
    return int(_lib.load().fdipt_embed_table_rows(C.byref(d), b, n, n_rel))


@pytest.mark.parametrize("prec", ["fp16", "fp16x"])
def test_rows_against_half_the_pairs(prec):
    """One chain (n_rel = 2 N - 1), 22 bins + the overflow row: (2 N - 1) * 23 <= N^2 / 2 from N = 92 on."""
    d = _dims(prec)
    assert d.num_bins == 22 and not d.use_aatype
    assert _rows(d, 2, 64, 127) == 0 and _rows(d, 2, 88, 175) == 0
    for n in (92, 96, 100, 128, 300):
        assert _rows(d, 2, n, 2 * n - 1) == (2 * n - 1) * 23, n
    assert _rows(d, 8, 300, 599) == 13777


def test_what_declines():
    from framedipt_amd import _lib
    d = _dims()
    n = 128
    assert _rows(d, 2, n, 295) == 295 * 23        # a chain break of 20 positions: still <= 5 N / 2 and <= N^2 / 2 rows
    assert _rows(d, 2, n, 5 * n // 2) == 320 * 23
    assert _rows(d, 2, n, 5 * n // 2 + 1) == 0    # more relative positions than the workspace region holds
    assert _rows(d, 2, n, 357) == 0               # 357 * 23 = 8211 rows > 128^2 / 2
    assert _rows(d, 2, 126, 251) == 0             # N % 4 != 0: not on edge_transition4
    assert _rows(d, 8, 300, 599) > 0 and _rows(d, 24, 300, 599) == 0   # 64 MB cap: 24 * 13777 * 352 B = 116 MB
    assert _rows(_dims("fp32"), 2, n, 255) == 0
    assert _rows(_dims(use_aatype=1), 2, n, 255) == 0
    assert _rows(_dims(num_bins=0), 2, n, 255) == 0
    for flag in (_lib.KF_ET3, _lib.KF_GENERIC_PAIR, _lib.KF_GENERIC_ATTN, _lib.KF_UNFOLDED, _lib.KF_PASS_Z, _lib.KF_UNFUSED_NODE):
        assert _rows(_dims(kernel_flags=flag), 2, n, 255) == 0, flag
    for flag in (_lib.KF_NO_MERGE, _lib.KF_ROWS32, _lib.KF_POINTS_LAUNCH):
        assert _rows(_dims(kernel_flags=flag), 2, n, 255) == 255 * 23, flag


def test_the_workspace_holds_the_table_where_the_shape_allows_it():
    """Table (four class pairs of 5 N / 2 relative positions, + the zero row, 352 B per row) and row index (4 B per pair), each rounded
    up to 256 B, against the same dims with a flag that keeps the per-pair launch."""
    from framedipt_amd import _lib
    lib = _lib.load()
    b, n = 8, 300
    with_table = lib.fdipt_forward_workspace_bytes(C.byref(_dims()), b, n)
    without = lib.fdipt_forward_workspace_bytes(C.byref(_dims(kernel_flags=_lib.KF_PASS_Z)), b, n)
    al = lambda x: -(-x // 256) * 256  # noqa: E731
    assert with_table - without == al(b * (4 * 750 * 23 + 1) * 352) + al(b * n * n * 4)
    assert lib.fdipt_forward_workspace_bytes(C.byref(_dims()), 2, 64) == lib.fdipt_forward_workspace_bytes(C.byref(_dims(kernel_flags=_lib.KF_PASS_Z)), 2, 64)
