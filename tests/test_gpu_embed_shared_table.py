"""GPU tests (-m gpu) of the shared rows of the edge embedder's row table (csrc/edge_embed2.hip: ee2_leaders_kernel, the TABLE launch,
ee2_spread_kernel; csrc/model.hip: embed_stage).  Samples whose first-layer rows carry the same bits read ONE set of table rows, those of
their leader; which sample leads is decided on the device and read back here through fdipt_embed_table_leaders.

Every case runs one whole forward on the table path and one with FdiptForwardArgs.pair_embed = 1 (every pair evaluated by
edge_embed2_kernel) and compares frames, psi, both scores and the node rows of every block bit for bit, then asserts the leaders.
Shapes: N = 92 (the smallest length inside the predicate), N = 100 (no multiple of 16 or 32: ragged key tiles) and N = 128."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OUT = ("rigids", "psi", "rot_score", "trans_score", "trace_node")


@pytest.fixture(scope="module", params=["fp16", "fp16x"])
def net(request):
    from framedipt_amd import config
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    conf = config.base_config()
    d = SE3Diffuser(conf.diffuser, device="cuda")
    return ScoreNetwork(conf.model, d, precision=request.param).load_synthetic(7).to("cuda")


def _inputs(n, b, seed, t=0.37, two_class=(), gap_at=None, holes=False, priming=False):
    """Random inputs of one forward (a CA random walk of 3.8 A steps, random frames).  ``two_class``: the samples that keep a motif
    (fixed_mask = 1) around a diffused window; every other sample is diffused throughout (one class)."""
    rng = np.random.default_rng(seed)
    seq = np.tile(np.arange(n, dtype=np.int64), (b, 1))
    if gap_at is not None:  # a second chain behind a gap of 20 positions
        seq[:, gap_at:] += 20
    fixed = np.zeros((b, n), np.float32)
    for s in two_class:
        fixed[s] = 1.0
        fixed[s, 30:52] = 0.0
    mask = np.ones((b, n), np.float32)
    if holes:
        mask[:, 5] = 0.0
        mask[0, n - 3:] = 0.0
        mask[b - 1, 40:47] = 0.0
    steps = rng.standard_normal((b, n, 3))
    ca = np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=-1, keepdims=True), axis=1).astype(np.float32)
    q = rng.standard_normal((b, n, 4))
    rigids = np.concatenate([q / np.linalg.norm(q, axis=-1, keepdims=True), ca + rng.standard_normal((b, n, 3))], -1).astype(np.float32)
    sc = np.zeros_like(ca) if priming else ca
    psi = rng.standard_normal((b, n, 2)).astype(np.float32)
    return dict(seq=seq, fixed=fixed, mask=mask, rigids=rigids, sc=sc, psi=psi, t=np.broadcast_to(np.asarray(t, np.float64), (b,)).copy())


def _forward(net, x, pair_embed, rel_rows_differ=False):
    """One forward: its outputs, the table rows fdipt_embed_table_rows names for its shape, and (table path) the leaders it left."""
    from framedipt_amd import _lib
    from framedipt_amd.model.score_network import BatchState
    lib = _lib.load()
    dev = lambda v: torch.as_tensor(v, device="cuda").contiguous()  # noqa: E731
    st = BatchState(net, torch.as_tensor(x["seq"]))
    st.pair_embed = pair_embed
    b, n = x["seq"].shape
    d = net.dims
    if rel_rows_differ:  # `setup` made again from a rel_emb whose last sample differs from the others in one element
        from framedipt_amd import embedding
        rel_emb = np.broadcast_to(embedding.get_index_embedding(np.arange(st.n_rel) - st.rel_off, d.index_embed)[None], (b, st.n_rel, d.index_embed)).copy()
        rel_emb[b - 1, st.n_rel // 2, 3] += 0.25
        rel_emb = dev(rel_emb.astype(np.float32))
        _lib.check(lib.fdipt_sample_setup(C.byref(d), _lib.ptr(net.params), _lib.ptr(net.derived), b, n, st.n_rel, _lib.ptr(rel_emb), _lib.ptr(st.setup),
                                          _lib.stream_ptr()), "sample_setup")
    st.trace_node = torch.zeros(d.num_blocks + 1, b, n, d.c_s, dtype=torch.float32, device="cuda")
    t32, temb, sig = net.step_scalars(x["t"])
    st.forward(dev(x["rigids"]), dev(x["mask"]), dev(x["fixed"]), dev(x["sc"]), None, dev(x["psi"]), dev(t32), dev(temb), dev(sig))
    torch.cuda.synchronize()
    out = {k: getattr(st, k).cpu().numpy().copy() for k in OUT}
    rows = int(lib.fdipt_embed_table_rows(C.byref(d), b, n, st.n_rel))
    leaders = None
    if not pair_embed and rows > 0:
        got = torch.full((b,), -1, dtype=torch.int32, device="cuda")
        _lib.check(lib.fdipt_embed_table_leaders(C.byref(d), _lib.ptr(st.ws), b, n, st.n_rel, _lib.ptr(got)), "embed_table_leaders")
        leaders = got.cpu().tolist()
    return out, rows, leaders


# name -> (inputs, leaders)
CASES = {
    # one t for the batch (what inference_fn, run_sharded and the benchmark do): one leader
    "equal_t_n92": (dict(n=92, b=2), [0, 0]),
    "equal_t_n100": (dict(n=100, b=2), [0, 0]),
    "equal_t_n128": (dict(n=128, b=2), [0, 0]),
    # per-sample t: a follower must not take the rows of another t, and a later sample finds the earlier one of its own t
    "three_t_n92": (dict(n=92, b=3, t=[0.37, 0.52, 0.37]), [0, 1, 0]),
    "three_t_n100": (dict(n=100, b=3, t=[0.37, 0.52, 0.37]), [0, 1, 0]),
    # mixed classes at one t: a one-class sample follows a two-class one; a two-class sample cannot follow a one-class one
    "two_class_first_n100": (dict(n=100, b=2, two_class=(0,)), [0, 0]),
    "one_class_first_n100": (dict(n=100, b=2, two_class=(1,)), [0, 1]),
    "one_two_one_class_n92": (dict(n=92, b=3, two_class=(1,)), [0, 1, 0]),
    # ... with two chains (a seq_idx gap of 20) and masked rows
    "two_class_first_gap_holes_n128": (dict(n=128, b=2, two_class=(0,), gap_at=70, holes=True), [0, 0]),
    "one_class_first_gap_holes_n128": (dict(n=128, b=2, two_class=(1,), gap_at=70, holes=True), [0, 1]),
    # a priming-style forward: sc_ca_t = 0, every distance in one bin
    "priming_n128": (dict(n=128, b=2, priming=True), [0, 0]),
    # the relative-position rows are laid out per sample: where a caller's differ, the sample leads itself
    "rel_rows_differ_n100": (dict(n=100, b=2, rel_rows_differ=True), [0, 1]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_shared_rows_against_the_pair_kernel(net, case):
    """The table path with shared rows gives the forward of the per-pair path bit for bit, and the device chose the leaders the rule names:
    the first sample b' <= b that has b's classes and whose Pi / Pj rows of those classes and R rows carry b's bits."""
    kw, want = CASES[case]
    kw = dict(kw)
    differ = kw.pop("rel_rows_differ", False)
    x = _inputs(seed=sum(map(ord, case)), **kw)
    (a, rows, leaders), (b, _, _) = _forward(net, x, 0, differ), _forward(net, x, 1, differ)
    assert rows > 0, "the predicate declined: the case would not run the table"
    for k in OUT:
        assert np.isfinite(a[k]).all() and np.isfinite(b[k]).all(), k
    worst = {k: float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()) for k in OUT}
    print(f"{case}: leaders {leaders}, max |table - per pair| {worst}")
    assert leaders == want
    for k in OUT:
        assert np.array_equal(a[k], b[k]), (case, k, worst[k])
