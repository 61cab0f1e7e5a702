"""GPU parity tests (-m gpu) of the edge embedder's row table (csrc/edge_embed2.hip: fd_edge_embed2_table, fd_edge_embed2_spread;
csrc/model.hip: ForwardPlan.ee_table): the distinct (class_i, class_j, rel, bin) rows evaluated once and spread to the pairs, against
FdiptForwardArgs.pair_embed = 1 (every pair evaluated by edge_embed2_kernel: the path of the parent revision).  A whole forward with and
without the switch: frames, psi, both scores and the node rows of every block.  The table rows go through the arithmetic of the pair kernel (same
association of the layer-1 addends, same conversions, same hi + lo down_z), and the spread finds a pair's row with the pair kernel's own
rel / bin code."""
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


def _inputs(n, b, seed, gap_at=None, window=None, holes=False, priming=False):
    """Random inputs of one forward: a CA random walk (3.8 A steps: every distogram bin and the overflow bin occur), random frames."""
    rng = np.random.default_rng(seed)
    seq = np.tile(np.arange(n, dtype=np.int64), (b, 1))
    if gap_at is not None:  # a second chain behind a gap of 20 positions
        seq[:, gap_at:] += 20
    fixed = np.zeros((b, n), np.float32)
    if window is not None:
        fixed[:, :] = 1.0
        fixed[:, window[0]:window[1]] = 0.0  # the diffused window; sample 1 keeps one class
        if b > 1:
            fixed[1] = 0.0
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
    return dict(seq=seq, fixed=fixed, mask=mask, rigids=rigids, sc=sc, psi=psi, t=np.full(b, 0.37))


def _forward(net, x, pair_embed):
    """One forward; also the table rows fdipt_embed_table_rows names for its shape (0: the predicate declines)."""
    import ctypes as C
    from framedipt_amd import _lib
    from framedipt_amd.model.score_network import BatchState
    dev = lambda v: torch.as_tensor(v, device="cuda").contiguous()  # noqa: E731
    st = BatchState(net, torch.as_tensor(x["seq"]))
    st.pair_embed = pair_embed
    b, n = x["seq"].shape
    d = net.dims
    st.trace_node = torch.zeros(d.num_blocks + 1, b, n, d.c_s, dtype=torch.float32, device="cuda")  # (no trace_edge: a traced pair rep keeps the pair kernel)
    t32, temb, sig = net.step_scalars(x["t"])
    st.forward(dev(x["rigids"]), dev(x["mask"]), dev(x["fixed"]), dev(x["sc"]), None, dev(x["psi"]), dev(t32), dev(temb), dev(sig))
    torch.cuda.synchronize()
    out = {k: getattr(st, k).cpu().numpy().copy() for k in OUT}
    return out, int(_lib.load().fdipt_embed_table_rows(C.byref(net.dims), b, n, st.n_rel))


def _compare(tag, a, b):
    m = np.isfinite(b["trace_node"]).all() and np.isfinite(a["trace_node"]).all()
    rels = [float(np.linalg.norm(a["trace_node"][k] - b["trace_node"][k]) / np.linalg.norm(b["trace_node"][k])) for k in range(1, a["trace_node"].shape[0])]
    dca = float(np.abs(a["rigids"][..., 4:] - b["rigids"][..., 4:]).max())
    dpsi = float(np.abs(a["psi"] - b["psi"]).max())
    dsc = max(float(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()) for k in ("rot_score", "trans_score"))
    same = all(np.array_equal(a[k], b[k]) for k in OUT)
    print(f"{tag}: table vs pair kernel: bit-identical {same}, node rel per block [{' '.join(f'{r:.1e}' for r in rels)}], frames max {dca:.2e} A, "
          f"psi max {dpsi:.2e}, scores rel {dsc:.2e}")
    assert m
    # the tolerances of a path comparison (test_gpu_proj_points.py), where the compiler contracts the two instantiations differently
    for blk, rel in enumerate(rels, 1):
        assert rel < 5e-5, (tag, blk, rel)
    assert dca < 1e-4 and dpsi < 1e-4 and dsc < 1e-4, (tag, dca, dpsi, dsc)
    return same


CASES = {
    # de novo, B = 2: N = 92 is the smallest length of the predicate (rows of a class pair (2 N - 1) * 23 <= N^2 / 2), then 96, 100, 128
    "denovo_n92": dict(n=92, b=2),
    "denovo_n96": dict(n=96, b=2),
    "denovo_n100": dict(n=100, b=2),
    "denovo_n128": dict(n=128, b=2),
    # inpainting, N = 128: two chains with a seq_idx gap, a diffused window (2 x 2 classes in sample 0, one class in sample 1), masked rows
    "inpaint_n128": dict(n=128, b=2, gap_at=70, window=(30, 52), holes=True),
    # a priming-style forward: sc_ca_t = 0, every distance in one bin
    "priming_n128": dict(n=128, b=2, priming=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_row_table_against_the_pair_kernel(net, case):
    """Inside the predicate (fdipt_embed_table_rows > 0: the plan the forward itself makes) the two paths run different launches and give
    the same forward — bit for bit (measured on MI355X, fp16 and fp16x, every case: the table rows are the pair kernel's arithmetic
    instruction for instruction, and a masked pair's zero row differs from the pair kernel's signed zeros only where the next mask
    multiplies)."""
    kw = CASES[case]
    x = _inputs(seed=sum(map(ord, case)), **kw)
    (a, rows), (b, _) = _forward(net, x, 0), _forward(net, x, 1)
    assert rows > 0, "the predicate declined"
    assert _compare(case, a, b), "not bit-identical"


@pytest.mark.parametrize("n", [64, 88])
def test_outside_the_predicate_the_switch_changes_nothing(net, n):
    """N = 64 and N = 88 (the largest length below the predicate: 175 * 23 rows > 88^2 / 2): the same launches with and without
    pair_embed, every output bit for bit."""
    x = _inputs(n, 2, seed=n)
    (a, rows), (b, _) = _forward(net, x, 0), _forward(net, x, 1)
    assert rows == 0
    for k in OUT:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
