"""A torch restatement of the CA-only inverse-folding contract in this project's own words, on top of
tests/mpnn_ref.py: ``encode_ca`` builds the 167 edge inputs from the CA trace alone and runs the shared encoder; its result has the
layout of ``mpnn_ref.encode``, so ``mpnn_ref.score`` / ``design`` and the modes of tests/mpnn_controls_ref.py take it unchanged.  One
backbone at a time, any dtype and device.  The GPU tests compare the kernels with it, tests/test_mpnn_ca_host.py compares it with the
reference's recorded outputs (tests/golden/mpnn_ca_<case>.npz, written by tests/golden/make_goldens_mpnn_ca.py).
"""
import math

import numpy as np
import torch

import mpnn_ref as mr
from mpnn_ref import M, VOCAB, WEIGHT_SEED, TOLERANCE_FACTOR, Model, design, pick, score, valid_choice  # noqa: F401

# the nine RBF blocks: (shifted trace of row i, shifted trace of neighbour j); 0 = the row before, 1 = the row, 2 = the row after
PAIRS = [(1, 1), (0, 0), (2, 2), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
STEP_LO, STEP_HI = 3.6, 4.0   # a CA step outside this open interval is zeroed in the orientation frames

# name: (B, N, K); every case uses M = 2 sequences
CASES = {"ca_a": (1, 20, 48), "ca_b": (2, 70, 48), "ca_c": (1, 130, 48), "ca_d": (1, 40, 30), "ca_e": (1, 3, 48), "ca_f": (1, 7, 48)}
TEMPERATURES = {"ca_a": (1.0,), "ca_b": (1.0, 0.1), "ca_c": (1.0,), "ca_d": (1.0,), "ca_e": (1.0,), "ca_f": (1.0,)}
# The largest deviation of the reference's float32 outputs (CPU, ca_only=True) from this restatement in float64 over the rows with
# res_mask of the six fixtures, as printed by tests/golden/make_goldens_mpnn_ca.py (log_probs: 5.705e-6 in case ca_c; probs: 3.584e-6 in
# case ca_b at T = 0.1); the tests assert mpnn_ref.TOLERANCE_FACTOR times it.  Measured against the reference, never against the device.
DEVIATION = {"log_probs": 5.71e-6, "probs": 3.59e-6}


def bound(what):
    return TOLERANCE_FACTOR * DEVIATION[what]


def unit(x):
    """x / max(|x|, 1e-12) along the last axis: every ``normalize`` of the contract."""
    return x / torch.clamp(torch.sqrt((x * x).sum(-1, keepdim=True)), min=1e-12)


def shifted(ca):
    """[3,N,3]: the trace shifted along the array - row i-1 (row 0: the zero vector), row i, row i+1 (last row: the zero vector)."""
    zero = torch.zeros_like(ca[:1])
    return torch.stack([torch.cat([zero, ca[:-1]]), ca, torch.cat([ca[1:], zero])])


def steps(ca):
    """The kept unit steps u [N-1,3] (a step outside 3.6 .. 4.0 A is the zero vector) and the step lengths [N-1]."""
    dx = ca[1:] - ca[:-1]
    length = torch.sqrt((dx * dx).sum(-1))
    keep = (length > STEP_LO) & (length < STEP_HI)
    return unit(dx * keep[:, None].to(dx.dtype)), length


def frames(ca):
    """O [N,3,3], rows o_1, n_2, o_1 x n_2 for rows 1 .. N-3; zero at row 0 and the last two rows.  Always the geometric cross product."""
    n = ca.shape[0]
    o = torch.zeros((n, 3, 3), device=ca.device, dtype=ca.dtype)
    if n > 3:
        u, _ = steps(ca)
        u2, u1 = u[:-2], u[1:-1]          # row i of 1 .. N-3: the step into it and the step out of it
        o1 = unit(u2 - u1)
        n2 = unit(torch.cross(u2, u1, dim=-1))
        o[1:n - 2] = torch.stack([o1, n2, torch.cross(o1, n2, dim=-1)], dim=1)
    return o


def quaternions(r):
    """Q [...,4] of R [...,3,3] by the contract's formulas: sign(antisymmetric part) * 0.5 sqrt(|1 + ...|), sqrt(relu(1 + trace)) / 2."""
    xx, yy, zz = r[..., 0, 0], r[..., 1, 1], r[..., 2, 2]
    mag = 0.5 * torch.sqrt(torch.abs(1 + torch.stack([xx - yy - zz, -xx + yy - zz, -xx - yy + zz], -1)))
    anti = torch.stack([r[..., 2, 1] - r[..., 1, 2], r[..., 0, 2] - r[..., 2, 0], r[..., 1, 0] - r[..., 0, 1]], -1)
    w = torch.sqrt(torch.relu(1 + xx + yy + zz))[..., None] / 2
    return unit(torch.cat([torch.sign(anti) * mag, w], -1)), anti


def edge_inputs(model, ca_trace, res_mask, residue_index, chain_idx):
    """The 167 inputs of edge_embedding [N,K,167], E_idx, the adjusted distances [N,N], R [N,K,3,3] and its antisymmetric part."""
    mask = model.t(res_mask)
    ca = model.t(ca_trace)
    e_idx, d_nb, d_adj = mr.neighbours(model, ca, mask)
    tr = shifted(ca)
    blocks = []
    for p, (ai, aj) in enumerate(PAIRS):
        d = d_nb if p == 0 else torch.sqrt(((tr[ai][:, None] - tr[aj][e_idx]) ** 2).sum(-1) + 1e-6)
        blocks.append(mr.rbf(model, d))
    o = frames(ca)
    du = unit(torch.einsum("irc,ikc->ikr", o, ca[e_idx] - ca[:, None]))
    r = torch.einsum("ira,ikrb->ikab", o, o[e_idx])
    q, anti = quaternions(r)
    ri, ch = model.t(residue_index, torch.int64), model.t(chain_idx, torch.int64)
    same = ch[:, None] == ch[e_idx]
    klass = torch.where(same, torch.clamp(ri[:, None] - ri[e_idx] + 32, 0, 64), torch.full_like(e_idx, 65))
    pos = model.p["features.embeddings.linear.weight"].T[klass] + model.p["features.embeddings.linear.bias"]
    return torch.cat([pos] + blocks + [du, q], dim=-1), e_idx, d_adj, r, anti


def encode_ca(model, ca_trace, res_mask, residue_index, chain_idx, details=None):
    """h_V [N,128], h_E [N,K,128], E_idx [N,K] and the gap between the K-th and (K+1)-th distance per row (inf where N <= K): the tuple
    of ``mpnn_ref.encode``.  ca_trace [N,3].  ``details``: a dict that receives what the fixture conditions read (``min_anti``: the
    smallest antisymmetric component of R over the edges other than self edges whose R is not zero; ``step_margin``: the distance of
    the nearest CA step from 3.6 or 4.0; ``self_q``: Q on the self edges of the rows with res_mask whose R is not zero)."""
    mask = model.t(res_mask)
    e, e_idx, d_adj, r, anti = edge_inputs(model, ca_trace, res_mask, residue_index, chain_idx)
    n, k = e_idx.shape
    if n > k:
        srt = torch.sort(d_adj, dim=-1)[0]
        gap = (srt[:, k] - srt[:, k - 1]).cpu().numpy()
    else:
        gap = np.full(n, np.inf)
    if details is not None:
        rows = torch.arange(n, device=e_idx.device)[:, None]
        live = (e_idx != rows) & (r.abs().amax((-1, -2)) > 0)
        details["min_anti"] = float(anti.abs()[live].min()) if bool(live.any()) else math.inf
        _, length = steps(model.t(ca_trace))
        details["step_margin"] = float(torch.minimum((length - STEP_LO).abs(), (length - STEP_HI).abs()).min())
        framed = (e_idx == rows) & (r.abs().amax((-1, -2)) > 0) & (mask[:, None] != 0)
        details["self_q"] = e[..., -4:][framed].cpu().numpy()
    h_e = model.lin("W_e", model.ln("features.norm_edges", model.lin("features.edge_embedding", e)))
    h_v = torch.zeros((n, 128), device=model.device, dtype=model.dtype)
    attend = mask[:, None] * mask[e_idx]
    for l in range(3):
        layer = f"encoder_layers.{l}"
        cat = torch.cat([h_v[:, None].expand(-1, k, -1), h_e, h_v[e_idx]], dim=-1)
        dh = (attend[..., None] * model.message(layer, ("W1", "W2", "W3"), cat)).sum(-2) / 30.0
        h_v = mask[:, None] * model.node_tail(layer, h_v, dh)
        cat = torch.cat([h_v[:, None].expand(-1, k, -1), h_e, h_v[e_idx]], dim=-1)
        h_e = model.ln(f"{layer}.norm3", h_e + model.message(layer, ("W11", "W12", "W13"), cat))
    return h_v, h_e, e_idx, gap


# ------------------------------------------------------------------------------------------------ inputs
def trace(rng, n, step=3.8):
    """[N,3] float64: a random-walk CA trace with steps of ``step`` A (a number, or one length per step)."""
    d = rng.standard_normal((n, 3))
    d *= (np.broadcast_to(step, (n,)) / np.linalg.norm(d, axis=-1))[:, None]
    return np.cumsum(d, axis=0)


# case ca_c, inside chain 1: the step INTO the row has this length (two zeroed steps, two kept ones near the limits)
STEPS_C = {20: 3.3, 25: 4.3, 52: 3.65, 56: 3.95}


def make_case(name, seed):
    """The inputs of fixture case ``name`` from an input seed: ca [B,N,3] float32, res_mask, chain_mask, residue_index, chain_idx [B,N],
    S [B,N] letters, decoding_order [B,M,N], u [B,M,N], and the normal draw randn [B,M,N] the orders were sorted from."""
    b, n, _ = CASES[name]
    rng = np.random.default_rng((seed, sum(ord(c) for c in name)))
    lengths = np.full(n, 3.8)
    if name == "ca_c":
        for row, length in STEPS_C.items():
            lengths[row] = length
    ca = np.stack([trace(rng, n, lengths) for _ in range(b)])
    res_mask, chain_mask = np.ones((b, n), np.float32), np.ones((b, n), np.float32)
    residue_index, chain_idx = np.tile(np.arange(n, dtype=np.int32), (b, 1)), np.ones((b, n), np.int32)
    if name == "ca_c":  # two chains, the second displaced by 150 A; a numbering break; 7 masked tail rows; 20 fixed rows
        chain_idx[:, 60:] = 2
        residue_index[:, 60:] += 100
        shift = rng.standard_normal(3)
        ca[:, 60:] += 150.0 * shift / np.linalg.norm(shift)
        res_mask[:, -7:] = 0
        chain_mask[:, 30:50] = 0
    S = rng.integers(0, 20, size=(b, n)).astype(np.int64)
    gen = torch.Generator().manual_seed(int(seed) * 131 + sum(ord(c) for c in name))
    randn = torch.randn((b, M, n), generator=gen)
    order = torch.argsort((torch.from_numpy(chain_mask * res_mask)[:, None] + 0.0001) * torch.abs(randn), dim=-1).numpy()
    u = torch.rand((b, M, n), generator=gen, dtype=torch.float32).numpy()
    return {"ca": ca.astype(np.float32), "res_mask": res_mask, "chain_mask": chain_mask, "residue_index": residue_index, "chain_idx": chain_idx,
            "S": S, "decoding_order": order, "u": u, "randn": randn.numpy()}


def run_case(sd, name, case, dtype=torch.float64, device="cpu"):
    """The restatement on every backbone and sequence of a case: E_idx, gap, log_probs [B,M,N,21], per temperature S, probs, margin, and
    the fixture conditions of the features (min_anti, step_margin, self_q: ``encode_ca``)."""
    b, n, k = CASES[name]
    model = Model(sd, k, dtype, device)
    omit, bias = mr.omit_bias()
    out = {"E_idx": [], "gap": [], "log_probs": [], "min_anti": math.inf, "step_margin": math.inf, "self_q": [],
           "design": {t: {"S": [], "probs": [], "margin": math.inf} for t in TEMPERATURES[name]}}
    for i in range(b):
        details = {}
        enc = encode_ca(model, case["ca"][i], case["res_mask"][i], case["residue_index"][i], case["chain_idx"][i], details)
        out["min_anti"], out["step_margin"] = min(out["min_anti"], details["min_anti"]), min(out["step_margin"], details["step_margin"])
        out["self_q"].append(details["self_q"])
        out["E_idx"].append(enc[2].cpu().numpy())
        out["gap"].append(enc[3])
        out["log_probs"].append(np.stack([score(model, enc, case["res_mask"][i], case["S"][i], case["decoding_order"][i, m]).cpu().numpy() for m in range(M)]))
        for t, d in out["design"].items():
            runs = [design(model, enc, case["res_mask"][i], case["chain_mask"][i], case["S"][i], case["decoding_order"][i, m], case["u"][i, m], t, omit, bias)
                    for m in range(M)]
            d["S"].append(np.stack([r[0].cpu().numpy() for r in runs]))
            d["probs"].append(np.stack([r[1].cpu().numpy() for r in runs]))
            d["margin"] = min([d["margin"]] + [r[2] for r in runs])
    for key in ("E_idx", "gap", "log_probs"):
        out[key] = np.stack(out[key])
    out["self_q"] = np.concatenate(out["self_q"])
    for d in out["design"].values():
        d["S"], d["probs"] = np.stack(d["S"]), np.stack(d["probs"])
    return out
