"""GPU edge-case parity (-m gpu) of the confidence-walk kernels at the end of framedipt_amd/csrc/frames.hip — se3_forward_step_kernel,
se3_forward_step_gen_kernel, se3_step_log_prob_kernel, se3_prior_log_prob_kernel — on the cases of tests/confidence_cases.py: one row,
partial waves, one, two and three passes of the 256-thread row loop, several samples per launch with one that has no diffused residue,
NULL / binary / fractional masks, scores present and absent, rotations carried across pi, exact half turns, the ends of the walk.

Every comparison is against the float64 NumPy restatement (oracle/diffuser.py: forward, step_log_prob_terms, prior_log_prob), which
tests/test_oracle_diffuser.py holds to the reference's recorded walks; tests/test_confidence_cases_host.py shows on the CPU that the
inputs meet the conditions these assertions rest on and measures the log-probability tolerance (confidence_cases.DEVIATION)."""
import numpy as np
import pytest
import torch

import confidence_cases as cc
import frames_cases as fc
from oracle import diffuser as od
from oracle import frames as fr

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    from framedipt_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def odiff():
    from framedipt_amd import config
    return od.SE3Diffuser(config.base_config().diffuser)


def _consts(odiff):
    so3, r3 = odiff._so3_diffuser, odiff._r3_diffuser
    return (float(so3.min_sigma), float(so3.max_sigma), float(r3.min_b), float(r3.max_b), float(r3._conf.coordinate_scaling))


def _call(lib, name, *args):
    from framedipt_amd import _lib
    _lib.check(getattr(lib, name)(*[_lib.ptr(a) if torch.is_tensor(a) else a for a in args], _lib.stream_ptr()), name)


# ---------------------------------------------------------------- step log-probabilities
@pytest.mark.parametrize("B,N", cc.LOGPROB_SIZES)
def test_step_log_prob_edges_vs_oracle(lib, odiff, B, N):
    """fdipt_se3_step_log_prob, 36 cases per (B, N): each of the four columns — backward trans, backward rot, forward trans, forward rot
    — of each sample within TOLERANCE_FACTOR * DEVIATION * sum_rows |row term| of the restatement; columns 0 and 1 exactly 0 without
    scores; all four exactly 0 for a sample without a diffused residue (whose rows make NaN in align); no slot left unwritten (the
    buffer starts as NaN)."""
    so3 = odiff._so3_diffuser
    worst = np.zeros(4)
    n_cases = n_empty = 0
    for case in cc.logprob_cases():
        if (case["B"], case["N"]) != (B, N):
            continue
        inp = cc.logprob_inputs(case, so3.diffusion_coef(case["t"]))
        sums, rows = cc.logprob_reference(case, inp, odiff)
        out = torch.full((B, 4), float("nan"), dtype=torch.float64, device="cuda")
        _call(lib, "fdipt_se3_step_log_prob", B, N, dev(inp["rot_t"]), dev(inp["trans_t"]), dev(inp["rot_1"]), dev(inp["trans_1"]),
              dev(inp["rot_score"]), dev(inp["trans_score"]), dev(inp["mask"]), float(case["t"]), float(case["t_1"]), float(case["dt"]),
              *_consts(odiff), out)
        got = host(out)
        what = (case["k"], case["mask"], case["scores"], case["t_1"], case["dt"])
        assert np.isfinite(got).all(), (what, got)
        if not case["scores"]:
            assert (got[:, :2] == 0.0).all(), (what, got)
        if inp["mask"] is not None:
            empty = ~(inp["mask"] != 0).any(axis=1)
            assert (got[empty] == 0.0).all(), (what, got)
            n_empty += int(empty.sum())
        tol = cc.tolerance(rows)
        err = np.abs(got - sums)
        worst = np.maximum(worst, (err / np.where(tol > 0, tol, 1.0)).max(axis=0))
        assert (err <= tol).all(), (what, got, sums, err / np.where(tol > 0, tol, np.inf))
        n_cases += 1
    assert n_cases == 36 and n_empty == (24 if B > 1 else 0)
    print(f"step log-prob B={B} N={N}: {n_cases} cases; largest error / bound per column " + ", ".join(f"{v:.3f}" for v in worst) +
          f" (bound = {cc.TOLERANCE_FACTOR} x {cc.DEVIATION:.1e} x sum |row term|)")


# ---------------------------------------------------------------- forward noising
@pytest.mark.parametrize("B,N", cc.FORWARD_SIZES)
def test_forward_step_edges_vs_oracle(lib, odiff, B, N):
    """fdipt_se3_forward_step, 36 cases per (B, N).  rot_out within 1.2e-7 (one float32 spacing at 1: both sides round a float64 value
    that agrees to ~1e-14) of the restatement's float32 cast, fractional-mask rows under the near-pi rule of forward_reference;
    trans_out within one float32 spacing.  Rows with mask == 0: the translation is the input bit for bit; the rotation is compared with
    the restatement like every other row and NOT with the input bits, because the reference itself writes exp(log(R)) there, which
    moves a float32 bit of most matrices (counted in test_confidence_cases_host.py).  rigids_out: w >= 0, translation bit-equal to
    trans_out, quaternion within 2.4e-7 per component of oracle.frames.markley_quat of the float32 output matrix."""
    so3 = odiff._so3_diffuser
    worst = dict(rot=0.0, trans_spacings=0.0, quat=0.0)
    n_cases = n_t7 = n_cmp = 0
    for case in cc.forward_cases():
        if (case["B"], case["N"]) != (B, N):
            continue
        inp = cc.forward_inputs(case, so3.diffusion_coef(case["t_1"]))
        ref = cc.forward_reference(case, inp, odiff)
        rot_out, trans_out = torch.full((B, N, 3, 3), 7.0, device="cuda"), torch.full((B, N, 3), 7.0, device="cuda")
        t7 = torch.full((B, N, 7), 7.0, device="cuda") if case["with_t7"] else None
        _call(lib, "fdipt_se3_forward_step", B, N, dev(inp["rot_1"]), dev(inp["trans_1"]), dev(inp["mask"]), dev(inp["z_rot"]),
              dev(inp["z_trans"]), float(case["t_1"]), float(case["dt"]), float(case["noise_scale"]), *_consts(odiff), rot_out, trans_out, t7)
        rot, trans = host(rot_out), host(trans_out)
        what = (case["k"], case["mask"], case["t_1"], case["dt"], case["noise_scale"], case["with_t7"])
        assert np.isfinite(rot).all() and np.isfinite(trans).all(), what
        e_rot = np.abs(rot.astype(np.float64) - ref["rot"].astype(np.float64))[ref["keep"]].max(initial=0.0)
        assert e_rot <= 1.2e-7, (what, e_rot)
        e_tr = (np.abs(trans.astype(np.float64) - ref["trans"].astype(np.float64)) / np.spacing(np.abs(ref["trans"])).astype(np.float64)).max()
        assert e_tr <= 1.0, (what, e_tr)
        if inp["mask"] is not None:
            fixed = inp["mask"] == 0
            assert np.array_equal(trans[fixed], inp["trans_1"][fixed]), what
        if t7 is not None:
            t7h = host(t7)
            assert (t7h[..., 0] >= 0).all() and np.array_equal(t7h[..., 4:], trans), what
            q, _ = fr.markley_quat(rot.astype(np.float64))
            q = np.where(q[..., 3:4] < 0, -q, q)
            want = np.concatenate([q[..., 3:4], q[..., :3]], axis=-1)
            e_q = np.abs(t7h[..., :4] - want).max(-1)
            free = want[..., 0] == 0  # a half turn: the overall sign is open
            e_q[free] = np.minimum(e_q, np.abs(t7h[..., :4] + want).max(-1))[free]
            assert e_q.max() <= 2.4e-7, (what, e_q.max())
            worst["quat"] = max(worst["quat"], e_q.max())
            n_t7 += 1
        worst.update(rot=max(worst["rot"], e_rot), trans_spacings=max(worst["trans_spacings"], e_tr))
        n_cases += 1
        n_cmp += int(ref["keep"].sum())
    assert n_cases == 36 and 0 < n_t7 < 36
    print(f"forward step B={B} N={N}: {n_cases} cases ({n_t7} with rigids_out), {n_cmp} rotations compared; largest errors "
          f"rot {worst['rot']:.2e} (bound 1.2e-7), trans {worst['trans_spacings']:.2f} float32 spacings (bound 1), "
          f"quaternion {worst['quat']:.2e} (bound 2.4e-7)")


@pytest.mark.parametrize("B,N", [(3, 65), (2, 257)])
def test_forward_step_gen_equals_the_step_on_its_filled_tape(lib, odiff, B, N):
    """fdipt_se3_forward_step_gen at steps 0 and 7 with the keys 0, 2^63 - 1, 2^64 - 1 and a fractional mask: bit for bit
    fdipt_se3_forward_step fed with noise.fill of the forward purposes at that step, in rot_out, trans_out and rigids_out — each sample
    draws from its own key, each row by its index within the sample."""
    from framedipt_amd import noise
    keys = noise.keys_tensor(noise.as_keys([0, 2**63 - 1, 2**64 - 1][3 - B:], B), "cuda")
    case = dict(k=900 + N, B=B, N=N, t_1=0.5, dt=fc.DTS[1], noise_scale=0.5, mask="fractional", g0=0)
    inp = cc.forward_inputs(case, odiff._so3_diffuser.diffusion_coef(case["t_1"]))
    # (a sample without a diffused residue ignores its noise, and with it its key: here every sample has some)
    inp["mask"][~(inp["mask"] != 0).any(axis=1)] = np.resize(np.array([0.25, 1.0, 0.5, 0.0], dtype=F32), N)
    assert ((inp["mask"] > 0) & (inp["mask"] < 1)).any(axis=1).all()
    head = (B, N, dev(inp["rot_1"]), dev(inp["trans_1"]), dev(inp["mask"]))
    tail = (case["t_1"], case["dt"], case["noise_scale"], *_consts(odiff))
    seen = []
    for step in (0, 7):
        z_rot = noise.fill(keys, noise.FORWARD_ROT, 1, N, "cuda", k_begin=step)[0]
        z_trans = noise.fill(keys, noise.FORWARD_TRANS, 1, N, "cuda", k_begin=step)[0]
        outs = []
        for gen in (False, True):
            o = [torch.full((B, N, *s), 7.0, device="cuda") for s in ((3, 3), (3,), (7,))]
            if gen:
                _call(lib, "fdipt_se3_forward_step_gen", *head, keys, step, *tail, *o)
            else:
                _call(lib, "fdipt_se3_forward_step", *head, z_rot, z_trans, *tail, *o)
            outs.append(o)
        for name, a, b in zip(("rot_out", "trans_out", "rigids_out"), *outs):
            assert torch.equal(a, b), (step, name, (a != b).nonzero()[:4].tolist())
        seen.append(outs[1][1])
    assert not torch.equal(seen[0], seen[1])  # the step index reaches the draw


# ---------------------------------------------------------------- terminal prior term
def test_prior_log_prob_edges_vs_oracle(lib, odiff):
    """fdipt_se3_prior_log_prob on the 27 cases: column 0 within sum_rows spacing(|float32 term|) of the restatement (one float32
    rounding per element: the kernel may contract -(x x) / 2 - c into a fused multiply-add), column 1 = log(1 / pi^2) times the sum of
    the mask — fractional values as such — within 1e-14 relative; exactly 0 for a sample without a diffused residue."""
    cs = _consts(odiff)[4]
    worst0 = worst1 = 0.0
    for case in cc.prior_cases():
        B, N = case["B"], case["N"]
        inp = cc.prior_inputs(case)
        ref, terms = odiff.prior_log_prob(inp["trans"], inp["mask"])
        out = torch.full((B, 2), float("nan"), dtype=torch.float64, device="cuda")
        _call(lib, "fdipt_se3_prior_log_prob", B, N, dev(inp["trans"]), dev(inp["mask"]), cs, out)
        got = host(out)
        assert np.isfinite(got).all(), (case, got)
        if inp["mask"] is not None:
            empty = ~(inp["mask"] != 0).any(axis=1)
            assert (got[empty] == 0.0).all(), (case, got)
        tol0 = np.where(terms != 0, np.spacing(np.abs(terms)), F32(0)).astype(np.float64).sum(axis=(1, 2))
        e0, e1 = np.abs(got[:, 0] - ref[:, 0]), np.abs(got[:, 1] - ref[:, 1])
        assert (e0 <= tol0).all(), (case, got, ref, tol0)
        assert (e1 <= 1e-14 * np.abs(ref[:, 1])).all(), (case, got, ref)
        worst0 = max(worst0, (e0 / np.where(tol0 > 0, tol0, 1.0)).max())
        worst1 = max(worst1, (e1 / np.where(ref[:, 1] != 0, np.abs(ref[:, 1]), 1.0)).max())
    print(f"prior log-prob, 27 cases: translation term error / bound {worst0:.3f} (bound = one float32 spacing per element), rotation "
          f"term relative error {worst1:.2e} (bound 1e-14)")


# ---------------------------------------------------------------- Python surface
def test_log_prob_api_with_a_batched_rigid(odiff):
    """SE3Diffuser.log_prob_forward / log_prob_backward with Rigid arguments of lead dimension 3, N = 257 and a per-sample fractional
    mask: one value per sample, the sum of the matching two columns of the restatement."""
    from framedipt_amd import config
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.rigid import Rigid, Rotation
    d = SE3Diffuser(config.base_config().diffuser, device="cuda")
    case = dict(k=950, B=3, N=257, mask="fractional", scores=True, t=0.7, t_1=0.5, dt=fc.DTS[1], g0=0)
    inp = cc.logprob_inputs(case, odiff._so3_diffuser.diffusion_coef(case["t"]))
    sums, rows = cc.logprob_reference(case, inp, odiff)
    tol = cc.tolerance(rows)
    x_t = Rigid(Rotation(rot_mats=dev(inp["rot_t"])), dev(inp["trans_t"]))
    x_1 = Rigid(Rotation(rot_mats=dev(inp["rot_1"])), dev(inp["trans_1"]))
    lpf = d.log_prob_forward(rigids_t=x_t, rigids_t_1=x_1, t_1=case["t_1"], dt=case["dt"], diffuse_mask=inp["mask"])
    lpb = d.log_prob_backward(rigids_t=x_t, rigids_t_1=x_1, trans_score_t=inp["trans_score"], rot_score_t=inp["rot_score"], t=case["t"],
                              dt=case["dt"], diffuse_mask=inp["mask"])
    assert lpf.shape == (3,) and lpb.shape == (3,)
    e_f, e_b = np.abs(lpf - (sums[:, 2] + sums[:, 3])), np.abs(lpb - (sums[:, 0] + sums[:, 1]))
    print(f"log_prob_forward / log_prob_backward, B=3 N=257: error / bound {np.max(e_f / np.where(tol[:, 2:].sum(1) > 0, tol[:, 2:].sum(1), 1)):.3f}, "
          f"{np.max(e_b / np.where(tol[:, :2].sum(1) > 0, tol[:, :2].sum(1), 1)):.3f}")
    assert (e_f <= tol[:, 2] + tol[:, 3]).all() and (e_b <= tol[:, 0] + tol[:, 1]).all(), (lpf, lpb, sums)
    empty = ~(inp["mask"] != 0).any(axis=1)
    assert empty.sum() == 1 and (lpf[empty] == 0.0).all() and (lpb[empty] == 0.0).all()
