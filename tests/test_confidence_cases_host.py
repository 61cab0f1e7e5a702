"""CPU: the cases of tests/confidence_cases.py and, with the NumPy oracle alone, the conditions that make the assertions of
tests/test_gpu_confidence_edges.py fair — no row is dropped for a condition, the inputs are built to meet them all — the rounding error
of the restatement itself (confidence_cases.DEVIATION), and the argument checks of the four entries that need no launch."""
import numpy as np
import pytest

import confidence_cases as cc
import frames_cases as fc
from oracle import diffuser as od

F32 = np.float32


@pytest.fixture(scope="module")
def odiff():
    from framedipt_amd import config
    return od.SE3Diffuser(config.base_config().diffuser)


def test_case_counts_and_determinism():
    R, live, still = cc.frame_pools()
    assert R.shape == (67 * 46 + 42, 3, 3) and R.dtype == F32
    assert len(still) == 3 * 46 and len(live) > 2500 and not set(live) & set(still)
    lp = cc.logprob_cases()
    assert len(lp) == 9 * 3 * 2 * 3 * 2 == 324 and lp == cc.logprob_cases()
    assert sum(c["B"] * c["N"] for c in lp) == 36 * 3636
    assert {(c["t_1"], c["t"]) for c in lp} == {cc.step_times(i, dt) for i in range(3) for dt in fc.DTS}
    assert max(c["B"] * c["N"] for c in lp) == 1200
    a, b = cc.logprob_inputs(lp[40], 1.3), cc.logprob_inputs(lp[40], 1.3)
    assert all(np.array_equal(a[k], b[k]) for k in a if a[k] is not None)
    fw = cc.forward_cases()
    assert len(fw) == 6 * 4 * 3 * 3 == 216 and fw == cc.forward_cases()
    # the two hashed switches meet every value of every other factor
    for key in ("t_1", "mask", "noise_scale"):
        for v in {c[key] for c in fw}:
            assert {(c["dt"], c["with_t7"]) for c in fw if c[key] == v} == {(dt, w) for dt in fc.DTS for w in (False, True)}, (key, v)
    for size in cc.FORWARD_SIZES:
        assert {(c["dt"], c["with_t7"]) for c in fw if (c["B"], c["N"]) == size} == {(dt, w) for dt in fc.DTS for w in (False, True)}
    a, b = cc.forward_inputs(fw[7], 0.9), cc.forward_inputs(fw[7], 0.9)
    assert all(np.array_equal(a[k], b[k]) for k in a if a[k] is not None)
    assert len(cc.prior_cases()) == 27


def test_log_prob_inputs_meet_every_condition_and_the_deviation_is_held(odiff):
    """Over all 324 cases, on the float32 arrays the kernel gets: every summed row has |cos| >= 1e-6 between the axes of both align
    calls, a target angle (x_{t-1}, the backward mean) of at most pi - 1e-4 and no zero rotation vector; at least 30 summed rows take
    the 2 pi - angle branch in the forward and in the backward term, at least 30 have a fractional mask, at least 30 have an exact half
    turn for x_t, every perturbation scale is met; rows outside the mask do produce NaN in the restatement's align (and are left out);
    the outputs are finite, exactly 0 for a sample without a diffused residue and in columns 0 and 1 without scores.  Then the
    restatement in float64 against itself in longdouble: DEVIATION is not below the largest relative difference."""
    so3 = odiff._so3_diffuser
    flips = dict(forward=0, backward=0)
    n_rows = n_sel = n_frac = n_half = n_zero_samples = n_nan_rows = 0
    seen_scale = np.zeros(len(fc.PERT_SCALES), dtype=int)
    dev = np.zeros(4)
    min_dot, max_target, min_angle = np.inf, 0.0, np.inf
    for case in cc.logprob_cases():
        inp = cc.logprob_inputs(case, so3.diffusion_coef(case["t"]))
        info = {}
        sums, rows = cc.logprob_reference(case, inp, odiff, info=info)
        assert sums.dtype == np.float64 and sums.shape == (case["B"], 4) and rows.shape == (case["B"], case["N"], 4)
        assert np.isfinite(sums).all() and np.isfinite(rows).all(), case
        sel = info["selected"]
        assert np.array_equal(sel, np.ones_like(sel) if inp["mask"] is None else inp["mask"] != 0)
        ang_t, ang_1 = np.linalg.norm(info["rv_t"], axis=-1), np.linalg.norm(info["rv_1"], axis=-1)
        assert (ang_t[sel] > 0).all() and (ang_1[sel] >= 0.99 * cc.MIN_ANGLE).all() and (ang_1[sel] <= cc.MAX_ANGLE).all(), case
        min_angle, max_target = min(min_angle, ang_1[sel].min(initial=np.inf)), max(max_target, ang_1[sel].max(initial=0.0))
        dots = [info["dot_forward"][sel]]
        flips["forward"] += int((info["dot_forward"][sel] < 0).sum())
        if case["scores"]:
            ang_mu = np.linalg.norm(info["mu"], axis=-1)
            assert (ang_mu[sel] <= cc.MAX_ANGLE).all() and (ang_mu[sel] > 0).all(), case
            max_target = max(max_target, ang_mu[sel].max(initial=0.0))
            dots.append(info["dot_backward"][sel])
            flips["backward"] += int((info["dot_backward"][sel] < 0).sum())
        else:
            assert inp["rot_score"] is None and inp["trans_score"] is None and (sums[:, :2] == 0).all() and (rows[..., :2] == 0).all()
        for d in dots:
            assert (np.abs(d) >= cc.MIN_DOT).all(), case
            min_dot = min(min_dot, np.abs(d).min(initial=np.inf))
        n_rows += sel.size
        n_sel += int(sel.sum())
        n_half += int((inp["half_turn"] & sel).sum())
        seen_scale += np.bincount(inp["scale_index"][sel], minlength=len(fc.PERT_SCALES))
        if inp["mask"] is not None:
            n_frac += int(((inp["mask"] > 0) & (inp["mask"] < 1)).sum())
            n_nan_rows += int((~sel & np.isnan(info["dot_forward"])).sum())
            empty = ~sel.any(axis=1)
            assert empty.sum() == (1 if case["B"] > 1 else 0), case
            assert (sums[empty] == 0).all() and (np.abs(sums[~empty, 2:]) > 0).all(), case
            n_zero_samples += int(empty.sum())
        sums_ld, _ = cc.logprob_reference(case, inp, odiff, dtype=np.longdouble)
        assert sums_ld.dtype == np.longdouble
        scale = np.abs(rows).sum(axis=1)
        with np.errstate(invalid="ignore"):
            rel = np.where(scale > 0, np.abs(sums - sums_ld).astype(np.float64) / np.where(scale > 0, scale, 1.0), 0.0)
        dev = np.maximum(dev, rel.max(axis=0))
    print(f"log-prob cases: {n_rows} rows, {n_sel} summed, {n_frac} with a fractional mask, {n_half} exact half turns, {n_zero_samples} "
          f"samples without a diffused residue, {n_nan_rows} rows outside the mask with NaN in align; 2 pi - angle branch: {flips}; rows per "
          f"perturbation scale {seen_scale.tolist()}; smallest |cos| {min_dot:.2e}, x_t-1 angle from {min_angle:.6e}, largest target angle "
          f"pi - {np.pi - max_target:.3e}")
    print("measured DEVIATION (float64 against longdouble, relative to the sum of |row term|) per column: " +
          ", ".join(f"{v:.3e}" for v in dev) + f"; constant {cc.DEVIATION:.3e}, bound factor {cc.TOLERANCE_FACTOR}")
    assert flips["forward"] >= 30 and flips["backward"] >= 30
    assert n_frac >= 30 and n_half >= 30 and n_zero_samples >= 50 and n_nan_rows >= 30
    assert (seen_scale >= 1000).all()
    assert np.finfo(np.longdouble).eps < 1e-18  # the wider type is wider
    assert dev.max() <= cc.DEVIATION <= 2 * dev.max(), dev  # not below what is measured (and no idle slack above it)


def test_forward_cases_hold_for_the_restatement(odiff):
    """The restatement on all 216 forward cases: finite; at least 80 % of the fractional-mask rows pass the near-pi rule, binary and
    NULL masks exclude nothing; every frame of the grid and 95 % of its (frame, perturbation scale) pairs are met; rows with mask == 0 keep their
    translation bit for bit.  Their rotation is the float32 cast of exp(log(R)), which is what the reference computes for them too
    (se3_diffuser.py:16-36 on every row, whatever the mask): it is the input matrix up to float32 rounding but NOT bit for bit, since the
    float32 input is not exactly orthogonal — counted here; the GPU test therefore compares those rows with the restatement."""
    so3 = odiff._so3_diffuser
    R = cc.frame_pools()[0]
    seen = np.zeros((len(R), len(fc.PERT_SCALES)), dtype=bool)
    n_frac = n_frac_kept = n_fixed = n_fixed_moved = n_half = 0
    worst_fixed = 0.0
    for case in cc.forward_cases():
        inp = cc.forward_inputs(case, so3.diffusion_coef(case["t_1"]))
        ref = cc.forward_reference(case, inp, odiff)
        assert np.isfinite(ref["rot64"]).all() and np.isfinite(ref["trans"]).all(), case
        assert np.array_equal(ref["rot64"].astype(F32), ref["rot"]) and ref["trans"].dtype == F32
        assert ref["keep"][~ref["frac"]].all()
        n_frac += int(ref["frac"].sum())
        n_frac_kept += int((ref["frac"] & ref["keep"]).sum())
        n_half += int(inp["half_turn"].sum())
        plain = ~inp["half_turn"]
        seen[inp["frame_index"][plain], inp["scale_index"][plain]] = True
        if inp["mask"] is not None:
            fixed = inp["mask"] == 0
            assert np.array_equal(ref["trans"][fixed], inp["trans_1"][fixed])
            diff = np.abs(ref["rot"][fixed] - inp["rot_1"][fixed]).reshape(-1, 9).max(-1, initial=0.0)
            n_fixed += int(fixed.sum())
            n_fixed_moved += int((diff > 0).sum())
            worst_fixed = max(worst_fixed, diff.max(initial=0.0))
    print(f"forward cases: fractional rows kept {n_frac_kept}/{n_frac}; exact half turns {n_half}; (frame, scale) pairs met {seen.mean():.3f}; "
          f"rows with mask == 0: {n_fixed}, of which the reference's exp(log(R)) changes a float32 bit in {n_fixed_moved} (by {worst_fixed:.2e} at most)")
    assert n_frac > 3000 and n_frac_kept >= 0.8 * n_frac
    assert seen.mean() >= 0.95 and seen.any(1).all() and n_half >= 100  # (a pair is missed only where a half turn takes its row)
    assert n_fixed > 2000 and n_fixed_moved >= 30 and worst_fixed <= 2.4e-7


def test_prior_cases_hold_for_the_restatement(odiff):
    """prior_log_prob on the 27 cases: finite, float32 element terms, column 1 = log(1 / pi^2) times the sum of the mask (fractional values
    count as such), exactly 0 for a sample without a diffused residue; |x_T| reaches 300 A."""
    top = 0.0
    for case in cc.prior_cases():
        inp = cc.prior_inputs(case)
        out, terms = odiff.prior_log_prob(inp["trans"], inp["mask"])
        assert out.shape == (case["B"], 2) and out.dtype == np.float64 and terms.dtype == F32 and np.isfinite(out).all()
        msum = np.full(case["B"], float(case["N"])) if inp["mask"] is None else inp["mask"].astype(np.float64).sum(-1)
        np.testing.assert_allclose(out[:, 1], -2 * np.log(np.pi) * msum, rtol=1e-15)
        np.testing.assert_array_equal(out[:, 0], terms.astype(np.float64).sum((1, 2)))
        if inp["mask"] is not None:
            empty = ~(inp["mask"] != 0).any(1)
            assert empty.sum() == (1 if case["B"] > 1 else 0) and (out[empty] == 0).all()
            if case["mask"] == "fractional" and case["N"] > 60:
                assert (msum[~empty] != (inp["mask"] != 0).sum(-1)[~empty]).all()  # the sum of the mask is not the row count
        top = max(top, np.abs(inp["trans"]).max())
    assert top == 300.0


# ---------------------------------------------------------------- argument checks that need no launch
SDE = (0.1, 1.5, 0.1, 20.0, 0.1)  # so3 min / max sigma, r3 min / max b, coordinate scaling


@pytest.fixture(scope="module")
def lib():
    from framedipt_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def buf():
    """A host buffer whose address stands in for every pointer: the calls below must return before anything reads it."""
    keep = np.zeros(64)
    return keep, keep.ctypes.data


def _forward(lib, p, B=2, N=3, t_1=0.5, rot_out="p", trans_out="p", z="p"):
    s = lambda v: p if v == "p" else v  # noqa: E731
    return lib.fdipt_se3_forward_step(B, N, p, p, None, s(z), s(z), t_1, 0.2, 1.0, *SDE, s(rot_out), s(trans_out), None, None)


def _forward_gen(lib, p, B=2, N=3, t_1=0.5, step=0, rot_out="p", trans_out="p", keys="p"):
    s = lambda v: p if v == "p" else v  # noqa: E731
    return lib.fdipt_se3_forward_step_gen(B, N, p, p, None, s(keys), step, t_1, 0.2, 1.0, *SDE, s(rot_out), s(trans_out), None, None)


def _log_prob(lib, p, B=2, N=3, rot_score="p", trans_score="p", out="p"):
    s = lambda v: p if v == "p" else v  # noqa: E731
    return lib.fdipt_se3_step_log_prob(B, N, p, p, p, p, s(rot_score), s(trans_score), None, 0.7, 0.5, 0.2, *SDE, s(out), None)


def test_entries_refuse_bad_arguments_without_a_launch(lib, buf):
    """B = 0 or N = 0: FDIPT_OK and nothing done, whatever else is passed; t_1 outside [0, 1] or NaN, one score without the other,
    a negative step, NULL outputs: FDIPT_EINVAL."""
    from framedipt_amd import _lib
    _, p = buf
    OK, EINVAL = 0, _lib.EINVAL
    for B, N in ((0, 5), (5, 0), (0, 0)):
        assert _forward(lib, p, B=B, N=N, t_1=7.0, rot_out=None) == OK
        assert _forward_gen(lib, p, B=B, N=N, step=-1, keys=None) == OK
        assert _log_prob(lib, p, B=B, N=N, out=None) == OK
        assert lib.fdipt_se3_prior_log_prob(B, N, None, None, 0.1, None, None) == OK
    for t_1 in (-0.1, 1.1, float("nan")):
        assert _forward(lib, p, t_1=t_1) == EINVAL, t_1
        assert _forward_gen(lib, p, t_1=t_1) == EINVAL, t_1
    assert _log_prob(lib, p, trans_score=None) == EINVAL
    assert _log_prob(lib, p, rot_score=None) == EINVAL
    assert _forward_gen(lib, p, step=-1) == EINVAL
    assert _forward_gen(lib, p, keys=None) == EINVAL
    assert _forward(lib, p, z=None) == EINVAL
    for name in ("rot_out", "trans_out"):
        assert _forward(lib, p, **{name: None}) == EINVAL, name
        assert _forward_gen(lib, p, **{name: None}) == EINVAL, name
    assert _log_prob(lib, p, out=None) == EINVAL
    assert lib.fdipt_se3_prior_log_prob(2, 3, p, None, 0.1, None, None) == EINVAL
    assert lib.fdipt_se3_prior_log_prob(2, 3, None, None, 0.1, p, None) == EINVAL
