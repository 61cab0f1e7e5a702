"""Deterministic edge cases for the confidence-walk kernels at the end of framedipt_amd/csrc/frames.hip (forward noising, the step
log-probabilities, the terminal prior term) — test infrastructure.

NumPy only, nothing happens at import beyond definitions; the frames, axes, perturbation scales, mask kinds and time grids are those of
tests/frames_cases.py.  tests/test_confidence_cases_host.py pins the counts, shows with the oracle alone that the inputs meet every
condition the GPU assertions rest on, and measures DEVIATION; tests/test_gpu_confidence_edges.py then asks the kernels.  Every array is
a pure function of the constants below (seeded ``np.random.default_rng``).  The schedule is the caller's: the generators take the SO(3)
diffusion coefficient they need and know no configuration.
"""
import functools
import itertools

import numpy as np

import frames_cases as fc

F32 = np.float32
PI = np.pi

# one row; a partial wave; one row per thread of the 256-thread block (and one short, one over); a second and a third pass of the
# strided row loop; several samples per launch
LOGPROB_SIZES = ((1, 1), (1, 63), (3, 64), (2, 65), (1, 255), (3, 256), (2, 257), (1, 513), (2, 600))
# B * N around the edges of the forward step's 64-thread blocks
FORWARD_SIZES = ((1, 1), (1, 63), (1, 64), (1, 65), (3, 43), (2, 257))
FORWARD_T1 = (0.0, 0.01, 0.5, 1.0)
NOISE_SCALES = (1.0, 0.5, 0.0)
MIN_ANGLE, MAX_ANGLE = 9.99e-4, PI - 1e-4  # of x_{t-1} and of the backward mean on the rows that are summed
MIN_DOT = 1e-6                             # |cos| between the two axes of an align call: its sign is then no rounding matter
DRIFT_SCALES = (0.0, 1e-9, 1e-3, 0.3, 1.0)  # |g^2 score dt| in rad
SHIFT_SCALES = (0.0, 1e-3, 1.0, 30.0)       # |x_t - x_{t-1}| per component, in A
TRANS_RANGE = 100.0
PRIOR_RANGE = 300.0

# Rounding error of the float64 restatement itself: the largest |terms(float64) - terms(longdouble)| / sum_rows |row term| over every
# log-probability case, sample and column (measured and held by tests/test_confidence_cases_host.py, which prints it; per column:
# backward trans 1.8e-15, backward rot 3.2e-15, forward trans 1.9e-15 — NumPy's row-after-row sum over up to 600 residues — and forward
# rot 1.41e-14, at the one-residue cases with t_1 = 0.01, dt = 1/5, where -log(std) and -log(sqrt(2 pi)) nearly cancel and the row
# term is 0.047).  The GPU test allows TOLERANCE_FACTOR times it: the factor covers a second math library (the device's exp / log /
# sin / cos / atan2 / sqrt) and a second summation order (per-thread rows, wave tree, four-wave sum) on the same algorithm.  Nothing
# here is taken from the kernel.
DEVIATION = 1.5e-14
TOLERANCE_FACTOR = 16


def tolerance(rows):
    """Bound on |kernel - restatement| per sample and column; ``rows`` [B,N,4] = the restatement's per-residue terms."""
    return TOLERANCE_FACTOR * DEVIATION * np.abs(np.asarray(rows, dtype=np.float64)).sum(axis=1)


def step_times(ti, dt):
    """(t_1, t) of a step at the start, in the middle and at the end of the walk."""
    return ((0.01, 0.01 + dt), (0.5, 0.5 + dt), (1.0 - dt, 1.0))[ti]


@functools.lru_cache(maxsize=None)
def frame_pools():
    """(R [F,3,3] float32 matrices of frames_cases.frame_quats(), live, still).  ``live``: frames whose grid angle lies in
    [MIN_ANGLE, MAX_ANGLE] (the exact ties by their own angle) and whose float32 matrix still has a logarithm of at most MAX_ANGLE;
    ``still``: the identity, 1e-12 and 1e-7 frames, for rows outside the mask."""
    from oracle import frames as fr
    R = fr.quat_to_rot(fc.frame_quats())
    ang = np.linalg.norm(fr.scipy_from_matrix_as_rotvec(R), axis=-1)
    n_grid = len(fc.angles()) * len(fc.axes())
    nominal = np.concatenate([np.repeat(fc.angles(), len(fc.axes())), ang[n_grid:]])
    live = np.nonzero((nominal >= MIN_ANGLE) & (nominal <= MAX_ANGLE) & (ang <= MAX_ANGLE))[0]
    still = np.nonzero(nominal[:n_grid] <= 1e-7)[0]
    return R, live, still


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _mask(rng, kind, B, N, k):
    """None / {0, 1} / {0, 1/4, 1/2, 1}; every sample keeps a diffused residue, except — with B > 1 — sample k mod B, which has none."""
    if kind == "null":
        return None
    if kind == "binary":
        m = (rng.random((B, N)) < 0.75).astype(F32)
    else:
        m = rng.choice(np.array([0.0, 1.0, *fc.FRACTIONS], dtype=F32), size=(B, N), p=[0.1, 0.3, 0.3, 0.3])
    for b in range(B):
        if not m[b].any():
            m[b, 0] = 1.0 if kind == "binary" else 0.5
    if B > 1:
        m[k % B] = 0.0
    return m


def _trans(rng, n, rng_r):
    x = rng.uniform(-rng_r, rng_r, (n, 3))
    x[::7] = 0.0
    x[3::11] = np.sign(x[3::11]) * rng_r
    return x


# ---------------------------------------------------------------- step log-probabilities
def logprob_cases():
    """Every (B, N) x mask kind x scores present / absent x place in the walk x dt.  ``g0``: the case's first index into the sweep of
    (frame, perturbation scale) pairs, which runs on from case to case."""
    cases, g0 = [], 0
    for k, ((B, N), mask, scores, ti, dt) in enumerate(itertools.product(LOGPROB_SIZES, fc.MASK_KINDS, (True, False), range(3), fc.DTS)):
        t_1, t = step_times(ti, dt)
        cases.append(dict(k=k, B=B, N=N, mask=mask, scores=scores, t=t, t_1=t_1, dt=dt, g0=g0))
        g0 += B * N
    return cases


def _angle_and_dot(rv_in, rv_target):
    """(|rv_in|, cos between the two axes); NaN where either vector is 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = np.linalg.norm(rv_in, axis=-1), np.linalg.norm(rv_target, axis=-1)
        return a, (rv_in * rv_target).sum(-1) / (a * b)


def logprob_inputs(case, g_rot):
    """Arrays of one case; ``g_rot`` = the SO(3) diffusion coefficient at the case's t.

    Rows inside the mask: x_{t-1} from the live frames; x_t = x_{t-1} exp(p), stored as the float32 cast of the float64 product (the
    state the walk carries), |p| cycling through PERT_SCALES, p along +-the axis of x_{t-1} on every other row (so that 3.0 and 6.0
    carry the angle across pi and the rotation vector of x_t points against that of x_{t-1}) and in a random direction on the rest;
    every 23rd such row has an exact half turn for x_t.  The rotation score realises a drift g^2 s dt m of length DRIFT_SCALES[...].
    A direction is drawn again (up to 20 times, the drift then 0.3 rad long) where the float32 inputs would miss a condition the
    assertions need: both align calls see axes with |cos| >= MIN_DOT and non-zero vectors, the backward mean has an angle of at
    most MAX_ANGLE.  Rows outside the mask: x_t = x_{t-1} = an identity, 1e-12 or 1e-7 frame.
    Translations: x_{t-1} within +-100 A with zeros and range ends, x_t = x_{t-1} + a shift of 0, 1e-3, 1 or 30 A per component."""
    from oracle import frames as fr
    B, N, dt = case["B"], case["N"], case["dt"]
    n = B * N
    rng = np.random.default_rng(60_000 + case["k"])
    R, live, still = frame_pools()
    mask = _mask(rng, case["mask"], B, N, case["k"])
    sel = np.ones(n, dtype=bool) if mask is None else mask.reshape(-1) != 0
    m = np.ones(n) if mask is None else mask.reshape(-1).astype(np.float64)
    g = case["g0"] + np.arange(n)
    fi = np.where(sel, live[g % len(live)], still[g % len(still)])
    si = (g + g // len(live)) % len(fc.PERT_SCALES)
    rot_1 = R[fi]
    rv1 = fr.scipy_from_matrix_as_rotvec(rot_1)
    with np.errstate(divide="ignore", invalid="ignore"):
        axis1 = np.where(sel[:, None], rv1 / np.linalg.norm(rv1, axis=-1, keepdims=True), 0.0)
    mag = np.where(sel, np.array(fc.PERT_SCALES)[si], 0.0)
    dirn = np.where((g % 2 == 0)[:, None], axis1 * np.where((g // 2) % 2 == 0, 1.0, -1.0)[:, None], _unit(rng, n))
    half = sel & (g % 23 == 5)
    half_mats, half_axes = fc.exact_half_turns()
    half_pick = np.abs(axis1 @ half_axes.T).argmax(-1)  # the half turn whose axis is least perpendicular to that of x_{t-1}
    todo = np.ones(n, dtype=bool)
    rot_t = np.empty_like(rot_1)
    for _ in range(20):
        prod = rot_1[todo].astype(np.float64) @ fr.scipy_from_rotvec_as_matrix(mag[todo, None] * dirn[todo])
        rot_t[todo] = np.where(half[todo, None, None], half_mats[half_pick[todo]], prod).astype(F32)
        ang_t, dot_f = _angle_and_dot(fr.scipy_from_matrix_as_rotvec(rot_t), rv1)
        todo = sel & ~((ang_t > 0) & (np.abs(dot_f) >= MIN_DOT))
        if not todo.any():
            break
        dirn[todo] = _unit(rng, int(todo.sum()))
    assert not todo.any(), case
    rvt = fr.scipy_from_matrix_as_rotvec(rot_t)
    rot_score = None
    if case["scores"]:
        dmag = np.array(DRIFT_SCALES)[(g // len(fc.PERT_SCALES)) % len(DRIFT_SCALES)]
        ddir = _unit(rng, n)
        rot_score = np.empty((n, 3))
        todo = np.ones(n, dtype=bool)
        for _ in range(20):
            rot_score[todo] = (dmag[todo, None] * ddir[todo]) / (g_rot**2 * dt * np.where(sel, m, 1.0)[todo, None])
            mu = fr.compose_rotvec(rvt, g_rot**2 * rot_score * dt * m[:, None])
            _, dot_b = _angle_and_dot(rv1, mu)
            todo = sel & ~((np.linalg.norm(mu, axis=-1) <= MAX_ANGLE) & (np.abs(dot_b) >= MIN_DOT))
            if not todo.any():
                break
            dmag[todo], ddir[todo] = 0.3, _unit(rng, int(todo.sum()))
        assert not todo.any(), case
        rot_score = rot_score.reshape(B, N, 3)
    trans_1 = _trans(rng, n, TRANS_RANGE)
    shift = np.array(SHIFT_SCALES)[(g // 3) % len(SHIFT_SCALES)][:, None] * rng.uniform(-1.0, 1.0, (n, 3))
    trans_t = np.clip(trans_1 + shift, -TRANS_RANGE, TRANS_RANGE)
    trans_score = (0.1 * rng.standard_normal((B, N, 3))).astype(F32) if case["scores"] else None
    return dict(rot_t=rot_t.reshape(B, N, 3, 3), trans_t=trans_t.astype(F32).reshape(B, N, 3), rot_1=rot_1.reshape(B, N, 3, 3),
                trans_1=trans_1.astype(F32).reshape(B, N, 3), rot_score=rot_score, trans_score=trans_score, mask=mask,
                scale_index=si.reshape(B, N), half_turn=half.reshape(B, N))


def logprob_reference(case, inp, odiff, dtype=np.float64, info=None):
    """oracle.diffuser.SE3Diffuser.step_log_prob_terms on one case -> (sums [B,4], rows [B,N,4])."""
    return odiff.step_log_prob_terms(inp["rot_t"], inp["trans_t"], inp["rot_1"], inp["trans_1"], inp["rot_score"], inp["trans_score"],
                                     inp["mask"], case["t"], case["t_1"], case["dt"], dtype=dtype, info=info)


# ---------------------------------------------------------------- forward noising
def forward_cases():
    """Every (B, N) x t_1 x mask kind x noise_scale; dt and the optional tensor_7 output spread over them by a multiplicative hash of
    the case index.  ``g0`` as in logprob_cases()."""
    cases, g0 = [], 0
    for k, ((B, N), t_1, mask, ns) in enumerate(itertools.product(FORWARD_SIZES, FORWARD_T1, fc.MASK_KINDS, NOISE_SCALES)):
        h = (k * 2654435761 % 2**32) >> 7
        cases.append(dict(k=k, B=B, N=N, t_1=t_1, mask=mask, noise_scale=ns, dt=fc.DTS[h & 1], with_t7=bool((h >> 1) & 1), g0=g0))
        g0 += B * N
    return cases


def forward_inputs(case, g_rot):
    """Arrays of one case; ``g_rot`` = the SO(3) diffusion coefficient at the case's t_1.  x_{t-1} walks the whole grid, exact ties
    included, every 29th row an exact half turn; z_rot is scaled so that the rotation perturbation g sqrt(dt) noise_scale z has length
    PERT_SCALES[...] (noise_scale 0: z_rot is a plain N(0,1) draw, the perturbation is 0)."""
    B, N, dt, ns = case["B"], case["N"], case["dt"], case["noise_scale"]
    n = B * N
    rng = np.random.default_rng(70_000 + case["k"])
    R = frame_pools()[0]
    g = case["g0"] + np.arange(n)
    fi = g % len(R)
    si = (g + g // len(R)) % len(fc.PERT_SCALES)
    half = g % 29 == 3
    rot_1 = np.where(half[:, None, None], fc.exact_half_turns()[0][(g // 29) % 6].astype(F32), R[fi])
    z_rot = rng.standard_normal((n, 3))
    if ns != 0.0:
        z_rot = np.array(fc.PERT_SCALES)[si][:, None] * _unit(rng, n) / (g_rot * np.sqrt(dt) * ns)
    return dict(rot_1=rot_1.reshape(B, N, 3, 3), trans_1=_trans(rng, n, TRANS_RANGE).astype(F32).reshape(B, N, 3),
                z_rot=z_rot.reshape(B, N, 3), z_trans=rng.standard_normal((B, N, 3)), mask=_mask(rng, case["mask"], B, N, case["k"]),
                frame_index=fi.reshape(B, N), scale_index=si.reshape(B, N), half_turn=half.reshape(B, N))


def forward_reference(case, inp, odiff):
    """oracle.diffuser.SE3Diffuser.forward on one case -> dict(rot f32, trans f32, rot64, frac = residues with a mask strictly between
    0 and 1, keep = residues whose rotation is compared).

    A fractional mask interpolates rotation VECTORS, whose sign flips at pi in the reference itself: such a residue is compared only
    if the angle of x_{t-1} and the composed angle are below frames_cases.NEAR_PI (the rule of frames_cases.reverse_reference)."""
    from oracle import frames as fr
    B, N = case["B"], case["N"]
    rot, trans, rot64 = odiff.forward(inp["rot_1"], inp["trans_1"], case["t_1"], case["dt"], inp["mask"], inp["z_rot"], inp["z_trans"],
                                      noise_scale=case["noise_scale"])
    m = np.ones((B, N)) if inp["mask"] is None else inp["mask"].astype(np.float64)
    rv1 = fr.scipy_from_matrix_as_rotvec(inp["rot_1"])
    pert = odiff._so3_diffuser.diffusion_coef(case["t_1"]) * np.sqrt(case["dt"]) * case["noise_scale"] * inp["z_rot"] * m[..., None]
    rvc = fr.compose_rotvec(rv1.reshape(-1, 3), pert.reshape(-1, 3)).reshape(rv1.shape)
    frac = (m > 0) & (m < 1)
    bad = (np.linalg.norm(rv1, axis=-1) >= fc.NEAR_PI) | (np.linalg.norm(rvc, axis=-1) >= fc.NEAR_PI)
    return dict(rot=rot, trans=trans, rot64=rot64, frac=frac, keep=~(frac & bad), pert=pert)


# ---------------------------------------------------------------- terminal prior term
def prior_cases():
    return [dict(k=k, B=B, N=N, mask=mask) for k, ((B, N), mask) in enumerate(itertools.product(LOGPROB_SIZES, fc.MASK_KINDS))]


def prior_inputs(case):
    """x_T translations within +-300 A (zeros and range ends among them) and the mask."""
    B, N = case["B"], case["N"]
    rng = np.random.default_rng(80_000 + case["k"])
    return dict(trans=_trans(rng, B * N, PRIOR_RANGE).astype(F32).reshape(B, N, 3), mask=_mask(rng, case["mask"], B, N, case["k"]))
