"""Deterministic edge cases for the frame / reverse-step kernels of framedipt_amd/csrc/frames.hip — test infrastructure.

NumPy only, nothing happens at import beyond definitions.  tests/test_frames_cases_host.py pins the counts and shows, with the oracle
alone, that the assertions of tests/test_gpu_frames_edges.py hold for the reference on these inputs; the GPU file then asks the
kernels the same.  Every array is a pure function of the constants below (seeded ``np.random.default_rng``).
"""
import itertools

import numpy as np

F32 = np.float32
PI = np.pi

# ---------------------------------------------------------------- angle / axis / sign grid
# both sides of the series switches at 1e-3 (d_so3_exp, d_so3_log, d_quat_to_rotvec), angles whose sixth-order series term is visible
# at 1e-13 (0.03, 0.0999), the Markley branch change (trace < largest diagonal entry: beyond ~2 rad), and pi approached from below
FIXED_ANGLES = (0.0, 1e-12, 1e-7, 9.99e-4, 1e-3, 1.001e-3, 0.03, 0.0999, 1.0, PI / 2, 2.2, 2.8,
                PI - 1e-2, PI - 1e-4, PI - 1e-7, PI - 1e-10, PI)
N_RANDOM_ANGLES = 50
N_RANDOM_AXES = 20
NEAR_PI = PI - 1e-2  # rotation vectors (not matrices) are compared below this angle only


def angles():
    rng = np.random.default_rng(101)
    return np.concatenate([np.array(FIXED_ANGLES), rng.uniform(0.0, PI, N_RANDOM_ANGLES)])


def axes():
    """+-e_x, +-e_y, +-e_z, the 12 face diagonals, the 8 body diagonals, 20 random unit vectors."""
    ax = [np.array(v, dtype=np.float64) for v in itertools.product((-1, 0, 1), repeat=3) if any(v)]
    ax.sort(key=lambda v: (int(np.abs(v).sum()), tuple(-v)))
    rng = np.random.default_rng(102)
    ax += list(rng.standard_normal((N_RANDOM_AXES, 3)))
    ax = np.stack(ax)
    return ax / np.linalg.norm(ax, axis=-1, keepdims=True)


def rotvec_grid(extra_angles=()):
    """[n_angles * n_axes, 3] float64 rotation vectors, angle-major."""
    a = np.concatenate([angles(), np.array(extra_angles, dtype=np.float64)])
    return (a[:, None, None] * axes()[None]).reshape(-1, 3)


BEYOND_PI = (3.5, 6.0, 2 * PI, 7.0)  # the exponential takes any angle (reverse-step perturbations above pi)


def tie_quats():
    """float32 quaternions (scalar first) whose float32 matrix has two or more of m00, m11, m22, trace EXACTLY equal.

    a = 0, |b| = |c|, d = 0 or +-1/4 (a half turn): m00 = (0 + v) - v - d^2 and m11 = (0 - v) + v - d^2 with v = fl(b*b): both -d^2
    exactly and above m22 = d^2 - 2v; with d = 0 the same for the other two pairs.  (s, +-s, 0, 0) with s = fl(sqrt(1/2)) (a quarter turn about an axis): m00 = 2v = trace.  (+-1/2)^4 (a third
    of a turn about a body diagonal): all four are 0.
    """
    s, h, w = F32(np.sqrt(0.5)), F32(0.5), F32(np.sqrt(15.0 / 32.0))
    out = []
    for i, j in ((1, 2), (1, 3), (2, 3)):
        k = 6 - i - j
        for si, sj in itertools.product((1, -1), repeat=2):
            # (a third component keeps the tie exact only where it enters both entries last: the (b, c) pair)
            for third, mag in ((0.0, s), (F32(0.25), w), (F32(-0.25), w)) if (i, j) == (1, 2) else ((0.0, s),):
                q = np.zeros(4, dtype=F32)
                q[i], q[j], q[k] = si * mag, sj * mag, third
                out.append(q)
    for i in (1, 2, 3):
        for sg in (1, -1):
            q = np.zeros(4, dtype=F32)
            q[0], q[i] = s, sg * s
            out.append(q)
    out += [np.array(v, dtype=F32) * h for v in itertools.product((1, -1), repeat=4)]
    return np.stack(out)


def frame_quats():
    """[F,4] float32 quaternions (scalar first): the angle x axis grid with a random overall sign, then the exact ties."""
    rv = rotvec_grid()
    th = np.linalg.norm(rv, axis=-1)
    ax = np.tile(axes(), (len(angles()), 1))
    q = np.concatenate([np.cos(th / 2)[:, None], np.sin(th / 2)[:, None] * ax], axis=-1)
    sign = np.where(np.random.default_rng(103).random(len(q)) < 0.5, -1.0, 1.0)
    return np.concatenate([(q * sign[:, None]).astype(F32), tie_quats()])


def exact_half_turns():
    """Half turns about (e_i +- e_j) / sqrt 2 as exact signed permutation matrices [6,3,3] float64 and their axes: the two largest
    diagonal entries tie at 0 and every Markley expression is exact, so the logarithm is pi * axis with the sign the FIRST maximum gives."""
    mats, ax = [], []
    for i, j in ((0, 1), (0, 2), (1, 2)):
        for sg in (1.0, -1.0):
            a = np.zeros(3)
            a[i], a[j] = 1.0, sg
            a /= np.sqrt(2.0)
            k = 3 - i - j
            m = np.zeros((3, 3))
            m[i, j] = m[j, i] = sg
            m[k, k] = -1.0
            mats.append(m)
            ax.append(a)
    return np.stack(mats), np.stack(ax)


# ---------------------------------------------------------------- reverse step
SIZES_N = (1, 15, 16, 17, 63, 64, 65, 257, 301)
SIZES_B = (1, 3)
TS = (0.01, 0.5, 1.0)
DTS = (1.0 / 500, 1.0 / 5)
PERT_SCALES = (0.0, 1e-9, 1e-3, 0.3, 3.0, 6.0)  # |perturbation| in rad: none, below float32, small, moderate, near and above pi
MASK_KINDS = ("null", "binary", "fractional")
FRACTIONS = (0.25, 0.5)
# |x_t| <= 100 A at dt = 1/500.  At dt = 1/5 and t = 1 the drift alone triples x (x + 0.5 b(t) dt x with b(1) = 20), so those cases
# start from |x_t| <= 25 A: x_{t-1} then stays below 256 A, where float32 spacing (1.5e-5) still resolves the 3e-5 A bound.
TRANS_RANGE = {DTS[0]: 100.0, DTS[1]: 25.0}


def reverse_cases():
    """Every (B, N) x mask kind x center x diffuse_rot x diffuse_trans x t; dt, in-place / out-of-place, noise_scale and the optional
    aatype spread over them by a multiplicative hash of the case index.  ``g0``: the case's first index into the (frame, scale) sweep of
    its group (binary / NULL masks and fractional masks, with and without rotation diffusion, each walk the whole sweep on their own)."""
    cases, counters = [], {}
    for k, (B, N, mask, center, drot, dtrans, t) in enumerate(itertools.product(
            SIZES_B, SIZES_N, MASK_KINDS, (1, 0), (1, 0), (1, 0), TS)):
        h = (k * 2654435761 % 2**32) >> 7
        key = (mask == "fractional", drot)
        g0 = counters.get(key, 0)
        counters[key] = g0 + B * N
        cases.append(dict(k=k, B=B, N=N, mask=mask, center=center, diffuse_rot=drot, diffuse_trans=dtrans, t=t, dt=DTS[h & 1],
                          inplace=bool((h >> 1) & 1), noise_scale=(1.0, 0.5)[(h >> 2) & 1], with_aatype=bool((h >> 3) & 1), g0=g0))
    return cases


def reverse_inputs(case, g_rot, frames=None):
    """Arrays of one case.  ``g_rot`` = the SO(3) diffusion coefficient at the case's t (the schedule is the caller's: this module knows
    no configuration); the rotation perturbation g^2 score dt + g sqrt(dt) noise_scale z of residue i then has length PERT_SCALES[...],
    realised through the score alone, the noise alone or half each (i mod 3)."""
    frames = frame_quats() if frames is None else frames
    B, N, dt, ns = case["B"], case["N"], case["dt"], case["noise_scale"]
    n = B * N
    rng = np.random.default_rng(10_000 + case["k"])
    g = case["g0"] + np.arange(n)
    fi, si = g % len(frames), (g // len(frames)) % len(PERT_SCALES)
    quat = frames[fi]
    rng_r = TRANS_RANGE[dt]
    trans = rng.uniform(-rng_r, rng_r, (n, 3))
    trans[::7] = 0.0
    trans[3::11] = np.sign(trans[3::11]) * rng_r
    dirn = rng.standard_normal((n, 3))
    dirn /= np.linalg.norm(dirn, axis=-1, keepdims=True)
    pert = np.array(PERT_SCALES)[si][:, None] * dirn
    w_score = np.array([1.0, 0.0, 0.5])[g % 3][:, None]
    rot_score = pert * w_score / (g_rot**2 * dt)
    z_rot = pert * (1 - w_score) / (g_rot * np.sqrt(dt) * ns)
    if case["mask"] == "null":
        mask = None
    elif case["mask"] == "binary":
        mask = (rng.random((B, N)) < 0.75).astype(F32)
    else:
        mask = rng.choice(np.array([0.0, 1.0, *FRACTIONS], dtype=F32), size=(B, N), p=[0.1, 0.3, 0.3, 0.3])
    if mask is not None:
        # the reference divides the sum over ALL residues by the sum of the mask: at least half of it, so that the centring
        # amplifies an input rounding by no more than 2 (and a sample always has a diffused residue)
        for b in range(B):
            i = 0
            while mask[b].sum() < N / 2:
                mask[b, i] = 1.0 if (case["mask"] == "binary" or N > 1) else 0.5
                i += 1
    out = dict(rigids_t=np.concatenate([quat, trans.astype(F32)], axis=-1).reshape(B, N, 7), frame_index=fi.reshape(B, N),
               scale_index=si.reshape(B, N), rot_score=rot_score.reshape(B, N, 3), z_rot=z_rot.reshape(B, N, 3),
               trans_score=(0.1 * rng.standard_normal((B, N, 3))).astype(F32), z_trans=rng.standard_normal((B, N, 3)), mask=mask)
    psi = rng.standard_normal((B, N, 2))
    out["psi"] = (psi / np.linalg.norm(psi, axis=-1, keepdims=True)).astype(F32)
    out["aatype"] = rng.integers(0, 21, (B, N)).astype(np.int32) if case["with_aatype"] else None
    out["pred_rigids"] = np.concatenate([np.tile(np.array([1, 0, 0, 0], dtype=F32), (B, N, 1)),
                                         rng.uniform(-50, 50, (B, N, 3)).astype(F32)], axis=-1)
    out["traj_fixed"] = (rng.random((B, N)) < 0.3).astype(F32)
    return out


# ---------------------------------------------------------------- IGSO(3) rotation score
SCORE_SIGMAS = (0.1, 0.37, 0.9, 1.5)
SCORE_NS = (5, 16, 20, 300)
SCORE_B = 4
SCORE_OMEGAS = (0.0, 1e-7, 1e-4, 9.99e-4, 1.001e-3, 0.01, 0.03, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5, 0.8, 1.0, 1.5, 2.0, 2.5, 3.0,
                PI - 1e-2, PI - 1e-4, PI)


def _unit_quats(rng, n):
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _quat_mul(p, q):
    a1, b1, c1, d1 = (p[..., i] for i in range(4))
    a2, b2, c2, d2 = (q[..., i] for i in range(4))
    return np.stack([a1 * a2 - b1 * b2 - c1 * c2 - d1 * d2, a1 * b2 + b1 * a2 + c1 * d2 - d1 * c2,
                     a1 * c2 - b1 * d2 + c1 * a2 + d1 * b2, a1 * d2 + b1 * c2 - c1 * b2 + d1 * a2], axis=-1)


def score_cases():
    """(N, rotation of the sigma order, res_mask or not): B = 4 samples, one sigma each."""
    return [dict(N=N, shift=s, with_mask=bool((i + s) % 2 == 0 or N == 300)) for i, N in enumerate(SCORE_NS) for s in range(4)]


def score_inputs(case, omegas=SCORE_OMEGAS):
    """q_0 random, q_t = q_0 * exp(omega * axis): the relative rotation q_0^-1 q_t has angle omega (0: q_t == q_0 bit for bit)."""
    B, N = SCORE_B, case["N"]
    rng = np.random.default_rng(20_000 + 10 * N + case["shift"])
    sig = np.roll(np.array(SCORE_SIGMAS), case["shift"])
    q0 = _unit_quats(rng, B * N).astype(F32)
    om = np.array(omegas)[(np.arange(B * N) * 7 + case["shift"]) % len(omegas)]
    ax = axes()[(np.arange(B * N) * 5 + 3 * case["shift"]) % len(axes())]
    rel = np.concatenate([np.cos(om / 2)[:, None], np.sin(om / 2)[:, None] * ax], axis=-1)
    qt = _quat_mul(q0.astype(np.float64), rel).astype(F32)
    qt[om == 0.0] = q0[om == 0.0]
    mask = None
    if case["with_mask"]:
        mask = np.ones((B, N), dtype=F32)
        mask.reshape(-1)[2::5] = 0.0
    return dict(sigma=sig, q0=q0.reshape(B, N, 4), qt=qt.reshape(B, N, 4), omega=om.reshape(B, N), mask=mask)


CACHED_WIDTHS = (2, 3, 1000)


def cached_inputs(n_omega, N=40, B=3):
    """so3.use_cached_score: table [B, n_omega] and the n_omega - 1 inner edges of linspace(0, pi, n_omega + 1)[1:]; omegas from 0
    (below the first edge) to pi (above the last), and next to the first and last edge on either side."""
    rng = np.random.default_rng(30_000 + n_omega)
    edges = np.linspace(0.0, PI, n_omega + 1)[1:][:-1]
    special = [0.0, 1e-4, edges[0] * 0.5, edges[0] - 1e-3, edges[0] + 1e-3, edges[-1] - 1e-3, edges[-1] + 1e-3, (edges[-1] + PI) / 2,
               PI - 1e-4, PI]
    om = np.concatenate([np.array(special), rng.uniform(0, PI, B * N - len(special))])
    q0 = _unit_quats(rng, B * N).astype(F32)
    ax = rng.standard_normal((B * N, 3))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    rel = np.concatenate([np.cos(om / 2)[:, None], np.sin(om / 2)[:, None] * ax], axis=-1)
    qt = _quat_mul(q0.astype(np.float64), rel).astype(F32)
    qt[om == 0.0] = q0[om == 0.0]
    mask = np.ones((B, N), dtype=F32)
    mask.reshape(-1)[4::9] = 0.0
    return dict(table=rng.standard_normal((B, n_omega)), edges=edges, q0=q0.reshape(B, N, 4), qt=qt.reshape(B, N, 4), mask=mask)


# ---------------------------------------------------------------- backbone atoms / quaternion update
def backbone_inputs(per_type=6):
    """Every residue type 0..20 ``per_type`` times: tensor_7 frames, psi, aatype."""
    rng = np.random.default_rng(40_000)
    n = 21 * per_type
    t7 = np.concatenate([_unit_quats(rng, n), rng.uniform(-50, 50, (n, 3))], axis=-1).astype(F32)
    psi = rng.standard_normal((n, 2))
    psi = (psi / np.linalg.norm(psi, axis=-1, keepdims=True)).astype(F32)
    psi[:4] = np.array([[0, 1], [1, 0], [0, -1], [-1, 0]], dtype=F32)
    return dict(t7=t7, psi=psi, aatype=np.tile(np.arange(21, dtype=np.int32), per_type))


def update_inputs():
    """Rigid.compose_q_update_vec: frames from the grid, updates of length 0, 1e-4, 1 and 10 (quaternion part) / the same in scaled
    translation units, mask 0 and 1.  Translations within +-10 (the trunk's scaled units)."""
    rng = np.random.default_rng(50_000)
    q = frame_quats()[::7]
    n = len(q)
    t7 = np.concatenate([q, rng.uniform(-10, 10, (n, 3)).astype(F32)], axis=-1)
    size = np.array([0.0, 1e-4, 1.0, 10.0])[np.arange(n) % 4]
    upd = (rng.standard_normal((n, 6)) * size[:, None]).astype(F32)
    mask = ((np.arange(n) // 4) % 2).astype(F32)
    return dict(t7=t7, upd=upd, mask=mask)


# ---------------------------------------------------------------- the reference's answers (oracle/, float64 NumPy)
def reverse_reference(case, inp, odiff):
    """oracle.diffuser.SE3Diffuser.reverse on one case -> dict(rot f32 [B,N,3,3], trans f32 [B,N,3], rot64 = the same matrices before the
    float32 cast, ang_t / ang_c = angle of x_t / of the composed rotation, frac = residues with a mask strictly between 0 and 1,
    keep = residues whose rotation is compared).

    Fractional masks interpolate rotation VECTORS, whose sign flips at pi in the reference itself: such a residue is compared only if the
    angle of x_t and (where rotations are diffused: otherwise nothing is composed) the composed angle are below NEAR_PI.
    """
    from oracle import frames as fr
    B, N, t, dt, ns = case["B"], case["N"], case["t"], case["dt"], case["noise_scale"]
    q, tr = inp["rigids_t"][..., :4], inp["rigids_t"][..., 4:]
    m = None if inp["mask"] is None else inp["mask"].astype(np.float64)
    rot, trans = odiff.reverse(q, tr, inp["rot_score"], inp["trans_score"], t, dt, diffuse_mask=m, center=bool(case["center"]),
                               noise_scale=ns, z_rot=inp["z_rot"], z_trans=inp["z_trans"], diffuse_rot=bool(case["diffuse_rot"]),
                               diffuse_trans=bool(case["diffuse_trans"]))
    _, rv = odiff._extract(q, tr)
    g = odiff._so3_diffuser.diffusion_coef(t)
    pert = (g**2) * inp["rot_score"] * dt + g * np.sqrt(dt) * (ns * inp["z_rot"])
    rvc = fr.compose_rotvec(rv.reshape(-1, 3), pert.reshape(-1, 3)).reshape(rv.shape)
    rv1 = rvc if case["diffuse_rot"] else rv
    if m is not None:
        rv1 = m[..., None] * rv1 + (1 - m[..., None]) * rv
    rot64 = fr.scipy_from_rotvec_as_matrix(rv1)
    ang_t, ang_c = np.linalg.norm(rv, axis=-1), np.linalg.norm(rvc, axis=-1)
    frac = np.zeros((B, N), dtype=bool) if m is None else (m > 0) & (m < 1)
    bad = (ang_t >= NEAR_PI) | ((ang_c >= NEAR_PI) & bool(case["diffuse_rot"]))
    return dict(rot=rot, trans=trans, rot64=rot64, ang_t=ang_t, ang_c=ang_c, frac=frac, keep=~(frac & bad), pert=pert)


def score_reference(inp):
    """oracle.diffuser.torch_score_mixed per sample -> dict(score f64 [B,N,3] (res_mask applied), rv f32, omega f32 (with the reference's
    +1e-6), conditioned = the float64 series value f > 1e-2: where the float32 series of the reference itself is conditioned)."""
    from oracle import diffuser as od
    from oracle import frames as fr
    rv = fr.quat_to_rotvec(fr.quat_multiply(fr.invert_quat(inp["q0"]).astype(F32), inp["qt"]).astype(F32))
    sc = np.stack([od.torch_score_mixed(rv[b], s) for b, s in enumerate(inp["sigma"])])
    om = np.linalg.norm(rv, axis=-1)
    f = np.stack([od.igso3_expansion_np(np.maximum(om[b].astype(np.float64), 1e-9), s) for b, s in enumerate(inp["sigma"])])
    if inp["mask"] is not None:
        sc = sc * inp["mask"][..., None]
    return dict(score=sc, rv=rv, omega=(om + F32(1e-6)).astype(F32), conditioned=f > 1e-2)
