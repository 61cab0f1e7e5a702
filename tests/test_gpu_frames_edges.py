"""GPU edge-case parity (-m gpu) of framedipt_amd/csrc/frames.hip: the fused reverse step, the float64 SO(3) exp / log, the IGSO(3) score,
the frame algebra and the backbone builder on the cases of tests/frames_cases.py — rotations at 0, at the 1e-3 series switches and at
pi, exact ties of the Markley comparisons, fractional masks, every switch of the step, block and wave edges.

Every comparison is against the float64 NumPy oracle (oracle/frames.py, oracle/diffuser.py), never against another HIP path;
tests/test_frames_cases_host.py shows on the CPU that the reference itself meets each bound and exclusion cap used here.  The
near-pi exclusions of test_gpu_parity.py::test_frame_ops_vs_reference_goldens and test_gpu_sizes.py::
test_round2_frame_ops_vs_reference_goldens are covered here through the rotation MATRIX, which is well conditioned at pi."""
import numpy as np
import pytest
import torch

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


def _call(lib, name, *args):
    from framedipt_amd import _lib
    _lib.check(getattr(lib, name)(*[_lib.ptr(a) if torch.is_tensor(a) else a for a in args], _lib.stream_ptr()), name)


# ---------------------------------------------------------------- reverse step
@pytest.mark.parametrize("B", fc.SIZES_B)
@pytest.mark.parametrize("N", fc.SIZES_N)
def test_reverse_step_edges_vs_oracle(lib, odiff, tables, B, N):
    """fdipt_se3_reverse_step (in place, one block per sample) and fdipt_se3_reverse_step_traj with atoms and the trans_traj row (out of
    place, N/64 blocks) against oracle.diffuser.SE3Diffuser.reverse: mask NULL / binary / fractional x center x diffuse_rot x
    diffuse_trans x t, 72 cases per (B, N), frames from the adversarial grid.  Binary and NULL masks exclude nothing."""
    from framedipt_amd import residue_tables
    so3, r3 = odiff._so3_diffuser, odiff._r3_diffuser
    consts = (so3.min_sigma, so3.max_sigma, r3.min_b, r3.max_b, r3._conf.coordinate_scaling)
    tb = dev(residue_tables.packed_bytes())
    frames = fc.frame_quats()
    worst = dict(out_rot=0.0, trans=0.0, quat_rot=0.0, quat_norm=0.0, fixed_rot=0.0, atom37=0.0, trans_traj=0.0)
    n_cases = n_res = n_cmp = 0
    for case in fc.reverse_cases():
        if (case["B"], case["N"]) != (B, N):
            continue
        inp = fc.reverse_inputs(case, so3.diffusion_coef(case["t"]), frames)
        ref = fc.reverse_reference(case, inp, odiff)
        t7 = dev(inp["rigids_t"])
        mask = dev(inp["mask"])
        head = (B, N, t7, dev(inp["rot_score"]), dev(inp["trans_score"]), mask, dev(inp["z_rot"]), dev(inp["z_trans"]),
                float(case["t"]), float(case["dt"]), float(case["noise_scale"]), case["center"], case["diffuse_rot"],
                case["diffuse_trans"], *consts)
        out_rot = torch.full((B, N, 3, 3), 7.0, device="cuda")
        if case["inplace"]:
            out = t7.clone()
            _call(lib, "fdipt_se3_reverse_step", *head[:2], out, *head[3:], out, out_rot)
        else:
            out = torch.full((B, N, 7), 7.0, device="cuda")
            a37, ttraj = torch.full((B, N, 37, 3), 7.0, device="cuda"), torch.full((B, N, 3), 7.0, device="cuda")
            _call(lib, "fdipt_se3_reverse_step_traj", *head, out, out_rot, dev(inp["psi"]), dev(inp["aatype"]), tb, a37,
                  dev(inp["pred_rigids"]), dev(inp["traj_fixed"]), ttraj)
        out, rot = host(out), host(out_rot)
        keep = ref["keep"]
        what = (case["k"], case["mask"], case["center"], case["diffuse_rot"], case["diffuse_trans"], case["t"], case["inplace"])
        e_rot = np.abs(rot.astype(np.float64) - ref["rot"])[keep].max(initial=0.0)
        e_tr = np.abs(out[..., 4:].astype(np.float64) - ref["trans"]).max()
        qr = fr.quat_to_rot(out[..., :4])
        e_q = np.abs(qr.astype(np.float64) - ref["rot"])[keep].max(initial=0.0)
        e_n = np.abs(np.linalg.norm(out[..., :4].astype(np.float64), axis=-1) - 1).max()
        worst.update(out_rot=max(worst["out_rot"], e_rot), trans=max(worst["trans"], e_tr), quat_rot=max(worst["quat_rot"], e_q),
                     quat_norm=max(worst["quat_norm"], e_n))
        assert np.isfinite(out).all() and np.isfinite(rot).all(), what
        assert e_rot <= 1e-6, (what, e_rot)
        assert e_tr <= 3e-5, (what, e_tr)
        assert e_q <= 3e-6, (what, e_q)
        assert (out[..., 0] >= 0).all() and e_n <= 1e-6, (what, e_n)
        if inp["mask"] is not None:  # fixed residues keep their frame
            fixed = inp["mask"] == 0
            e_f = np.abs(rot - fr.quat_to_rot(inp["rigids_t"][..., :4]))[fixed].max(initial=0.0)
            worst["fixed_rot"] = max(worst["fixed_rot"], e_f)
            assert e_f <= 1e-6, (what, e_f)
            assert np.array_equal(out[..., 4:][fixed], inp["rigids_t"][..., 4:][fixed]), what
        if not case["diffuse_trans"]:
            assert np.array_equal(out[..., 4:], inp["rigids_t"][..., 4:]), what
        if not case["inplace"]:
            # the atom37 frame and the trans_traj row are functions of the step's own x_{t-1} (asserted above): the oracle's builder on it
            ref37, _ = compute_backbone_of(rot, out[..., 4:], inp, tables)
            e_a = np.abs(host(a37) - ref37).max()
            dm = np.ones((B, N), dtype=F32) if inp["mask"] is None else inp["mask"]
            ref_tt = dm[..., None] * inp["pred_rigids"][..., 4:] + inp["traj_fixed"][..., None] * out[..., 4:]
            e_t = np.abs(host(ttraj) - ref_tt).max()
            worst.update(atom37=max(worst["atom37"], e_a), trans_traj=max(worst["trans_traj"], e_t))
            assert e_a <= 3e-5, (what, e_a)
            assert e_t <= 3e-5, (what, e_t)
        n_cases += 1
        n_res += B * N
        n_cmp += int(keep.sum())
    assert n_cases == 72
    print(f"reverse step B={B} N={N}: {n_cases} cases, {n_res} residues ({n_cmp} rotations compared); largest errors " +
          ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def compute_backbone_of(rot, trans, inp, tables):
    from oracle.score_network import compute_backbone
    return compute_backbone(None, trans, inp["psi"], inp["aatype"], tables, rot=rot)


# ---------------------------------------------------------------- SO(3) entry points
def _so3(lib, name, x, out_shape):
    x = dev(np.asarray(x, dtype=np.float64))
    out = torch.empty(*out_shape, dtype=torch.float64, device="cuda")
    _call(lib, name, x.shape[0], x, out)
    return host(out)


def test_so3_exp_log_edges_vs_oracle(lib):
    """fdipt_so3_exp at 1e-13 on the whole grid (both sides of the 1e-3 switch, angles above pi); fdipt_so3_log through exp(log(R)) = R
    at 1e-12 for every angle, pi included, on float64 rotations and on the float32-rounded matrices the reverse step feeds it; the
    rotation vector itself at 1e-9 below pi - 1e-2 (the negative-scalar flip decides it on hundreds of these); exact half turns whose
    two largest diagonal entries tie: pi * axis with the sign of the first maximum (SciPy's argmax)."""
    rv = fc.rotvec_grid(fc.BEYOND_PI)
    n = len(rv)
    got = _so3(lib, "fdipt_so3_exp", rv, (n, 3, 3))
    ref = fr.scipy_from_rotvec_as_matrix(rv)
    e_exp = np.abs(got - ref).max()
    assert e_exp <= 1e-13, e_exp
    worst = {}
    for tag, R in (("float64", fr.scipy_from_rotvec_as_matrix(fc.rotvec_grid())),
                   ("float32", fr.quat_to_rot(fc.frame_quats()).astype(np.float64))):
        lg = _so3(lib, "fdipt_so3_log", R, (len(R), 3))
        ref_lg = fr.scipy_from_matrix_as_rotvec(R)
        e_rt = np.abs(fr.scipy_from_rotvec_as_matrix(lg) - fr.scipy_from_rotvec_as_matrix(ref_lg)).max()
        if tag == "float64":
            e_rt = max(e_rt, np.abs(fr.scipy_from_rotvec_as_matrix(lg) - R).max())
        ok = np.linalg.norm(ref_lg, axis=-1) < fc.NEAR_PI
        e_rv = np.abs(lg - ref_lg)[ok].max()
        worst[tag] = (e_rt, e_rv, int(ok.sum()))
        assert np.isfinite(lg).all() and (np.linalg.norm(lg, axis=-1) <= np.pi + 1e-12).all()
        assert e_rt <= 1e-12, (tag, e_rt)
        assert e_rv <= 1e-9, (tag, e_rv)
    mats, ax = fc.exact_half_turns()
    lg = _so3(lib, "fdipt_so3_log", mats, (len(mats), 3))
    e_tie = np.abs(lg - fr.scipy_from_matrix_as_rotvec(mats)).max()
    assert e_tie <= 1e-12, (e_tie, lg, np.pi * ax)
    print(f"so3 exp: {n} items, largest error {e_exp:.2e}; log: " +
          "; ".join(f"{k} exp(log) {v[0]:.2e}, rotvec {v[1]:.2e} on {v[2]} items" for k, v in worst.items()) + f"; exact ties {e_tie:.2e}")


def test_geomstats_maps_edges_vs_oracle(lib):
    """fdipt_so3_exp_geomstats / fdipt_so3_omega at 1e-12 on the whole grid; fdipt_so3_log_geomstats at the two-tier bound of
    test_round2_frame_ops_vs_reference_goldens (2e-5, and 2e-3 above pi - 3e-2) on float64 rotations and float32-rounded ones.  Within
    the near-pi branch the reference takes the signs of the vector from the longest row of (I + R) / 2; for a mixed-sign diagonal axis
    two rows are equally long and give opposite vectors (both are logarithms of a half turn), so such an item is compared up to that
    sign — where the two longest rows differ by less than 1e-9, nowhere else."""
    rv = fc.rotvec_grid()
    n = len(rv)
    got = _so3(lib, "fdipt_so3_exp_geomstats", rv, (n, 3, 3))
    e_exp = np.abs(got - fr.gs_exp(rv)).max()
    assert e_exp <= 1e-12, e_exp
    R64 = fr.scipy_from_rotvec_as_matrix(rv)
    om = torch.empty(n, dtype=torch.float64, device="cuda")
    _call(lib, "fdipt_so3_omega", n, dev(R64), 1e-4, om)
    e_om = np.abs(host(om) - fr.gs_omega(R64)).max()
    assert e_om <= 1e-12, e_om
    e_lo = e_hi = 0.0
    n_hi = 0
    for R, ang in ((R64, np.linalg.norm(rv, axis=-1)),
                   (fr.quat_to_rot(fc.frame_quats()[:n]).astype(np.float64), np.linalg.norm(rv, axis=-1))):
        lg = _so3(lib, "fdipt_so3_log_geomstats", R, (n, 3))
        ref = fr.gs_log(R)
        near = ang > np.pi - 3e-2
        rows = np.sort(fr.gs_log_line_norms(R), axis=-1)
        tied = near & (rows[:, -1] - rows[:, -2] < 1e-9)
        err = np.abs(lg - ref).max(-1)
        err[tied] = np.minimum(err, np.abs(lg + ref).max(-1))[tied]
        assert near.sum() >= 30
        n_hi += int(near.sum())
        e_lo, e_hi = max(e_lo, err[~near].max()), max(e_hi, err[near].max())
        assert err[~near].max() <= 2e-5 and err[near].max() <= 2e-3, (err[~near].max(), err[near].max())
    print(f"geomstats: exp {e_exp:.2e}, omega {e_om:.2e}, log {e_lo:.2e} / near pi {e_hi:.2e} ({n_hi} near-pi items)")


def test_quaternion_maps_edges_vs_oracle(lib):
    """fdipt_rot_to_quat through quat_to_rot(rot_to_quat(R)) at 3e-6 (every Markley branch 270 times or more and the exact ties:
    counted by the host test), stored with w >= 0; fdipt_quat_to_rot at 1e-6; fdipt_quat_to_rotvec at 3e-6 on both sides of its 1e-3
    switch and up to pi."""
    q = fc.frame_quats()
    n = len(q)
    R = torch.empty(n, 3, 3, device="cuda")
    _call(lib, "fdipt_quat_to_rot", n, dev(q), R)
    e_r = np.abs(host(R) - fr.quat_to_rot(q)).max()
    assert e_r <= 1e-6, e_r
    ref_R = fr.quat_to_rot(q)
    back = torch.empty(n, 4, device="cuda")
    _call(lib, "fdipt_rot_to_quat", n, dev(ref_R), back)
    back = host(back)
    e_b = np.abs(fr.quat_to_rot(back).astype(np.float64) - fr.quat_to_rot(fr.rot_to_quat(ref_R.astype(np.float64)))).max()
    assert e_b <= 3e-6, e_b
    assert (back[:, 0] >= 0).all() and np.abs(np.linalg.norm(back.astype(np.float64), axis=-1) - 1).max() <= 1e-6
    rv = torch.empty(n, 3, device="cuda")
    _call(lib, "fdipt_quat_to_rotvec", n, dev(q), rv)
    e_v = np.abs(host(rv) - fr.quat_to_rotvec(q)).max()
    assert e_v <= 3e-6, e_v
    print(f"quaternion maps on {n} frames: quat_to_rot {e_r:.2e}, rot_to_quat round trip {e_b:.2e}, quat_to_rotvec {e_v:.2e}")


# ---------------------------------------------------------------- rotation score
def test_rot_score_edges_vs_oracle(lib):
    """fdipt_igso3_rot_score against oracle.diffuser.torch_score_mixed: sigma 0.1 / 0.37 / 0.9 / 1.5 one per sample in every order, omega
    from 0 (q_t == q_0) to pi, N = 5 (weights per lane), 16, 20 (blocks spanning two samples), 300, res_mask with zeros.  Compared where
    the float64 series value f > 1e-2 (the conditioned regime of the reference's float32 series, as test_scores_vs_reference_goldens) at
    2e-3 |ref| + 1e-5; finite everywhere; exactly 0 under a zero mask."""
    worst = 0.0
    n_cmp = n_all = 0
    for case in fc.score_cases():
        inp = fc.score_inputs(case)
        ref = fc.score_reference(inp)
        B, N = fc.SCORE_B, case["N"]
        out = torch.full((B, N, 3), 7.0, dtype=torch.float64, device="cuda")
        _call(lib, "fdipt_igso3_rot_score", B, N, dev(inp["qt"]), dev(inp["q0"]), dev(inp["sigma"]), dev(inp["mask"]), out)
        got = host(out)
        assert np.isfinite(got).all(), case
        if inp["mask"] is not None:
            assert (got[inp["mask"] == 0] == 0).all(), case
        ok = ref["conditioned"]
        err, mag = np.abs(got - ref["score"]).max(-1), np.abs(ref["score"]).max(-1)
        ratio = (err / (2e-3 * mag + 1e-5))[ok]
        worst = max(worst, ratio.max())
        n_cmp += int(ok.sum())
        n_all += B * N
        assert (ratio <= 1).all(), (case, ratio.max())
    print(f"rotation score: {n_all} residues, {n_cmp} compared; largest error / bound {worst:.3f}")


@pytest.mark.parametrize("n_omega", fc.CACHED_WIDTHS)
def test_cached_rot_score_edges_vs_oracle(lib, n_omega):
    """fdipt_igso3_rot_score_cached: the bucket of np.searchsorted(edges, omega, "left") on the oracle's float32 omega, for tables 2, 3 and
    1000 wide and omegas below the first edge and above the last.  An omega within 4 float32 spacings of an edge is left out (its bucket
    hangs on the last bit of a float32 chain; at most 1 % of the residues, asserted on the CPU)."""
    inp = fc.cached_inputs(n_omega)
    ref = fc.score_reference(dict(inp, sigma=[1.0] * 3))
    B, N = inp["mask"].shape
    om = ref["omega"].astype(np.float64)
    idx = np.searchsorted(inp["edges"], om, "left")
    norm = np.take_along_axis(inp["table"], idx, axis=1)
    want = norm[..., None] * ref["rv"].astype(np.float64) / om[..., None] * inp["mask"][..., None]
    out = torch.full((B, N, 3), 7.0, dtype=torch.float64, device="cuda")
    _call(lib, "fdipt_igso3_rot_score_cached", B, N, dev(inp["qt"]), dev(inp["q0"]), dev(inp["table"]), dev(inp["edges"]), n_omega,
          dev(inp["mask"]), out)
    got = host(out)
    assert np.isfinite(got).all() and (got[inp["mask"] == 0] == 0).all()
    ok = np.abs(om[..., None] - inp["edges"]).min(-1) > 4 * np.spacing(ref["omega"])
    err, mag = np.abs(got - want).max(-1), np.abs(want).max(-1)
    ratio = (err / (2e-3 * mag + 1e-5))[ok]
    print(f"cached score n_omega={n_omega}: {int(ok.sum())} of {B * N} compared; largest error / bound {ratio.max():.2e}")
    assert (ratio <= 1).all(), ratio.max()


# ---------------------------------------------------------------- backbone atoms / quaternion update
def test_backbone_every_residue_type_vs_oracle(lib, tables):
    """fdipt_backbone_atoms for every aatype 0..20 (the golden holds 17 of them) and for aatype = NULL, atom37 and atom14, at 3e-5 A."""
    from framedipt_amd import residue_tables
    from oracle.score_network import compute_backbone
    inp = fc.backbone_inputs()
    n = len(inp["aatype"])
    tb = dev(residue_tables.packed_bytes())
    assert set(inp["aatype"]) == set(range(21))
    for aatype in (inp["aatype"], None):
        a37, a14 = torch.full((n, 37, 3), 7.0, device="cuda"), torch.full((n, 14, 3), 7.0, device="cuda")
        _call(lib, "fdipt_backbone_atoms", n, dev(inp["t7"]), None, None, dev(inp["psi"]), dev(aatype), tb, a37, a14)
        r37, r14 = compute_backbone(inp["t7"][:, :4], inp["t7"][:, 4:], inp["psi"], aatype, tables)
        e37, e14 = np.abs(host(a37) - r37), np.abs(host(a14) - r14)
        print(f"backbone aatype={'given' if aatype is not None else 'NULL'}: atom37 {e37.max():.2e}, atom14 {e14.max():.2e}")
        assert e37.max() <= 3e-5 and e14.max() <= 3e-5, (e37.reshape(n, -1).max(-1), e14.reshape(n, -1).max(-1))
        assert (np.abs(r14).reshape(n, -1).max(-1) > 0).all()


def test_compose_q_update_edges_vs_oracle(lib):
    """fdipt_rigid_compose_q_update with mask 0 and 1, zero, tiny, unit and large updates, frames from the grid: quaternion at 1e-6 up
    to its free sign, translation at 1e-5."""
    inp = fc.update_inputs()
    n = len(inp["mask"])
    out = torch.full((n, 7), 7.0, device="cuda")
    _call(lib, "fdipt_rigid_compose_q_update", n, dev(inp["t7"]), dev(inp["upd"]), dev(inp["mask"]), out)
    got = host(out)
    rq, rt = fr.compose_q_update_vec(inp["t7"][:, :4], inp["t7"][:, 4:], inp["upd"], inp["mask"][:, None])
    sgn = np.where((got[:, :4] * rq).sum(-1, keepdims=True) < 0, -1.0, 1.0)
    e_q, e_t = np.abs(got[:, :4] * sgn - rq).max(), np.abs(got[:, 4:] - rt).max()
    print(f"compose_q_update on {n} frames: quaternion {e_q:.2e}, translation {e_t:.2e}")
    assert e_q <= 1e-6 and e_t <= 1e-5, (e_q, e_t)
    fixed = inp["mask"] == 0
    assert np.array_equal(got[fixed, 4:], inp["t7"][fixed, 4:])


# ---------------------------------------------------------------- step addressing of the cursor entries
STEP_B, STEP_T = 3, 4
STEP_MODES = {  # (state_ring, frame_rows): step-major; ring with a row map that skips steps 0 and 2; ring with the step-major frame rows
    "step_major": (0, None),
    "ring_map": (1, (-1, 0, -1, 1)),
    "ring_no_map": (1, None),
}
_step_runs = {}


def _step_reference(lib, N, gen):
    """Random inputs of STEP_T steps and, per step, what the non-indexed entry (fdipt_se3_reverse_step_traj / _traj_gen: pinned to the
    oracle by test_reverse_step_edges_vs_oracle) writes for it: x_{t-1}, the atom37 frame, the trans_traj row.  Computed once per
    (N, gen) and shared by the addressing modes."""
    if (N, gen) in _step_runs:
        return _step_runs[N, gen]
    from framedipt_amd import config, residue_tables
    from framedipt_amd import noise as noise_mod
    B, T = STEP_B, STEP_T
    rng = np.random.default_rng(1000 + N)
    so3, r3 = (lambda c: (c.so3, c.r3))(config.base_config().diffuser)
    consts = (float(so3.min_sigma), float(so3.max_sigma), float(r3.min_b), float(r3.max_b), float(r3.coordinate_scaling))
    q = rng.normal(size=(B, N, 4))
    q = q / np.linalg.norm(q, axis=-1, keepdims=True) * np.where(q[..., :1] < 0, -1.0, 1.0)
    psi = rng.normal(size=(B, N, 2))
    mask = (rng.random((B, N)) < 0.7).astype(F32)
    inp = dict(
        x0=dev(np.concatenate([q, 5.0 * rng.normal(size=(B, N, 3))], -1).astype(F32)),
        rot_score=dev(0.3 * rng.normal(size=(B, N, 3))), trans_score=dev((0.3 * rng.normal(size=(B, N, 3))).astype(F32)),
        mask=dev(mask), fixed=dev((1 - mask).astype(F32)), psi=dev((psi / np.linalg.norm(psi, axis=-1, keepdims=True)).astype(F32)),
        aatype=dev(rng.integers(0, 21, size=(B, N)).astype(np.int32)), pred=dev(rng.normal(size=(B, N, 7)).astype(F32)),
        z_rot=None if gen else dev(rng.normal(size=(T, B, N, 3))), z_trans=None if gen else dev(rng.normal(size=(T, B, N, 3))),
        keys=noise_mod.keys_tensor(noise_mod.as_keys(77, B), "cuda") if gen else None,
        t_table=np.linspace(1.0, 0.25, T), t_dev=dev(np.linspace(1.0, 0.25, T)), dt=1.0 / T, noise_scale=0.1, consts=consts, tables=dev(residue_tables.packed_bytes()))
    x, steps = inp["x0"], []
    for k in range(T):
        out, a37, tt = (torch.full((B, N, *s), 7.0, device="cuda") for s in ((7,), (37, 3), (3,)))
        noise = (inp["keys"], k) if gen else (inp["z_rot"][k], inp["z_trans"][k])
        _call(lib, "fdipt_se3_reverse_step_traj_gen" if gen else "fdipt_se3_reverse_step_traj", B, N, x, inp["rot_score"], inp["trans_score"],
              inp["mask"], *noise, float(inp["t_table"][k]), inp["dt"], inp["noise_scale"], 1, 1, 1, *consts, out, None, inp["psi"],
              inp["aatype"], inp["tables"], a37, inp["pred"], inp["fixed"], tt)
        steps.append(dict(x=out, atom37=a37, trans_traj=tt))
        x = out
    torch.cuda.synchronize()
    _step_runs[N, gen] = (inp, steps)
    return inp, steps


@pytest.mark.parametrize("mode", list(STEP_MODES))
@pytest.mark.parametrize("N", [12, 70])
def test_step_addressing_of_the_indexed_reverse_step(lib, N, mode):
    """fdipt_se3_reverse_step_indexed / _indexed_gen driven from cursor 0 through STEP_T steps, atoms and trans_traj on, for the three
    addressing modes of FdiptReverseIndexed: after every step the row it had to write — of the state, prot_traj, trans_traj and
    kept_rigids — is bit for bit what the non-indexed entry writes for that step, every other row (all of them on a step whose frame row
    is -1) is as it was before the launch, and the cursor reads [k + 1, 0].  N = 12: below one 16-residue block and no multiple of 4;
    N = 70: two row blocks per sample, the second ragged, a ticket of 6 blocks."""
    import ctypes as C

    from framedipt_amd import _lib
    B, T = STEP_B, STEP_T
    ring, frame_rows = STEP_MODES[mode]
    for gen in (False, True):
        inp, ref = _step_reference(lib, N, gen)
        n_frames = T if frame_rows is None else 1 + max(frame_rows)
        state = torch.full((2 if ring else T + 1, B, N, 7), 7.0, device="cuda")
        state[0] = inp["x0"]
        arrays = dict(prot_traj=torch.full((n_frames, B, N, 37, 3), 7.0, device="cuda"),
                      trans_traj=torch.full((n_frames, B, N, 3), 7.0, device="cuda"))
        if frame_rows is not None:
            arrays["kept_rigids"] = torch.full((n_frames, B, N, 7), 7.0, device="cuda")
        cursor = torch.zeros(2, dtype=torch.int32, device="cuda")
        rows_dev = None if frame_rows is None else torch.tensor(frame_rows, dtype=torch.int32, device="cuda")
        a = _lib.ReverseIndexed()
        a.B, a.N = B, N
        for name, tns in dict(rigid_traj=state, rot_score=inp["rot_score"], trans_score=inp["trans_score"], diffuse_mask=inp["mask"],
                              z_rot=inp["z_rot"], z_trans=inp["z_trans"], t_table=inp["t_dev"], psi=inp["psi"], aatype=inp["aatype"],
                              bb_tables=inp["tables"], pred_rigids=inp["pred"], traj_fixed_mask=inp["fixed"], step_cursor=cursor,
                              frame_rows=rows_dev, **arrays).items():
            setattr(a, name, _lib.ptr(tns))
        a.state_ring = ring
        a.dt, a.noise_scale, a.center, a.diffuse_rot, a.diffuse_trans = inp["dt"], inp["noise_scale"], 1, 1, 1
        a.so3_min_sigma, a.so3_max_sigma, a.r3_min_b, a.r3_max_b, a.coordinate_scaling = inp["consts"]
        for k in range(T):
            what = f"N={N} {mode} gen={gen} step {k}"
            before = {name: v.clone() for name, v in dict(arrays, state=state).items()}
            if gen:
                _lib.check(lib.fdipt_se3_reverse_step_indexed_gen(C.byref(a), _lib.ptr(inp["keys"]), _lib.stream_ptr()), what)
            else:
                _lib.check(lib.fdipt_se3_reverse_step_indexed(C.byref(a), _lib.stream_ptr()), what)
            assert cursor.tolist() == [k + 1, 0], what
            frame = k if frame_rows is None else frame_rows[k]
            wrote = dict(state=((k + 1) & 1 if ring else k + 1, ref[k]["x"]))
            if frame >= 0:
                wrote.update({name: (frame, ref[k][dict(prot_traj="atom37", kept_rigids="x").get(name, name)]) for name in arrays})
            for name, v in dict(arrays, state=state).items():
                row, want = wrote.get(name, (None, None))
                for i in range(v.shape[0]):
                    assert torch.equal(v[i], want if i == row else before[name][i]), (what, name, i, row)
        assert cursor.tolist() == [T, 0]
