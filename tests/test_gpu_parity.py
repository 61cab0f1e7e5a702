"""GPU parity tests (-m gpu): the HIP path through the C ABI vs the reference goldens and the NumPy oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import kabsch_free_rmsd, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from framedipt_amd import _lib
    return _lib.load()


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x), device="cuda")
    return t.to(dtype) if dtype is not None else t


def test_mfma_fragment_maps(lib):
    for prec, tol in ((0, 2e-4), (2, 0.05)):
        err = C.c_double(-1)
        assert lib.fdipt_selftest_mfma(prec, C.byref(err)) == 0
        assert 0 <= err.value < tol, (prec, err.value)


def test_frame_ops_vs_reference_goldens():
    from framedipt_amd import rigid as R
    from framedipt_amd.diffusion import se3_diffuser as sd
    G = load_golden("ops.npz")
    q1, q2, t1, t2 = dev(G["q1"]), dev(G["q2"]), dev(G["t1"]), dev(G["t2"])
    cmp = lambda a, b, tol: np.testing.assert_allclose(a.cpu().numpy(), b, atol=tol)  # noqa: E731
    cmp(R.quat_to_rot(q1), G["quat_to_rot"], 1e-6)
    cmp(R.quat_multiply(q1, q2), G["quat_multiply"], 1e-6)
    cmp(R.quat_multiply_by_vec(q1, dev(G["vec"])), G["quat_multiply_by_vec"], 1e-6)
    cmp(R.invert_quat(q1), G["invert_quat"], 1e-6)
    cmp(R.quat_to_rot(R.rot_to_quat(R.quat_to_rot(q1))), G["rot_to_quat_rot"], 3e-6)
    r1 = R.Rigid.from_tensor_7(torch.cat([q1, t1], -1))
    r2 = R.Rigid.from_tensor_7(torch.cat([q2, t2], -1))
    cmp(r1.apply(dev(G["pts"])), G["apply"], 1e-5)
    cmp(r1.invert_apply(dev(G["pts"])), G["invert_apply"], 1e-5)
    c = r1.compose(r2)
    cmp(c.get_rots().get_rot_mats(), G["compose_rot"], 1e-6)
    cmp(c.get_trans(), G["compose_trans"], 1e-5)
    iv = r1.invert()
    cmp(iv.get_rots().get_rot_mats(), G["invert_rot"], 1e-6)
    cmp(iv.get_trans(), G["invert_trans"], 1e-5)
    cu = r1.compose_q_update_vec(dev(G["upd"]), dev(G["mask"]))
    cmp(cu.get_rots().get_quats(), G["cqu_quat"], 1e-6)
    cmp(cu.get_trans(), G["cqu_trans"], 1e-5)
    # SciPy conventions
    cmp(sd.so3_exp(dev(G["rv1"])), G["rotvec_to_matrix"], 1e-13)
    m = sd.so3_exp(dev(G["rv1"]))
    m2 = sd.so3_exp(dev(G["rv2"]))
    cmp(sd.so3_log(m @ m2), G["compose_rotvec"], 1e-9)
    # float32-rounded matrices: plain Markley (SciPy 1.7.3 pin) vs the SVD-projecting SciPy 1.15 golden
    rv = sd.so3_log(R.quat_to_rot(q1).double()).cpu().numpy()
    ang = np.linalg.norm(G["extract_rotvec"], axis=-1)
    ok = ang < np.pi - 1e-2  # (the excluded region: test_gpu_frames_edges.py::test_so3_exp_log_edges_vs_oracle, through exp(log(R)))
    assert np.abs(rv - G["extract_rotvec"])[ok].max() < 5e-7
    # quat_to_rotvec (float32 twin)
    from framedipt_amd import _lib
    out = torch.empty(q1.shape[0], 3, device="cuda")
    _lib.check(_lib.load().fdipt_quat_to_rotvec(q1.shape[0], _lib.ptr(q1), _lib.ptr(out), _lib.stream_ptr()))
    cmp(out, G["quat_to_rotvec"], 3e-6)


def _diffuser():
    from framedipt_amd import config
    from framedipt_amd.diffusion import SE3Diffuser
    return SE3Diffuser(config.base_config().diffuser)


def test_scores_vs_reference_goldens():
    from framedipt_amd.rigid import Rotation
    from oracle import diffuser as od
    from oracle import frames as fr
    G = load_golden("ops.npz")
    d = _diffuser()
    qt = Rotation(quats=dev(G["q1"])[None], normalize_quats=False)
    q0 = Rotation(quats=dev(G["rot_score_q0"])[None], normalize_quats=False)
    for i, t in enumerate([0.01, 0.5, 1.0]):
        tt = torch.tensor([t], dtype=torch.float32)
        rs = d.calc_rot_score(qt, q0, tt).cpu().numpy()[0]
        ref = G[f"rot_score_{i}"]
        rv = fr.quat_to_rotvec(fr.quat_multiply(fr.invert_quat(G["rot_score_q0"]), G["q1"]).astype(np.float32))
        sig = d._so3_diffuser.score_sigma(np.float32(t))[0]
        f = od.igso3_expansion_np(np.linalg.norm(rv, axis=-1).astype(np.float64), sig)
        ok = f > 1e-2  # conditioned regime of the float32 series
        assert ok.sum() >= 3
        err, mag = np.abs(rs - ref).max(-1), np.abs(ref).max(-1)
        assert (err[ok] <= 2e-3 * mag[ok] + 1e-5).all(), (i, err[ok], mag[ok])
        ts = d.calc_trans_score(dev(G["t1"])[None], dev(G["t2"])[None], tt, use_torch=True).cpu().numpy()[0]
        np.testing.assert_allclose(ts, G[f"trans_score_{i}"], rtol=3e-6, atol=2e-6)


def test_backbone_vs_reference_goldens():
    from framedipt_amd import _lib, residue_tables
    G = load_golden("ops.npz")
    lib = _lib.load()
    n = G["q1"].shape[0]
    t7 = dev(np.concatenate([G["q1"], G["t1"]], -1))
    tb = dev(residue_tables.packed_bytes())
    for aatype, k37, k14 in ((dev(G["bb_aatype"][0].astype(np.int32)), "bb_atom37", "bb_atom14"),
                             (None, "bb_atom37_none", "bb_atom14_none")):
        a37, a14 = torch.empty(n, 37, 3, device="cuda"), torch.empty(n, 14, 3, device="cuda")
        _lib.check(lib.fdipt_backbone_atoms(n, _lib.ptr(t7), None, None, _lib.ptr(dev(G["bb_psi"][0])), _lib.ptr(aatype),
                                            _lib.ptr(tb), _lib.ptr(a37), _lib.ptr(a14), _lib.stream_ptr()))
        np.testing.assert_allclose(a37.cpu().numpy(), G[k37][0], atol=3e-5)
        np.testing.assert_allclose(a14.cpu().numpy(), G[k14][0], atol=3e-5)


def test_sample_ref_vs_reference_goldens():
    from framedipt_amd import rigid as R
    X = load_golden("xT.npz")
    d = _diffuser()
    t7 = d.sample_ref(50, as_tensor_7=True)["rigids_t"]
    np.testing.assert_allclose(R.quat_to_rot(t7[:, :4]).cpu().numpy(),
                               R.quat_to_rot(dev(X["denovo_t7"][:, :4])).cpu().numpy(), atol=3e-6)
    np.testing.assert_allclose(t7[:, 4:].cpu().numpy(), X["denovo_t7"][:, 4:], atol=1e-6)
    imp = R.Rigid.from_tensor_7(dev(X["imp_t7"].astype(np.float32)))
    r = d.sample_ref(30, impute=imp, diffuse_mask=X["imp_mask"])["rigids_t"]
    np.testing.assert_allclose(r.get_rots().get_rot_mats().cpu().numpy(), X["inpaint_rot"], atol=2e-6)
    np.testing.assert_allclose(r.get_trans().cpu().numpy(), X["inpaint_trans"], atol=1e-5)
    with pytest.raises(ValueError):
        d.sample_ref(10, diffuse_mask=np.ones(10))
    with pytest.raises(ValueError):
        d.sample_ref(10, impute=imp)


@pytest.mark.parametrize("name", ["traj_small_denovo_n16_T10.npz", "traj_small_inpaint_n24_T10.npz",
                                  "traj_full_denovo_n64_T20.npz"])
def test_reverse_step_teacher_forced(name):
    T = load_golden(name)
    d = _diffuser()
    dm = dev(((1 - T["in_fixed_mask"]) * T["in_res_mask"]).astype(np.float32))
    dt = 1.0 / int(T["num_t"])
    for s in range(len(T["step_t"])):
        rot_out = torch.empty(1, dm.shape[1], 3, 3, device="cuda")
        out = d.reverse_device(dev(T["step_rigids_t"][s]), dev(T["step_rot_score"][s]),
                               dev(T["step_trans_score"][s].astype(np.float32)), dm, dev(T["noise_tape"][2 * s]),
                               dev(T["noise_tape"][2 * s + 1]), float(T["step_t"][s]), dt, True, float(T["noise_scale"]),
                               rot_out=rot_out)
        np.testing.assert_allclose(rot_out.cpu().numpy(), T["step_out_rot"][s], atol=1e-6)
        np.testing.assert_allclose(out[..., 4:].cpu().numpy(), T["step_out_trans"][s], atol=3e-5)


def _conf(name):
    from framedipt_amd import config
    inp = "inpaint" in name
    return (config.small_config(inp) if name.startswith("small") else config.base_config(inp)), inp


def _net(name, G, precision, kernel_flags=0):
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    conf, inp = _conf(name)
    d = SE3Diffuser(conf.diffuser)
    net = ScoreNetwork(conf.model, d, inpainting=inp, precision=precision, kernel_flags=kernel_flags)
    net.load_synthetic(int(G["weight_seed"]), float(G["bb_gain"])).to("cuda")
    return net, d, conf


def _feats(G):
    return {k[3:]: dev(G[k]) for k in G if k.startswith("in_")}


FWD = ["small_denovo_n16", "small_inpaint_n24", "small_denovo_n16_stress", "full_denovo_n64", "full_inpaint_n40"]


@pytest.mark.parametrize("name", FWD)
def test_forward_fp32_vs_reference_goldens(name):
    G = load_golden(f"fwd_{name}.npz")
    net, _, conf = _net(name, G, "fp32")
    out = net(_feats(G), trace=True)
    rows = list(G["trace_rows"])
    tn, te = out["trace_node"].cpu().numpy(), out["trace_edge"].cpu().numpy()
    np.testing.assert_allclose(tn[0], G["tr_node_init"], atol=1e-4)
    np.testing.assert_allclose(te[0][:, rows], G["tr_edge_init"], atol=1e-4)
    nb = conf.model.ipa.num_blocks
    for b in range(nb):
        np.testing.assert_allclose(tn[b + 1], G[f"tr_node_{b}"] * G["in_res_mask"][..., None], atol=2e-4)
        if b < nb - 1:
            np.testing.assert_allclose(te[b + 1][:, rows], G[f"tr_edge_{b}"], atol=2e-4)
    o = {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("trace")}
    np.testing.assert_allclose(o["rigids"][..., 4:], G["out_rigids"][..., 4:], atol=2e-4)
    np.testing.assert_allclose(np.abs(o["rigids"][..., :4]), np.abs(G["out_rigids"][..., :4]), atol=1e-5)
    np.testing.assert_allclose(o["psi"], G["out_psi"], atol=2e-4)
    np.testing.assert_allclose(o["atom37"], G["out_atom37"], atol=5e-4)
    np.testing.assert_allclose(o["atom14"], G["out_atom14"], atol=5e-4)
    ts = max(np.abs(G["out_trans_score"]).max(), 1.0)
    np.testing.assert_allclose(o["trans_score"], G["out_trans_score"], atol=3e-4 * ts)
    if "stress" not in name and name != "full_inpaint_n40":
        rs = max(np.abs(G["out_rot_score"]).max(), 1.0)
        np.testing.assert_allclose(o["rot_score"], G["out_rot_score"], atol=3e-3 * rs)
    assert o["psi"].dtype == G["out_psi"].dtype and o["rot_score"].dtype == np.float64


@pytest.mark.parametrize("name", ["small_denovo_n16", "full_denovo_n64"])
def test_forward_fp16_vs_reference_goldens(name):
    """fp16 mode against the reference at the two oldest fixtures, at the bounds of tests/test_gpu_sizes.py::test_forward_fp16_at_size
    (FP16_BOUND there: measured values x 2-3): node representation 3e-4 relative, CA 5e-4 A, backbone RMSD 5e-4 A.  The small-config
    network (widths the split-operand kernels are not compiled for: plain fp16 operands on the node path) gets 1e-3 / 1e-3 A."""
    G = load_golden(f"fwd_{name}.npz")
    net, _, conf = _net(name, G, "fp16")
    small = name.startswith("small")
    out = net(_feats(G), trace=True)
    tn = out["trace_node"].cpu().numpy()
    nb = conf.model.ipa.num_blocks
    for b in range(nb):
        ref = G[f"tr_node_{b}"]
        rel = np.linalg.norm(tn[b + 1] - ref) / np.linalg.norm(ref)
        assert rel < (1e-3 if small else 3e-4), (b, rel)
    o = {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("trace")}
    np.testing.assert_allclose(o["rigids"][..., 4:], G["out_rigids"][..., 4:], atol=1e-3 if small else 5e-4)
    assert kabsch_free_rmsd(o["atom37"], G["out_atom37"]) < (1e-3 if small else 5e-4)


def _teacher_forced_steps(name, precision):
    """Reference state in -> one HIP step; per step: t, backbone RMSD of x_{t-1} against the reference's, backbone RMSD of the
    forward's x_0 prediction (atom37 of the predicted frames / psi) against the reference's."""
    from framedipt_amd import inference as inf
    G = load_golden(f"traj_{name}.npz")
    net, d, _ = _net(name, G, precision)
    base = _feats(G)
    num_t, min_t = int(G["num_t"]), float(G["min_t"])
    steps = np.linspace(min_t, 1.0, num_t)[::-1]
    rigid_traj, prot, bb0 = G["res_rigid_traj"][::-1], G["res_prot_traj"][::-1], G["res_rigid_0_traj"][::-1]
    inp = "inpaint" in name
    rows = []
    for i, t in enumerate(steps):
        f = dict(base)
        f["rigids_t"] = dev(rigid_traj[i])
        f["sc_ca_t"] = dev(G["sc_in"][i + 1])
        # one-step trajectory: num_t=1 would change dt, so drive the pieces directly
        f["t"] = torch.tensor([t], dtype=torch.float32, device="cuda")
        out = net(f)
        aatype = None
        if inp:
            from framedipt_amd.model.score_network import preprocess_aatype
            aatype = preprocess_aatype(f["aatype"], f["fixed_mask"].float(), True, False).to(torch.int32).contiguous()
        atom37 = torch.empty(1, f["rigids_t"].shape[1], 37, 3, device="cuda")
        n = f["rigids_t"].shape[1]
        if t > min_t:
            dm = ((1 - f["fixed_mask"]) * f["res_mask"]).float().contiguous()
            rot_out = torch.empty(1, n, 3, 3, device="cuda")
            nxt = d.reverse_device(f["rigids_t"].float().contiguous(), out["rot_score"], out["trans_score"], dm,
                                   dev(G["noise_tape"][2 * i]), dev(G["noise_tape"][2 * i + 1]), t, 1 / num_t, True,
                                   float(G["noise_scale"]), rot_out=rot_out)
            inf._backbone(net, n, None, rot_out, nxt[..., 4:].contiguous(), out["psi"].float().contiguous(), aatype, atom37)
        else:
            inf._backbone(net, n, out["rigids"].contiguous(), None, None, out["psi"].float().contiguous(), aatype, atom37)
        rows.append((float(t), kabsch_free_rmsd(atom37.cpu().numpy(), prot[i]), kabsch_free_rmsd(out["atom37"].cpu().numpy(), bb0[i])))
    return np.array(rows)


def _teacher_forced_worst_rmsd(name, precision):
    """worst per-step backbone RMSD of x_{t-1} over all steps / over the reverse (noisy) steps only."""
    r = _teacher_forced_steps(name, precision)
    min_t = float(load_golden(f"traj_{name}.npz")["min_t"])
    return float(r[:, 1].max()), float(r[r[:, 0] > min_t, 1].max())


@pytest.mark.parametrize("name", ["small_denovo_n16_T10", "small_inpaint_n24_T10", "full_denovo_n64_T20"])
def test_teacher_forced_steps_fp32(name):
    """Per-step parity: reference state in -> one HIP step -> x_{t-1} backbone RMSD < 1e-3 A."""
    worst, _ = _teacher_forced_worst_rmsd(name, "fp32")
    assert worst < 1e-3, worst


def test_free_running_small_fp32():
    from framedipt_amd import inference as inf
    G = load_golden("traj_small_denovo_n16_T10.npz")
    net, d, _ = _net("small_denovo_n16_T10", G, "fp32")
    n = len(G["noise_tape"]) // 2
    tape = (np.stack([G["noise_tape"][2 * i] for i in range(n)]), np.stack([G["noise_tape"][2 * i + 1] for i in range(n)]))
    res = inf.inference_fn(net, d, _feats(G), int(G["num_t"]), float(G["min_t"]), aux_traj=True,
                           noise_scale=float(G["noise_scale"]), noise_tape=tape)
    for k in ("prot_traj", "rigid_traj", "trans_traj", "rigid_0_traj"):
        assert res[k].shape == G["res_" + k].shape, k
    assert tuple(res["psi_pred"].shape) == tuple(G["res_psi_pred"].shape)
    # free-running: against the reference's own thread-count divergence floor (5e-2 A at T=10)
    assert kabsch_free_rmsd(res["prot_traj"][0], G["res_prot_traj"][0]) < 5e-2
    assert kabsch_free_rmsd(res["rigid_0_traj"][-1], G["res_rigid_0_traj"][-1]) < 1e-3


def test_fails_loudly_on_cpu_tensors():
    from framedipt_amd import _lib
    from framedipt_amd import rigid as R
    with pytest.raises(_lib.FdiptError):
        R.quat_to_rot(torch.zeros(4, 4))


def test_edge_transition_register_kernel_vs_lds_kernel():
    """Half-precision EdgeTransition: the two register-resident kernels (edge_transition4.hip: 8x4-pair patches with the
    e_i / e_j parts folded into one k-step, default for N % 4 == 0; edge_transition3.hip: 16-pair waves, the N % 4 != 0
    path, here forced with FDIPT_KF_ET3) vs the any-width LDS-chain kernel (pair_mlp.hip, FDIPT_KF_GENERIC_PAIR) on the
    full-width network, and all three against the fp32 reference golden."""
    from framedipt_amd import _lib
    G = load_golden("fwd_full_denovo_n64.npz")
    rows = list(G["trace_rows"])
    outs = {}
    for tag, kf in (("v4", 0), ("v3", _lib.KF_ET3), ("v1", _lib.KF_GENERIC_PAIR)):
        net, _, conf = _net("full_denovo_n64", G, "fp16", kf)
        out = net(_feats(G), trace=True)
        outs[tag] = out["trace_edge"].cpu().numpy().copy()
    for tag in outs:  # edge embedder (trace slot 0): edge_embed2_kernel vs edge_embed_kernel
        rel = np.linalg.norm(outs[tag][0][:, rows] - G["tr_edge_init"]) / np.linalg.norm(G["tr_edge_init"])
        assert rel < 2e-3, (tag, "embed", rel)
    assert np.linalg.norm(outs["v1"][0] - outs["v3"][0]) / np.linalg.norm(outs["v1"][0]) < 2e-3
    for b in range(3):
        ref = G[f"tr_edge_{b}"]
        for tag in outs:
            got = outs[tag][b + 1][:, rows]
            rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
            assert rel < 3e-3, (tag, b, rel)
        for tag in ("v3", "v4"):
            a, c = outs["v1"][b + 1], outs[tag][b + 1]
            assert np.linalg.norm(a - c) / np.linalg.norm(a) < 3e-3, (tag, b)


def test_fused_paths_vs_separate_launches():
    """Half-precision node path with the fusions of the default path switched off (FDIPT_KF_UNFUSED_NODE: plain GEMM +
    LayerNorm launches instead of the row-block kernels / split-K output projection; FDIPT_KF_UNFOLDED: pair bias,
    feature split, torsion head and fills as their own launches) vs the default: same representation after every block."""
    from framedipt_amd import _lib
    G = load_golden("fwd_full_denovo_n64.npz")
    outs = {}
    for tag, kf in (("fused", 0), ("plain", _lib.KF_UNFUSED_NODE | _lib.KF_UNFOLDED), ("unfolded", _lib.KF_UNFOLDED)):
        net, _, conf = _net("full_denovo_n64", G, "fp16", kf)
        out = net(_feats(G), trace=True)
        outs[tag] = (out["trace_node"].cpu().numpy().copy(), out["rigids"].cpu().numpy().copy(),
                     out["psi"].cpu().numpy().copy())
    for tag in ("plain", "unfolded"):
        for b in range(5):
            a, c = outs[tag][0][b], outs["fused"][0][b]
            assert np.linalg.norm(a - c) / np.linalg.norm(a) < 2e-3, (tag, b)
        np.testing.assert_allclose(outs[tag][1][..., 4:], outs["fused"][1][..., 4:], atol=3e-3)
        np.testing.assert_allclose(outs[tag][2], outs["fused"][2], atol=5e-3)


def test_register_attention_vs_lds_attention():
    """Half-precision attention: attention3.hip / attention_seq.hip (scores in registers, N <= 512) vs the LDS-score kernels
    of attention.hip (the N > 512 path, here forced with FDIPT_KF_GENERIC_ATTN): node representation after every block on
    the full-width network."""
    from framedipt_amd import _lib
    G = load_golden("fwd_full_denovo_n64.npz")
    outs = {}
    for tag, kf in (("v3", 0), ("v1", _lib.KF_GENERIC_ATTN)):
        net, _, conf = _net("full_denovo_n64", G, "fp16", kf)
        out = net(_feats(G), trace=True)
        outs[tag] = (out["trace_node"].cpu().numpy().copy(), out["rigids"].cpu().numpy().copy())
    for b in range(4):
        a, c = outs["v1"][0][b + 1], outs["v3"][0][b + 1]
        assert np.linalg.norm(a - c) / np.linalg.norm(a) < 2e-3, b
        ref = G[f"tr_node_{b}"]
        assert np.linalg.norm(c - ref) / np.linalg.norm(ref) < 4e-3, b
    np.testing.assert_allclose(outs["v1"][1][..., 4:], outs["v3"][1][..., 4:], atol=3e-3)


@pytest.mark.parametrize("n,B,prec,inp", [(128, 2, "fp16", False), (450, 1, "fp16", True), (800, 1, "fp16", False),
                                          (1000, 1, "fp32", True), (77, 3, "fp16", False), (301, 2, "fp16", False),
                                          (45, 2, "fp16", False)])
def test_baseline_config_shapes_run(n, B, prec, inp):
    """BASELINE.json configs (N=128 de novo fp16, N~450 / ~800 TCR-like, N=1000 fp32 inpainting) and ragged sizes (N not
    a multiple of 4 / 32, batches whose 32-row blocks straddle samples): two
    reverse steps run through every kernel variant these sizes select; outputs finite, frames orthonormal, motif kept fixed."""
    from framedipt_amd import config, inference
    from framedipt_amd import rigid as R
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import ConditionalSampler, UnconditionalSampler
    conf = config.base_config(inpainting=inp)
    d = SE3Diffuser(conf.diffuser, device="cuda")
    net = ScoreNetwork(conf.model, d, inpainting=inp, precision=prec).load_synthetic(5).to("cuda")
    rng = np.random.default_rng(n)
    if inp:
        q = rng.standard_normal((n, 4)); q /= np.linalg.norm(q, axis=-1, keepdims=True)
        tr = np.cumsum(rng.standard_normal((n, 3)) * 2.0, 0); tr -= tr.mean(0)
        dm = np.zeros(n); dm[40:90] = 1  # one diffused window of 50 (config 5)
        n1 = n // 2
        feats_np = {"rigids_0": np.concatenate([q, tr], -1).astype(np.float32), "diffuse_mask": dm,
                    "aatype": rng.integers(0, 20, n), "seq_idx": np.concatenate([np.arange(n1), np.arange(n - n1) + n1 + 200]),
                    "chain_idx": np.concatenate([np.zeros(n1), np.ones(n - n1)]),
                    "torsion_angles_sin_cos": np.tile(np.array([0.0, 1.0]), (n, 7, 1))}
        ds = ConditionalSampler.from_features([("synthetic", feats_np)], d, "cuda", samples=B)
        items = [ds[i][2] for i in range(B)]
    else:
        ds = UnconditionalSampler(config.to_conf({"min_length": n, "max_length": n, "length_step": 1,
                                                  "samples_per_length": B}), d, "cuda")
        items = [ds[i][2] for i in range(B)]
    feats = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    res = inference.inference_fn(net, d, feats, num_t=2, min_t=0.01, aux_traj=True, noise_scale=0.1, inpainting=inp)
    assert res["prot_traj"].shape == (2, B, n, 37, 3) and res["rigid_traj"].shape == (3, B, n, 7)
    for k in ("prot_traj", "rigid_traj", "trans_traj", "rigid_0_traj"):
        assert np.isfinite(res[k]).all(), k
    rot = R.quat_to_rot(torch.as_tensor(res["rigid_traj"][0][..., :4].copy(), device="cuda")).cpu().numpy()
    np.testing.assert_allclose(rot @ np.swapaxes(rot, -1, -2), np.broadcast_to(np.eye(3), rot.shape), atol=1e-4)
    if inp:  # motif residues never move (se3_diffuser.py:397-399); the last step returns the x0 prediction for all
        fixed = feats["fixed_mask"][0].cpu().numpy().astype(bool)
        x_T, x_1 = res["rigid_traj"][-1][0], res["rigid_traj"][1][0]
        np.testing.assert_allclose(x_1[fixed, 4:], x_T[fixed, 4:], atol=1e-4)


@pytest.mark.parametrize("n,B", [(77, 3), (301, 2), (129, 4), (44, 3), (100, 2), (300, 2)])
def test_forward_fp16_vs_fp32_path_ragged_sizes(n, B):
    """Ragged shapes (N not a multiple of 4 / 32; 32-row blocks, 128-pair tiles and key tiles that straddle samples and
    padded keys; N % 8 == 4: the 8 x 4 patches of edge_transition4 straddle two samples): the fp16 kernels against the
    fp32 path of the same network (itself pinned to the reference goldens), at the bounds of the fp16 mode against the reference
    (test_gpu_sizes.py: node representation 3e-4, pair rows 2.5e-3 relative, CA 5e-4 A, backbone RMSD 5e-4 A)."""
    from framedipt_amd import config
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import UnconditionalSampler
    conf = config.base_config(inpainting=False)
    d = SE3Diffuser(conf.diffuser, device="cuda")
    ds = UnconditionalSampler(config.to_conf({"min_length": n, "max_length": n, "length_step": 1, "samples_per_length": B}), d, "cuda")
    items = [ds[i][2] for i in range(B)]
    feats = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    feats["res_mask"] = feats["res_mask"].clone()
    feats["res_mask"][0, n - 3:] = 0  # a few masked residues in the first sample
    feats["t"] = torch.full((B,), 0.4, device="cuda")
    if "sc_ca_t" not in feats:
        feats["sc_ca_t"] = torch.zeros(B, n, 3, device="cuda")
    outs = {}
    for prec in ("fp32", "fp16"):
        net = ScoreNetwork(conf.model, d, inpainting=False, precision=prec).load_synthetic(11).to("cuda")
        out = net(feats, trace=True)
        outs[prec] = {k: v.cpu().numpy().copy() for k, v in out.items()}
    tn32, tn16 = outs["fp32"]["trace_node"], outs["fp16"]["trace_node"]
    for b in range(1, tn32.shape[0]):
        rel = np.linalg.norm(tn16[b] - tn32[b]) / np.linalg.norm(tn32[b])
        assert rel < 3e-4, (b, rel)
    te32, te16 = outs["fp32"]["trace_edge"], outs["fp16"]["trace_edge"]
    for b in range(te32.shape[0]):  # edge embedder, then the EdgeTransition of every block but the last
        rel = np.linalg.norm(te16[b] - te32[b]) / np.linalg.norm(te32[b])
        assert rel < 2.5e-3, ("edge", b, rel)
    np.testing.assert_allclose(outs["fp16"]["rigids"][..., 4:], outs["fp32"]["rigids"][..., 4:], atol=5e-4)
    # psi is the unit vector of a small 2-vector (ill-conditioned where its norm is tiny): bound the outlier fraction
    bad = np.abs(outs["fp16"]["psi"] - outs["fp32"]["psi"]).max(-1) > 5e-3
    assert bad.mean() < 0.01, bad.mean()
    assert kabsch_free_rmsd(outs["fp16"]["atom37"], outs["fp32"]["atom37"]) < 5e-4


def test_reverse_step_blocks_and_fused_atoms():
    """The reverse step over N/64 row blocks per sample (out of place) vs one block per sample (in place), and its fused
    atom37 frame vs fdipt_backbone_atoms on the same x_{t-1}: bit-identical."""
    from framedipt_amd import _lib, residue_tables
    lib = _lib.load()
    d = _diffuser()
    B, N = 3, 301
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, N, 4, generator=g)
    t7 = torch.cat([q / q.norm(dim=-1, keepdim=True), 10 * torch.randn(B, N, 3, generator=g)], -1).float().cuda().contiguous()
    rs = (0.3 * torch.randn(B, N, 3, generator=g, dtype=torch.float64)).cuda()
    ts = (0.1 * torch.randn(B, N, 3, generator=g)).cuda()
    dm = (torch.rand(B, N, generator=g) > 0.2).float().cuda()
    zr, zt = torch.randn(B, N, 3, generator=g, dtype=torch.float64).cuda(), torch.randn(B, N, 3, generator=g, dtype=torch.float64).cuda()
    psi = torch.nn.functional.normalize(torch.randn(B, N, 2, generator=g), dim=-1).cuda().contiguous()
    aat = torch.randint(0, 21, (B, N), generator=g).int().cuda()
    tb = dev(residue_tables.packed_bytes())
    rot_a = torch.empty(B, N, 3, 3, device="cuda")
    a37 = torch.full((B, N, 37, 3), 7.0, device="cuda")
    out = d.reverse_device(t7, rs, ts, dm, zr, zt, 0.4, 0.01, True, 0.5, rot_out=rot_a, atoms=(psi, aat, tb, a37))
    inpl = t7.clone()
    rot_b = torch.empty_like(rot_a)
    d.reverse_device(inpl, rs, ts, dm, zr, zt, 0.4, 0.01, True, 0.5, rigids_out=inpl, rot_out=rot_b)
    assert torch.equal(out, inpl) and torch.equal(rot_a, rot_b)
    ref37 = torch.empty_like(a37)
    _lib.check(lib.fdipt_backbone_atoms(B * N, None, _lib.ptr(rot_a), _lib.ptr(out[..., 4:].contiguous()), _lib.ptr(psi),
                                        _lib.ptr(aat), _lib.ptr(tb), _lib.ptr(ref37), None, _lib.stream_ptr()))
    assert torch.equal(a37, ref37)
    with pytest.raises(_lib.FdiptError):  # the fused atoms need the out-of-place form
        d.reverse_device(inpl, rs, ts, dm, zr, zt, 0.4, 0.01, True, 0.5, rigids_out=inpl, atoms=(psi, aat, tb, a37))


@pytest.mark.parametrize("N", [5, 20, 300])
def test_rot_score_batched_vs_per_sample(N):
    """IGSO(3) score of a batch whose samples sit at different noise levels (series cut, weight table per sample; blocks
    spanning two samples at N=20, per-lane weights at N=5) vs one call per sample."""
    from framedipt_amd import _lib
    lib = _lib.load()
    B = 4
    g = torch.Generator().manual_seed(N)
    nq = lambda: torch.nn.functional.normalize(torch.randn(B, N, 4, generator=g), dim=-1).cuda().contiguous()  # noqa: E731
    qt, q0 = nq(), nq()
    sig = torch.tensor([0.1, 1.5, 0.37, 0.9], dtype=torch.float64).cuda()
    full = torch.empty(B, N, 3, dtype=torch.float64, device="cuda")
    _lib.check(lib.fdipt_igso3_rot_score(B, N, _lib.ptr(qt), _lib.ptr(q0), _lib.ptr(sig), None, _lib.ptr(full), _lib.stream_ptr()))
    for b in range(B):
        one = torch.empty(1, N, 3, dtype=torch.float64, device="cuda")
        _lib.check(lib.fdipt_igso3_rot_score(1, N, _lib.ptr(qt[b].contiguous()), _lib.ptr(q0[b].contiguous()),
                                             _lib.ptr(sig[b:b + 1].contiguous()), None, _lib.ptr(one), _lib.stream_ptr()))
        assert torch.equal(one[0], full[b]), b
    assert torch.isfinite(full).all()


def test_ca_hand_over_of_the_forward():
    """The forward's own hand-over of the predicted CA positions (self-conditioning input of the next step)."""
    from framedipt_amd import inference as inf
    G = load_golden("fwd_full_denovo_n64.npz")
    net, d, conf = _net("full_denovo_n64", G, "fp16")
    loop = inf.ReverseLoop(net, d, _feats(G), num_t=10, min_t=0.01, noise_scale=0.1)
    before = loop.sc_ca.clone()
    loop.prime()
    assert torch.equal(loop.sc_ca, loop.st.rigids[..., 4:]) and not torch.equal(loop.sc_ca, before)
