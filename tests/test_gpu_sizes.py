"""GPU parity tests (-m gpu) at the benchmarked sizes: reference goldens at N = 128 / 300 / 724 (4 chains) / 1000, a masked
res_mask, a bb_gain = 0.3 trajectory (tests/golden/make_goldens_r2.py), for the fp32 mode and the fp16 throughput mode —
each with its stated bound — on the kernel instantiations those sizes select (three key tiles per wave, the persistent
EdgeTransition tile walk, patches straddling samples, the N > 512 attention path)."""
import numpy as np
import pytest
import torch

from conftest import kabsch_free_rmsd, load_golden
from test_gpu_parity import _feats, _net, _teacher_forced_steps, _teacher_forced_worst_rmsd, dev

pytestmark = pytest.mark.gpu

SIZES = ["full_denovo_n128", "full_denovo_n300_t50", "full_denovo_n300_t02", "full_denovo_n64_inner", "full_denovo_n64_masked",
         "full_inpaint_n724_4chain", "full_inpaint_n1000"]


def _psi_err(a, b):
    ang = lambda p: np.arctan2(p[..., 0], p[..., 1])  # noqa: E731
    return np.abs(np.angle(np.exp(1j * (ang(a) - ang(b)))))


def _conditioned(G, d, t):
    """Residues where the reference's float32 IGSO(3) series is conditioned (f > 1e-2): the rotation score is
    asserted there; elsewhere the reference's own value is float32 round-off over the 1e-4 regulariser."""
    from oracle import diffuser as od
    from oracle import frames as fr
    q0, qt = G["out_rigids"][..., :4].astype(np.float32), G["in_rigids_t"][..., :4].astype(np.float32)
    rv = fr.quat_to_rotvec(fr.quat_multiply(fr.invert_quat(q0), qt).astype(np.float32))
    sig = d._so3_diffuser.score_sigma(np.float32(t))[0]
    f = od.igso3_expansion_np(np.linalg.norm(rv, axis=-1).astype(np.float64), sig)
    return f > 1e-2


@pytest.mark.parametrize("name", SIZES)
def test_forward_fp32_at_size(name):
    """fp32 mode vs the reference: every node trace <= 2e-4, the stored pair rows <= 2e-4, frames / psi / atoms as at N = 64."""
    G = load_golden(f"fwd_{name}.npz")
    net, d, conf = _net(name, G, "fp32")
    out = net(_feats(G), trace=True)
    rows = list(G["trace_rows"])
    tn, te = out["trace_node"].cpu().numpy(), out["trace_edge"].cpu().numpy()
    m = G["in_res_mask"][..., None]
    np.testing.assert_allclose(tn[0], G["tr_node_init"] * m, atol=1e-4)
    em = (G["in_res_mask"][:, rows, None] * G["in_res_mask"][:, None, :])[..., None]
    np.testing.assert_allclose(te[0][:, rows], G["tr_edge_init"] * em, atol=1e-4)
    for b in range(4):
        np.testing.assert_allclose(tn[b + 1], G[f"tr_node_{b}"] * m, atol=2e-4, err_msg=f"node {b}")
        if b < 3:
            np.testing.assert_allclose(te[b + 1][:, rows], G[f"tr_edge_{b}"] * em, atol=2e-4, err_msg=f"edge {b}")
    o = {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("trace")}
    np.testing.assert_allclose(o["rigids"][..., 4:], G["out_rigids"][..., 4:], atol=3e-4)
    np.testing.assert_allclose(np.abs(o["rigids"][..., :4]), np.abs(G["out_rigids"][..., :4]), atol=1e-5)
    assert _psi_err(o["psi"], G["out_psi"]).max() < 3e-4
    assert kabsch_free_rmsd(o["atom37"], G["out_atom37"]) < 1e-4
    np.testing.assert_allclose(o["atom14"], G["out_atom14"], atol=1e-3)
    ts = max(np.abs(G["out_trans_score"]).max(), 1.0)
    np.testing.assert_allclose(o["trans_score"], G["out_trans_score"], atol=3e-4 * ts)
    ok = _conditioned(G, d, float(G["in_t"][0])) & (G["in_res_mask"] > 0)
    err, mag = np.abs(o["rot_score"] - G["out_rot_score"]).max(-1), np.abs(G["out_rot_score"]).max(-1)
    print(f"{name}: rot score asserted on {ok.mean():.0%} of the residues (conditioned series)")
    assert (err[ok] <= 3e-3 * mag[ok] + 1e-5).all()
    if name != "full_denovo_n300_t02":  # t = 0.02: sigma = 0.13 rad, no residue of this fixture sits within ~5 sigma of its prediction
        assert ok.mean() > 0.5


# fp16 throughput mode (fp16 MFMA operands / pair representation, split operands on the node path): stated bounds per forward
FP16_BOUND = dict(node_rel=3e-4, edge_rel=1.2e-3, ca=5e-4, psi_rms=5e-4, bb_rmsd=3e-4)


@pytest.mark.parametrize("name", SIZES)
def test_forward_fp16_at_size(name):
    G = load_golden(f"fwd_{name}.npz")
    net, d, conf = _net(name, G, "fp16")
    out = net(_feats(G), trace=True)
    rows = list(G["trace_rows"])
    tn, te = out["trace_node"].cpu().numpy(), out["trace_edge"].cpu().numpy()
    m = G["in_res_mask"][..., None]
    em = (G["in_res_mask"][:, rows, None] * G["in_res_mask"][:, None, :])[..., None]
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))  # noqa: E731
    nrel = [rel(tn[b + 1], G[f"tr_node_{b}"] * m) for b in range(4)]
    erel = [rel(te[0][:, rows], G["tr_edge_init"] * em)] + [rel(te[b + 1][:, rows], G[f"tr_edge_{b}"] * em) for b in range(3)]
    o = {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("trace")}
    diffused = (1 - G["in_fixed_mask"]) * G["in_res_mask"] > 0
    ca = np.abs(o["rigids"][..., 4:] - G["out_rigids"][..., 4:]).max()
    pe = _psi_err(o["psi"], G["out_psi"])[diffused]
    rm = kabsch_free_rmsd(o["atom37"], G["out_atom37"])
    print(f"fp16 {name}: node rel {max(nrel):.2e} edge rel {max(erel):.2e} CA max {ca:.2e} A psi rms {np.sqrt((pe**2).mean()):.2e} "
          f"max {pe.max():.2e} rad backbone rmsd {rm:.2e} A")
    assert max(nrel) < FP16_BOUND["node_rel"] and max(erel) < FP16_BOUND["edge_rel"]
    assert ca < FP16_BOUND["ca"] and np.sqrt((pe**2).mean()) < FP16_BOUND["psi_rms"] and rm < FP16_BOUND["bb_rmsd"]


def test_inner_traces_unfused_node_path():
    """Per-block IPA output, post-IPA LayerNorm, sequence-transformer output and BackboneUpdate of the reference
    (tr_ipa / tr_ipa_ln / tr_tfmr / tr_bbupd) vs the forward's inner traces (fp32 mode: every tensor exists in memory)."""
    G = load_golden("fwd_full_denovo_n64_inner.npz")
    net, d, conf = _net("full_denovo_n64_inner", G, "fp32")
    out = net(_feats(G), trace=True, trace_inner=True)
    ti = out["trace_inner"].cpu().numpy()  # [blocks, 4, B, N, 320]
    for b in range(4):
        np.testing.assert_allclose(ti[b, 0, ..., :256], G[f"tr_ipa_{b}"], atol=2e-4, err_msg=f"ipa {b}")
        np.testing.assert_allclose(ti[b, 1, ..., :256], G[f"tr_ipa_ln_{b}"], atol=2e-4, err_msg=f"ipa_ln {b}")
        np.testing.assert_allclose(ti[b, 2], G[f"tr_tfmr_{b}"], atol=2e-4, err_msg=f"tfmr {b}")
        np.testing.assert_allclose(ti[b, 3, ..., :6], G[f"tr_bbupd_{b}"], atol=2e-5, err_msg=f"bb_update {b}")


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_batch_of_equal_samples_matches_single(prec):
    """B > 1: the same sample twice in a batch gives the B = 1 result (bit-identical: every per-pair / per-row computation
    is independent of its position in the batch)."""
    G = load_golden("fwd_full_denovo_n128.npz")
    net, d, conf = _net("full_denovo_n128", G, prec)
    f1 = _feats(G)
    one = {k: v.clone() for k, v in net(f1).items()}
    f2 = {k: torch.cat([v, v], 0) for k, v in f1.items()}
    two = net(f2)
    for k in ("rigids", "psi", "rot_score", "trans_score", "atom37"):
        for s in range(2):
            assert torch.equal(two[k][s], one[k][0]), (k, s, float((two[k][s] - one[k][0]).abs().max()))


def test_teacher_forced_fp32_n300():
    worst, _ = _teacher_forced_worst_rmsd("full_denovo_n300_T5", "fp32")
    assert worst < 1e-3, worst


@pytest.mark.parametrize("name", ["small_denovo_n16_T10", "small_inpaint_n24_T10", "full_denovo_n64_T20", "full_denovo_n300_T5"])
def test_teacher_forced_fp16_meets_the_north_star_bound(name):
    """fp16 throughput mode, per-step parity: reference state in -> one HIP step -> backbone RMSD of x_{t-1}
    against the reference's < 1e-3 A at every step (the mode bench.py times)."""
    worst, worst_noisy = _teacher_forced_worst_rmsd(name, "fp16")
    print(f"fp16 teacher-forced per-step backbone RMSD {name}: worst step {worst:.3e} A (reverse steps {worst_noisy:.3e} A)")
    assert worst < 1e-3, worst


# bb_gain = 0.3: BackboneUpdate moves frames by ~3 A per block instead of ~0.3 A, so an error of the node representation moves the
# predicted frames ten times further.  It also takes the reference's own rotation score out of its conditioned regime at small t
# ("conditioning of the rotation score"): at t = 0.114 and 0.062 of the N = 64 trajectory the float32 IGSO(3) series of the
# reference is round-off over the 1e-4 regulariser for most residues, and the NumPy restatement of the very same dtype flow
# (oracle/, x_0 prediction equal to 7e-6 A) already lands 1.2e-3 / 6.4e-3 A away from the reference's x_{t-1}.  Per-step parity
# is therefore asserted on x_{t-1} where the series is conditioned (t > 0.15) and on the x_0 prediction at every step.
# Round 3: the fp16 mode holds the north-star bound here as well (round 2: 1.8e-3 / 1.9e-3 A) — every product whose operands are
# per-residue quantities (IPA input projection, EdgeTransition fold rows, o_pair down-projection, skip_embed: their rounding
# errors are coherent over all keys of a row) and the attention's P V run on split operands (tests/err_budget.py at bb_gain 0.3).
@pytest.mark.parametrize("prec,bound_next,bound_x0", [("fp32", 1e-4, 1e-4), ("fp16", 1e-3, 1e-3)])
def test_teacher_forced_large_frame_updates(prec, bound_next, bound_x0):
    r = _teacher_forced_steps("full_denovo_n64_T20_gain03", prec)
    cond = (r[:, 0] > 0.15) | (r[:, 0] < 0.011)
    print(f"{prec} bb_gain 0.3: x_(t-1) worst {r[cond, 1].max():.3e} A on conditioned steps ({r[~cond, 1].max():.3e} A on the two "
          f"unconditioned ones), x_0 prediction worst {r[:, 2].max():.3e} A")
    assert r[cond, 1].max() < bound_next and r[:, 2].max() < bound_x0


@pytest.mark.parametrize("prec,bound", [("fp32", 1e-4), ("fp16", 1e-3)])
def test_teacher_forced_large_frame_updates_n300(prec, bound):
    """The benchmarked size with BackboneUpdate weights at trained-weight scale (tests/golden/make_goldens_r3.py): N = 300, T = 5
    (t = 1, 0.7525, 0.505, 0.2575, 0.01: every reverse step is in the conditioned regime of the rotation score)."""
    r = _teacher_forced_steps("full_denovo_n300_T5_gain03", prec)
    fmt = lambda v: " ".join(f"{x:.2e}" for x in v)  # noqa: E731
    print(f"{prec} bb_gain 0.3 N=300: x_(t-1) per step [{fmt(r[:, 1])}] A, x_0 prediction [{fmt(r[:, 2])}] A")
    assert r[:, 1].max() < bound and r[:, 2].max() < bound


def test_sampler_dict_matches_reference_sampler():
    """UnconditionalSampler items vs dicts captured from the reference sampler (keys, dtypes, shapes, values; fixed seed)."""
    from framedipt_amd import config
    from framedipt_amd import rigid as R
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.sampler import UnconditionalSampler
    S = load_golden("sampler_dicts.npz")
    conf = config.base_config()
    d = SE3Diffuser(conf.diffuser, device="cuda")  # reseeds np.random as the reference constructor does
    ds = UnconditionalSampler(config.to_conf({"min_length": 20, "max_length": 24, "length_step": 4, "samples_per_length": 2}), d, "cuda")
    assert len(ds) == int(S["uncond_len"][0])
    for i in (0, 3):  # (the capture drew items 0 and 3, in this order, from the global stream)
        length, sample_i, feats = ds[i]
        assert [int(length), int(sample_i)] == list(S[f"uncond_{i}_meta"])
        keys = sorted(k[len(f"uncond_{i}_"):] for k in S if k.startswith(f"uncond_{i}_") and not k.endswith("_dtype") and not k.endswith("_meta"))
        assert sorted(feats) == keys
        for k in keys:
            ref = S[f"uncond_{i}_{k}"]
            assert str(feats[k].dtype) == str(S[f"uncond_{i}_{k}_dtype"]), k
            assert tuple(feats[k].shape) == ref.shape, k
            if k == "rigids_t":
                np.testing.assert_allclose(R.quat_to_rot(feats[k][0, :, :4]).cpu().numpy(),
                                           R.quat_to_rot(dev(ref[0, :, :4])).cpu().numpy(), atol=3e-6)
                np.testing.assert_allclose(feats[k][..., 4:].cpu().numpy(), ref[..., 4:], atol=1e-6)
            else:
                np.testing.assert_array_equal(feats[k].cpu().numpy(), ref)


@pytest.mark.parametrize("name", ["traj_small_inpaint_n24_T10.npz", "traj_full_denovo_n64_T20.npz"])
def test_reverse_api_with_rigid_objects(name):
    """SE3Diffuser.reverse(Rigid, rot_score, trans_score, ...) (se3_diffuser.py:346-401), the documented drop-in surface:
    NumPy scores in, Rigid out, noise drawn from the global np.random stream in the reference's order."""
    from framedipt_amd import config
    from framedipt_amd import rigid as R
    from framedipt_amd.diffusion import SE3Diffuser
    T = load_golden(name)
    d = SE3Diffuser(config.base_config().diffuser)
    dm = ((1 - T["in_fixed_mask"]) * T["in_res_mask"])
    dt = 1.0 / int(T["num_t"])
    orig = np.random.normal
    for s in (0, len(T["step_t"]) // 2, len(T["step_t"]) - 1):
        tape = [T["noise_tape"][2 * s], T["noise_tape"][2 * s + 1]]
        np.random.normal = lambda size=None, _t=tape: _t.pop(0).reshape(size)  # the reference's draws, in its order
        try:
            out = d.reverse(R.Rigid.from_tensor_7(dev(T["step_rigids_t"][s])), T["step_rot_score"][s], T["step_trans_score"][s],
                            float(T["step_t"][s]), dt, diffuse_mask=dm, center=True, noise_scale=float(T["noise_scale"]))
        finally:
            np.random.normal = orig
        assert not tape
        assert isinstance(out, R.Rigid)
        np.testing.assert_allclose(out.get_rots().get_rot_mats().cpu().numpy(), T["step_out_rot"][s], atol=1e-6)
        np.testing.assert_allclose(out.get_trans().cpu().numpy(), T["step_out_trans"][s], atol=3e-5)


def test_round2_frame_ops_vs_reference_goldens():
    """geomstats-fork SO(3) exp / log / omega (framedipt/diffusion/so3_utils.py:90-231), Rigid.from_3_points / from_tensor_4x4
    (rigid_utils.py:1233-1275,1180-1198), calc_trans_score(scale=False) (r3_diffuser.py:410-440)."""
    from framedipt_amd import _lib, config
    from framedipt_amd import rigid as R
    from framedipt_amd.diffusion import SE3Diffuser
    lib = _lib.load()
    G = load_golden("ops_r2.npz")
    n = G["gs_rotvec"].shape[0]
    rv = dev(G["gs_rotvec"])
    rot = torch.empty(n, 3, 3, dtype=torch.float64, device="cuda")
    _lib.check(lib.fdipt_so3_exp_geomstats(n, _lib.ptr(rv), _lib.ptr(rot), _lib.stream_ptr()))
    np.testing.assert_allclose(rot.cpu().numpy(), G["gs_R64"], atol=1e-12)
    np.testing.assert_allclose(rot.cpu().numpy(), G["gs_exp"], atol=2e-6)  # the reference's own (float32) evaluation
    om = torch.empty(n, dtype=torch.float64, device="cuda")
    _lib.check(lib.fdipt_so3_omega(n, _lib.ptr(dev(G["gs_R64"])), 1e-4, _lib.ptr(om), _lib.stream_ptr()))
    np.testing.assert_allclose(om.cpu().numpy(), G["gs_omega"], atol=1e-12)
    lg = torch.empty(n, 3, dtype=torch.float64, device="cuda")
    _lib.check(lib.fdipt_so3_log_geomstats(n, _lib.ptr(dev(G["gs_log_in"].astype(np.float64))), _lib.ptr(lg), _lib.stream_ptr()))
    # float32 reference flow; near pi the log of a float32-rounded matrix is conditioned like sqrt(eps): looser there
    ang = np.linalg.norm(G["gs_rotvec"], axis=-1)
    near_pi = ang > np.pi - 3e-2  # (30 or more near-pi items: test_gpu_frames_edges.py::test_geomstats_maps_edges_vs_oracle)
    np.testing.assert_allclose(lg.cpu().numpy()[~near_pi], G["gs_log"][~near_pi], atol=2e-5)
    np.testing.assert_allclose(lg.cpu().numpy()[near_pi], G["gs_log"][near_pi], atol=2e-3)
    r = R.Rigid.from_3_points(dev(G["p3_a"]), dev(G["p3_o"]), dev(G["p3_c"]))
    np.testing.assert_allclose(r.get_rots().get_rot_mats().cpu().numpy(), G["p3_rot"], atol=1e-6)
    np.testing.assert_array_equal(r.get_trans().cpu().numpy(), G["p3_trans"])
    m44 = dev(G["t4x4"])
    np.testing.assert_allclose(r.to_tensor_4x4().cpu().numpy(), G["t4x4"], atol=1e-6)
    t7 = R.Rigid.from_tensor_4x4(m44).to_tensor_7().cpu().numpy()
    sgn = np.sign((t7[:, :4] * G["t4x4_t7"][:, :4]).sum(-1, keepdims=True))  # quaternion sign is free (rot_to_quat, eigh)
    np.testing.assert_allclose(t7[:, :4] * sgn, G["t4x4_t7"][:, :4], atol=2e-6)
    np.testing.assert_array_equal(t7[:, 4:], G["t4x4_t7"][:, 4:])
    cat = R.Rigid.cat([r[:10], r[10:]], dim=0)
    assert cat.shape == r.shape and torch.equal(cat.get_trans(), r.get_trans())
    assert r.unsqueeze(0).shape == (1, n) and torch.equal(r.scale_translation(0.1).get_trans(), r.get_trans() * 0.1)
    d = SE3Diffuser(config.base_config().diffuser)
    for i, t in enumerate([0.01, 0.5, 1.0]):
        ts = d.calc_trans_score(dev(G["ts_t1"]), dev(G["ts_t2"]), torch.tensor([t]), use_torch=True, scale=False).cpu().numpy()
        np.testing.assert_allclose(ts, G[f"ts_unscaled_{i}"], rtol=3e-6, atol=2e-6)


def test_conditional_sampler_items_on_device():
    """ConditionalSampler.from_features -> items with the reference's keys (sampler.py:267-354), motif frames kept, t = 1."""
    from framedipt_amd import config
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.sampler import ConditionalSampler
    import bench
    d = SE3Diffuser(config.base_config(inpainting=True).diffuser, device="cuda")
    f = bench.synthetic_complex((30, 40, 9, 21), ((5, 12), (40, 50)))
    ds = ConditionalSampler.from_features([("cplx", f)], d, "cuda", samples=2)
    assert len(ds) == 2
    name, si, it = ds[1]
    assert (name, si) == ("cplx", 1)
    for k in ("aatype", "seq_idx", "chain_idx", "res_mask", "fixed_mask", "rigids_0", "rigids_t", "sc_ca_t", "t", "torsion_angles_sin_cos"):
        assert k in it and it[k].shape[0] == 1, k
    fixed = it["fixed_mask"][0].bool().cpu().numpy()
    assert fixed.sum() == 100 - 17
    np.testing.assert_allclose(it["rigids_t"][0, fixed, 4:].cpu().numpy(), f["rigids_0"][fixed, 4:], atol=1e-5)
    assert float(it["t"][0]) == 1.0 and it["rigids_t"].dtype == torch.float32


@pytest.mark.parametrize("prec,tol", [("fp32", 3e-4), ("fp16", 4e-3)])
def test_per_module_entries_vs_oracle(prec, tol):
    """fdipt_edge_embed_fwd / fdipt_ipa_project_points / fdipt_ipa_attention_fwd / fdipt_edge_transition_fwd on the golden's
    inputs against the NumPy oracle's sub-modules (Embedder.forward, IPA point projections, InvariantPointAttention.forward,
    EdgeTransition.forward).  Tolerance relative to the largest magnitude of the output (fp16: operand rounding of one module)."""
    import ctypes as C
    from framedipt_amd import _lib, embedding
    from oracle import frames as fr
    from test_oracle_forward import _feats as ofeats, _model as omodel
    lib = _lib.load()
    name = "full_denovo_n64"
    G = load_golden(f"fwd_{name}.npz")
    net, d, conf = _net(name, G, prec)
    onet, _ = omodel(name, G, None)  # (no residue tables: the backbone builder is not called here)
    f = ofeats(G)
    B, N = f["seq_idx"].shape
    mask = f["res_mask"].astype(np.float32)
    t = np.asarray(f["t"], dtype=np.float32)
    # ---- oracle sub-modules
    node0, edge0 = onet.embed(f["seq_idx"], t, f["fixed_mask"].astype(np.float32), f["sc_ca_t"].astype(np.float32), None)
    rig = f["rigids_t"].astype(np.float32)
    quat, trans = rig[..., :4], (rig[..., 4:] * np.float32(0.1)).astype(np.float32)
    blk = 1
    s_in = node0 * np.float32(1.0)
    ipa_ref = onet.ipa(blk, s_in, edge0, quat, trans, mask)
    et_ref = onet.edge_transition(blk, s_in, edge0)
    rot = fr.quat_to_rot(quat).astype(np.float32)
    p = f"score_model.trunk.ipa_{blk}."
    H, Pq, Pv = 8, 8, 12

    def pts(pname, n_pts):
        x = onet._lin(p + pname, s_in)
        x = np.stack(np.split(x, 3, axis=-1), axis=-1)
        return fr.rigid_apply(rot[:, :, None], trans[:, :, None], x).astype(np.float32).reshape(B, N, H, n_pts, 3)

    qp_ref, kvp = pts("linear_q_points", Pq), pts("linear_kv_points", Pq + Pv)
    # ---- HIP per-module entries
    st = net.batch_state(dev(f["seq_idx"]))
    zt = torch.float32 if prec == "fp32" else torch.float16
    f32 = dict(dtype=torch.float32, device="cuda")
    a = _lib.ForwardArgs()
    a.B, a.N, a.n_rel, a.rel_off = B, N, st.n_rel, st.rel_off
    keep = [dev(mask), dev(f["fixed_mask"].astype(np.float32)), dev(f["sc_ca_t"].astype(np.float32)),
            torch.as_tensor(embedding.get_timestep_embedding(t, 32), device="cuda")]
    for nm, tn in (("res_mask", keep[0]), ("fixed_mask", keep[1]), ("sc_ca_t", keep[2]), ("seq_idx", st.seq_idx), ("idx_emb", st.idx_emb),
                   ("t_emb", keep[3]), ("t_emb_eps", st.t_emb_eps)):
        setattr(a, nm, _lib.ptr(tn))
    node_out, z_out = torch.empty(B, N, 256, **f32), torch.empty(B, N, N, 128, dtype=zt, device="cuda")
    ws, wsb, sp = _lib.ptr(st.ws), st.ws_bytes, _lib.stream_ptr()
    dm, pr, dr = C.byref(net.dims), _lib.ptr(net.params), _lib.ptr(net.derived)
    _lib.check(lib.fdipt_edge_embed_fwd(dm, pr, dr, _lib.ptr(st.setup), C.byref(a), _lib.ptr(node_out), _lib.ptr(z_out), ws, wsb, sp))
    rel = lambda x, r: float(np.abs(x - r).max() / np.abs(r).max())  # noqa: E731
    assert rel(node_out.cpu().numpy(), node0) < tol / 4, "node embedder"
    assert rel(z_out.float().cpu().numpy(), edge0) < tol, "edge embedder"
    node_in, z_in, rig_d = dev(s_in), dev(edge0).to(zt).contiguous(), dev(rig)
    qp, kp, vp = torch.empty(B, N, H, Pq, 3, **f32), torch.empty(B, N, H, Pq, 3, **f32), torch.empty(B, N, H, Pv, 3, **f32)
    _lib.check(lib.fdipt_ipa_project_points(dm, pr, dr, blk, B, N, _lib.ptr(node_in), _lib.ptr(rig_d), keep[0].data_ptr(), _lib.ptr(qp),
                                            _lib.ptr(kp), _lib.ptr(vp), ws, wsb, sp))
    assert rel(qp.cpu().numpy(), qp_ref) < tol and rel(kp.cpu().numpy(), kvp[..., :Pq, :]) < tol and rel(vp.cpu().numpy(), kvp[..., Pq:, :]) < tol
    out = torch.empty(B, N, 256, **f32)
    _lib.check(lib.fdipt_ipa_attention_fwd(dm, pr, dr, blk, B, N, _lib.ptr(node_in), _lib.ptr(z_in), _lib.ptr(rig_d), keep[0].data_ptr(),
                                           _lib.ptr(out), ws, wsb, sp))
    assert rel(out.cpu().numpy(), ipa_ref) < tol, ("ipa", rel(out.cpu().numpy(), ipa_ref))
    z2 = torch.empty_like(z_in)
    _lib.check(lib.fdipt_edge_transition_fwd(dm, pr, dr, blk, B, N, _lib.ptr(node_in), keep[0].data_ptr(), _lib.ptr(z_in), _lib.ptr(z2), ws, wsb, sp))
    assert rel(z2.float().cpu().numpy(), et_ref) < tol, ("et", rel(z2.float().cpu().numpy(), et_ref))
    assert lib.fdipt_edge_transition_fwd(dm, pr, dr, 3, B, N, _lib.ptr(node_in), keep[0].data_ptr(), _lib.ptr(z_in), _lib.ptr(z2), ws, wsb, sp) == -1


def test_sharded_run_is_world_size_independent(tmp_path):
    """framedipt_amd.run_sharded.run_rank with the real sampler: every sample's final structure is bit-identical whether it runs at
    world size 1 (batches of 3) or as one of two ranks' shards (other batch composition, other rank) - per-sample seeds + kernels
    whose per-sample results do not depend on the batch."""
    import json
    import os
    from framedipt_amd import config, inference, run_sharded
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import UnconditionalSampler
    conf = config.base_config()
    d = SE3Diffuser(conf.diffuser, device="cuda")
    net = ScoreNetwork(conf.model, d, precision="fp16").load_synthetic(7).to("cuda")
    ds = UnconditionalSampler(config.to_conf({"min_length": 44, "max_length": 48, "length_step": 4, "samples_per_length": 3}), d, "cuda")
    T = 4

    def run_batch(feats, tape):
        return inference.inference_fn(net, d, feats, num_t=T, min_t=0.01, aux_traj=True, noise_scale=0.1, noise_tape=tape)

    d1, d2 = str(tmp_path / "w1"), str(tmp_path / "w2")
    run_sharded.run_rank(ds, d, run_batch, 0, 1, d1, seed=9, num_t=T, min_t=0.01, max_batch=3)
    m1 = run_sharded.write_manifest(d1, 1, len(ds), {})
    for r in range(2):
        run_sharded.run_rank(ds, d, run_batch, r, 2, d2, seed=9, num_t=T, min_t=0.01, max_batch=2)
    m2 = run_sharded.write_manifest(d2, 2, len(ds), {})
    assert len(m1) == len(m2) == 6 and sorted({s["rank"] for s in m2}) == [0, 1]
    for s1, s2 in zip(m1, m2):
        a, b = np.load(os.path.join(d1, s1["file"])), np.load(os.path.join(d2, s2["file"]))
        assert a["prot_traj"].shape == (s1["n_res"], 37, 3)
        np.testing.assert_array_equal(a["prot_traj"], b["prot_traj"], err_msg=str(s1))
    assert json.load(open(os.path.join(d2, "manifest.json")))["world_size"] == 2
