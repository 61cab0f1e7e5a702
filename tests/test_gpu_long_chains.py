"""Key-streaming attention kernels (FDIPT_KF_STREAM_ATTN): the fp16 forward with the flag at N <= 1024 against the reference goldens,
above 1024 against the oracle, at 64-bit pair indices, padded, replayed as a graph, and its limits."""
import os

import numpy as np
import pytest
import torch

import test_gpu_parity
from conftest import kabsch_free_rmsd, load_golden
from test_gpu_parity import _feats, _net
from test_gpu_sizes import FP16_BOUND, _psi_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream_net(precision="fp16", seed=5):
    from framedipt_amd import _lib, config
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    conf = config.base_config()
    d = SE3Diffuser(conf.diffuser, device="cuda")
    net = ScoreNetwork(conf.model, d, precision=precision, kernel_flags=_lib.KF_STREAM_ATTN).load_synthetic(seed).to("cuda")
    return net, d, conf


def _denovo_feats(d, n, seed=0):
    from framedipt_amd import config
    from framedipt_amd.sampler import UnconditionalSampler
    ds = UnconditionalSampler(config.to_conf({"min_length": n, "max_length": n, "length_step": 1, "samples_per_length": 1}), d, "cuda")
    np.random.seed(seed)
    feats = dict(ds[0][2])
    feats["t"] = torch.full((1,), 0.6, device="cuda")
    return feats


@pytest.mark.parametrize("name", ["full_denovo_n64", "full_denovo_n300_t50", "full_inpaint_n724_4chain", "full_inpaint_n1000"])
def test_flag_within_the_fp16_bound_of_the_reference(name):
    """The flagged fp16 forward meets FP16_BOUND (test_gpu_sizes.py) against the reference goldens, and it is not the default path's
    result (the streaming kernels ran)."""
    from framedipt_amd import _lib
    G = load_golden(f"fwd_{name}.npz")
    net, d, conf = _net(name, G, "fp16", kernel_flags=_lib.KF_STREAM_ATTN)
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
    print(f"stream fp16 {name}: node rel {max(nrel):.2e} edge rel {max(erel):.2e} CA max {ca:.2e} A psi rms {np.sqrt((pe**2).mean()):.2e} "
          f"backbone rmsd {rm:.2e} A")
    assert max(nrel) < FP16_BOUND["node_rel"] and max(erel) < FP16_BOUND["edge_rel"]
    assert ca < FP16_BOUND["ca"] and np.sqrt((pe**2).mean()) < FP16_BOUND["psi_rms"] and rm < FP16_BOUND["bb_rmsd"]
    ref, _, _ = _net(name, G, "fp16")
    tn0 = ref(_feats(G), trace=True)["trace_node"].cpu().numpy()
    assert not np.array_equal(tn, tn0)


def test_flag_teacher_forced_n300(monkeypatch):
    """Teacher-forced bb_gain 0.3 trajectory with the flag: every step's x_{t-1} within 1e-3 A of the reference's."""
    from framedipt_amd import _lib
    net_of = test_gpu_parity._net
    monkeypatch.setattr(test_gpu_parity, "_net", lambda name, G, prec: net_of(name, G, prec, kernel_flags=_lib.KF_STREAM_ATTN))
    worst, _ = test_gpu_parity._teacher_forced_worst_rmsd("full_denovo_n300_T5_gain03", "fp16")
    assert worst < 1e-3, worst


def _vs_torch_port(net, conf, inp, sd, feats):
    """The flagged fp16 forward of `feats` (torch, cuda) against oracle.torch_port.TorchScoreNetwork (fp32, CPU) on the same weights:
    max CA error, psi rms over the diffused residues, backbone RMSD over the real residues."""
    from oracle import diffuser as od
    from oracle.torch_port import TorchScoreNetwork
    out = {k: v.cpu().numpy() for k, v in net(feats).items()}
    tables = dict(np.load(os.path.join(ROOT, "framedipt_amd", "data", "residue_tables.npz")))
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        onet = TorchScoreNetwork(conf.model, od.SE3Diffuser(conf.diffuser), sd, inpainting=inp, tables=tables)
        ref = onet({k: v.cpu().numpy() for k, v in feats.items()})
    finally:
        torch.set_num_threads(threads)
    real = feats["res_mask"].cpu().numpy() > 0
    diffused = real & (feats["fixed_mask"].cpu().numpy() == 0)
    ca = np.abs(out["rigids"][..., 4:] - ref["rigids"][..., 4:])[real].max()
    pe = _psi_err(out["psi"], ref["psi"])[diffused]
    rm = kabsch_free_rmsd(out["atom37"][:, real[0]], ref["atom37"][:, real[0]])
    return ca, float(np.sqrt((pe ** 2).mean())), rm


def _inpaint_feats_4chain(n=1100, gap=200):
    """A 4-chain inpainting sample of n residues from the N = 1000 golden's inputs: its rows, then its first n - 1000 rows again 60 A
    further along x; chains of n / 4 residues with seq_idx gaps of `gap` (relative offsets up to n + 3 gap)."""
    G = load_golden("fwd_full_inpaint_n1000.npz")
    idx = np.concatenate([np.arange(1000), np.arange(n - 1000)])
    f = {k[3:]: G[k][:, idx] for k in G if k.startswith("in_") and k != "in_t"}
    for k in ("rigids_t", "sc_ca_t"):
        x = f[k].copy()
        x[:, 1000:, -3] += 60.0
        f[k] = x
    chain = np.repeat(np.arange(4), n // 4)[None]
    f["chain_idx"] = chain.astype(G["in_chain_idx"].dtype)
    f["seq_idx"] = (np.arange(n)[None] + gap * chain).astype(G["in_seq_idx"].dtype)
    f["t"] = G["in_t"]
    return G, f


@pytest.mark.parametrize("case", ["denovo_n1100_masked", "inpaint_n1100_4chain", "denovo_n1301"])
def test_flag_above_1024_matches_the_oracle(case):
    """Above 1024 the flagged fp16 forward against the torch-CPU port of the oracle (fp32) on the same synthetic weights, within
    FP16_BOUND's frame, psi and backbone bounds: a de novo sample with its last 40 residues masked; a 4-chain inpainting sample
    (fixed residues, seq_idx gaps of 200); N = 1301 (N % 4 != 0: edge_transition3, the sequence attention without the fused in_proj,
    o_pair as five passes of opair_mfma_kernel over z)."""
    from framedipt_amd import weights as W
    if case.startswith("inpaint"):
        G, fnp = _inpaint_feats_4chain()
        net, d, conf = _net("full_inpaint_n1000", G, "fp16", kernel_flags=1024)
        sd = W.synth_state_dict(W.param_shapes(conf.model, True), int(G["weight_seed"]), float(G["bb_gain"]))
        feats, inp = {k: test_gpu_parity.dev(v) for k, v in fnp.items()}, True
    else:
        n = 1301 if case.endswith("1301") else 1100
        net, d, conf = _stream_net()
        sd = W.synth_state_dict(W.param_shapes(conf.model), 5)
        feats, inp = _denovo_feats(d, n, seed=3), False
        if "masked" in case:
            feats["res_mask"][:, n - 40:] = 0
    ca, psi, rm = _vs_torch_port(net, conf, inp, sd, feats)
    print(f"stream fp16 {case} vs oracle: CA max {ca:.2e} A psi rms {psi:.2e} backbone rmsd {rm:.2e} A")
    assert ca < FP16_BOUND["ca"] and psi < FP16_BOUND["psi_rms"] and rm < FP16_BOUND["bb_rmsd"]


def test_per_module_entries_with_the_flag_n1100():
    """fdipt_edge_embed_fwd / fdipt_ipa_project_points / fdipt_ipa_attention_fwd / fdipt_edge_transition_fwd with the flag at N = 1100
    against the NumPy oracle's sub-modules, at the fp16 tolerance of test_per_module_entries_vs_oracle.  The per-op IPA takes the
    reference's formulation (per-head K / V images, the separate point launch) and o_pair as a pass over z."""
    import ctypes as C
    from framedipt_amd import _lib, embedding
    from framedipt_amd import weights as W
    from oracle import diffuser as od
    from oracle import frames as fr
    from oracle.score_network import ScoreNetwork as OracleNet
    tol = 4e-3
    lib = _lib.load()
    net, d, conf = _stream_net()
    N = 1100
    feats = _denovo_feats(d, N, seed=4)
    feats["res_mask"][:, N - 40:] = 0
    f = {k: v.cpu().numpy() for k, v in feats.items()}
    onet = OracleNet(conf.model, od.SE3Diffuser(conf.diffuser), W.synth_state_dict(W.param_shapes(conf.model), 5), inpainting=False, tables=None)
    B = 1
    mask = f["res_mask"].astype(np.float32)
    t = np.asarray(f["t"], dtype=np.float32)
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
    dev = test_gpu_parity.dev
    st = net.batch_state(dev(f["seq_idx"]))
    f32 = dict(dtype=torch.float32, device="cuda")
    a = _lib.ForwardArgs()
    a.B, a.N, a.n_rel, a.rel_off = B, N, st.n_rel, st.rel_off
    keep = [dev(mask), dev(f["fixed_mask"].astype(np.float32)), dev(f["sc_ca_t"].astype(np.float32)),
            torch.as_tensor(embedding.get_timestep_embedding(t, 32), device="cuda")]
    for nm, tn in (("res_mask", keep[0]), ("fixed_mask", keep[1]), ("sc_ca_t", keep[2]), ("seq_idx", st.seq_idx), ("idx_emb", st.idx_emb),
                   ("t_emb", keep[3]), ("t_emb_eps", st.t_emb_eps)):
        setattr(a, nm, _lib.ptr(tn))
    node_out, z_out = torch.empty(B, N, 256, **f32), torch.empty(B, N, N, 128, dtype=torch.float16, device="cuda")
    ws, wsb, sp = _lib.ptr(st.ws), st.ws_bytes, _lib.stream_ptr()
    dm, pr, dr = C.byref(net.dims), _lib.ptr(net.params), _lib.ptr(net.derived)
    _lib.check(lib.fdipt_edge_embed_fwd(dm, pr, dr, _lib.ptr(st.setup), C.byref(a), _lib.ptr(node_out), _lib.ptr(z_out), ws, wsb, sp))
    rel = lambda x, r: float(np.abs(x - r).max() / np.abs(r).max())  # noqa: E731
    r = mask[0] > 0  # (the library's embedder zeroes the masked rows and pairs; the oracle's Embedder takes no mask)
    assert rel(node_out.cpu().numpy()[:, r], node0[:, r]) < tol / 4, "node embedder"
    assert rel(z_out.float().cpu().numpy()[:, r][:, :, r], edge0[:, r][:, :, r]) < tol, "edge embedder"
    node_in, z_in, rig_d = dev(s_in), dev(edge0).half().contiguous(), dev(rig)
    del z_out
    qp, kp, vp = torch.empty(B, N, H, Pq, 3, **f32), torch.empty(B, N, H, Pq, 3, **f32), torch.empty(B, N, H, Pv, 3, **f32)
    _lib.check(lib.fdipt_ipa_project_points(dm, pr, dr, blk, B, N, _lib.ptr(node_in), _lib.ptr(rig_d), keep[0].data_ptr(), _lib.ptr(qp),
                                            _lib.ptr(kp), _lib.ptr(vp), ws, wsb, sp))
    assert rel(qp.cpu().numpy(), qp_ref) < tol and rel(kp.cpu().numpy(), kvp[..., :Pq, :]) < tol and rel(vp.cpu().numpy(), kvp[..., Pq:, :]) < tol
    out = torch.empty(B, N, 256, **f32)
    _lib.check(lib.fdipt_ipa_attention_fwd(dm, pr, dr, blk, B, N, _lib.ptr(node_in), _lib.ptr(z_in), _lib.ptr(rig_d), keep[0].data_ptr(),
                                           _lib.ptr(out), ws, wsb, sp))
    ipa_rel = rel(out.cpu().numpy()[:, r], ipa_ref[:, r])  # (the entry applies the node mask the trunk applies after the IPA)
    print(f"stream per-op N={N}: ipa rel {ipa_rel:.2e}")
    assert ipa_rel < tol, ("ipa", ipa_rel)
    z2 = torch.empty_like(z_in)
    _lib.check(lib.fdipt_edge_transition_fwd(dm, pr, dr, blk, B, N, _lib.ptr(node_in), keep[0].data_ptr(), _lib.ptr(z_in), _lib.ptr(z2), ws, wsb, sp))
    et_rel = rel(z2.float().cpu().numpy()[:, r][:, :, r], et_ref[:, r][:, :, r])
    print(f"stream per-op N={N}: edge transition rel {et_rel:.2e}")
    assert et_rel < tol, ("et", et_rel)


def test_flag_below_16_keys_writes_fp32_weights():
    """N = 12 with the flag: o_pair reads fp32 attention weights there (no half-precision rows below 16 keys), so the streaming IPA kernel
    takes its fp32-weight branch.  The result agrees with the default kernels' to round-off."""
    from framedipt_amd import config
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    net, d, conf = _stream_net()
    ref = ScoreNetwork(conf.model, SE3Diffuser(conf.diffuser, device="cuda"), precision="fp16").load_synthetic(5).to("cuda")
    feats = _denovo_feats(d, 12, seed=2)
    a, b = net(feats), ref(feats)
    for k in ("rigids", "psi", "atom37"):
        assert torch.isfinite(a[k]).all(), k
        np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), rtol=1e-4, atol=5e-4, err_msg=k)


def test_64bit_pair_indices_n2048_b5():
    """N = 2048, B = 5 different samples: B N^2 128 > 2^31 pair elements.  Every output is finite, and samples 0 and 4 are
    bit-identical to their own B = 1 runs."""
    net, d, _ = _stream_net()
    n = 2048
    fs = [_denovo_feats(d, n, seed=s) for s in range(5)]
    both = {k: v.clone() for k, v in net({k: torch.cat([f[k] for f in fs], 0) for k in fs[0]}).items()}
    for k, v in both.items():
        if v.is_floating_point():
            assert torch.isfinite(v).all(), k
    for s in (0, 4):
        one = net(fs[s])
        for k in ("rigids", "psi", "rot_score", "trans_score", "atom37"):
            assert torch.equal(both[k][s], one[k][0]), (s, k, float((both[k][s] - one[k][0]).abs().max()))


def test_padded_1100_next_to_2048_is_bit_identical_to_its_own_run():
    """An 1100-residue sample padded to 2048 (sharding.stack_items_padded) beside a 2048-residue one, T = 4: its real residues are
    bit-identical to its unpadded run (the flag puts no kernel-class boundary inside (1024, 2048])."""
    from framedipt_amd import config, inference, sharding
    from framedipt_amd.sampler import UnconditionalSampler
    net, d, _ = _stream_net()
    T = 4
    ds = UnconditionalSampler(config.to_conf({"min_length": 1100, "max_length": 2048, "length_step": 948, "samples_per_length": 1}), d, "cuda")
    items = [sharding.seeded_item(ds, i, 5, d, T, 0.01) for i in range(2)]
    assert [int(it[2]["rigids_t"].shape[1]) for it in items] == [1100, 2048]
    feats, tape, lengths = sharding.stack_items_padded(items)
    both = inference.inference_fn(net, d, feats, num_t=T, min_t=0.01, aux_traj=True, noise_scale=0.1, noise_tape=tape)
    one = inference.inference_fn(net, d, items[0][2], num_t=T, min_t=0.01, aux_traj=True, noise_scale=0.1, noise_tape=items[0][3])
    for k in ("prot_traj", "rigid_0_traj"):
        np.testing.assert_array_equal(both[k][:, 0, :1100], one[k][:, 0], err_msg=k)


def test_graph_replay_n1500_is_bit_identical():
    from framedipt_amd import config, inference, sharding
    from framedipt_amd.sampler import UnconditionalSampler
    net, d, _ = _stream_net()
    T = 4
    ds = UnconditionalSampler(config.to_conf({"min_length": 1500, "max_length": 1500, "length_step": 1, "samples_per_length": 1}), d, "cuda")
    it = sharding.seeded_item(ds, 0, 7, d, T, 0.01)
    g = inference.inference_fn(net, d, it[2], num_t=T, min_t=0.01, aux_traj=True, noise_scale=0.1, noise_tape=it[3], graph=True)
    e = inference.inference_fn(net, d, it[2], num_t=T, min_t=0.01, aux_traj=True, noise_scale=0.1, noise_tape=it[3], graph=False)
    assert np.isfinite(g["prot_traj"]).all()
    for k in ("prot_traj", "rigid_0_traj"):
        np.testing.assert_array_equal(g[k], e[k], err_msg=k)


def test_limits_with_the_flag():
    """N = 2052 is refused with the flag; in the fp32 mode the flag has no effect and N = 1100 stays refused."""
    from framedipt_amd import _lib
    for prec, n in (("fp16", 2052), ("fp32", 1100)):
        net, d, _ = _stream_net(prec)
        with pytest.raises(_lib.FdiptError, match="FDIPT_ESIZE"):
            net(_denovo_feats(d, n))
        torch.cuda.empty_cache()
