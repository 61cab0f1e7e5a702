"""CPU tests (-m 'not gpu'): host logic, C-ABI surface, loud failure without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def test_library_exports_every_declared_symbol():
    from framedipt_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "fdipt.h")).read()
    declared = set(re.findall(r"\b(fdipt_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in lib.fdipt_version()


def test_kernel_class_bounds_match_the_library():
    """sharding.KERNEL_CLASS_BOUNDS (mixed-length batches never span two kernel-selection classes) is the list the library exports."""
    from framedipt_amd import _lib, sharding
    lib = _lib.load()
    buf = (C.c_int32 * 16)()
    n = lib.fdipt_kernel_class_bounds(buf, 16)
    assert tuple(buf[:n]) == sharding.KERNEL_CLASS_BOUNDS
    assert sharding.kernel_class(956) != sharding.kernel_class(964) and sharding.kernel_class(772) == sharding.kernel_class(960)


def test_shared_gpu_guard_reads_the_kfd_process_list(tmp_path):
    """gpu_guard on a fake /sys/class/kfd tree: gpu_id from the PCI address, owners of queues on that gpu_id."""
    from framedipt_amd import gpu_guard
    root = tmp_path / "kfd"
    for node, gid, loc in ((0, 0, 0), (1, 51234, (0x75 << 8) | (0 << 3)), (2, 7777, (0xf5 << 8))):
        d = root / "topology" / "nodes" / str(node)
        d.mkdir(parents=True)
        (d / "gpu_id").write_text(f"{gid}\n")
        (d / "properties").write_text(f"cpu_cores_count 0\nlocation_id {loc}\ndomain 0\n")
    assert gpu_guard.kfd_gpu_id(0, 0x75, 0, str(root)) == 51234 and gpu_guard.kfd_gpu_id(0, 0xf5, 0, str(root)) == 7777
    assert gpu_guard.kfd_gpu_id(0, 0x11, 0, str(root)) is None
    assert gpu_guard.processes_with_queues(51234, str(root)) is None  # (no proc directory: unknown)
    for pid, gids in ((100, (51234,)), (200, (7777, 7777)), (300, (51234, 7777)), (400, ())):
        for q, g in enumerate(gids):
            d = root / "proc" / str(pid) / "queues" / str(q)
            d.mkdir(parents=True)
            (d / "gpuid").write_text(f"{g}\n")
        (root / "proc" / str(pid)).mkdir(parents=True, exist_ok=True)
    assert sorted(gpu_guard.processes_with_queues(51234, str(root))) == ["100", "300"]
    assert sorted(gpu_guard.processes_with_queues(7777, str(root))) == ["200", "300"]


def test_inventory_matches_reference_state_dict():
    from framedipt_amd import _lib, config, weights
    from framedipt_amd.model.score_network import dims_from_conf
    lib = _lib.load()
    for name in ("fwd_small_denovo_n16.npz", "fwd_small_inpaint_n24.npz", "fwd_full_denovo_n64.npz",
                 "fwd_full_inpaint_n40.npz"):
        G = load_golden(name)
        inp = "inpaint" in name
        conf = config.small_config(inp) if "small" in name else config.base_config(inp)
        shapes = weights.param_shapes(conf.model, inp)
        assert list(shapes) == [str(s) for s in G["param_names"]]
        d = dims_from_conf(conf.model, conf.diffuser, inp, 0)
        n = lib.fdipt_param_count(C.byref(d))
        assert n == len(shapes)
        offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes.values()])])
        assert all(lib.fdipt_param_offset(C.byref(d), i) == offs[i] for i in range(n + 1))
    assert weights.n_params(weights.param_shapes(config.base_config().model)) == 17446190
    bad = dims_from_conf(conf.model, conf.diffuser, inp, 7)
    assert lib.fdipt_param_count(C.byref(bad)) == -1 and lib.fdipt_derived_bytes(C.byref(bad)) == 0


def test_host_embeddings_pinned():
    from framedipt_amd import embedding as E
    O = load_golden("ops.npz")
    np.testing.assert_array_equal(E._TIMESTEP_FREQS, O["timestep_freqs"])
    np.testing.assert_allclose(E.get_timestep_embedding(O["temb_t"], 32), O["temb"], atol=2e-6)
    np.testing.assert_allclose(E.get_index_embedding(O["iemb_i"], 32), O["iemb"], atol=2e-6)
    with pytest.raises(ValueError):
        E.get_timestep_embedding(np.zeros((2, 2)))


def test_host_diffuser_schedules_and_tables():
    from framedipt_amd import config
    from framedipt_amd.diffusion import SE3Diffuser
    G = load_golden("ops.npz")
    d = SE3Diffuser(config.base_config().diffuser)
    so3, r3 = d._so3_diffuser, d._r3_diffuser
    np.testing.assert_allclose([so3.sigma(t) for t in G["ts"]], G["so3_sigma"], rtol=1e-14)
    np.testing.assert_allclose([so3.diffusion_coef(t) for t in G["ts"]], G["so3_g"], rtol=1e-14)
    np.testing.assert_array_equal([so3.t_to_idx(t) for t in G["ts"]], G["so3_idx"])
    rs = np.array([d.score_scaling(t) for t in G["ts"]])
    np.testing.assert_allclose(rs[:, 0], G["so3_score_scaling"], rtol=1e-10)
    np.testing.assert_allclose(rs[:, 1], G["r3_score_scaling"], rtol=1e-14)
    np.testing.assert_allclose(so3._row(so3.t_to_idx(1.0))[1], G["cdf_t1"], rtol=1e-12)
    with pytest.raises(ValueError):
        so3.sigma(np.float64(1.5))


def test_noise_tape_order_matches_reference_stream():
    """Per step: SO(3) normal(B,N,3) then R^3 normal(B,N,3) from the global legacy stream (finding 10)."""
    from framedipt_amd import config, inference
    from framedipt_amd.diffusion import SE3Diffuser
    G = load_golden("traj_small_denovo_n16_T10.npz")
    d = SE3Diffuser(config.small_config().diffuser)
    np.random.seed(123)  # the fixture restarts the global stream right before x_T is drawn
    n = 16
    np.random.randn(n, 3); np.random.rand(n); np.random.normal(size=(n, 3))  # x_T draws of sample_ref
    zr, zt = inference.draw_noise_tape(d, 9, 1, n)
    tape = G["noise_tape"]
    np.testing.assert_array_equal(zr, tape[0::2])
    np.testing.assert_array_equal(zt, tape[1::2])


def test_product_fails_loudly_without_gpu():
    from framedipt_amd import _lib, config
    from framedipt_amd import rigid as R
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    d = SE3Diffuser(config.small_config().diffuser)
    with pytest.raises(_lib.FdiptError):
        d.sample_ref(8)
    with pytest.raises(_lib.FdiptError):
        R.quat_to_rot(torch.zeros(3, 4))
    net = ScoreNetwork(config.small_config().model, d).load_synthetic(1)
    with pytest.raises(_lib.FdiptError):
        net.to("cpu")
    with pytest.raises(KeyError):
        net.load_state_dict({})


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "framedipt_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp")):
                src = open(os.path.join(dp, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "/root/reference" not in src, f


def test_unconditional_sampler_lengths():
    from framedipt_amd import config
    from framedipt_amd.sampler import UnconditionalSampler
    cfg = config.to_conf({"min_length": 100, "max_length": 200, "length_step": 50, "samples_per_length": 3})
    s = UnconditionalSampler(cfg, diffuser=None, device="cpu")
    assert list(s.all_sampling_lengths) == [100] * 3 + [150] * 3 + [200] * 3 and len(s) == 9


def test_redaction_and_padding_ports_vs_reference_goldens():
    """create_redacted_regions / pad_feats (framedipt/data/utils.py:613-689,311-378) restated in framedipt_amd.sampler."""
    import torch
    from framedipt_amd import sampler
    G = load_golden("ops_r2.npz")
    for seed in (0, 1, 7):
        got = sampler.create_redacted_regions(G["red_chain_idx"], G["red_res_mask"], np.random.default_rng(seed), 5, 12)
        np.testing.assert_array_equal(got, G[f"red_{seed}"])
    np.testing.assert_array_equal(sampler.create_redacted_regions(G["red_chain_idx"], G["red_res_mask"], np.random.default_rng(0), None, None),
                                  G["red_none"])
    feats = {k[len("pad_in_"):]: torch.tensor(v) for k, v in G.items() if k.startswith("pad_in_")}
    out = sampler.pad_feats(feats, 9)
    for k, v in out.items():
        np.testing.assert_array_equal(v.numpy(), G["pad_out_" + k], err_msg=k)
        assert v.numpy().dtype == G["pad_out_" + k].dtype, k


def test_conditional_sampler_surface_without_gpu(tmp_path):
    """Reference constructor signatures (experiments/sampler.py:141,363); metadata.csv handling; the mask logic; loud failure
    where the mmCIF preparation step has not been run."""
    import inspect
    import pandas as pd
    from framedipt_amd import _lib, config, sampler
    for cls in (sampler.ConditionalSampler, sampler.TCRSampler):
        assert list(inspect.signature(cls.__init__).parameters)[1:] == ["data_conf", "diffuser", "device"]
    assert list(inspect.signature(sampler.UnconditionalSampler.__init__).parameters)[1:] == ["cfg", "diffuser", "device"]
    conf = config.to_conf({"download_dir": str(tmp_path), "data_path": str(tmp_path / "none.csv"), "samples": 3, "seed": 1,
                           "redaction": {"redact_min_len": 4, "redact_max_len": 6}, "cdr_loops": ["CDR3"]})
    with pytest.raises(_lib.FdiptError):
        sampler.ConditionalSampler(conf, None, "cpu")
    n = 30
    feats = {"aatype": np.zeros(n, dtype=np.int64), "seq_idx": np.arange(n), "chain_idx": np.repeat([0, 1], 15),
             "res_mask": np.ones(n), "rigids_0": np.tile(np.array([1, 0, 0, 0, 0, 0, 0], dtype=np.float32), (n, 1)),
             "torsion_angles_sin_cos": np.zeros((n, 7, 2))}
    (tmp_path / "processed").mkdir()
    np.savez(tmp_path / "processed" / "1abc.npz", **feats)
    pd.DataFrame([{"pdb_name": "1abc", "processed_path": str(tmp_path / "processed" / "1abc.npz"), "modeled_seq_len": n}]).to_csv(
        tmp_path / "processed" / "metadata.csv", index=False)
    ds = sampler.ConditionalSampler(conf, None, "cpu")
    assert len(ds) == 3
    m = ds.create_diffusion_mask(ds._chain_feats(0), 0)
    assert m.shape == (n,) and 8 <= m.sum() <= 12 and m[:15].sum() >= 4 and m[15:].sum() >= 4
    assert ds.create_diffusion_mask(None, 0) is m  # cached per example
    tcr = sampler.TCRSampler(conf, None, "cpu")
    with pytest.raises(_lib.FdiptError):  # no CDR mask in the features, no ANARCI here
        tcr.create_diffusion_mask(tcr._chain_feats(0), 0)


def test_score_sigma_float32_evaluation():
    """sigma(t) before the grid snap is evaluated in float32 (value-based casting of the reference's pinned numpy 1.22.4); the
    float64 evaluation of NumPy >= 2 lands in the neighbouring grid bin for a few steps of a num_t = 1000 schedule only."""
    from framedipt_amd import config
    from framedipt_amd.diffusion import so3_diffuser
    so3 = so3_diffuser.SO3Diffuser(config.base_config().diffuser.so3)
    for num_t, max_diff in ((10, 0), (20, 0), (50, 0), (100, 0), (200, 0), (500, 0), (1000, 5)):
        t32 = np.linspace(0.01, 1.0, num_t)[::-1].astype(np.float32)
        got = so3.score_sigma(t32)
        f64 = so3.discrete_sigma[so3.t_to_idx(t32.astype(np.float64))]
        ndiff = int((got != f64).sum())
        assert ndiff <= max_diff, (num_t, ndiff)
        assert np.all(np.abs(got - f64) <= 0.004 * f64)
    conf = config.base_config().diffuser.so3
    conf.use_cached_score = True
    cached = so3_diffuser.SO3Diffuser(conf)  # so3_diffuser.py:389-396: rows of the score-norm table, built on demand
    rows = cached.score_table_rows(np.array([1.0, 0.5], dtype=np.float32))
    assert rows.shape == (2, 1000) and rows.dtype == np.float64 and cached.omega_edges.shape == (999,)
    np.testing.assert_array_equal(rows[0], cached._row(cached.t_to_idx(1.0))[2])
    assert np.shape(so3.score_scaling(np.array([0.1, 0.5]))) == (2,)


def test_output_writers_byte_equal_reference_files(tmp_path):
    """framedipt_amd.output vs files written by the reference from the same arrays (tests/golden/writers.npz): PDB files
    (single model, trajectory, no_indexing, index suffix of a second call) and diffusion_info.csv, byte for byte."""
    from framedipt_amd import output
    G = load_golden("writers.npz")
    pos, aatype, ci, ri, dm = G["pos"], G["aatype"], G["chain_index"], G["residue_index"], G["diffuse_mask"]
    bfac = np.tile((dm * 100)[:, None], (1, 37))
    p1 = output.write_prot_to_pdb(pos[0], tmp_path / "sample_0", b_factors=bfac, aatype=aatype, residue_index=ri, chain_index=ci)
    p2 = output.write_prot_to_pdb(pos, tmp_path / "bb_traj_0", b_factors=bfac, aatype=aatype, residue_index=ri, chain_index=ci)
    p3 = output.write_prot_to_pdb(pos[1], tmp_path / "plain", no_indexing=True)
    p4 = output.write_prot_to_pdb(pos[0], tmp_path / "sample_0", b_factors=bfac)
    assert [p.name for p in (p1, p2, p3, p4)] == [str(x) for x in G["pdb_names"]]
    for p, k in zip((p1, p2, p3, p4), ("pdb_sample", "pdb_traj", "pdb_plain", "pdb_second")):
        assert p.read_bytes() == bytes(G[k]), k
    seq = output.aatype_to_seq(aatype)
    assert seq == str(G["info_seq"])
    output.save_diffusion_info(tmp_path, "1abc", seq, dm, ci)
    assert (tmp_path / "diffusion_info.csv").read_bytes() == bytes(G["info_csv"])
    ch, st, en = output.get_diffused_region_per_chain(dm, ci)
    assert (list(ch), list(st), list(en)) == (list(G["region_chains"]), list(G["region_starts"]), list(G["region_ends"]))
    paths = output.save_traj(pos, pos, dm, tmp_path, 7, aatype=aatype, residue_index=ri, chain_index=ci)
    assert paths["sample_path"].name == "sample_7_1.pdb" and paths["traj_path"].name == "bb_traj_7_1.pdb"
    assert paths["traj_path"].read_bytes() == bytes(G["pdb_traj"])
    with pytest.raises(ValueError):
        output.write_prot_to_pdb(pos[0, :, :5], tmp_path / "bad")
    # EigenFold columns (experiments/inference.py:357-372): same pandas round trip as the reference
    import pandas as pd
    output.save_confidence(tmp_path / "diffusion_info.csv", tmp_path, 2, -130.5, [-1.0, -2.5], int(dm.sum()))
    df = pd.read_csv(tmp_path / "diffusion_info.csv", sep="\t")
    assert df["log_p_sample_2"][0] == -130.5 and df["log_p_sample_2_per_residue"][0] == -130.5 / dm.sum()
    assert df["log_p_sample_2_per_residue_norm"][0] == -130.5 / (6 * dm.sum() - 1) and df["pdb_name"][0] == "1abc"
    assert list(pd.read_csv(tmp_path / "log_probs.csv")["log_probs"]) == [-1.0, -2.5]


_FAKE_OMEGACONF = '''
"""Minimal package with the pickle layout of omegaconf 2.x containers / nodes (test double: the real package is not installed)."""
class ContainerMetadata:
    def __init__(self): self.ref_type = None; self.object_type = dict; self.optional = True; self.key = None; self.flags = {}
class Metadata(ContainerMetadata): pass
class Node:
    def __getstate__(self):
        d = dict(self.__dict__); d.pop("_flags_cache", None); return d
    def __setstate__(self, d): self.__dict__.update(d); self.__dict__["_flags_cache"] = None
class AnyNode(Node):
    def __init__(self, v, parent=None): self.__dict__.update(_val=v, _metadata=Metadata(), _parent=parent, _flags_cache=None)
class DictConfig(Node):
    def __init__(self, content, parent=None):
        self.__dict__.update(_metadata=ContainerMetadata(), _parent=parent, _flags_cache=None, _content={})
        for k, v in content.items(): self._content[k] = wrap(v, self)
class ListConfig(Node):
    def __init__(self, content, parent=None):
        self.__dict__.update(_metadata=ContainerMetadata(), _parent=parent, _flags_cache=None, _content=[wrap(v, self) for v in content])
def wrap(v, parent):
    if isinstance(v, dict): return DictConfig(v, parent)
    if isinstance(v, list): return ListConfig(v, parent)
    return AnyNode(v, parent)
'''


def test_checkpoint_ingest_without_omegaconf(tmp_path):
    """framedipt_amd.checkpoint: a checkpoint in the reference's format (torch.save of {"model", "conf": DictConfig, ...},
    ``module.`` prefixes, ``${...}`` interpolations) written by a subprocess that has an omegaconf-shaped package, read here
    without one; then the configuration steps of Inference._load_ckpt."""
    import subprocess
    import sys
    from framedipt_amd import checkpoint, config
    from framedipt_amd import weights as W
    pkg = tmp_path / "fake" / "omegaconf"
    pkg.mkdir(parents=True)
    (pkg / "__init__.py").write_text(_FAKE_OMEGACONF)
    shapes = W.param_shapes(config.small_config().model)
    names = list(shapes)[:6]
    writer = f'''
import sys; sys.path.insert(0, {str(tmp_path / "fake")!r}); sys.path.insert(0, {ROOT!r})
import torch, omegaconf
from framedipt_amd import config, weights as W
shapes = W.param_shapes(config.small_config().model)
sd = W.synth_state_dict(shapes, 3)
conf = {{"model": {{"node_embed_size": 64, "edge_embed_size": 32, "input_aatype": False,
                  "embed": {{"index_embed_size": 32, "num_bins": 22, "min_bin": "1e-5", "max_bin": 20.0, "embed_self_conditioning": True}},
                  "ipa": {{"c_s": "${{model.node_embed_size}}", "c_z": "${{model.edge_embed_size}}", "c_hidden": 16, "c_skip": 16, "no_heads": 4,
                          "no_qk_points": 4, "no_v_points": 6, "seq_tfmr_num_heads": 2, "seq_tfmr_num_layers": 1, "num_blocks": 2,
                          "coordinate_scaling": "${{diffuser.r3.coordinate_scaling}}"}}}},
        "diffuser": {{"r3": {{"min_b": 0.1, "max_b": 20.0, "coordinate_scaling": 0.1}}, "so3": {{"num_omega": 1000}}}},
        "experiment": {{"tags": ["a", "b"], "nested": [{{"x": 1}}]}}}}
torch.save({{"model": {{"module." + k: torch.tensor(v) for k, v in sd.items()}}, "conf": omegaconf.DictConfig(conf), "optim": {{}},
            "epoch": 7, "step": 1234}}, {str(tmp_path / "ckpt.pth")!r})
'''
    subprocess.run([sys.executable, "-c", writer], check=True)
    assert "omegaconf" not in sys.modules or getattr(sys.modules["omegaconf"], "__file__", None) is None
    sd, conf, extra = checkpoint.load_checkpoint(tmp_path / "ckpt.pth")
    ref = W.synth_state_dict(shapes, 3)
    assert list(sd) == list(ref) and all(not k.startswith("module.") for k in sd)
    for k in names:
        np.testing.assert_array_equal(sd[k], ref[k])
    assert extra == {"epoch": 7, "step": 1234}
    assert conf["model"]["ipa"]["c_s"] == 64 and conf["model"]["ipa"]["coordinate_scaling"] == 0.1  # interpolations resolved
    assert conf["experiment"] == {"tags": ["a", "b"], "nested": [{"x": 1}]}
    cfg = checkpoint.apply_checkpoint_conf(config.base_config(), conf, seed=11)
    assert cfg.model.ipa.c_hidden == 16 and cfg.model.ipa.c_z == 32 and cfg.model.embed.min_bin == 1e-5
    assert cfg.diffuser.r3.seed == 11 and cfg.diffuser.so3.seed == 11 and cfg.diffuser.so3.num_sigma == 1000
    assert W.param_shapes(cfg.model) == shapes
    checkpoint.main([str(tmp_path / "ckpt.pth"), str(tmp_path / "out")])
    z = np.load(tmp_path / "out.npz")
    assert sorted(z.files) == sorted(ref) and (tmp_path / "out.yaml").exists()


@pytest.mark.parametrize("name", ["1fyt", "5ksa", "7t2d"])
def test_feature_builder_vs_reference_process_csv_row(name):
    """framedipt_amd.data.features.process_csv_row (row f2) vs the reference's on the complexes of the reference's own test data
    (tests/golden/features.npz): all chains, and one randomly extracted chain cut to 150 residues (same Generator stream)."""
    from framedipt_amd.data import features
    G = load_golden("features.npz")
    pre = f"{name}_in_"
    cf = {k[len(pre):]: (G[k].astype(np.float64) if G[k].dtype.kind == "f" else G[k]) for k in G if k.startswith(pre)}
    for tag, kw in (("all", {}), ("one", {"extract_single_chain": True, "rng": np.random.default_rng(11), "chain_max_len": 150})):
        out = features.process_csv_row(dict(cf), **kw)
        ref = {k[len(f"{name}_{tag}_"):]: G[k] for k in G if k.startswith(f"{name}_{tag}_") and not k.endswith("_dtype")}
        assert set(out) == set(ref)
        for k, v in out.items():
            assert str(v.dtype) == str(G[f"{name}_{tag}_{k}_dtype"]), (k, v.dtype)
            if v.dtype.kind in "iu":
                np.testing.assert_array_equal(v, ref[k], err_msg=k)
            elif k == "rigidgroups_0":
                # float32 frames from float64 Gram-Schmidt; groups whose base atoms are missing are degenerate in both
                np.testing.assert_allclose(v, ref[k], atol=2e-6, err_msg=k)
            elif k == "torsion_angles_sin_cos":
                np.testing.assert_allclose(v, ref[k], atol=2e-6, err_msg=k)
            else:
                np.testing.assert_allclose(v, ref[k], rtol=1e-6, atol=1e-6, err_msg=k)


def test_mmcif_reader_on_synthetic_file(tmp_path):
    """framedipt_amd.data.mmcif on a hand-written _atom_site loop: author chain ids, insertion codes, alternate locations by
    occupancy, second model ignored, hetero residues -> X, waters at the chain end trimmed from the modelled range, quoted names."""
    from framedipt_amd.data import features, mmcif
    cols = ["group_PDB", "id", "type_symbol", "label_atom_id", "label_alt_id", "label_comp_id", "label_asym_id", "label_seq_id",
            "pdbx_PDB_ins_code", "Cartn_x", "Cartn_y", "Cartn_z", "occupancy", "B_iso_or_equiv", "auth_seq_id", "auth_asym_id",
            "pdbx_PDB_model_num"]
    rows, n = [], [0]

    def atom(grp, name, alt, comp, seq, ins, xyz, occ, chain, model=1):
        n[0] += 1
        nm = f'"{name}"' if "'" in name else name
        rows.append(f"{grp} {n[0]} C {nm} {alt} {comp} Z {seq} {ins} {xyz[0]} {xyz[1]} {xyz[2]} {occ} 10.0 {seq} {chain} {model}")

    for i, comp in enumerate(["MSE", "ALA", "GLY", "LYS"]):  # MSE: non-standard -> X at the start (trimmed)
        for j, a in enumerate(["N", "CA", "C", "O"]):
            atom("HETATM" if comp == "MSE" else "ATOM", a, ".", comp, 10 + i, "?", (i * 3.8 + j, j, 0.5), 1.0, "b")
    atom("ATOM", "CB", "A", "ALA", 11, "?", (1.0, 2.0, 3.0), 0.4, "b")
    atom("ATOM", "CB", "B", "ALA", 11, "?", (9.0, 9.0, 9.0), 0.6, "b")      # higher occupancy wins
    atom("ATOM", "CA", ".", "SER", 12, "A", (5.0, 5.0, 5.0), 1.0, "b")      # insertion code: its own residue
    atom("HETATM", "O", ".", "HOH", 201, "?", (0.0, 0.0, 0.0), 1.0, "b")    # water at the end
    atom("ATOM", "O5'", ".", "DA", 1, "?", (0.0, 0.0, 0.0), 1.0, "C")       # nucleotide chain: no modelled residue -> dropped
    atom("ATOM", "CA", ".", "ALA", 10, "?", (7.0, 7.0, 7.0), 1.0, "b", model=2)
    p = tmp_path / "1abc-assembly1.cif"
    p.write_text("data_1ABC\n#\n_entry.id 1ABC\n#\nloop_\n" + "".join(f"_atom_site.{c}\n" for c in cols) + "\n".join(rows) + "\n#\n")
    num_chains, lens, mlens, cf = mmcif.extract_features_from_mmcif(p)
    assert num_chains == 2 and lens == [6] and mlens == [4]
    assert list(cf["aatype"]) == [20, 0, 7, 11, 15, 20] and list(cf["residue_index"]) == [10, 11, 12, 13, 12, 201]
    assert list(cf["min_modeled_idxs"]) == [1] and list(cf["max_modeled_idxs"]) == [4]
    assert set(cf["chain_index"]) == {features.chain_str_to_int("A")} and features.chain_str_to_int("A") == 26
    ca, cb = features.ATOM_ORDER["CA"], features.ATOM_ORDER["CB"]
    center = cf["atom_positions"][:, ca].sum(0) / 6  # every residue but the water has a CA; parse_chain_feats centres on them
    np.testing.assert_allclose(cf["atom_positions"][1, cb] - cf["atom_positions"][1, ca], np.array([9, 9, 9]) - np.array([4.8, 1.0, 0.5]),
                               atol=1e-5)
    assert cf["atom_mask"][4].sum() == 1 and cf["bb_mask"][5] == 0 and abs(center).max() < 1e-3
    row = mmcif.process_mmcif(p, tmp_path / "processed")
    assert row["pdb_name"] == "1abc-assembly1" and row["modeled_seq_len"] == 4 and row["seq_len"] == 6
    # ConditionalSampler(data_conf, ...) processes <download_dir>/cifs itself when metadata.csv is absent (sampler.py:189-222)
    from framedipt_amd import config
    from framedipt_amd.sampler import ConditionalSampler, TCRSampler
    (tmp_path / "dl" / "cifs").mkdir(parents=True)
    (tmp_path / "dl" / "cifs" / p.name).write_text(p.read_text())
    (tmp_path / "set.csv").write_text("pdb_id,tcr_alpha_chain,tcr_beta_chain\n1abc,B,B\n")
    dc = config.to_conf({"download_dir": str(tmp_path / "dl"), "data_path": str(tmp_path / "set.csv"), "samples": 3, "seed": 1,
                         "first_assembly": True, "cdr_loops": ["CDR3"], "redaction": {"redact_min_len": 1, "redact_max_len": 2}})
    ds = ConditionalSampler(dc, None, "cuda")
    assert len(ds) == 3 and ds.metadata[0]["modeled_seq_len"] == 4 and (tmp_path / "dl" / "processed" / "metadata.csv").exists()
    assert ds._chain_feats(0)["rigidgroups_0"].shape == (4, 8, 4, 4)
    assert TCRSampler(dc, None, "cuda").all_chains_to_process == [["B", "B"]]
    out = features.process_csv_row(row["processed_path"])
    assert out["aatype"].shape == (4,) and list(out["seq_idx"]) == [0, 1, 2, 3] and out["rigidgroups_0"].shape == (4, 8, 4, 4)
    assert features.map_to_new_str_name(26) == "AA" and features.map_to_new_str_name(676) == "ZA"


def test_hot_kernels_have_no_three_dword_stores(tmp_path):
    """ISA audit (cross-compiled, no GPU): the kernels of the sampler loop contain no `global_store_dwordx3`.  A merged three-float
    store in points16_kernel read its data registers late under memory-pipeline contention and stored the next point's x coordinate
    (the concurrent-forward mismatch); three-float runs are written dword by dword (common.hpp: fd_store3)."""
    import shutil
    import subprocess
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "framedipt_amd", "csrc")
    hot = {"attention": ("points16_kernel", "points_kernel", "opair_mfma_kernel"), "rowblock": ("rowblock_kernel", "tfmr_tail_kernel"),
           "frames": ("reverse_step_kernel", "backbone_kernel", "rot_score_kernel", "build_feats_kernel", "finish_kernel", "split_rigids_kernel",
                      "se3_forward_step_kernel", "se3_step_log_prob_kernel", "compose_q_update_kernel", "trans_score_kernel")}
    for unit, kernels in hot.items():
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-w", "-c", os.path.join(csrc, unit + ".hip"), "-o",
                        str(tmp_path / (unit + ".o")), "-save-temps=obj"], check=True, cwd=csrc)
        asm = open(tmp_path / f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s").read().split("\n")
        cur, bad = None, []
        for line in asm:
            if line.startswith("_Z") and line.rstrip().endswith(":"):
                cur = line
            if "_store_dwordx3" in line and cur and any(k in cur for k in kernels):
                bad.append((cur.strip(), line.strip()))
        assert not bad, bad[:4]


def test_checkpoint_loader_refuses_foreign_globals(tmp_path):
    """A ``.pth`` is a pickle: the loader constructs omegaconf stand-ins, torch's tensor-rebuild helpers and plain containers,
    and refuses every other global a file names (os.system and friends)."""
    import pickle

    import torch

    from framedipt_amd import checkpoint

    class Evil:
        def __reduce__(self):
            import os
            return (os.system, ("echo pwned > /dev/null",))

    bad = tmp_path / "bad.pth"
    torch.save({"model": {"w": torch.zeros(2)}, "conf": Evil()}, bad)
    with pytest.raises(pickle.UnpicklingError, match="refused"):
        checkpoint.load_checkpoint(bad)
    good = tmp_path / "good.pth"
    torch.save({"model": {"module.w": torch.arange(4.0).reshape(2, 2)}, "epoch": 3}, good)
    sd, conf, extra = checkpoint.load_checkpoint(good)
    assert list(sd) == ["w"] and sd["w"].dtype == np.float32 and conf is None and extra == {"epoch": 3}
    # conf_overrides merge last (Inference._load_ckpt)
    from framedipt_amd import config
    cfg = checkpoint.apply_checkpoint_conf(config.base_config(), {"model": {"ipa": {"num_blocks": 2}}},
                                           conf_overrides={"model": {"ipa": {"num_blocks": 3}}})
    assert cfg.model.ipa.num_blocks == 3


def test_checkpoint_loader_refuses_getattr_gadgets(tmp_path):
    """The allow-list must not contain a way to walk attributes: ``getattr(_rebuild_tensor_v2, "__globals__")`` reaches ``sys.modules`` and
    ``os.system`` through allowed names only (round-3 advisor finding); protocol-4 dotted names are the same walk; ``omegaconf.*`` names
    never resolve to real attributes (``omegaconf.omegaconf`` + ``os.system``), they become inert stand-ins."""
    import io
    import pickle
    import pickletools  # noqa: F401  (documented aid for reading the hand-written streams below)

    from framedipt_amd import checkpoint, config

    def load(b):
        return checkpoint._ShimUnpickler(io.BytesIO(b)).load()

    # (1) GLOBAL builtins getattr / builtins object are refused
    for mod, name in (("builtins", "getattr"), ("builtins", "object"), ("pathlib", "Path"), ("pathlib", "PosixPath")):
        with pytest.raises(pickle.UnpicklingError, match="refused"):
            load(b"c" + mod.encode() + b"\n" + name.encode() + b"\n.")
    # (2) the gadget itself: getattr(torch._utils._rebuild_tensor_v2, "__globals__")
    gadget = (b"cbuiltins\ngetattr\n(ctorch._utils\n_rebuild_tensor_v2\nV__globals__\ntR.")
    with pytest.raises(pickle.UnpicklingError, match="refused"):
        load(gadget)
    # (3) protocol-4 dotted names: STACK_GLOBAL with "torch._utils" / "_rebuild_tensor_v2.__globals__", and through the omegaconf branch
    def stack_global(mod, name):
        return (b"\x80\x04" + b"\x8c" + bytes([len(mod)]) + mod.encode() + b"\x8c" + bytes([len(name)]) + name.encode() + b"\x93.")
    for mod, name in (("torch._utils", "_rebuild_tensor_v2.__globals__"), ("omegaconf.omegaconf", "os.system"), ("omegaconf", "omegaconf.os.system")):
        with pytest.raises(pickle.UnpicklingError, match="refused"):
            load(stack_global(mod, name))
    # (4) an omegaconf name is a stand-in, never a resolved attribute — also when it names something a real package would export
    cls = load(stack_global("omegaconf.omegaconf", "os"))
    assert getattr(cls, "_fd_stub", False) and isinstance(cls, type)
    # (5) an override of diffuser.r3 wins over the checkpoint's diffuser.r3 (Inference._load_ckpt assigns r3 first, merges overrides last)
    r3 = dict(config.base_config().diffuser.r3)
    r3["min_b"] = 0.2
    cfg = checkpoint.apply_checkpoint_conf(config.base_config(), {"diffuser": {"r3": r3}}, conf_overrides={"diffuser": {"r3": {"min_b": 0.3}}})
    assert cfg.diffuser.r3.min_b == 0.3
    cfg = checkpoint.apply_checkpoint_conf(config.base_config(), {"diffuser": {"r3": r3}})
    assert cfg.diffuser.r3.min_b == 0.2


def test_mixed_batches_stay_inside_one_kernel_selection_class():
    """sharding.batches_mixed: a batch never spans a length at which the library switches kernels (so a sample's bits do not depend on
    its batch mates: round-3 advisor finding), equal lengths share a batch, every position appears once."""
    from framedipt_amd import sharding
    rng = np.random.default_rng(0)
    lengths = [int(x) for x in rng.integers(290, 800, 200)] + [300] * 5 + [384, 385, 388, 512, 513, 640, 641]
    for max_batch, waste in ((8, 0.15), (4, 0.05), (64, 0.9)):
        groups = sharding.batches_mixed(lengths, max_batch, waste)
        assert sorted(p for g in groups for p in g) == list(range(len(lengths)))
        for g in groups:
            assert 1 <= len(g) <= max_batch
            n_pad = -(-max(lengths[p] for p in g) // 4) * 4
            classes = {sharding.kernel_class(lengths[p]) for p in g} | {sharding.kernel_class(n_pad)}
            assert len(classes) == 1, (g, [lengths[p] for p in g])
    assert sharding.kernel_class(384) == sharding.kernel_class(381) != sharding.kernel_class(385)
    assert sharding.kernel_class(300) == sharding.kernel_class(320) != sharding.kernel_class(321)


def test_kernel_flag_constants_match_the_header():
    """framedipt_amd._lib.KF_* (what ScoreNetwork(kernel_flags=...) passes in FdiptDims; the FDIPT_KF_* macros of include/fdipt.h, their
    values pinned by tests/test_abi_host.py) against the library: bit 32 (the retired plain-operand node path) is unassigned, and the
    library refuses it in every precision like any unknown bit, while it takes each remaining flag alone."""
    from framedipt_amd import _lib, config
    from framedipt_amd.model.score_network import dims_from_conf
    macros = {k[len("KF_"):]: v for k, v in vars(_lib).items() if k.startswith("KF_")}
    names = [k for k in macros if k != "ALL"]
    assert len(names) >= 9 and 32 not in macros.values()
    lib = _lib.load()
    conf = config.base_config()
    for prec in (_lib.PREC_F32, _lib.PREC_F16, _lib.PREC_F16X):
        d = dims_from_conf(conf.model, conf.diffuser, False, prec)
        n = lib.fdipt_param_count(C.byref(d))
        assert n > 0
        d.kernel_flags = 32
        assert lib.fdipt_param_count(C.byref(d)) == -1, prec
        for k in names:
            d.kernel_flags = macros[k]
            assert lib.fdipt_param_count(C.byref(d)) == n, (prec, k)


def test_bench_dump_outputs_names_and_size_cap(tmp_path):
    """bench.dump_outputs (--dump-outputs): every array as <name>.npy (rank r > 0: <name>_rank<r>.npy); above DUMP_BYTES / world, the
    same seeded sample of batch rows on every call, under the cap."""
    import bench
    rng = np.random.default_rng(1)
    arrays = {"prot_traj": rng.standard_normal((64, 1000, 37, 3)).astype(np.float32), "psi_pred": rng.standard_normal((64, 1000, 2)).astype(np.float32)}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    for k, v in arrays.items():
        np.testing.assert_array_equal(np.load(tmp_path / "all" / f"{k}.npy"), v)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, rank=3, world=4)
        assert sorted(os.listdir(tmp_path / run)) == ["prot_traj_rank3.npy", "psi_pred_rank3.npy"]
        assert sum(os.path.getsize(tmp_path / run / f) for f in os.listdir(tmp_path / run)) <= bench.DUMP_BYTES / 4
    a, b = (np.load(tmp_path / r / "prot_traj_rank3.npy") for r in ("a", "b"))
    assert 1 <= a.shape[0] < 64 and a.tobytes() == b.tobytes()
    rows = [int(np.flatnonzero((arrays["prot_traj"] == x).all(axis=(1, 2, 3)))[0]) for x in a]
    assert rows == sorted(set(rows))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "psi_pred_rank3.npy"), arrays["psi_pred"][rows])
