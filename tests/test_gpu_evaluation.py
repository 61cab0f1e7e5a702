"""GPU tests (-m gpu) of sample evaluation (framedipt_amd/evaluation.py -> fdipt_sample_evaluate, csrc/evaluate.hip) against the reference
fixture tests/golden/evaluation_cases.npz.  ``pytest tests/test_gpu_evaluation.py -m gpu -s`` prints the worst device error per output
next to its bound (32 x the reference's own change under the fixture's recorded perturbations)."""
import functools

import numpy as np
import pytest
import torch

import evaluation_ref as er
from conftest import load_golden

pytestmark = pytest.mark.gpu

ARRAYS = er.FLOAT_OUTPUTS + er.EXACT_OUTPUTS + ("status",)


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("evaluation_cases.npz")


def _call(inp, **over):
    from framedipt_amd import evaluation
    kw = dict(prot=inp["prot"], reference=inp["ref"], diffuse_mask=inp["diffuse_mask"], chain_idx=inp["chain_idx"], ref_index=inp["ref_index"],
              res_mask=inp["res_mask"])
    kw.update(over)
    return evaluation.evaluate_samples(**kw)


@functools.lru_cache(maxsize=None)
def _single(name):
    """One case as a launch of its own (NumPy inputs, uploaded)."""
    return _call(er.case_inputs(_fix(), name))


def _same_sample(a, i, b, j, n):
    """Sample i of result a equals sample j of result b bit for bit on the first n rows (NaN = NaN)."""
    for k in ARRAYS:
        if k == "gt_dihedral":
            x, y = a[k][int(a["ref_index"][i])], b[k][int(b["ref_index"][j])]
        else:
            x, y = np.asarray(a[k][i]), np.asarray(b[k][j])
        if k in ("res_bb_rmsd", "dihedral", "gt_dihedral", "angle_error"):
            assert not x[..., n:].any() and not y[..., n:].any(), k
            x, y = x[..., :n], y[..., :n]
        assert np.array_equal(x, y, equal_nan=True), k
    assert a["regions"][i] == b["regions"][j] and a["region_rows"][i] == b["region_rows"][j]


@pytest.mark.parametrize("name", er.CASES)
def test_case_matches_the_reference(name):
    fix, got = _fix(), _single(name)
    report = {}
    for s in range(got["bb_rmsd"].shape[0]):
        er.check_sample(fix, name, s, er.sample_of(got, s), report)
    for k, (err, lim) in report.items():
        print(f"{name}: {k}: worst |device - reference| = {err:.3e}, bound {lim:.3e}")
    assert not got["status"].any()


def test_all_cases_in_one_padded_launch_equal_their_own_launches():
    """Seven cases, 16 samples of N = 9 .. 260 padded to 261 rows, seven ground-truth rows: every sample's outputs equal its own
    launch bit for bit, and the rows behind a sample stay zero."""
    joint, first = er.joint_batch(_fix())
    got = _call({**joint, "ref": joint["reference"]})
    for name, b0 in zip(er.CASES, first):
        one = _single(name)
        n = one["res_bb_rmsd"].shape[1]
        for s in range(one["bb_rmsd"].shape[0]):
            _same_sample(got, b0 + s, one, s, n)


def test_padded_two_chains_with_a_longer_batch_mate():
    """``two_chains`` (N = 19) padded to N = 24 with res_mask = 0 rows, next to a sample of 24 real rows: bit-identical to the unpadded launch."""
    fix = _fix()
    inp, mate = er.case_inputs(fix, "two_chains"), er.case_inputs(fix, "wrap")
    pad = lambda x, n=24: np.concatenate([x, np.zeros((x.shape[0], n - x.shape[1]) + x.shape[2:], dtype=x.dtype)], axis=1)  # noqa: E731
    batch = {k: np.concatenate([pad(inp[k]), mate[k][:1, :24]]) for k in ("prot", "diffuse_mask", "res_mask", "chain_idx")}
    batch["ref"] = np.concatenate([pad(inp["ref"]), mate["ref"][:, :24]])
    batch["ref_index"] = np.array([0, 0, 0, 1], dtype=np.int32)
    got, one = _call(batch), _single("two_chains")
    for s in range(3):
        _same_sample(got, s, one, s, 19)
    assert got["regions"][3] == [(0, 2, 23)] and got["status"].tolist() == [0, 0, 0, 0]


def test_device_tensor_and_numpy_array_agree():
    inp = er.case_inputs(_fix(), "two_chains")
    dev = _call(inp, prot=torch.from_numpy(inp["prot"]).cuda(), reference=torch.from_numpy(inp["ref"]).cuda(),
                diffuse_mask=torch.from_numpy(inp["diffuse_mask"]).cuda(), chain_idx=torch.from_numpy(inp["chain_idx"]).cuda())
    for s in range(3):
        _same_sample(dev, s, _single("two_chains"), s, 19)


def test_shared_own_and_sample_against_sample_ground_truth():
    """R = 1 shared by default, R = B with each sample's own row, and ``reference = prot`` with a permuted ref_index."""
    from framedipt_amd import evaluation
    inp = er.case_inputs(_fix(), "two_chains")
    one = _single("two_chains")
    shared = evaluation.evaluate_samples(inp["prot"], inp["ref"], inp["diffuse_mask"], inp["chain_idx"])
    own = evaluation.evaluate_samples(inp["prot"], np.tile(inp["ref"], (3, 1, 1, 1)), inp["diffuse_mask"], inp["chain_idx"])
    assert shared["ref_index"].tolist() == [0, 0, 0] and own["ref_index"].tolist() == [0, 1, 2]
    for s in range(3):
        _same_sample(shared, s, one, s, 19)
        _same_sample(own, s, one, s, 19)
    order = np.array([1, 2, 0])
    pair = evaluation.evaluate_samples(inp["prot"], inp["prot"], inp["diffuse_mask"], inp["chain_idx"], ref_index=order)
    for s in range(3):
        want = er.evaluate(inp["prot"][s], inp["prot"][order[s]], inp["diffuse_mask"][s], inp["chain_idx"][s])
        assert abs(pair["bb_rmsd"][s] - want["bb_rmsd"]) <= er.bound(_fix(), "two_chains", "bb_rmsd")
        assert np.abs(pair["angle_error"][s] - want["angle_error"]).max() <= er.bound(_fix(), "two_chains", "angle_error")
        assert np.array_equal(pair["gt_dihedral"][order[s]], pair["dihedral"][order[s]])
    itself = evaluation.evaluate_samples(inp["prot"], inp["prot"], inp["diffuse_mask"], inp["chain_idx"])
    assert not itself["bb_rmsd"].any() and not itself["angle_error"].any() and np.abs(itself["aligned_rmsd"]).max() <= 1e-12


def test_degenerate_alignment_sets_its_bit_and_stays_finite():
    from framedipt_amd import evaluation
    inp = er.case_inputs(_fix(), "two_chains")
    align = np.zeros_like(inp["res_mask"])
    align[:, [2, 9]] = 1
    align[2, :] = 0  # (and no aligned row at all)
    got = _call(inp, align_mask=align)
    assert (got["status"] == evaluation.DEGENERATE_ALIGNMENT).all()
    for k in ("aligned_mean_dev", "aligned_rmsd", "rotation", "translation"):
        assert np.isfinite(got[k]).all(), k
    assert np.abs(got["rotation"] @ got["rotation"].transpose(0, 2, 1) - np.eye(3)).max() <= 1e-14
    assert np.array_equal(got["bb_rmsd"], _single("two_chains")["bb_rmsd"])


def test_end_to_end_inpainting_small_config():
    """Five inpainting samples of one two-chain structure (small config, N = 24, T = 3), the result left on the device: evaluation on
    the device tensor against the ground truth built from ``rigids_0`` agrees with the restatement on the downloaded array, and the
    fixed residues contribute exactly 0 to ``res_bb_rmsd``."""
    from framedipt_amd import config, evaluation, inference
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import ConditionalSampler
    n, b = 24, 5
    conf = config.small_config(True)
    d = SE3Diffuser(conf.diffuser)
    net = ScoreNetwork(conf.model, d, inpainting=True, precision="fp32").load_synthetic(5).to("cuda")
    rng = np.random.default_rng(n)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    tr = np.cumsum(rng.standard_normal((n, 3)) * 2.0, 0) + 30.0
    dm = np.zeros(n)
    dm[5:11], dm[16:20] = 1, 1
    feats_np = {"rigids_0": np.concatenate([q, tr], -1).astype(np.float32), "diffuse_mask": dm, "aatype": rng.integers(0, 20, n),
                "seq_idx": np.concatenate([np.arange(12), np.arange(12) + 212]), "chain_idx": np.repeat([0.0, 1.0], 12),
                "torsion_angles_sin_cos": np.tile(np.array([0.0, 1.0]), (n, 7, 1))}
    ds = ConditionalSampler.from_features([("synthetic", feats_np)], d, "cuda", samples=b)
    np.random.seed(3)
    items = [ds[i][2] for i in range(b)]
    feats = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    res = inference.inference_fn(net, d, feats, num_t=3, min_t=0.01, aux_traj=True, noise_scale=0.1, inpainting=True, return_device=True)
    prot = res["prot_traj"][0]
    assert prot.is_cuda and tuple(prot.shape) == (b, n, 37, 3)
    gt = inference.get_atom_positions_from_rigids(net, feats["rigids_0"][:1], feats["torsion_angles_sin_cos"][:1, :, 2, :], feats["aatype"][:1])
    gt = np.asarray(gt, dtype=np.float32).reshape(1, n, 37, 3)
    diffuse = (1 - feats["fixed_mask"]) * feats["res_mask"]
    got = evaluation.evaluate_samples(prot, gt, diffuse, feats["chain_idx"], res_mask=feats["res_mask"])
    assert got["regions"][0] == [(0, 5, 10), (1, 4, 7)] and not got["status"].any()
    host = prot.cpu().numpy()
    fix = _fix()
    for s in range(b):
        want = er.evaluate(host[s], gt[0], dm, feats_np["chain_idx"])
        for k in er.FLOAT_OUTPUTS:
            have = got["gt_dihedral"][0] if k == "gt_dihedral" else got[k][s]
            assert np.array_equal(np.isnan(have), np.isnan(np.asarray(want[k]))), k
            assert np.nanmax(np.abs(have - want[k])) <= er.bound(fix, "two_chains", k), (s, k)
        assert got["num_ca_steric_clashes"][s] == want["num_ca_steric_clashes"] and got["reflection"][s] == want["reflection"]
    assert not got["res_bb_rmsd"][:, dm == 0].any() and (got["res_bb_rmsd"][:, dm != 0] > 0).all()
    row = evaluation.eval_columns(got, 0, ["alpha", "beta"])
    assert row["bb_rmsd"] == got["bb_rmsd"][0] and row["bb_rmsd_beta_-1"] == got["res_bb_rmsd"][0, 19] and "gt_phi_alpha_2" in row


def _gathered(fix, names=("two_chains", "wrap")):
    """Manifest records and the gathered per-item entries of a run over fixture cases as structures (what ``run_rank(collect=...)`` leaves)."""
    records, gathered, item = [], {}, 0
    for name in names:
        inp = er.case_inputs(fix, name)
        for s in range(inp["prot"].shape[0]):
            records.append({"item": item, "name": name, "sample_i": s, "file": f"{name}/sample_{s}/sample_{s}_1.pdb"})
            gathered[item] = {"prot": inp["prot"][s], "diffused": inp["diffuse_mask"][s] != 0, "res_mask": inp["res_mask"][s],
                              "chain_idx": inp["chain_idx"][s].astype(np.float32), **({"gt": inp["ref"][0]} if s == 0 else {})}
            item += 1
    return records, gathered


def test_run_evaluation_rows_equal_a_direct_call(tmp_path):
    """``run_sharded.run_evaluation`` (what ``--evaluate`` runs on rank 0) on two structures of different length, with the five selected
    structures of each: ``evaluation.json`` and ``metrics.csv`` hold, per structure and sample or strategy, the numbers of a direct
    ``evaluate_samples`` call on the same structure; without ground truth only the geometry columns are written."""
    import csv
    import json

    from framedipt_amd import evaluation, run_sharded, selection
    fix = _fix()
    records, gathered = _gathered(fix)
    kept = {}
    run_sharded.run_selection(str(tmp_path), records, gathered, reference_layout=False, max_iterations=50, keep=kept)
    summary = run_sharded.run_evaluation(str(tmp_path), records, gathered, tcr=True, selected=kept)
    with open(tmp_path / "evaluation.json") as f:
        assert json.load(f) == json.loads(json.dumps(summary))
    with open(tmp_path / "metrics.csv", newline="") as f:
        table = list(csv.DictReader(f))
    assert [r["sample"] for r in table] == ["0", "1", "2"] + list(selection.STRATEGIES) + ["0", "1", "2", "3"] + list(selection.STRATEGIES)
    assert summary["structures"]["two_chains"]["region_names"] == ["alpha", "beta"] and summary["structures"]["wrap"]["regions"] == [[0, 2, 41]]
    for g, name in enumerate(("two_chains", "wrap")):
        inp = er.case_inputs(fix, name)
        n = inp["prot"].shape[1]
        structures = {str(s): inp["prot"][s] for s in range(inp["prot"].shape[0])}
        structures.update({k: selection.selected_structure(kept["selection"], g, k, kept["prot"])[:n] for k in selection.STRATEGIES})
        labels = list(structures)
        direct = evaluation.evaluate_samples(np.stack([structures[k] for k in labels]), inp["ref"], np.tile(inp["diffuse_mask"][:1], (len(labels), 1)),
                                             np.tile(inp["chain_idx"][:1], (len(labels), 1)))
        for b, label in enumerate(labels):
            row = next(r for r in table if r["pdb_name"] == name and r["sample"] == label)
            want = {**{k: direct[k][b].item() for k in evaluation.SCALARS}, **evaluation.eval_columns(direct, b, ["alpha", "beta"])}
            for k, v in want.items():
                assert float(row[k]) == v or (v != v and row[k] == "nan"), (name, label, k)
            assert summary["structures"][name]["samples"][label]["bb_rmsd"] == direct["bb_rmsd"][b]
        other = next(r for r in table if r["pdb_name"] != name)
        assert any(k.startswith("bb_rmsd_beta") and other[k] == "" for k in other) or name == "wrap"
    bare = {i: {k: v for k, v in it.items() if k != "gt"} for i, it in gathered.items()}
    plain = run_sharded.run_evaluation(str(tmp_path), records, bare)
    assert not plain["ground_truth"] and set(plain["structures"]["wrap"]["samples"]["3"]) == set(evaluation.GEOMETRY_SCALARS)
    assert plain["structures"]["wrap"]["samples"]["3"]["num_ca_steric_clashes"] == int(fix["wrap.num_ca_steric_clashes"][3])


def test_run_sharded_select_evaluate_on_the_test_complexes(tmp_path):
    """``run_sharded --select --evaluate`` on the three TCR-pMHC complexes of the reference's test data (set up as the two-rank inpainting
    test does; one rank here): ``evaluation.json`` and ``metrics.csv`` appear with one row per structure and sample or strategy, and
    agree with each other."""
    import csv
    import json
    import os
    import pickle
    import subprocess
    import sys

    import pandas as pd

    from conftest import ROOT
    from framedipt_amd import evaluation, selection
    F = load_golden("features.npz")
    data = tmp_path / "data"
    (data / "processed").mkdir(parents=True)
    meta = []
    for name in ("1fyt", "5ksa", "7t2d"):
        cf = {k[len(name) + 4:]: (v.astype(np.float64) if v.dtype.kind == "f" else v) for k, v in F.items() if k.startswith(name + "_in_")}
        with open(data / "processed" / f"{name}.pkl", "wb") as f:
            pickle.dump(cf, f)
        n = int(np.sum(np.asarray(cf["max_modeled_idxs"]) - np.asarray(cf["min_modeled_idxs"]) + 1))
        meta.append({"pdb_name": f"{name}-assembly1", "processed_path": str(data / "processed" / f"{name}.pkl"), "modeled_seq_len": n})
    pd.DataFrame(meta).to_csv(data / "processed" / "metadata.csv", index=False)
    out_dir = tmp_path / "out"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", "29661",
           "-m", "framedipt_amd.run_sharded", "--out-dir", str(out_dir), "--download-dir", str(data), "--samples-per-structure", "2", "--num-t", "3",
           "--max-batch", "4", "--precision", "fp16", "--keep", "last", "--select", "--select-iterations", "50", "--evaluate"]
    r = subprocess.run(cmd, env=dict(os.environ, FDIPT_ONE_GPU="1", MASTER_ADDR="127.0.0.1"), cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out_dir / "evaluation.json") as f:
        summary = json.load(f)
    with open(out_dir / "metrics.csv", newline="") as f:
        table = list(csv.DictReader(f))
    assert summary["ground_truth"] and len(summary["structures"]) == 3 and len(table) == 3 * (2 + len(selection.STRATEGIES))
    for name, entry in summary["structures"].items():
        assert list(entry["samples"]) == ["0", "1"] + list(selection.STRATEGIES) and entry["regions"]
        for label, scalars in entry["samples"].items():
            row = next(t for t in table if t["pdb_name"] == name and t["sample"] == label)
            assert scalars["status"] == 0 and scalars["bb_rmsd"] > 0 and scalars["reflection"] == 0
            for k in evaluation.SCALARS:
                assert float(row[k]) == scalars[k], (name, label, k)
            assert float(row[f"bb_rmsd_{entry['region_names'][0]}"]) == scalars["region_bb_rmsd"][0]
