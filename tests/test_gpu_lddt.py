"""GPU tests (-m gpu) of the superposition-free accuracy scores (framedipt_amd/lddt.py -> fdipt_sample_lddt, csrc/lddt.hip) against the
reference fixture tests/golden/lddt_cases.npz and the NumPy restatement tests/lddt_ref.py.  ``pytest tests/test_gpu_lddt.py -m gpu -s``
prints the worst device error per float output next to its bound (32 x the reference's or the restatement's own change under the
fixture's recorded row permutations), and the distance of the device result to the reference's float32 run next to the distance between
the reference's own two runs."""
import functools

import numpy as np
import pytest
import torch

import lddt_ref as lr
from conftest import load_golden

pytestmark = pytest.mark.gpu

OUTPUTS = lr.EXACT_OUTPUTS + lr.FLOAT_OUTPUTS
VARIANTS = [(name, mode, same) for name, mode in lr.CASE_MODES for same in ((False,) if mode == "ca" else (False, True))]


@functools.lru_cache(maxsize=None)
def _fix():
    return load_golden("lddt_cases.npz")


def _call(inp, mode, **over):
    from framedipt_amd import lddt
    kw = dict(inp, atoms=mode, per_atom=True)
    kw.update(over)
    return lddt.local_accuracy(**kw)


@functools.lru_cache(maxsize=None)
def _single(name, mode, same=False):
    """One case as a call of its own (NumPy inputs, uploaded)."""
    return _call(lr.case_inputs(_fix(), name), mode, same_residue=same)


@functools.lru_cache(maxsize=None)
def _restated(name, mode, same=False):
    return lr.restate_case(_fix(), name, mode, same)


def _same_pairs(a, pa, b, pb, n):
    """Pairs ``pa`` of result a equal pairs ``pb`` of result b bit for bit in every output on the first n rows; the rows behind are zero."""
    for k in OUTPUTS:
        x, y = np.asarray(a[k])[pa], np.asarray(b[k])[pb]
        if x.ndim > 1:
            assert not x[:, n:].any() and not y[:, n:].any(), k
            x, y = x[:, :n], y[:, :n]
        assert x.dtype == y.dtype and np.array_equal(x, y), k


@pytest.mark.parametrize("name,mode,same", VARIANTS)
def test_case_matches_the_reference_and_the_restatement(name, mode, same):
    """Every case alone.  lDDT per pair, per residue and per atom and the integers they come from: the restatement bit for bit everywhere,
    the reference's float64 run bit for bit where its function applies (``lddt_ca``; ``lddt`` on the flattened atoms = ``same_residue``;
    per score row, and globally where every existing row is one).  dRMSD and FAPE within 32 x the yardstick; status exactly."""
    fix, got, want = _fix(), _single(name, mode, same), _restated(name, mode, same)
    lr.check_exact(want, got)
    models = lr.case_pairs(fix, name)[:, 0]
    keep = (fix[f"{name}.res_mask"][models] != 0) & (fix[f"{name}.score_mask"][models] != 0)
    if mode == "ca" or same:
        ref = fix[f"{name}.{mode}.ref_atom"]
        assert np.array_equal(got["atom_lddt"][keep], ref[keep])
        if mode == "ca":
            assert np.array_equal(got["res_lddt"][keep], ref[..., 0][keep])
        if lr.reference_applies_globally(fix, name):
            assert np.array_equal(got["lddt"], fix[f"{name}.{mode}.ref_lddt"])
        shipped = fix[f"{name}.{mode}.ref_atom.f32"].astype(np.float64)
        print(f"{name} {mode}: lddt per atom: |device - float32 run| = {np.abs(got['atom_lddt'] - shipped)[keep].max(initial=0.0):.3e}, "
              f"|float64 run - float32 run| = {np.abs(ref - shipped)[keep].max(initial=0.0):.3e}")
    assert np.array_equal(got["pairs"], lr.case_pairs(fix, name))
    report = {}
    try:
        lr.check_floats({k: fix[f"{name}.{k}"] for k in lr.FLOAT_OUTPUTS}, got, lambda k: lr.bound(fix, name, k), lambda k, err, lim: report.__setitem__(k, (err, lim)))
        lr.check_floats(want, got, lambda k: lr.bound(fix, name, k))
    finally:
        for k, (err, lim) in report.items():
            print(f"{name} {mode}: {k}: |device - expected| = {err:.3e}, bound {lim:.3e}")
    for k in ("drmsd", "fape"):
        shipped, exact = fix[f"{name}.{k}.f32"], fix[f"{name}.{k}"]
        own, dev = float(np.abs(exact - shipped).max()), float(np.abs(got[k] - shipped).max())
        print(f"{name} {mode}: {k}: |device - float32 run| = {dev:.3e}, |float64 run - float32 run| = {own:.3e}")
        assert dev <= own + lr.bound(fix, name, k), k


def test_edges_of_the_contract_on_the_device():
    """N = 1: no partner, lDDT 1.0 with the status bit, dRMSD 0.  A row whose N is missing has no frame and is still a FAPE point.  The
    planted pair 1e-3 inside the cutoff is scored, the one 1e-3 outside is not.  Atoms count only where both structures have them."""
    from framedipt_amd import _lib
    fix = _fix()
    one = _single("n1", "ca")
    assert one["lddt"].tolist() == [1.0] and one["res_lddt"].tolist() == [[1.0]] and one["drmsd"].tolist() == [0.0] and one["status"].tolist() == [_lib.LDDT_NO_PARTNER]
    no_n = _single("no_n", "backbone")
    assert no_n["res_fape"][0, 5] == 0 and np.count_nonzero(no_n["res_fape"][0]) == 11 and no_n["status"].tolist() == [0]
    inp = lr.case_inputs(fix, "cutoff")
    (i, j), (k, l) = fix["cutoff.planted"]
    base, near, far = _single("cutoff", "ca"), _call(inp, "ca", cutoff=15.0 - 2e-3), _call(inp, "ca", cutoff=15.0 + 2e-3)
    assert base["n_scored"][0, [i, j]].tolist() == (near["n_scored"][0, [i, j]] + 1).tolist()
    assert base["n_scored"][0, [k, l]].tolist() == (far["n_scored"][0, [k, l]] - 1).tolist()
    bare = fix["sidechain.xb"].copy()
    bare[:, :, 5:] = 0
    side, same = _single("sidechain", "all"), _call(dict(lr.case_inputs(fix, "sidechain"), prot_b=bare), "all")
    _same_pairs(side, [0], same, [0], 24)
    # atom masks say the same as zeroed coordinates
    masked = _call(dict(lr.case_inputs(fix, "sidechain"), atom_mask_b=np.any(bare != 0, axis=-1)), "all")
    _same_pairs(side, [0], masked, [0], 24)
    skipped = _call(dict(lr.case_inputs(fix, "n65"), pairs=np.array([[0, 0], [0, 3], [-1, 0]])), "ca")
    assert skipped["status"].tolist() == [0, _lib.LDDT_SKIPPED, _lib.LDDT_SKIPPED] and not skipped["res_lddt"][1:].any() and not skipped["lddt"][1:].any()
    _same_pairs(skipped, [0], _single("n65", "ca"), [0], 65)


@pytest.mark.parametrize("mode", lr.MODES)
def test_all_cases_in_one_padded_launch_equal_their_own_launches(mode):
    """Every case of an atom set as one atom37 launch, padded to the longest with res_mask = 0 rows that hold garbage, garbage also in the
    atom columns the set does not read: every output of every pair equals the case's own launch bit for bit, the rows behind stay zero."""
    joint, where = lr.joint_batch(_fix(), mode)
    got = _call(joint, mode)
    for name, first, count in where:
        one = _single(name, mode)
        _same_pairs(got, np.arange(first, first + count), one, np.arange(count), one["res_lddt"].shape[1])


def test_input_routes_agree():
    """A device tensor against a NumPy array and [S,N,5,3] against [S,N,37,3] give the same bits; a CA trace [S,N,3] gives the lDDT and the
    dRMSD of the ``ca`` set with the FAPE outputs zero and their status bit."""
    from framedipt_amd import _lib
    fix, inp = _fix(), lr.case_inputs(_fix(), "n65")
    for mode in ("ca", "backbone"):
        one = _single("n65", mode)
        on_device = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}
        wide = dict(inp, prot_a=lr.to_atom37(inp["prot_a"]), prot_b=lr.to_atom37(inp["prot_b"]))
        mixed = dict(inp, prot_a=torch.from_numpy(lr.to_atom37(inp["prot_a"])).cuda())
        for other in (_call(on_device, mode), _call(wide, mode), _call(mixed, mode)):
            _same_pairs(other, [0], one, [0], 65)
    one = _single("n65", "ca")
    trace = _call(dict(inp, prot_a=np.ascontiguousarray(inp["prot_a"][:, :, 1]), prot_b=torch.from_numpy(np.ascontiguousarray(inp["prot_b"][:, :, 1])).cuda()), "ca")
    for k in lr.EXACT_OUTPUTS[:-1] + ("drmsd",):
        assert np.array_equal(trace[k], one[k]), k
    assert trace["status"].tolist() == [_lib.LDDT_NO_FRAME] and not trace["fape"].any() and not trace["res_fape"].any() and not trace["region_fape"].any()
    half = _call(dict(inp, prot_a=np.ascontiguousarray(inp["prot_a"][:, :, 1])), "ca")  # (a trace against a full reference: no frames either)
    assert np.array_equal(half["res_lddt"], one["res_lddt"]) and half["status"].tolist() == [_lib.LDDT_NO_FRAME]


def test_ordered_all_pairs_matrix_and_consensus():
    """S = 3 as ordered all-pairs: ``matrix[i, j]`` is the pairwise call (model i, reference j) - not assumed symmetric - and ``consensus``
    its NumPy definition."""
    fix = _fix()
    for mode in ("ca", "backbone"):
        got = _single("s3", mode)
        assert got["matrix"].shape == (3, 3) and np.array_equal(np.diag(got["matrix"]), np.ones(3)) and not np.diag(got["drmsd_matrix"]).any()
        for i in range(3):
            for j in range(3):
                if i != j:
                    pair = _call({"prot_a": fix["s3.xa"], "pairs": np.array([[i, j]])}, mode)
                    assert got["matrix"][i, j] == pair["lddt"][0] and got["drmsd_matrix"][i, j] == pair["drmsd"][0]
                    direct = _call({"prot_a": fix["s3.xa"][i:i + 1], "prot_b": fix["s3.xa"][j:j + 1]}, mode)
                    _same_pairs(direct, [0], pair, [0], 20)
        assert not np.array_equal(got["matrix"], got["matrix"].T)  # (the reference structure chooses the scored pairs)
        want = np.stack([np.mean([got["res_lddt"][p] for p in range(6) if got["pairs"][p, 0] == i], axis=0) for i in range(3)])
        assert np.array_equal(got["consensus"], want) and got["consensus"].shape == (3, 20)


def test_a_structure_against_itself():
    """Every scored pair passes every threshold (n_passed = n_scored: lDDT is 1), every score is the reference's formula on those integers
    - which is exactly 1.0 or, for counts such as c = 3, the 1 - 2^-53 that the reference's reciprocal-then-product gives - dRMSD is
    exactly 0 and FAPE is sqrt(1e-4) / 10 * n_f n_p / ((1e-4 + n_f)(1e-4 + n_p)) to the bound."""
    fix = _fix()
    for name, mode in (("n65", "backbone"), ("tile", "ca"), ("all48", "all")):
        x = fix[f"{name}.xb"]
        got = _call({"prot_a": x, "prot_b": x.copy()}, mode)
        assert np.array_equal(got["n_passed"], np.repeat(got["n_scored"][..., None], 4, axis=-1)) and got["n_scored"].min() > 0
        assert np.array_equal(got["res_lddt"], lr.score(got["n_scored"], got["n_passed"]))
        assert np.abs(got["res_lddt"] - 1.0).max() <= 2.0 ** -52 and abs(got["lddt"][0] - 1.0) <= 2.0 ** -52 and np.abs(got["atom_lddt"] - 1.0).max() <= 2.0 ** -52
        assert (got["res_lddt"] == 1.0).mean() > 0.5
        assert got["drmsd"].tolist() == [0.0] and got["status"].tolist() == [0]
        n = x.shape[1]
        want = np.sqrt(1e-4) / 10 * n * n / ((1e-4 + n) * (1e-4 + n))
        print(f"{name}: self FAPE {got['fape'][0]!r}, expected {want!r}, bound {lr.bound(fix, name, 'fape'):.3e}")
        assert abs(got["fape"][0] - want) <= lr.bound(fix, name, "fape")
        assert np.abs(got["res_fape"][0] - np.sqrt(1e-4) / 10 * n / (1e-4 + n)).max() <= lr.bound(fix, name, "res_fape")


@pytest.mark.parametrize("name", lr.MOTION_CASES)
def test_rigid_motion_of_the_model(name):
    """The fixture's rotation and 100 Angstrom shift of the model, rounded to float32 again (the device takes float32): no integer output
    and no lDDT bit changes (the generator asserts that the moved model is as decidable).  The floats of the moved model are within the
    32 x yardstick bound of the restatement on the same moved input.  Against the unmoved call they can only agree to what the float32
    rounding of the moved coordinates allows: a coordinate below 256 moves by at most 2^-17, a point by r = sqrt(3) 2^-17 = 1.4e-5, a
    distance by 2 r and so does dRMSD.  A model frame's axes turn by at most 1.6 r (e0: two end points over a bond of at least 1.3
    Angstrom), 3.7 r (e1: N - CA moves by 2 r and loses e0's share of at most 1.5 x 1.6 r, over a rejection of at least 1.2) and their
    sum 5.3 r (e2), together by less than 6.7 r; so a local point at distance D moves by at most 2 r + 6.7 r D, and FAPE - 1-Lipschitz in
    it, in units of 10 - by a tenth of that with D the largest CA-CA distance of the model."""
    fix = _fix()
    inp = lr.case_inputs(fix, name)
    moved = lr.move(inp["prot_a"], fix["motion.rot"], fix["motion.shift"])
    assert moved.dtype == np.float32 and np.abs(moved).max() < 256 and np.abs(moved - inp["prot_a"]).max() > 30
    r = np.sqrt(3.0) * 2.0 ** -17
    ca = inp["prot_a"][0, :, 1].astype(np.float64)
    reach = np.sqrt(((ca[:, None] - ca[None]) ** 2).sum(-1)).max()
    for mode in lr.CASES[name]:
        for same in ((False,) if mode == "ca" else (False, True)):
            base, got = _single(name, mode, same), _call(dict(inp, prot_a=moved), mode, same_residue=same)
            lr.check_exact(base, got)
            want = lr.restate_case(fix, name, mode, same, transform=lambda x: lr.move(x, fix["motion.rot"], fix["motion.shift"]))
            lr.check_exact(want, got)
            lr.check_floats(want, got, lambda k: lr.bound(fix, name, k))
            limit = {"drmsd": 2 * r, "fape": (2 * r + 6.7 * r * reach) / 10}
            limit.update(res_fape=limit["fape"], region_fape=limit["fape"])
            lr.check_floats(base, got, lambda k: limit[k], lambda k, err, lim: print(f"{name} {mode}: {k}: |moved - unmoved| = {err:.3e}, float32 limit {lim:.3e}"))


def test_end_to_end_sampler_small_config():
    """Two de novo samples (small config, N = 24, T = 6), the result left on the device: the scores of the device tensor, every ordered
    pair, agree with the restatement on the downloaded coordinates - integers and lDDT bit for bit, floats within the fixture's widest
    bound; nothing between the two calls waits for the device."""
    from framedipt_amd import config, inference, lddt
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import UnconditionalSampler
    n, b, num_t = 24, 2, 6
    conf = config.small_config()
    d = SE3Diffuser(conf.diffuser, device="cuda:0")
    net = ScoreNetwork(conf.model, d, precision="fp32").load_synthetic(3).to("cuda:0")
    ds = UnconditionalSampler(config.to_conf({"min_length": n, "max_length": n, "length_step": 1, "samples_per_length": b}), d, "cuda:0")
    np.random.seed(11)
    items = [ds[i][2] for i in range(b)]
    feats = {k: torch.cat([it[k] for it in items], 0) for k in items[0]}
    res = inference.inference_fn(net, d, feats, num_t=num_t, min_t=0.01, aux_traj=True, noise_scale=0.1, return_device=True)
    prot = res["prot_traj"][0]
    assert prot.is_cuda and tuple(prot.shape) == (b, n, 37, 3)
    host, fix = prot.cpu().numpy(), _fix()
    for mode in ("ca", "backbone"):
        got = lddt.local_accuracy(prot, atoms=mode, per_atom=True)
        assert got["pairs"].tolist() == [[0, 1], [1, 0]] and got["matrix"].shape == (2, 2)
        for p, (i, j) in enumerate(got["pairs"]):
            want = lr.local_accuracy(host[i], host[j], mode)
            mine = {k: got[k][p] for k in OUTPUTS}
            print(f"sampler ({i}, {j}) {mode}: lddt {mine['lddt']:.4f}, drmsd {mine['drmsd']:.3f}, fape {mine['fape']:.4f}, decision margin {want['margin']:.1e}")
            lr.check_exact(want, mine)
            lr.check_floats(want, mine, lambda k: lr.widest_bound(fix, k))
        assert list(lddt.lddt_metrics(got, 1)) == [lddt.METRIC_NAMES[mode], "drmsd", "fape", "region_fape"]


def _run_sharded(out_dir, *flags):
    import os
    import subprocess
    import sys

    from conftest import ROOT
    cmd = [sys.executable, "-m", "framedipt_amd.run_sharded", "--out-dir", str(out_dir), "--num-t", "2", "--max-batch", "4", "--keep", "last", *flags]
    r = subprocess.run(cmd, env=dict(os.environ, FDIPT_SHARED_GPU="allow"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return sorted(str(p.relative_to(out_dir)) for p in out_dir.rglob("*") if p.is_file())


def test_run_sharded_lddt_on_a_de_novo_run(tmp_path):
    """``run_sharded --lddt`` on a de novo run of two lengths: ``pairwise_lddt_ca_length_<L>.npy`` and ``consistency.json`` hold the numbers
    of a direct call on the written samples; without the flag the run writes the same files but these."""
    import json

    from framedipt_amd import lddt
    flags = ("--min-length", "9", "--max-length", "14", "--length-step", "5", "--samples-per-length", "3", "--precision", "fp32")
    with_flag, without = _run_sharded(tmp_path / "a", *flags, "--lddt"), _run_sharded(tmp_path / "b", *flags)
    extra = ["consistency.json", "pairwise_lddt_ca_length_14.npy", "pairwise_lddt_ca_length_9.npy"]
    assert sorted(set(with_flag) - set(without)) == extra and set(without) <= set(with_flag)
    for f in without:
        if f.endswith(".npz"):
            x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
            assert x.files == y.files and all(np.array_equal(x[k], y[k]) for k in x.files), f
    with open(tmp_path / "a" / "consistency.json") as f:
        summary = json.load(f)
    with open(tmp_path / "a" / "manifest.json") as f:
        records = {(r["name"], r["sample_i"]): r for r in json.load(f)["samples"]}
    assert [e["length"] for e in summary["lengths"]] == [9, 14] and summary["atoms"] == "ca"
    for entry in summary["lengths"]:
        prot = np.stack([np.load(tmp_path / "a" / records[(s["pdb_name"], s["sample"])]["file"])["prot_traj"] for s in entry["samples"]])
        assert prot.shape == (3, entry["length"], 37, 3)
        direct = lddt.local_accuracy(prot, atoms="ca")
        matrix = np.load(tmp_path / "a" / f"pairwise_lddt_ca_length_{entry['length']}.npy")
        assert matrix.dtype == np.float64 and np.array_equal(matrix, direct["matrix"])
        for s, sample in enumerate(entry["samples"]):
            assert sample["consensus"] == direct["consensus"][s].tolist() and sample["mean_lddt"] == np.delete(direct["matrix"][s], s).mean().item()


def test_run_lddt_scores_an_inpainting_run_against_its_ground_truth(tmp_path):
    """``run_sharded.run_lddt`` (what ``--lddt`` runs on rank 0) on gathered entries as an inpainting run leaves them - the fixture's
    two-chain complex with its 12-row loop diffused, two samples and the ground truth: ``lddt.json`` and ``lddt.csv`` carry the numbers of
    direct calls in the ``ca`` and the ``backbone`` set with score_mask = the diffused rows."""
    import csv
    import json

    from framedipt_amd import lddt, run_sharded
    fix = _fix()
    truth, diffused = lr.to_atom37(fix["loop.xb"])[0], fix["loop.score_mask"][0] != 0
    samples = [lr.to_atom37(fix["loop.xa"])[0], lr.to_atom37(fix["loop.xb"])[0].copy()]
    samples[1][diffused] += np.float32(0.7)
    records = [{"item": s, "name": "complex", "sample_i": s, "file": f"complex/sample_{s}/sample_{s}_1.pdb"} for s in range(2)]
    gathered = {s: {"prot": samples[s], "diffused": diffused, "res_mask": np.ones(48, dtype=np.float32), **({"gt": truth} if s == 0 else {})} for s in range(2)}
    summary = run_sharded.run_lddt(str(tmp_path), records, gathered, inpainting=True)
    with open(tmp_path / "lddt.json") as f:
        assert json.load(f) == json.loads(json.dumps(summary))
    with open(tmp_path / "lddt.csv", newline="") as f:
        table = list(csv.DictReader(f))
    assert [e["sample"] for e in summary["samples"]] == ["0", "1"] == [t["sample"] for t in table] and not summary["skipped"]
    prot = np.stack(samples)
    ca, bb = (lddt.local_accuracy(prot, truth[None], atoms=mode, score_mask=np.stack([diffused, diffused])) for mode in ("ca", "backbone"))
    for s, (entry, row) in enumerate(zip(summary["samples"], table)):
        want = {**lddt.lddt_metrics(ca, s), "lddt_bb": float(bb["lddt"][s])}
        assert entry["rows"] == list(range(10, 22)) and entry["res_lddt_ca"] == ca["res_lddt"][s][10:22].tolist()
        assert entry["res_lddt_bb"] == bb["res_lddt"][s][10:22].tolist() and entry["res_fape"] == ca["res_fape"][s][10:22].tolist()
        for k, v in want.items():
            assert entry[k] == v == float(row[k]), k
    assert np.array_equal(_single("loop", "ca")["res_lddt"][0], ca["res_lddt"][0])
    bare = {i: {k: v for k, v in it.items() if k != "gt"} for i, it in gathered.items()}
    assert run_sharded.run_lddt(str(tmp_path), records, bare, inpainting=True)["skipped"] == ["complex"]


def test_run_sharded_lddt_on_an_inpainting_run(tmp_path):
    """``run_sharded --lddt --select`` on one of the test complexes (two samples, two steps): ``lddt.json`` lists the two samples and the five
    selected structures with the diffused rows of the run and scores in range; the same command without ``--lddt`` writes the same files
    but ``lddt.json`` and ``lddt.csv``."""
    import csv
    import json
    import pickle

    import pandas as pd

    from framedipt_amd import selection
    F = load_golden("features.npz")
    data = tmp_path / "data"
    (data / "processed").mkdir(parents=True)
    name = "1fyt"
    cf = {k[len(name) + 4:]: (v.astype(np.float64) if v.dtype.kind == "f" else v) for k, v in F.items() if k.startswith(name + "_in_")}
    with open(data / "processed" / f"{name}.pkl", "wb") as f:
        pickle.dump(cf, f)
    n = int(np.sum(np.asarray(cf["max_modeled_idxs"]) - np.asarray(cf["min_modeled_idxs"]) + 1))
    pd.DataFrame([{"pdb_name": f"{name}-assembly1", "processed_path": str(data / "processed" / f"{name}.pkl"), "modeled_seq_len": n}]).to_csv(
        data / "processed" / "metadata.csv", index=False)
    flags = ("--download-dir", str(data), "--samples-per-structure", "2", "--precision", "fp16", "--select", "--select-iterations", "20")
    with_flag, without = _run_sharded(tmp_path / "a", *flags, "--lddt"), _run_sharded(tmp_path / "b", *flags)
    assert sorted(set(with_flag) - set(without)) == ["lddt.csv", "lddt.json"] and set(without) <= set(with_flag)
    for f in without:
        if f.endswith((".pdb", ".csv")) or f == "selection.json":
            assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    assert sum(f.endswith(".pdb") for f in without) >= 2 + 5 and "selection.json" in without
    with open(tmp_path / "a" / "lddt.json") as f:
        summary = json.load(f)
    with open(tmp_path / "a" / "lddt.csv", newline="") as f:
        table = list(csv.DictReader(f))
    assert [e["sample"] for e in summary["samples"]] == ["0", "1"] + list(selection.STRATEGIES) == [t["sample"] for t in table]
    rows = summary["samples"][0]["rows"]
    assert 8 <= len(rows) <= n and not summary["skipped"]
    for entry, row in zip(summary["samples"], table):
        assert entry["rows"] == rows and len(entry["res_lddt_ca"]) == len(entry["res_lddt_bb"]) == len(entry["res_fape"]) == len(rows)
        assert 0 < entry["lddt_ca"] <= 1 and 0 < entry["lddt_bb"] <= 1 and entry["drmsd"] >= 0 and 0 < entry["region_fape"] <= 1 and 0 < entry["fape"] <= 1
        assert all(float(row[k]) == entry[k] for k in ("lddt_ca", "lddt_bb", "drmsd", "fape", "region_fape"))
        assert entry["status"] == 0 and min(entry["res_lddt_ca"]) > 0
