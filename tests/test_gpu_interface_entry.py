"""GPU test (-m gpu) of ``run_sharded --interface``: an inpainting run of one of the test complexes scored against its ground truth on
``loop_sides`` (framedipt_amd/interface.py), in the style of the ``--lddt`` entry test."""
import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


def _run_sharded(out_dir, *flags):
    import os
    import subprocess
    import sys
    cmd = [sys.executable, "-m", "framedipt_amd.run_sharded", "--out-dir", str(out_dir), "--num-t", "2", "--max-batch", "4", "--keep", "last", *flags]
    r = subprocess.run(cmd, env=dict(os.environ, FDIPT_SHARED_GPU="allow"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return sorted(str(p.relative_to(out_dir)) for p in out_dir.rglob("*") if p.is_file())


def test_run_sharded_interface_on_an_inpainting_run(tmp_path):
    """``run_sharded --interface --select`` on 1fyt (two samples, two steps): ``interface.json`` lists, per chain with diffused rows, the two
    samples and the five selected structures with numbers in range, the csv carries the same numbers, and the native contacts - the
    ground truth's own - are the same for every structure of a chain; the same command without ``--interface`` writes the same files but
    ``interface.json`` and ``interface.csv``."""
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
    with_flag, without = _run_sharded(tmp_path / "a", *flags, "--interface"), _run_sharded(tmp_path / "b", *flags)
    assert sorted(set(with_flag) - set(without)) == ["interface.csv", "interface.json"] and set(without) <= set(with_flag)
    for f in without:
        if f.endswith((".pdb", ".csv")) or f == "selection.json":
            assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    with open(tmp_path / "a" / "interface.json") as f:
        summary = json.load(f)
    with open(tmp_path / "a" / "interface.csv", newline="") as f:
        table = list(csv.DictReader(f))
    assert summary["atoms"] == "cb" and summary["contact_cutoff"] == 8.0 and not summary["skipped"] and len(summary["samples"]) == len(table) > 0
    chains = sorted({e["chain"] for e in summary["samples"]})
    labels = ["0", "1"] + list(selection.STRATEGIES)
    assert [(e["sample"], e["chain"]) for e in summary["samples"]] == [(s, c) for s in labels for c in chains] == [(t["sample"], int(t["chain"])) for t in table]
    for c in chains:
        entries = [e for e in summary["samples"] if e["chain"] == c]
        assert len({(e["n_native"], e["n_interface_rows"], tuple(e["res_native"]), tuple(e["ligand_rows"])) for e in entries}) == 1
    for entry, row in zip(summary["samples"], table):
        assert len(entry["ligand_rows"]) == len(entry["res_native"]) == len(entry["res_model"]) == len(entry["res_shared"]) >= 1
        assert 0 <= entry["n_shared"] <= min(entry["n_native"], entry["n_model"]) and 0.0 <= entry["fnat"] <= 1.0 and 0.0 <= entry["fnonnat"] <= 1.0
        assert sum(entry["res_native"]) == entry["n_native"] and sum(entry["res_model"]) == entry["n_model"] and sum(entry["res_shared"]) == entry["n_shared"]
        assert entry["lrmsd"] is not None and entry["lrmsd"] >= 0 and (entry["dockq"] is None or 0.0 <= entry["dockq"] <= 1.0)
        for k in ("n_native", "n_model", "n_shared", "n_interface_rows", "fnat", "fnonnat", "irmsd", "lrmsd", "dockq", "capri_class", "status"):
            assert (row[k] == "" and entry[k] is None) or float(row[k]) == entry[k], k
