"""Sample-sharded sampling over the GPUs of one node (torchrun entry; SURVEY.md section 8e, experiments/inference.py:198-242 de novo,
:244-389 inpainting).

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29511 \
        -m framedipt_amd.run_sharded --out-dir samples/ --min-length 300 --max-length 300 --samples-per-length 64 --num-t 500

Inpainting (BASELINE configs[2]: every structure of a database CSV, k samples each): ``--download-dir D`` names the reference's
``data.download_dir`` (``D/cifs/*.cif`` and / or ``D/processed/metadata.csv``), ``--csv`` its ``data.data_path``, ``--tcr`` selects
``TCRSampler`` (CDR masks must be in the processed features), ``--samples-per-structure k``; the outputs are then written in the
reference's directory layout (``<out>/<pdb>_length_<L>/{<pdb>_1.pdb, diffusion_info.csv, sample_<i>/sample_<i>_1.pdb [, bb_traj_<i>_1.pdb,
x0_traj_<i>_1.pdb]}``, experiments/inference.py:267-389,480-556) through ``framedipt_amd.output``:

    python -m torch.distributed.run ... -m framedipt_amd.run_sharded --out-dir samples/ --download-dir data/ --csv database/TCR_pMHC_I.csv \
        --tcr --samples-per-structure 5 --num-t 100

One process per GPU.  Dataset items (length, sample index) are dealt round-robin to the ranks; every rank runs its items -
batched by equal length - through ``inference_fn`` and writes one ``sample_<item>.npz`` per item into the shared output
directory; rank 0 writes ``manifest.json`` once every rank is done.  No collective touches the data path: the only
``torch.distributed`` call is the final barrier.  Per-sample seeds (``seed + item``) make a sample's trajectory independent
of the world size (framedipt_amd/sharding.py).
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import time

import numpy as np


def run_rank(dataset, diffuser, run_batch, rank: int, world: int, out_dir: str, seed: int, num_t: int, min_t: float,
             max_batch: int = 8, keep=("prot_traj",), final_only: bool = True, mixed: bool = True, write_item=None,
             noise: str = "host", collect=None, ground_truth=None):
    """Run this rank's share of ``dataset``.  ``run_batch(feats, tape) -> dict of arrays with a batch axis at dim 1`` (the
    keys of ``inference_fn``).  ``noise="device"``: ``run_batch`` receives the batch's noise keys [B] in the tape's place and no tape is
    drawn before the first launch.  ``mixed``: samples of similar (not only equal) length share a batch, padded with res_mask = 0
    rows (sharding.batches_mixed / stack_items_padded; a batch never spans two kernel-selection classes, so a sample's bits do not
    depend on its batch mates); results are cut back to each sample's own length.  ``collect`` (a dict, ``--select``): every item's final
    atom37 and what ``run_selection`` needs to group and write it stay on the host under the item's index; ``ground_truth(feats) -> atom37
    [N,37,3]`` (``--evaluate``, inpainting) is called for the first sample of every structure and kept with it under ``gt``.
    Returns the list of records written by this rank."""
    from . import sharding
    os.makedirs(out_dir, exist_ok=True)
    mine = sharding.shard_indices(len(dataset), rank, world)
    items = [sharding.seeded_item(dataset, i, seed, diffuser, num_t, min_t, noise=noise) for i in mine]
    lengths = [int(it[2]["rigids_t"].shape[1]) for it in items]
    records = []
    groups = sharding.batches_mixed(lengths, max_batch) if mixed else sharding.batches_by_length(lengths, max_batch)

    def write(group, res):
        for b, p in enumerate(group):
            item, (name, sample_i) = mine[p], items[p][:2]
            n = lengths[p]  # (every per-residue output carries the residues on the axis behind the batch)
            arrays = {k: (np.asarray(res[k])[0, b, :n] if final_only else np.asarray(res[k])[:, b, :n]) for k in keep}
            if write_item is not None:  # caller-defined layout (the reference's directories for inpainting runs)
                path = write_item(int(item), name, int(sample_i), arrays, items[p][2])
            else:
                path = os.path.join(out_dir, f"sample_{item:06d}.npz")
                np.savez(path, item=item, name=str(name), sample_i=int(sample_i), **arrays)
            if collect is not None:
                f = items[p][2]
                host = lambda k: f[k][0, :n].detach().cpu().numpy() if k in f else None  # noqa: E731
                collect[int(item)] = {"prot": np.array(np.asarray(res["prot_traj"])[0, b, :n], dtype=np.float32),
                                      "diffused": (1 - host("fixed_mask")) * host("res_mask") != 0,
                                      **{k: host(k) for k in ("res_mask", "aatype", "residue_index", "chain_idx")}}
                if ground_truth is not None and int(sample_i) == 0:
                    collect[int(item)]["gt"] = np.array(ground_truth(f), dtype=np.float32)[:n]
            records.append({"item": int(item), "name": str(name), "sample_i": int(sample_i), "n_res": lengths[p],
                            "rank": rank, "file": os.path.relpath(str(path), out_dir)})

    # The trajectories of batch k leave the device (pinned buffers, a copy stream) and are written to disk while batch k + 1
    # computes: the loop enqueues k + 1 before it waits for k's copy.  (At 8 samples x T = 500 x N = 300 the copy is 1.1 GB =
    # 8 - 12 % of a batch's wall time when it is not overlapped.)  run_batch may also return NumPy arrays (no overlap then).
    pending = None  # (group, {key: pinned host tensor}, copy-done event)
    for group in groups:
        if mixed:
            feats, tape, _ = sharding.stack_items_padded([items[p] for p in group])
        else:
            feats, tape = sharding.stack_items([items[p] for p in group])
        res = run_batch(feats, tape)
        on_device = all(hasattr(res[k], "is_cuda") and res[k].is_cuda for k in keep)
        if not on_device:
            write(group, res)
            continue
        import torch
        dev = res[keep[0]].device
        with torch.cuda.device(dev):
            done = torch.cuda.Event()
            done.record()                       # batch k's kernels are enqueued up to here
            if pending is not None:             # batch k - 1: its copy ran under batch k - 1's tail / this batch's set-up
                pending[2].synchronize()
                write(pending[0], {k: v.numpy() for k, v in pending[1].items()})
            copy_stream = _copy_stream(dev)
            copy_stream.wait_event(done)
            host = {}
            with torch.cuda.stream(copy_stream):
                for k in keep:
                    src = res[k][:1] if final_only else res[k]   # (only what is written crosses PCIe)
                    src = src.contiguous()
                    src.record_stream(copy_stream)
                    host[k] = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
                    host[k].copy_(src, non_blocking=True)
                copied = torch.cuda.Event()
                copied.record(copy_stream)
            pending = (group, host, copied)
    if pending is not None:
        pending[2].synchronize()
        write(pending[0], {k: v.numpy() for k, v in pending[1].items()})
    with open(os.path.join(out_dir, f"records_rank{rank}.json"), "w") as f:
        json.dump(records, f)
    return records


_COPY_STREAMS: dict = {}


def _copy_stream(dev):
    import torch
    key = str(dev)
    if key not in _COPY_STREAMS:
        _COPY_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _COPY_STREAMS[key]


def write_manifest(out_dir: str, world: int, n_items: int, meta: dict):
    """Rank 0, after the barrier: merge the per-rank record files; raises if an item is missing."""
    recs = []
    for r in range(world):
        with open(os.path.join(out_dir, f"records_rank{r}.json")) as f:
            recs += json.load(f)
    recs.sort(key=lambda x: x["item"])
    if [x["item"] for x in recs] != list(range(n_items)):
        raise RuntimeError("sharded run is incomplete: items " + str(sorted(set(range(n_items)) - {x["item"] for x in recs})))
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump({"n_items": n_items, "world_size": world, **meta, "samples": recs}, f, indent=1)
    return recs


def group_records_by_name(records):
    """{structure name: its records in sample order} of manifest records, names in the order of their first item: the groups of
    ``--select`` (the samples of one complex)."""
    groups = {}
    for r in sorted(records, key=lambda x: x["item"]):
        groups.setdefault(str(r["name"]), []).append(r)
    return {name: sorted(rs, key=lambda x: (x["sample_i"], x["item"])) for name, rs in groups.items()}


# ---- what the rank-0 stages below share: batches of gathered entries (NumPy only) and the two file writers -------------------------

def rows_that_exist(it):
    """[n] float32: the gathered entry's res_mask, ones where it has none."""
    return np.ones(it["prot"].shape[0], dtype=np.float32) if it.get("res_mask") is None else np.asarray(it["res_mask"], dtype=np.float32)


def diffused_rows_that_exist(it):
    """[n] float32: the entry's diffused rows among those that exist."""
    return np.asarray(it["diffused"], dtype=np.float32) * rows_that_exist(it)


def padded_batch(entries, **dtypes):
    """``entries``: [(atom37 [n,37,3], gathered entry)] -> (prot [B,n_max,37,3] float32, then one [B,n_max] array of the given dtype per
    keyword in their order), every sample zero-padded to the longest.  ``diffused``: the entry's value; ``res_mask``: 1 where the entry has
    none; ``chain_idx`` and ``aatype``: rounded, 0 where the entry has none."""
    n_max = max(pos.shape[0] for pos, _ in entries)
    prot = np.zeros((len(entries), n_max, 37, 3), dtype=np.float32)
    out = {k: np.zeros((len(entries), n_max), dtype=dt) for k, dt in dtypes.items()}
    for b, (pos, it) in enumerate(entries):
        n = pos.shape[0]
        prot[b, :n] = pos
        for k, rows in out.items():
            if k == "diffused":
                rows[b, :n] = it[k]
            elif k == "res_mask":
                rows[b, :n] = 1 if it.get(k) is None else it[k]
            else:
                rows[b, :n] = 0 if it.get(k) is None else np.rint(it[k])
    return (prot, *out.values())


def records_by_length(records, gathered: dict):
    """{sample length: its records}, lengths and records in the order the records come in."""
    by_length = {}
    for r in records:
        by_length.setdefault(int(gathered[r["item"]]["prot"].shape[0]), []).append(r)
    return by_length


def stack_group(rs, gathered: dict):
    """Records of one length -> (prot [S,L,37,3] float32, the rows that exist [S,L] float32)."""
    items = [gathered[r["item"]] for r in rs]
    return np.stack([it["prot"] for it in items]).astype(np.float32), np.stack([rows_that_exist(it) for it in items])


Structure = collections.namedtuple("Structure", "g name records items truth labels structures sources")


def structures_by_name(records, gathered: dict, selected=None):
    """One ``Structure`` per name of ``group_records_by_name``: its index ``g``, its records and their gathered entries ``items``, the ground
    truth (``gt`` of the first entry that has one, else None) and, row for row, ``labels`` (the sample indices as strings), ``structures``
    (atom37 [n,37,3]) and ``sources`` (the gathered entry whose masks a row takes).  With ``selected`` (what ``run_selection`` kept) the five
    selected structures follow the samples, each with the first sample's entry as its source."""
    from . import selection
    for g, (name, rs) in enumerate(group_records_by_name(records).items()):
        items = [gathered[r["item"]] for r in rs]
        labels, structures, sources = [str(r["sample_i"]) for r in rs], [it["prot"] for it in items], list(items)
        if selected is not None:
            n = items[0]["prot"].shape[0]
            labels += list(selection.STRATEGIES)
            structures += [selection.selected_structure(selected["selection"], g, strategy, selected["prot"])[:n] for strategy in selection.STRATEGIES]
            sources += [items[0]] * len(selection.STRATEGIES)
        yield Structure(g, str(name), rs, items, next((it["gt"] for it in items if "gt" in it), None), labels, structures, sources)


def number(v):
    """A JSON value of a Python number: None for NaN."""
    return None if v != v else v


def numbers(values):
    """The JSON list of an array of floats (NumPy scalars become Python's): None for NaN."""
    return [number(v) for v in np.asarray(values).tolist()]


def cell(v):
    """A CSV cell: a float through ``repr``, nothing for None."""
    return "" if v is None else repr(v) if isinstance(v, float) else v


def write_json(out_dir: str, name: str, summary):
    with open(os.path.join(out_dir, name), "w") as f:
        json.dump(summary, f, indent=1)
    return summary


def write_csv(out_dir: str, name: str, fieldnames, rows, restval="", extrasaction="raise"):
    import csv
    with open(os.path.join(out_dir, name), "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(fieldnames), restval=restval, extrasaction=extrasaction)
        w.writeheader()
        w.writerows(rows)


def run_selection(out_dir: str, records, gathered: dict, reference_layout: bool, sigma: float = 30.0, max_iterations: int = 10000, keep=None):
    """Rank 0, after the gather (``--select``): one ``selection.select_samples`` launch for every structure of the run - the samples of
    a name form a group, shorter structures are padded with undiffused rows - then ``selection.json`` (indices, weights, status per
    structure) and, with the reference's directory layout, ``sample_<strategy>.pdb`` next to the sample each strategy builds on (where
    get_selected_sample_model_and_path puts it; b-factor 100 = diffused).  Returns the summary written to ``selection.json``; ``keep`` (a
    dict, ``--evaluate``) receives the selection and the padded batch it ran on."""
    import pathlib

    from . import output, selection
    by_name = group_records_by_name(records)
    order = [r for rs in by_name.values() for r in rs]
    prot, mask = padded_batch([(gathered[r["item"]]["prot"], gathered[r["item"]]) for r in order], diffused=np.float32)
    groups = np.array([list(by_name).index(str(r["name"])) for r in order], dtype=np.int64)
    sel = selection.select_samples(prot, mask, groups, sigma=sigma, max_iterations=max_iterations)
    if keep is not None:
        keep.update(selection=sel, prot=prot)
    summary = {"sigma": sigma, "max_iterations": max_iterations, "structures": {}}
    for g, (name, rs) in enumerate(by_name.items()):
        entry = {"items": [r["item"] for r in rs], "sample_i": [r["sample_i"] for r in rs], "n_diffused": int(len(sel["residues"][g])),
                 "status": int(sel["status"][g]), **{k: sel[k][g].tolist() for k in ("weights", "density", "dist_to_mean", "dist_to_median")},
                 "strategies": {}}
        for strategy in selection.STRATEGIES:
            rec = rs[selection.carrier(sel, g, strategy)]
            chosen = {"item": rec["item"], "sample_i": rec["sample_i"], "file": None}
            if reference_layout:
                it = gathered[rec["item"]]
                n, rm = it["prot"].shape[0], it["res_mask"].astype(bool)
                pos = selection.selected_structure(sel, g, strategy, prot)[:n]
                path = (pathlib.Path(out_dir) / rec["file"]).parent / f"sample_{strategy}.pdb"
                output.write_prot_to_pdb(pos[rm], path, overwrite=True, no_indexing=True, aatype=it["aatype"][rm],
                                         b_factors=np.tile((it["diffused"] * 100)[:, None], (1, 37))[rm],
                                         residue_index=it["residue_index"][rm], chain_index=it["chain_idx"][rm])
                chosen["file"] = os.path.relpath(str(path), out_dir)
            entry["strategies"][strategy] = chosen
        summary["structures"][name] = entry
    return write_json(out_dir, "selection.json", summary)


def run_evaluation(out_dir: str, records, gathered: dict, tcr: bool = False, selected=None):
    """Rank 0, after the gather (``--evaluate``): one ``evaluation.evaluate_samples`` launch for every sample of every structure of the
    run - and, with ``selected`` (what ``run_selection`` kept), the five selected structures of each - against the structure's ground
    truth (``gt`` of its first sample's gathered entry); shorter structures are padded with res_mask = 0 rows.  Writes
    ``evaluation.json`` (per structure the regions and per sample or strategy the scalars) and ``metrics.csv`` (one row per structure and
    sample or strategy: pdb_name, sample, the scalars, then the reference's flattened per-residue columns; a structure with a region
    shorter than 4 residues has the scalars only).  Without ground truth (de novo runs) only the CA geometry checks are reported.
    Returns the summary written to ``evaluation.json``."""
    from . import evaluation
    rows, truth = [], {}  # (structure, label, atom37 [n,37,3], gathered entry); structure -> ground truth
    for st in structures_by_name(records, gathered, selected):
        rows += [(st.name, label, pos, it) for label, pos, it in zip(st.labels, st.structures, st.sources)]
        truth[st.name] = st.truth
    names = list(truth)
    with_truth = all(t is not None for t in truth.values())
    prot, diffuse, res_mask, chain = padded_batch([row[2:] for row in rows], diffused=np.float32, res_mask=np.float32, chain_idx=np.int32)
    if with_truth:
        reference = np.zeros((len(names),) + prot.shape[1:], dtype=np.float32)
        for r, name in enumerate(names):
            reference[r, :truth[name].shape[0]] = truth[name]
        res = evaluation.evaluate_samples(prot, reference, diffuse, chain, [names.index(row[0]) for row in rows], res_mask)
        scalars = evaluation.SCALARS + ("status",)
    else:  # (no ground truth: every sample against itself, only the geometry of the sample is reported)
        res = evaluation.evaluate_samples(prot, prot, diffuse, chain, None, res_mask)
        scalars = evaluation.GEOMETRY_SCALARS
    summary = {"ground_truth": with_truth, "structures": {}}
    table, columns = [], ["pdb_name", "sample"] + list(scalars)
    for b, (name, label, _, _) in enumerate(rows):
        entry = summary["structures"].setdefault(name, {"regions": [list(r) for r in res["regions"][b]], "region_rows": [list(r) for r in res["region_rows"][b]],
                                                        "region_names": evaluation.default_region_names(len(res["regions"][b]), tcr), "samples": {}})
        values = {k: res[k][b].item() for k in scalars}
        entry["samples"][label] = {k: number(v) for k, v in values.items()}  # (NaN: no bond / no pair)
        row = {"pdb_name": name, "sample": label, **values}
        if with_truth:
            entry["samples"][label]["region_bb_rmsd"] = res["region_bb_rmsd"][b].tolist()
            try:
                row.update(evaluation.eval_columns(res, b, entry["region_names"]))
            except ValueError:  # a region shorter than 4 residues has no evaluation indices
                pass
        columns += [k for k in row if k not in columns]
        table.append(row)
    write_csv(out_dir, "metrics.csv", columns, ({k: cell(v) for k, v in row.items()} for row in table), restval="")
    return write_json(out_dir, "evaluation.json", summary)


def run_violations(out_dir: str, records, gathered: dict):
    """Rank 0, after the gather (``--violations``): one ``violations.structural_violations`` call over every sample of the run, as the
    reference scores it (``atoms="diffused"``: undiffused rows sit at the origin and count); shorter samples are padded with res_mask = 0
    rows, residue_index is the position within the sample.  Writes ``violations.json`` (per sample the scalars, the counts and the
    indices of the violating residues) and ``violations.csv`` (one row per sample: pdb_name, sample, the scalars and counts).  Returns
    the summary written to ``violations.json``."""
    from . import violations
    order = [r for rs in group_records_by_name(records).values() for r in rs]
    prot, diffuse, res_mask = padded_batch([(gathered[r["item"]]["prot"], gathered[r["item"]]) for r in order], diffused=np.float32, res_mask=np.float32)
    res = violations.structural_violations(prot, diffuse, res_mask, atoms="diffused")
    columns = violations.SCALARS + violations.COUNTS
    summary, table = {"atoms": "diffused", "samples": []}, []
    for b, r in enumerate(order):
        values = {k: res[k][b].item() for k in columns}
        summary["samples"].append({"pdb_name": r["name"], "sample": r["sample_i"], "n_res": int(gathered[r["item"]]["prot"].shape[0]),
                                   **{k: number(v) for k, v in values.items()}, "residue_violations": violations.residue_violations(res, b)})  # (NaN: no kept row)
        table.append({"pdb_name": r["name"], "sample": r["sample_i"], **{k: cell(v) for k, v in values.items()}})
    write_csv(out_dir, "violations.csv", ["pdb_name", "sample"] + list(columns), table)
    return write_json(out_dir, "violations.json", summary)


def run_lddt(out_dir: str, records, gathered: dict, inpainting: bool = False, selected=None):
    """Rank 0, after the gather (``--lddt``; framedipt_amd/lddt.py).  Inpainting runs: per structure name every sample - and, with
    ``selected`` (what ``run_selection`` kept), the five selected structures - against the ground truth (``gt`` of a gathered entry) in
    the atom sets ``ca`` and ``backbone``, score_mask = the diffused rows that exist, the context as environment.  Writes ``lddt.json``
    (per sample the flat metrics and the per-residue arrays of the diffused rows) and ``lddt.csv`` (one row per sample: pdb_name, sample,
    lddt_ca, lddt_bb, drmsd, fape, region_fape); a structure without ground truth is listed as skipped.  De novo runs: per sample length
    one all-against-all call on the CA atoms: ``pairwise_lddt_ca_length_<L>.npy`` (row = model, column = reference) and
    ``consistency.json`` with every sample's mean off-diagonal lDDT and its ``consensus`` profile.  Returns the summary written."""
    from . import lddt
    if not inpainting:
        by_length = records_by_length(sorted(records, key=lambda x: x["item"]), gathered)
        summary = {"atoms": "ca", "lengths": []}
        for length in sorted(by_length):
            rs = by_length[length]
            prot, mask = stack_group(rs, gathered)
            res = lddt.local_accuracy(prot, atoms="ca", res_mask=mask)
            np.save(os.path.join(out_dir, f"pairwise_lddt_ca_length_{length}.npy"), res["matrix"])
            summary["lengths"].append({"length": length, "samples": [
                {"pdb_name": r["name"], "sample": r["sample_i"], "mean_lddt": float(np.delete(res["matrix"][s], s).mean()) if len(rs) > 1 else None,
                 "consensus": res["consensus"][s].tolist()} for s, r in enumerate(rs)]})
        return write_json(out_dir, "consistency.json", summary)
    columns = ["lddt_ca", "lddt_bb", "drmsd", "fape", "region_fape"]
    summary, table = {"atoms": ["ca", "backbone"], "score_mask": "diffused rows", "samples": [], "skipped": []}, []
    for st in structures_by_name(records, gathered, selected):
        if st.truth is None:
            summary["skipped"].append(st.name)
            continue
        prot = np.stack(st.structures).astype(np.float32)
        res_mask = np.stack([rows_that_exist(it) for it in st.sources])
        score = np.stack([diffused_rows_that_exist(it) for it in st.sources])
        reference = np.asarray(st.truth, dtype=np.float32)[None]
        ca = lddt.local_accuracy(prot, reference, atoms="ca", res_mask=res_mask, score_mask=score)
        bb = lddt.local_accuracy(prot, reference, atoms="backbone", res_mask=res_mask, score_mask=score)
        for s, label in enumerate(st.labels):
            rows = np.flatnonzero(score[s])
            values = {**lddt.lddt_metrics(ca, s), "lddt_bb": lddt.lddt_metrics(bb, s)["lddt_bb"]}
            summary["samples"].append({"pdb_name": st.name, "sample": label, **{k: values[k] for k in columns}, "status": int(ca["status"][s] | bb["status"][s]),
                                       "rows": rows.tolist(), "res_lddt_ca": ca["res_lddt"][s][rows].tolist(), "res_lddt_bb": bb["res_lddt"][s][rows].tolist(),
                                       "res_fape": ca["res_fape"][s][rows].tolist()})
            table.append({"pdb_name": st.name, "sample": label, **{k: repr(values[k]) for k in columns}})
    write_csv(out_dir, "lddt.csv", ["pdb_name", "sample"] + columns, table)
    return write_json(out_dir, "lddt.json", summary)


def run_interface(out_dir: str, records, gathered: dict, inpainting: bool = False, selected=None, atoms: str = "cb"):
    """Rank 0, after the gather (``--interface``; framedipt_amd/interface.py).  Inpainting runs: per structure name every sample - and,
    with ``selected`` (what ``run_selection`` kept), the five selected structures - against the ground truth (``gt`` of a gathered entry)
    on ``loop_sides``: per chain with diffused rows one interface, the ligand that chain's diffused rows, the receptor every row of the
    other chains - does the redesigned loop touch its partners where the native loop does.  Writes ``interface.json`` (per sample and
    chain the flat metrics of ``interface_metrics`` and the per-row contact counts of the ligand rows) and ``interface.csv`` (one row per
    sample and chain); a structure without ground truth, without a second chain or without diffused rows is listed as skipped.  De novo
    runs have no reference complex: the flag is refused.  Returns the summary written."""
    from . import interface
    if not inpainting:
        raise SystemExit("--interface scores the samples of an inpainting run against their ground-truth complex; a de novo run has none")
    columns = ["n_native", "n_model", "n_shared", "n_interface_rows", "fnat", "fnonnat", "irmsd", "lrmsd", "dockq", "capri_class", "status"]
    summary = {"atoms": atoms, "contact_cutoff": interface.CONTACT_CUTOFF[atoms], "interface_cutoff": 10.0, "sides": "ligand: the diffused rows of a chain; receptor: the other chains",
               "contract": "DESIGN.md section 7.18 (no parity with the DockQ program is claimed)", "samples": [], "skipped": []}
    table = []
    for st in structures_by_name(records, gathered, selected):
        first = st.items[0]
        chain = np.zeros(first["prot"].shape[0]) if first.get("chain_idx") is None else np.rint(np.asarray(first["chain_idx"]))
        sides, chains = interface.loop_sides(np.asarray(first["diffused"]) != 0, chain)
        if st.truth is None or len(sides) == 0 or not (sides == interface.RECEPTOR).any():
            summary["skipped"].append(st.name)
            continue
        res_mask = np.stack([rows_that_exist(it) for it in st.sources])
        res = interface.interface_accuracy(np.stack(st.structures).astype(np.float32), np.asarray(st.truth, dtype=np.float32)[None], sides, atoms=atoms, res_mask=res_mask)
        for s, label in enumerate(st.labels):
            for k, c in enumerate(chains):
                rows = np.flatnonzero(sides[k] == interface.LIGAND)
                values = interface.interface_metrics(res, s, k)
                summary["samples"].append({"pdb_name": st.name, "sample": label, "chain": int(c), **values, "ligand_rows": rows.tolist(),
                                           **{key: res[key][s, k][rows].tolist() for key in ("res_native", "res_model", "res_shared")}})
                table.append({"pdb_name": st.name, "sample": label, "chain": int(c), **{key: cell(values[key]) for key in columns}})
    write_csv(out_dir, "interface.csv", ["pdb_name", "sample", "chain"] + columns, table)
    return write_json(out_dir, "interface.json", summary)


def write_gdt(out_dir: str, structures: dict, skipped=()):
    """``structures``: name -> {"samples": [labels], "n_scored": [S], "fixed" and "search": {"gdt_ts": [S], "gdt_ha": [S]} (no
    superposition: the frame of the fixed context; the searched superposition per cutoff), "counts_fixed" and "counts": [S,5], "status":
    [S]}.  Writes ``gdt.json`` (all of it, with the names in ``skipped``) and ``gdt.csv`` (one row per sample: pdb_name, sample,
    n_scored, gdt_ts_fixed, gdt_ha_fixed, gdt_ts, gdt_ha).  Returns the summary written to ``gdt.json``."""
    from . import gdt
    summary = {"cutoffs": list(gdt.CUTOFFS), "rows": "diffused rows that exist", "superposition": "search: DESIGN.md section 7.14 (no parity with LGA is claimed)",
               "structures": {}, "skipped": [str(n) for n in skipped]}
    table = []
    for name, e in structures.items():
        summary["structures"][name] = {"samples": list(e["samples"]), "n_scored": [int(v) for v in e["n_scored"]],
                                       "gdt_ts_fixed": numbers(e["fixed"]["gdt_ts"]), "gdt_ha_fixed": numbers(e["fixed"]["gdt_ha"]),
                                       "gdt_ts": numbers(e["search"]["gdt_ts"]), "gdt_ha": numbers(e["search"]["gdt_ha"]),
                                       "counts_fixed": np.asarray(e["counts_fixed"]).tolist(), "counts": np.asarray(e["counts"]).tolist(),
                                       "status": [int(v) for v in e["status"]]}
        table += [{"pdb_name": name, "sample": label, "n_scored": int(e["n_scored"][s]), "gdt_ts_fixed": cell(float(e["fixed"]["gdt_ts"][s])),
                   "gdt_ha_fixed": cell(float(e["fixed"]["gdt_ha"][s])), "gdt_ts": cell(float(e["search"]["gdt_ts"][s])), "gdt_ha": cell(float(e["search"]["gdt_ha"][s]))}
                  for s, label in enumerate(e["samples"])]
    write_csv(out_dir, "gdt.csv", ["pdb_name", "sample", "n_scored", "gdt_ts_fixed", "gdt_ha_fixed", "gdt_ts", "gdt_ha"], table)
    return write_json(out_dir, "gdt.json", summary)


def run_gdt(out_dir: str, records, gathered: dict, inpainting: bool = False, selected=None):
    """Rank 0, after the gather (``--gdt``; framedipt_amd/gdt.py).  Inpainting runs: per structure name every sample - and, with
    ``selected`` (what ``run_selection`` kept), the five selected structures - against the ground truth (``gt`` of a gathered entry) over
    the diffused rows that exist, without a superposition and with the searched one, then ``write_gdt``; a structure without ground
    truth is listed as skipped.  De novo runs: per sample length one all-against-all searched call:
    ``pairwise_gdt_ts_length_<L>.npy``.  Returns the summary written (de novo: {"lengths": [...]})."""
    from . import gdt
    if not inpainting:
        by_length = records_by_length(sorted(records, key=lambda x: x["item"]), gathered)
        for length in sorted(by_length):
            prot, mask = stack_group(by_length[length], gathered)
            np.save(os.path.join(out_dir, f"pairwise_gdt_ts_length_{length}.npy"), gdt.gdt_scores(prot, mask_a=mask)["matrix_ts"])
        return {"lengths": sorted(by_length)}
    structures, skipped = {}, []
    for st in structures_by_name(records, gathered, selected):
        if st.truth is None:
            skipped.append(st.name)
            continue
        prot = np.stack(st.structures).astype(np.float32)
        mask = np.stack([diffused_rows_that_exist(it) for it in st.sources])
        reference = np.asarray(st.truth, dtype=np.float32)[None]
        fixed = gdt.gdt_scores(prot, reference, mask_a=mask, superpose="none")
        search = gdt.gdt_scores(prot, reference, mask_a=mask, superpose="search")
        structures[st.name] = {"samples": st.labels, "n_scored": search["n_scored"], "fixed": fixed, "search": search, "counts_fixed": fixed["counts"],
                               "counts": search["counts"], "status": fixed["status"] | search["status"]}
    return write_gdt(out_dir, structures, skipped)


def run_secondary_structure(out_dir: str, records, gathered: dict):
    """Rank 0, after the gather (``--secondary-structure``): one ``secondary_structure.secondary_structure`` call over every sample of the
    run with its res_mask, chain_idx and aatype (a proline donates no hydrogen bond); shorter samples are padded with res_mask = 0
    rows.  Writes ``secondary_structure.json`` (per sample the C / H / E string over the rows that exist and the four fractions of the
    reference's ``calc_mdtraj_metrics``) and ``secondary_structure.csv`` (one row per sample: pdb_name, sample, n_res, the fractions, the
    string).  Returns the summary written to ``secondary_structure.json``."""
    from . import secondary_structure as sec
    order = [r for rs in group_records_by_name(records).values() for r in rs]
    prot, res_mask, chain, aatype = padded_batch([(gathered[r["item"]]["prot"], gathered[r["item"]]) for r in order],
                                                 res_mask=np.float32, chain_idx=np.int32, aatype=np.int32)
    res = sec.secondary_structure(prot, res_mask, chain, aatype)
    summary, table = {"alphabet": "C coil, H helix (alpha, 3-10, pi), E strand", "samples": []}, []
    for b, r in enumerate(order):
        values = {k: res[k][b].item() for k in sec.FRACTIONS}
        head = {"pdb_name": r["name"], "sample": r["sample_i"], "n_res": int(gathered[r["item"]]["prot"].shape[0])}
        summary["samples"].append({**head, **{k: number(v) for k, v in values.items()}, "ss": res["ss_string"][b], "status": int(res["status"][b])})  # (NaN: no row exists)
        table.append({**head, **{k: cell(v) for k, v in values.items()}, "ss": res["ss_string"][b]})
    write_csv(out_dir, "secondary_structure.csv", ["pdb_name", "sample", "n_res"] + list(sec.FRACTIONS) + ["ss"], table)
    return write_json(out_dir, "secondary_structure.json", summary)


def run_sasa(out_dir: str, records, gathered: dict, inpainting: bool = False):
    """Rank 0, after the gather (``--sasa``): one ``sasa.solvent_accessibility`` call over every sample of the run, every chain of the
    complex shielding the diffused rows (the atoms with a non-zero coordinate exist); shorter samples are padded with res_mask = 0 rows.
    The RSA denominators follow the run's aatype in inpainting runs and ALA in de novo runs.  With ground truth (inpainting: ``gt`` of a
    structure's first sample, the structure written as ``<pdb>_1.pdb``) that structure is scored in a second call and every sample
    carries the reference's eight ASA / RSA keys against it.  Writes ``sasa.json`` (per sample the diffused rows, their ASA and RSA
    and the total) and ``sasa.csv`` (one row per sample: pdb_name, sample, n_res, total, mean ASA and mean RSA over the diffused rows).
    Returns the summary written to ``sasa.json``."""
    from . import sasa
    by_name = group_records_by_name(records)
    order = [r for rs in by_name.values() for r in rs]

    def batch(entries):  # [(atom37 [n,37,3], gathered entry)] -> one padded call
        prot, res_mask, aatype = padded_batch(entries, res_mask=np.float32, aatype=np.int64)
        return sasa.solvent_accessibility(prot, None, res_mask, aatype if inpainting else np.zeros_like(aatype))

    res = batch([(gathered[r["item"]]["prot"], gathered[r["item"]]) for r in order])
    names = list(by_name)
    truth = {name: next((gathered[r["item"]] for r in rs if "gt" in gathered[r["item"]]), None) for name, rs in by_name.items()}
    with_truth = inpainting and all(t is not None for t in truth.values())
    gt = batch([(truth[name]["gt"], truth[name]) for name in names]) if with_truth else None
    summary, table = {"unit": "square Angstrom", "probe_radius": 1.40, "n_points": 100, "ground_truth": with_truth, "samples": []}, []
    for b, r in enumerate(order):
        it = gathered[r["item"]]
        n = it["prot"].shape[0]
        rows = np.flatnonzero(it["diffused"])
        asa, rsa = res["residue_sasa"][b, rows], res["rsa"][b, rows]
        head = {"pdb_name": r["name"], "sample": r["sample_i"], "n_res": int(n)}
        total = float(res["residue_sasa"][b, :n].sum())
        entry = {**head, "n_atoms": int(res["n_atoms"][b]), "total": total, "rows": rows.tolist(), "asa": numbers(asa), "rsa": numbers(rsa)}  # (NaN: a residue type without a maximal ASA)
        if with_truth:  # (the diffused rows as single-row regions: the reference's keys per residue of the diffused regions)
            metrics = sasa.sasa_metrics(gt, names.index(str(r["name"])), res, b, [(k, k) for k in rows])
            entry["metrics"] = {k: numbers(v) for k, v in metrics.items()}
        summary["samples"].append(entry)
        mean = lambda v: cell(float(np.mean(v)) if len(v) else None)  # noqa: E731
        table.append({**head, "total": cell(total), "mean_asa": mean(asa), "mean_rsa": mean(rsa)})
    write_csv(out_dir, "sasa.csv", ["pdb_name", "sample", "n_res", "total", "mean_asa", "mean_rsa"], table)
    return write_json(out_dir, "sasa.json", summary)


def write_diversity(out_dir: str, matrices: dict, tm_score_th: float = 0.5):
    """``matrices``: sample length -> TM-score matrix [S,S] of the samples of that length.  Writes ``pairwise_tm_score_fixed_length_<L>.npy``
    per length - deliberately not the reference's cache name ``pairwise_tm_score_length_<L>.npy``: the numbers are those of the row-by-row
    correspondence, not TM-align's, and must not be picked up as such - and ``diversity.json`` / ``diversity.csv`` (length, samples,
    clusters, diversity at the threshold).  Returns the summary written to ``diversity.json``."""
    from . import tm_score
    summary = {"tm_score_th": tm_score_th, "alignment": "fixed: row i with row i (a lower bound of TM-align's score)", "lengths": []}
    for length in sorted(matrices):
        matrix = np.asarray(matrices[length], dtype=np.float64)
        np.save(os.path.join(out_dir, f"pairwise_tm_score_fixed_length_{int(length)}.npy"), matrix)
        d = tm_score.diversity(matrix, tm_score_th)
        summary["lengths"].append({"length": int(length), "samples": d["samples"], "clusters": d["clusters"], "diversity": d["diversity"],
                                   "labels": d["labels"].tolist()})
    write_csv(out_dir, "diversity.csv", ["length", "samples", "clusters", "diversity"], ({**e, "diversity": cell(e["diversity"])} for e in summary["lengths"]),
              extrasaction="ignore")
    return write_json(out_dir, "diversity.json", summary)


def write_tm_table(out_dir: str, structures: dict):
    """``structures``: name -> {"samples": [labels], "tm_score": [S] against the ground truth over the diffused rows, "n_aligned": [S],
    "matrix": [S,S] among the structure's samples}.  Writes ``tm_score.json`` (all of it) and ``tm_score.csv`` (one row per sample:
    pdb_name, sample, n_aligned, tm_score).  Returns the summary written to ``tm_score.json``."""
    summary = {"alignment": "fixed: row i with row i over the diffused rows", "structures": {}}
    table = []
    for name, e in structures.items():
        summary["structures"][name] = {"samples": list(e["samples"]), "tm_score": numbers(e["tm_score"]),  # (NaN: fewer than 3 rows)
                                       "n_aligned": [int(v) for v in e["n_aligned"]],
                                       "matrix": [numbers(row) for row in np.asarray(e["matrix"], dtype=np.float64)]}
        table += [{"pdb_name": name, "sample": label, "n_aligned": int(n), "tm_score": cell(float(v))}
                  for label, n, v in zip(e["samples"], e["n_aligned"], e["tm_score"])]
    write_csv(out_dir, "tm_score.csv", ["pdb_name", "sample", "n_aligned", "tm_score"], table)
    return write_json(out_dir, "tm_score.json", summary)


def run_tm_score(out_dir: str, records, gathered: dict, inpainting: bool = False, tm_score_th: float = 0.5):
    """Rank 0, after the gather (``--tm-score``; framedipt_amd/tm_score.py).  De novo runs: one all-against-all ``tm_scores`` call per
    sample length, then ``write_diversity``.  Inpainting runs: per structure name one call of every sample against the ground truth
    (``gt`` of a gathered entry) over the diffused rows that exist, the ``tm_score`` of the reference's protein_metrics, and one
    all-against-all call among the structure's samples over the same rows, then ``write_tm_table``.  Returns the summary written."""
    from . import tm_score
    if not inpainting:
        matrices = {}
        for length, rs in records_by_length(records, gathered).items():
            prot, mask = stack_group(rs, gathered)
            matrices[length] = tm_score.tm_scores(prot, mask_a=mask)["matrix"]
        return write_diversity(out_dir, matrices, tm_score_th)
    structures = {}
    for st in structures_by_name(records, gathered):
        prot = np.stack(st.structures).astype(np.float32)
        mask = np.stack([diffused_rows_that_exist(it) for it in st.items])
        entry = {"samples": st.labels, "matrix": tm_score.tm_scores(prot, mask_a=mask)["matrix"]}
        if st.truth is not None:
            against = tm_score.tm_scores(prot, np.asarray(st.truth, dtype=np.float32)[None], mask_a=mask)
            entry.update(tm_score=against["tm"], n_aligned=against["n_aligned"])
        else:
            entry.update(tm_score=np.full(len(st.records), np.nan), n_aligned=mask.sum(1).astype(np.int64))
        structures[st.name] = entry
    return write_tm_table(out_dir, structures)


def write_diversity_aligned(out_dir: str, aligned: dict, fixed: dict, tm_score_th: float = 0.5, skipped=(), inits: str = "default"):
    """``aligned``: sample length -> matrix [S,S] of ``tm_align`` (entry (i, j) = ``tm_b``, mirrored); ``fixed``: the matrix of ``tm_scores``
    of the same samples.  Both are scores of a valid alignment under the same normalisation, so the larger is the tighter lower bound of
    the optimum: ``fmax(aligned, fixed)`` - where one of the two is NaN (a status bit), the other - is written as
    ``pairwise_tm_score_aligned_length_<L>.npy`` - still not the reference's cache name, nothing is pinned against tmtools - and
    clustered into ``diversity_aligned.json`` / ``diversity_aligned.csv``.  Per length the json records ``fixed_won``, the pairs i < j
    where the fixed correspondence scored above the search or the search gave no score, and ``nan_pairs``, the pairs without either
    score: a length with such pairs is written but not clustered (``clusters`` and ``diversity`` null).  ``skipped``: lengths beyond the
    row limit of the search; ``inits``: the search's mode (``--tm-inits``), recorded.  Returns the summary written to
    ``diversity_aligned.json``."""
    from . import tm_score
    summary = {"tm_score_th": tm_score_th, "alignment": "searched (DESIGN.md section 7.9; no parity with tmtools.tm_align is claimed), "
               "the fixed row-by-row score where it is larger", "inits": str(inits), "lengths": [], "skipped_lengths": [int(v) for v in skipped]}
    for length in sorted(aligned):
        a, f = np.asarray(aligned[length], dtype=np.float64), np.asarray(fixed[length], dtype=np.float64)
        matrix = np.fmax(a, f)
        np.save(os.path.join(out_dir, f"pairwise_tm_score_aligned_length_{int(length)}.npy"), matrix)
        entry = {"length": int(length), "samples": int(len(a)), "clusters": None, "diversity": None,
                 "fixed_won": int(np.triu((f > a) | (np.isnan(a) & ~np.isnan(f)), 1).sum()), "nan_pairs": int(np.triu(np.isnan(matrix), 1).sum()),
                 "pairs": int(len(a) * (len(a) - 1) // 2), "labels": None}
        if entry["nan_pairs"] == 0:
            d = tm_score.diversity(matrix, tm_score_th)
            entry.update(clusters=d["clusters"], diversity=d["diversity"], labels=d["labels"].tolist())
        summary["lengths"].append(entry)
    write_csv(out_dir, "diversity_aligned.csv", ["length", "samples", "clusters", "diversity", "fixed_won", "nan_pairs"],
              ({**e, "diversity": cell(e["diversity"]), "clusters": cell(e["clusters"])} for e in summary["lengths"]), extrasaction="ignore")
    return write_json(out_dir, "diversity_aligned.json", summary)


def write_tm_align_table(out_dir: str, structures: dict, skipped=None, inits: str = "default"):
    """``structures``: name -> {"samples": [labels], "rows": the most rows any sample of the structure was aligned over, "matrix": [S,S] of
    ``tm_align`` among the structure's samples over the diffused rows}; ``skipped``: name -> rows, the structures with more diffused rows
    than the search takes; ``inits``: the search's mode, recorded.  Writes ``tm_align.json``.  Returns the summary written."""
    summary = {"alignment": "searched over the diffused rows (DESIGN.md section 7.9)", "inits": str(inits), "structures": {
        name: {"samples": list(e["samples"]), "rows": int(e["rows"]), "matrix": [numbers(row) for row in np.asarray(e["matrix"], dtype=np.float64)]}  # (NaN: a status bit)
        for name, e in structures.items()}, "skipped_structures": {str(k): int(v) for k, v in (skipped or {}).items()}}
    return write_json(out_dir, "tm_align.json", summary)


def compact_rows(prot, mask):
    """prot [S,N,A,3], mask [S,N] -> (prot [S,M,A,3] float32, mask [S,M] float32): per sample the rows whose mask is set, in ascending
    order, moved to the front; M is the largest number of set rows of a sample (at least 1), the rows behind a sample's own are masked
    out.  The alignment search takes each structure over its set rows only and limits the rows of the arrays it is given, so a few
    dozen diffused rows of a complex of any size pass."""
    prot, keep = np.asarray(prot, dtype=np.float32), np.asarray(mask) != 0
    m = max(int(keep.sum(1).max()), 1)
    out, out_mask = np.zeros((prot.shape[0], m) + prot.shape[2:], dtype=np.float32), np.zeros((prot.shape[0], m), dtype=np.float32)
    for s in range(prot.shape[0]):
        k = int(keep[s].sum())
        out[s, :k], out_mask[s, :k] = prot[s, keep[s]], 1.0
    return out, out_mask


def run_tm_align(out_dir: str, records, gathered: dict, inpainting: bool = False, tm_score_th: float = 0.5, inits: str = "default"):
    """Rank 0, after the gather (``--tm-align``; framedipt_amd/tm_align.py).  De novo runs: per sample length one all-against-all
    ``tm_align`` call and one ``tm_scores`` call, then ``write_diversity_aligned``.  Inpainting runs: the aligned matrix among the samples
    of every structure name over the diffused rows that exist, ``write_tm_align_table`` (the sample-against-ground-truth number stays the
    fixed one of ``--tm-score``).  The samples go to the search compacted to their set rows (``compact_rows``): its row limit then
    applies to those rows, not to the complex.  What still exceeds it is recorded as skipped.  ``inits``: the initial alignments of the
    search (``--tm-inits``), recorded in either file.  Returns the summary written."""
    from . import tm_align, tm_score
    tm_align.check_inits(inits)
    if not inpainting:
        aligned, fixed, skipped = {}, {}, []
        for length, rs in records_by_length(records, gathered).items():
            prot, mask = stack_group(rs, gathered)
            rows, rows_mask = compact_rows(prot, mask)
            if rows.shape[1] > tm_align.MAX_ROWS:
                skipped.append(length)
                continue
            aligned[length] = tm_align.tm_align(rows, mask_a=rows_mask, inits=inits)["matrix"]
            fixed[length] = tm_score.tm_scores(prot, mask_a=mask)["matrix"]
        return write_diversity_aligned(out_dir, aligned, fixed, tm_score_th, skipped, inits)
    structures, skipped = {}, {}
    for st in structures_by_name(records, gathered):
        rows, rows_mask = compact_rows(np.stack(st.structures), np.stack([diffused_rows_that_exist(it) for it in st.items]))
        if rows.shape[1] > tm_align.MAX_ROWS:
            skipped[st.name] = rows.shape[1]
            continue
        structures[st.name] = {"samples": st.labels, "rows": rows.shape[1], "matrix": tm_align.tm_align(rows, mask_a=rows_mask, inits=inits)["matrix"]}
    return write_tm_align_table(out_dir, structures, skipped, inits)


def run_novelty(out_dir: str, records, gathered: dict, set_path, top_k: int = 1, inpainting: bool = False, inits: str = "default", accuracy: bool = False):
    """Rank 0, after the gather (``--novelty SET.npz``; framedipt_amd/structure_search.py).  De novo runs only: every final sample is
    searched in the structure set, one ``search`` call per sample length, the samples compacted to their set rows (``compact_rows``).
    The reference (evaluation/eval_denovo.py:plot_novelty) searches the ESMFold refold of a sample with foldseek; here the query is
    the sample itself and the search is this project's own (no parity with foldseek is claimed) - both are said
    in the output.  Writes ``novelty.json`` (per sample pdbTM, the hit's name, tm_t, n_aligned, the counts and with top_k > 1 every hit)
    and ``novelty.csv`` (length, sample, pdbTM, hit).  A length beyond the search's row limit is recorded as skipped.  Inpainting runs
    are refused: a redesigned loop in a fixed context is not novel by construction.  ``inits``: the initial alignments of the search
    (``--tm-inits``), recorded in ``novelty.json``.  ``accuracy`` (``--novelty-accuracy``): also lDDT-CA and GDT of every sample against
    each of its hits through the hit's alignment (``structure_search.hit_accuracy``), written to
    ``novelty_accuracy.json`` / ``.csv`` - ``novelty.json`` and ``novelty.csv`` hold what they hold without it.  Returns the summary
    written."""
    if inpainting:
        raise ValueError("--novelty is for de novo runs: a redesigned region inside a fixed context is not novel by construction")
    from . import structure_search
    db = structure_search.StructureSet.load(set_path)
    samples, skipped, accurate = [], [], []
    for length, rs in records_by_length(records, gathered).items():
        rows, rows_mask = compact_rows(*stack_group(rs, gathered))
        if rows.shape[1] > structure_search.MAX_ROWS:
            skipped.append(length)
            continue
        res = structure_search.search(rows, db, mask=rows_mask, top_k=top_k, inits=inits)
        if accuracy:
            acc = structure_search.hit_accuracy(res, rows, db, mask=rows_mask)
            accurate += [{"length": length, "sample": r["sample_i"], "rank": j, "hit": res["names"][q][j], **structure_search.hit_accuracy_metrics(acc, q, j)}
                         for q, r in enumerate(rs) for j in range(top_k) if res["hit"][q, j] >= 0]
        for q, r in enumerate(rs):
            entry = {"length": length, "sample": r["sample_i"], **structure_search.novelty_metrics(res, q),
                     **{k: int(res[k][q]) for k in ("n_scored", "n_pruned", "n_skipped")}}
            if top_k > 1:
                entry["hits"] = [{"hit": res["names"][q][j], "tm_q": float(res["tm_q"][q, j]), "tm_t": float(res["tm_t"][q, j]),
                                  "n_aligned": int(res["n_aligned"][q, j])} for j in range(top_k) if res["hit"][q, j] >= 0]
            samples.append(entry)
    summary = {"set": str(set_path), "entries": len(db), "top_k": int(top_k), "inits": str(inits),
               "query": "the sample itself (the reference searches the ESMFold refold of a sample)",
               "search": "the alignment search of DESIGN.md sections 7.9 and 7.15, pdbTM normalised by the sample's rows; no parity with foldseek is claimed",
               "samples": samples, "skipped_lengths": sorted(skipped)}
    write_csv(out_dir, "novelty.csv", ["length", "sample", "pdbTM", "hit"],
              ({"length": e["length"], "sample": e["sample"], "pdbTM": repr(e["pdbTM"]), "hit": e["hit"]} for e in samples))
    if accuracy:
        write_json(out_dir, "novelty_accuracy.json", {"set": str(set_path), "top_k": int(top_k), "atoms": "ca", "coverage": "penalise", "superpose": "search",
                                                      "reference": "the hit: lDDT charges the hit's rows the sample has no partner for, GDT is divided by the hit's rows",
                                                      "hits": accurate})
        write_csv(out_dir, "novelty_accuracy.csv", ["length", "sample", "rank", "hit", "lddt_ca", "gdt_ts", "gdt_ha", "n_covered", "n_reference"],
                  ({**e, **{k: repr(e[k]) for k in ("lddt_ca", "gdt_ts", "gdt_ha")}} for e in accurate), extrasaction="ignore")
    return write_json(out_dir, "novelty.json", summary)


def run_design(out_dir: str, records, gathered: dict, inpainting: bool = False, seq_per_sample: int = 8, weights=None, temperature: float = 0.1,
               seed: int = 38, max_batch: int = 16, omit_aas: str = "X", ca_only: bool = False):
    """Rank 0, after the gather (``--design``; framedipt_amd/inverse_folding.py): ``seq_per_sample`` ProteinMPNN sequences per sample at the
    reference's settings (``--sampling_temp 0.1 --seed 38``, X omitted), what experiments/inference.py:run_protein_mpnn starts a subprocess
    for.  De novo runs design every row; inpainting runs design the diffused rows with the context fixed to its true residue types.
    Samples of one length share a call.  ``weights``: a checkpoint in the reference's layout, or None for SYNTHETIC parameters (stated in
    the output: such sequences exercise the path and mean nothing).  Writes ``seqs/<sample>.fa`` in the reference's FASTA layout and
    ``design.json``.  ``omit_aas`` (``--omit-aas``): the letters never drawn.  Inpainting runs add ``native_conditional_score`` per sample:
    the mean negative conditional log-probability (``conditional_probs``: every other letter given) of the TRUE letters of the diffused
    rows on the sampled backbone.  ``ca_only`` (``--ca-only``): the CA-only model (``weights`` must then be a CA
    checkpoint), which reads the CA trace of the samples alone; the same files, the FASTA header says ``CA_model_name=``.  Returns the
    summary written."""
    from . import inverse_folding
    model = inverse_folding.ProteinMPNN(ca_only=ca_only)
    model = model.load_checkpoint(weights) if weights else model.load_synthetic(0)
    os.makedirs(os.path.join(out_dir, "seqs"), exist_ok=True)
    samples = {}
    for length, rs in records_by_length(records, gathered).items():
        for start in range(0, len(rs), max_batch):
            chunk = rs[start:start + max_batch]
            items = [gathered[r["item"]] for r in chunk]
            rows = lambda k, default: np.stack([default if it.get(k) is None else it[k] for it in items])  # noqa: E731
            res = model.design(np.stack([it["prot"] for it in items]).astype(np.float32), num_seq=seq_per_sample, temperature=temperature, seed=seed,
                               res_mask=rows("res_mask", np.ones(length, np.float32)),
                               chain_mask=np.stack([it["diffused"] for it in items]).astype(np.float32) if inpainting else None,
                               aatype=np.clip(rows("aatype", np.full(length, 20)), 0, 20) if inpainting else None,
                               residue_index=rows("residue_index", np.arange(length)), chain_idx=rows("chain_idx", np.ones(length)), omit=omit_aas)
            native = None
            if inpainting:
                cond = model.conditional_probs(np.stack([it["prot"] for it in items]).astype(np.float32), res["S_input"], res_mask=res["res_mask"],
                                               chain_mask=res["chain_mask"], residue_index=rows("residue_index", np.arange(length)),
                                               chain_idx=rows("chain_idx", np.ones(length)), seed=seed)
                native = inverse_folding.native_scores(cond["log_probs"], res["S_input"], res["chain_mask"] * res["res_mask"])
            for b, r in enumerate(chunk):
                stem = os.path.splitext(r["file"])[0].replace(os.sep, "_")
                fasta = os.path.join("seqs", stem + ".fa")
                with open(os.path.join(out_dir, fasta), "w") as f:
                    f.write(inverse_folding.fasta_records(res, b, stem, model_name=os.path.basename(str(weights)) if weights else "synthetic"))
                samples[stem] = {"item": r["item"], "name": r["name"], "sample_i": r["sample_i"], "n_res": length,
                                 "designed_rows": int((res["chain_mask"][b] * res["res_mask"][b]).sum()), "sequences": res["sequences"][b],
                                 "score": [float(v) for v in res["score"][b]], "global_score": [float(v) for v in res["global_score"][b]],
                                 "seq_recovery": numbers(res["seq_recovery"][b]), "status": int(res["status"][b]),
                                 "fasta": fasta}
                if native is not None:
                    samples[stem]["native_conditional_score"] = float(native[b])
                gathered[r["item"]]["designed_sequences"] = list(res["sequences"][b])  # what --seq-diversity compares
    summary = {"weights": model.source, "synthetic": not weights, "ca_only": model.ca_only, "k_neighbors": model.k_neighbors, "temperature": temperature, "seed": seed,
               "seq_per_sample": seq_per_sample, "omit": omit_aas, "samples": samples}
    return write_json(out_dir, "design.json", summary)


def write_seq_diversity(out_dir: str, owners, matrix, scoring: dict, matrix_file: str = "pairwise_seq_identity.npy"):
    """``pairwise_seq_identity.npy`` (``matrix`` [Q,Q]: ``identity_short`` of every pair of designed sequences, unit diagonal) and
    ``seq_diversity.json``: ``owners`` [(sample stem, index among the sample's sequences)] in the matrix's order, the mean off-diagonal
    identity, per sample the largest identity of one of its sequences to a sequence of ANOTHER sample (None for a lone sample), and the
    scoring parameters.  ``matrix_file``: the matrix file's name (``run_seq_diversity`` names the mode in it unless it is global).  Returns
    the summary written."""
    matrix = np.asarray(matrix, dtype=np.float64)
    q = len(owners)
    stems = [o[0] for o in owners]
    other = np.array([[a != b for b in stems] for a in stems], dtype=bool).reshape(q, q)
    nearest = {}
    for stem in dict.fromkeys(stems):
        rows = np.array([o == stem for o in stems])
        block = matrix[rows][:, ~rows]
        nearest[stem] = float(block.max()) if block.size else None
    off = ~np.eye(q, dtype=bool)
    summary = {"n_sequences": q, "sequences": [{"sample": stem, "index": int(k)} for stem, k in owners],
               "mean_identity": float(matrix[off].mean()) if q > 1 else None,
               "mean_identity_between_samples": float(matrix[other].mean()) if other.any() else None,
               "max_identity_to_other_sample": nearest, "identity": "n_identical / min(len_a, len_b)", "scoring": scoring,
               "matrix": matrix_file}
    np.save(os.path.join(out_dir, matrix_file), matrix)
    return write_json(out_dir, "seq_diversity.json", summary)


def run_seq_diversity(out_dir: str, records, gathered: dict, matrix="blosum62", open_gap: float = -10.0, extend_gap: float = -0.5, mode: str = "global"):
    """Rank 0, after ``run_design`` (``--design --seq-diversity``, de novo runs; framedipt_amd/seq_align.py): every designed sequence of
    every sample (``designed_sequences`` of the gathered entries, which ``run_design`` leaves there) against every other in ONE
    score-only launch of the alignment - the lengths may differ - then ``write_seq_diversity``.  ``mode`` (``--seq-align-mode``): "global",
    or "local" / "semiglobal" (every end gap free) for sequences that share a motif or overlap; these write
    ``pairwise_seq_identity_<mode>.npy`` and leave the global file alone."""
    from . import seq_align
    owners, seqs = [], []
    for r in records:
        stem = os.path.splitext(r["file"])[0].replace(os.sep, "_")
        for k, seq in enumerate(gathered[r["item"]].get("designed_sequences") or ()):
            owners.append((stem, k))
            seqs.append(seq)
    if not seqs:
        raise ValueError("--seq-diversity needs designed sequences: run_design has left none on the gathered entries")
    found = seq_align.align_sequences(seqs, matrix=matrix, open_gap=open_gap, extend_gap=extend_gap, traceback=False, mode=mode)
    scoring = {"matrix": matrix if isinstance(matrix, str) else "custom", "open_gap": float(open_gap), "extend_gap": float(extend_gap), "mode": mode}
    if mode == "global":
        return write_seq_diversity(out_dir, owners, found["matrix"], scoring)
    if mode == "semiglobal":
        scoring["free_ends"] = "all"
    return write_seq_diversity(out_dir, owners, found["matrix"], scoring, matrix_file=f"pairwise_seq_identity_{mode}.npy")


def reference_layout_writer(out_dir: str, net, final_only: bool):
    """``write_item`` for inpainting runs: what ``Inference.run_conditional_sampling`` leaves on disk per sample
    (experiments/inference.py:250-389): ``<pdb>_length_<L>/`` with the ground-truth structure ``<pdb>_1.pdb`` (b-factor 100 = diffused) and
    ``diffusion_info.csv`` — written once per structure, by whichever rank gets there first: the content does not depend on the rank, the
    file appears atomically — and ``sample_<i>/sample_<i>_1.pdb`` (+ ``bb_traj_<i>_1.pdb`` / ``x0_traj_<i>_1.pdb`` with the trajectories kept)."""
    import pathlib
    import tempfile

    from . import inference, output

    def once(path: pathlib.Path, make):
        if path.exists():
            return
        tmp = pathlib.Path(tempfile.mkdtemp(dir=path.parent, prefix=".tmp_"))
        try:
            made = make(tmp)
            os.replace(made, path)
        finally:
            for f in tmp.iterdir():
                f.unlink()
            tmp.rmdir()

    def write_item(item, name, sample_i, arrays, feats):
        host = lambda k: feats[k][0].detach().cpu().numpy()  # noqa: E731
        res_mask, fixed = host("res_mask").astype(bool), host("fixed_mask").astype(bool)
        diffused = (1 - fixed) * res_mask
        aatype, residue_index, chain_index = host("aatype"), host("residue_index"), host("chain_idx")
        length_dir = pathlib.Path(out_dir) / f"{name}_length_{int(res_mask.sum() - (fixed * res_mask).sum())}"
        length_dir.mkdir(parents=True, exist_ok=True)
        kw = dict(aatype=aatype[res_mask], residue_index=residue_index[res_mask], chain_index=chain_index[res_mask])

        def gt(tmp):
            pos = inference.get_atom_positions_from_rigids(net, feats["rigids_0"], feats["torsion_angles_sin_cos"][..., 2, :], feats["aatype"])[0]
            b_factors = np.tile((diffused.astype(bool) * 100)[:, None], (1, 37))
            return output.write_prot_to_pdb(pos[res_mask], tmp / str(name), b_factors=b_factors[res_mask], overwrite=True, **kw)

        once(length_dir / f"{name}_1.pdb", gt)

        def info(tmp):
            output.save_diffusion_info(tmp, str(name), output.aatype_to_seq(aatype[res_mask]), diffused[res_mask], chain_index[res_mask])
            return tmp / "diffusion_info.csv"

        once(length_dir / "diffusion_info.csv", info)
        sample_dir = length_dir / f"sample_{sample_i}"
        sample_dir.mkdir(parents=True, exist_ok=True)
        for old in sample_dir.glob("*.pdb"):  # (a re-run replaces the sample: write_prot_to_pdb would otherwise number a second file)
            old.unlink()
        prot, x0 = arrays["prot_traj"], arrays.get("rigid_0_traj")
        n = prot.shape[-3]
        if final_only:  # [N,37,3]: the sample only
            prot, x0 = prot[None], None
        paths = output.save_traj(prot[:, res_mask[:n]], x0[:, res_mask[:n]] if x0 is not None else prot[:, res_mask[:n]],
                                 diffused[res_mask], sample_dir, sample_i, save_backbone_trajectory=not final_only,
                                 save_pred_x0_trajectory=not final_only and x0 is not None, **kw)
        return paths["sample_path"]

    return write_item


def parse_args(argv=None):
    """The command line (``argv``: the arguments, default ``sys.argv[1:]``) -> the namespace ``main()`` runs on; what the flags exclude among
    each other is refused here, before anything is loaded."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--min-length", type=int, default=300)
    ap.add_argument("--max-length", type=int, default=300)
    ap.add_argument("--length-step", type=int, default=1)
    ap.add_argument("--samples-per-length", type=int, default=8)
    ap.add_argument("--num-t", type=int, default=500)
    ap.add_argument("--min-t", type=float, default=0.01)
    ap.add_argument("--noise-scale", type=float, default=0.1)
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--precision", default="fp16", choices=["fp16", "fp16x", "fp32"])
    ap.add_argument("--kernel-flags", type=int, default=0, help="FdiptDims.kernel_flags (_lib.KF_*); 1024 = KF_STREAM_ATTN: fp16 chains up to 2048")
    ap.add_argument("--seed", type=int, default=123)
    ap.add_argument("--noise", default="host", choices=["host", "device"], help="host: the reference's np.random stream, a tape per sample; "
                    "device: the reverse-step kernel draws from the per-sample key seed + item (x_T still comes from np.random)")
    ap.add_argument("--weights-seed", type=int, default=7, help="synthetic weights (no checkpoint is available offline)")
    ap.add_argument("--full-trajectory", action="store_true", help="store every step of prot_traj instead of the final sample")
    ap.add_argument("--keep", default="all", help="inference_fn(keep=...): all (default: every step's frames are built and held on the device), "
                    "last (only the final structure: what a run without --full-trajectory writes anyway) or an integer stride; with "
                    "--full-trajectory the writers receive the kept frames only")
    # inpainting runs (experiments/inference.py:244-389)
    ap.add_argument("--download-dir", default=None, help="inpainting: the reference's data.download_dir (cifs/ and / or processed/metadata.csv)")
    ap.add_argument("--csv", default=None, help="inpainting: the reference's data.data_path (database CSV with a pdb_id column; TCR chain columns with --tcr)")
    ap.add_argument("--tcr", action="store_true", help="TCRSampler: CDR loops are redesigned (masks from the processed features)")
    ap.add_argument("--samples-per-structure", type=int, default=5)
    ap.add_argument("--redact-min-len", type=int, default=8)
    ap.add_argument("--redact-max-len", type=int, default=14)
    ap.add_argument("--no-input-aatype", action="store_true", help="inference.input_aatype = False (default True: backbone atoms are built with the true residue types)")
    ap.add_argument("--allow-shared-gpu", action="store_true", help="run although another compute process holds queues on this rank's GPU "
                    "(refused by default: kernels of two processes on one GPU can corrupt each other's results, DESIGN.md section 6)")
    ap.add_argument("--select", action="store_true", help="after the run, rank 0 forms the reference's five selected structures (mean, median, mode, "
                    "mean_closest, median_closest: framedipt_amd/selection.py) from the samples of every structure on its GPU: selection.json, "
                    "and sample_<strategy>.pdb files in inpainting runs")
    ap.add_argument("--select-sigma", type=float, default=30.0, help="--select: std of the density kernel (reference default)")
    ap.add_argument("--select-iterations", type=int, default=10000, help="--select: Weiszfeld iterations (reference default)")
    ap.add_argument("--evaluate", action="store_true", help="after the run, rank 0 evaluates every sample (and with --select the five selected structures) "
                    "against the ground truth of its structure on its GPU (framedipt_amd/evaluation.py): evaluation.json and metrics.csv; "
                    "de novo runs have no ground truth and report the CA geometry checks only")
    ap.add_argument("--violations", action="store_true", help="after the run, rank 0 scores the structural violations of every sample on its GPU "
                    "(framedipt_amd/violations.py: C-N bond, CA-C-N and C-N-CA angle, clash and within-residue terms of the reference's "
                    "violation metrics, radius of gyration): violations.json and violations.csv")
    ap.add_argument("--secondary-structure", action="store_true", help="after the run, rank 0 assigns the secondary structure of every sample on its GPU "
                    "(framedipt_amd/secondary_structure.py: hydrogen-bond patterns of Kabsch & Sander in the alphabet C / H / E, the coil, helix and "
                    "strand fractions of the reference's metric tables): secondary_structure.json and secondary_structure.csv")
    ap.add_argument("--sasa", action="store_true", help="after the run, rank 0 computes the solvent accessibility of every sample on its GPU "
                    "(framedipt_amd/sasa.py: Shrake-Rupley ASA per residue of the diffused rows with the whole complex as context, and RSA, "
                    "the ASA / RSA block of the reference's metric table): sasa.json and sasa.csv; inpainting runs score the ground truth too")
    ap.add_argument("--tm-score", action="store_true", help="after the run, rank 0 computes TM-scores on its GPU (framedipt_amd/tm_score.py: the score of the "
                    "row-by-row correspondence, not TM-align's alignment search).  De novo runs: all-against-all per sample length, Ward clusters and "
                    "diversity = clusters / samples: pairwise_tm_score_fixed_length_<L>.npy, diversity.json, diversity.csv.  Inpainting runs: every sample "
                    "against the ground truth over the diffused rows and the matrix per structure: tm_score.json, tm_score.csv")
    ap.add_argument("--tm-align", action="store_true", help="after the run, rank 0 searches structural alignments on its GPU (framedipt_amd/tm_align.py: "
                    "a TM-align style search, this project's own contract; no parity with tmtools is claimed).  De novo runs: all-against-all per sample "
                    "length, the larger of the searched and the fixed score: pairwise_tm_score_aligned_length_<L>.npy, diversity_aligned.json, "
                    "diversity_aligned.csv.  Inpainting runs: the aligned matrix per structure: tm_align.json")
    ap.add_argument("--lddt", action="store_true", help="after the run, rank 0 computes the superposition-free accuracy scores on its GPU (framedipt_amd/lddt.py: "
                    "lDDT, dRMSD and backbone FAPE).  Inpainting runs: every sample (and with --select the five selected structures) against the ground "
                    "truth on the CA and the backbone atoms, scored over the diffused rows with the context as environment: lddt.json and lddt.csv.  "
                    "De novo runs: all-against-all CA lDDT per sample length: pairwise_lddt_ca_length_<L>.npy and consistency.json (per sample the mean "
                    "lDDT against the others and the per-residue consensus)")
    ap.add_argument("--interface", action="store_true", help="after the run, rank 0 computes the interface accuracy on its GPU (framedipt_amd/interface.py: contacts, "
                    "fnat, fnonnat, iRMSD, LRMSD, DockQ; DESIGN.md section 7.18, no parity with the DockQ program is claimed).  Inpainting runs: every sample - and "
                    "with --select the five selected structures - against the ground truth, the ligand the diffused rows of a chain, the receptor the other "
                    "chains: interface.json and interface.csv.  De novo runs have no reference complex: the flag is refused")
    ap.add_argument("--interface-atoms", default="cb", choices=["ca", "cb", "backbone", "all"], help="the atom set of --interface (default cb: CB within 8 A, CA where "
                    "a row has no CB; backbone and all: 5 A)")
    ap.add_argument("--gdt", action="store_true", help="after the run, rank 0 computes GDT-TS and GDT-HA on its GPU (framedipt_amd/gdt.py).  Inpainting runs: every "
                    "sample (and with --select the five selected structures) against the ground truth over the diffused rows that exist, without a "
                    "superposition (the frame of the fixed context) and with the searched one: gdt.json and gdt.csv.  De novo runs: all-against-all searched "
                    "GDT-TS per sample length: pairwise_gdt_ts_length_<L>.npy")
    ap.add_argument("--design", action="store_true", help="after the run, rank 0 designs sequences for every sample on its GPU (framedipt_amd/inverse_folding.py: "
                    "ProteinMPNN at T = 0.1, seed 38, X omitted, as the reference's run_protein_mpnn): seqs/<sample>.fa and design.json.  De novo runs design "
                    "every row, inpainting runs the diffused rows with the context fixed")
    ap.add_argument("--seq-per-sample", type=int, default=8, help="--design: sequences per sample (the reference's inference.samples.seq_per_sample)")
    ap.add_argument("--omit-aas", default="X", help="--design: the letters never drawn (ProteinMPNN's --omit_AAs)")
    ap.add_argument("--ca-only", action="store_true", help="--design: the CA-only ProteinMPNN (reads the CA trace alone; --mpnn-weights must then be a CA checkpoint)")
    ap.add_argument("--mpnn-weights", default=None, help="--design: a ProteinMPNN checkpoint (.pt with model_state_dict, num_edges, noise_level); default: "
                    "SYNTHETIC parameters, stated as such in the output")
    ap.add_argument("--seq-diversity", action="store_true", help="--design, de novo runs: rank 0 then aligns all designed sequences of all samples all-against-all on "
                    "its GPU (framedipt_amd/seq_align.py: global alignment, BLOSUM62, open -10, extend -0.5, score only) and writes pairwise_seq_identity.npy "
                    "and seq_diversity.json")
    ap.add_argument("--seq-align-mode", default="global", choices=("global", "local", "semiglobal"), help="--seq-diversity: the alignment mode; local (the best "
                    "shared stretch) and semiglobal (every end gap free: overlaps) write pairwise_seq_identity_<mode>.npy and record the mode in seq_diversity.json")
    ap.add_argument("--novelty", default=None, metavar="SET.npz", help="de novo runs: after the run, rank 0 searches every final sample in the structure set "
                    "(framedipt_amd/structure_search.py: StructureSet.save) on its GPU and keeps the largest TM-score of the hits, the reference's pdbTM: "
                    "novelty.json, novelty.csv.  The query is the sample itself, not an ESMFold refold, and the search is this project's own: no parity "
                    "with foldseek is claimed.  Refused in inpainting runs")
    ap.add_argument("--tm-inits", choices=("default", "all"), default="default", help="--tm-align and --novelty: the initial alignments of the search; "
                    "all adds a local-superposition and a fragment-threading start (DESIGN.md section 7.9), for pairs that share a motif the three "
                    "default ones cannot see; recorded in diversity_aligned.json, tm_align.json and novelty.json")
    ap.add_argument("--novelty-top-k", type=int, default=1, help="--novelty: hits kept per sample (1 .. 64)")
    ap.add_argument("--novelty-accuracy", action="store_true", help="--novelty: also lDDT-CA and GDT-TS / GDT-HA of every sample against each of its hits, "
                    "through the hit's alignment -> novelty_accuracy.json, novelty_accuracy.csv (novelty.json and novelty.csv do not change)")
    ap.add_argument("--tm-score-th", type=float, default=0.5, help="--tm-score, --tm-align: the TM-score threshold of the clusters (reference default)")
    ap.add_argument("--verify", type=int, default=0, help="inference_fn(verify=k): the forward of every k-th step runs twice and must reproduce its bits")
    a = ap.parse_args(argv)
    if a.keep not in ("all", "last"):
        try:
            a.keep = int(a.keep)
        except ValueError:
            ap.error(f"--keep {a.keep}: expected all, last or an integer stride")
    if a.novelty and a.download_dir is not None:
        ap.error("--novelty is for de novo runs: a redesigned region inside a fixed context is not novel by construction")
    if a.interface and a.download_dir is None:
        ap.error("--interface scores the samples of an inpainting run against their ground-truth complex: a de novo run has none (give --download-dir)")
    if a.novelty_accuracy and not a.novelty:
        ap.error("--novelty-accuracy needs --novelty SET.npz")
    if a.seq_diversity and (not a.design or a.download_dir is not None):
        ap.error("--seq-diversity compares the designed sequences of a de novo run: it needs --design and no --download-dir")
    if a.seq_align_mode != "global" and not a.seq_diversity:
        ap.error("--seq-align-mode is the mode of --seq-diversity")
    if a.novelty and not 1 <= a.novelty_top_k <= 64:
        ap.error(f"--novelty-top-k {a.novelty_top_k}: expected 1 .. 64")
    return a


# The rank-0 stages that follow a run, in the order they run; ``main()`` knows a stage by its row alone.  ``flag``: the namespace attribute
# that switches it on.  ``run(a, records, gathered, inp, selected)``: the call of its ``run_*`` (``inp``: an inpainting run; ``selected``: what
# ``run_selection`` keeps for the stages that score the selected structures, None where nothing is kept) -> its summary.  ``ground_truth``:
# in inpainting runs it needs the ground-truth atom37 of every structure (``gt`` of the gathered entries).  ``selected``: it scores the
# selected structures.  ``report(a, done, inp, s)``: the line printed after it, ``s`` its seconds.
Stage = collections.namedtuple("Stage", "flag run ground_truth selected report")
STAGES = (
    Stage("select", lambda a, recs, g, inp, sel: run_selection(a.out_dir, recs, g, reference_layout=inp, sigma=a.select_sigma, max_iterations=a.select_iterations, keep=sel),
          False, False, lambda a, done, inp, s: f"selected structures of {len(done['structures'])} structure(s) in {s:.2f} s -> {a.out_dir}/selection.json"),
    Stage("evaluate", lambda a, recs, g, inp, sel: run_evaluation(a.out_dir, recs, g, tcr=a.tcr, selected=sel if inp else None),
          True, True, lambda a, done, inp, s: f"evaluated {sum(len(e['samples']) for e in done['structures'].values())} structure(s) in {s:.2f} s -> "
                                              f"{a.out_dir}/evaluation.json, metrics.csv"),
    Stage("violations", lambda a, recs, g, inp, sel: run_violations(a.out_dir, recs, g),
          False, False, lambda a, done, inp, s: f"structural violations of {len(done['samples'])} sample(s) in {s:.2f} s -> {a.out_dir}/violations.json, violations.csv"),
    Stage("secondary_structure", lambda a, recs, g, inp, sel: run_secondary_structure(a.out_dir, recs, g),
          False, False, lambda a, done, inp, s: f"secondary structure of {len(done['samples'])} sample(s) in {s:.2f} s -> "
                                                f"{a.out_dir}/secondary_structure.json, secondary_structure.csv"),
    Stage("sasa", lambda a, recs, g, inp, sel: run_sasa(a.out_dir, recs, g, inpainting=inp),
          True, False, lambda a, done, inp, s: f"solvent accessibility of {len(done['samples'])} sample(s) in {s:.2f} s -> {a.out_dir}/sasa.json, sasa.csv"),
    Stage("tm_score", lambda a, recs, g, inp, sel: run_tm_score(a.out_dir, recs, g, inpainting=inp, tm_score_th=a.tm_score_th),
          True, False, lambda a, done, inp, s: "TM-scores of " + (
              f"{len(done['structures'])} structure(s) -> {a.out_dir}/tm_score.json, tm_score.csv" if inp else
              f"{len(done['lengths'])} length(s) -> {a.out_dir}/diversity.json, diversity.csv, pairwise_tm_score_fixed_length_<L>.npy") + f" in {s:.2f} s"),
    Stage("tm_align", lambda a, recs, g, inp, sel: run_tm_align(a.out_dir, recs, g, inpainting=inp, tm_score_th=a.tm_score_th, inits=a.tm_inits),
          False, False, lambda a, done, inp, s: "structural alignments of " + (
              f"{len(done['structures'])} structure(s) -> {a.out_dir}/tm_align.json" if inp else
              f"{len(done['lengths'])} length(s) -> {a.out_dir}/diversity_aligned.json, diversity_aligned.csv, pairwise_tm_score_aligned_length_<L>.npy") + f" in {s:.2f} s"),
    Stage("lddt", lambda a, recs, g, inp, sel: run_lddt(a.out_dir, recs, g, inpainting=inp, selected=sel if inp else None),
          True, True, lambda a, done, inp, s: "lDDT, dRMSD and FAPE of " + (
              f"{len(done['samples'])} structure(s) -> {a.out_dir}/lddt.json, lddt.csv" if inp else
              f"{len(done['lengths'])} length(s) -> {a.out_dir}/consistency.json, pairwise_lddt_ca_length_<L>.npy") + f" in {s:.2f} s"),
    Stage("gdt", lambda a, recs, g, inp, sel: run_gdt(a.out_dir, recs, g, inpainting=inp, selected=sel if inp else None),
          True, True, lambda a, done, inp, s: "GDT-TS and GDT-HA of " + (
              f"{len(done['structures'])} structure(s) -> {a.out_dir}/gdt.json, gdt.csv" if inp else
              f"{len(done['lengths'])} length(s) -> {a.out_dir}/pairwise_gdt_ts_length_<L>.npy") + f" in {s:.2f} s"),
    Stage("interface", lambda a, recs, g, inp, sel: run_interface(a.out_dir, recs, g, inpainting=inp, selected=sel, atoms=a.interface_atoms),
          True, True, lambda a, done, inp, s: f"interface accuracy of {len(done['samples'])} (structure, chain) entr(ies) in {s:.2f} s -> "
                                              f"{a.out_dir}/interface.json, interface.csv"),
    Stage("novelty", lambda a, recs, g, inp, sel: run_novelty(a.out_dir, recs, g, a.novelty, top_k=a.novelty_top_k, inpainting=inp, inits=a.tm_inits,
                                                              accuracy=a.novelty_accuracy),
          False, False, lambda a, done, inp, s: f"novelty of {len(done['samples'])} sample(s) against {done['entries']} structure(s) in {s:.2f} s -> "
                                                f"{a.out_dir}/novelty.json, novelty.csv"),
    Stage("design", lambda a, recs, g, inp, sel: run_design(a.out_dir, recs, g, inpainting=inp, seq_per_sample=a.seq_per_sample, weights=a.mpnn_weights,
                                                             omit_aas=a.omit_aas, ca_only=a.ca_only),
          False, False, lambda a, done, inp, s: f"{a.seq_per_sample} sequence(s) for each of {len(done['samples'])} sample(s) with {'SYNTHETIC ' if done['synthetic'] else ''}"
                                                f"{'CA-only ' if done['ca_only'] else ''}ProteinMPNN parameters{'' if done['synthetic'] else ' of ' + str(done['weights'])} "
                                                f"in {s:.2f} s -> {a.out_dir}/seqs/<sample>.fa, design.json"),
    # (after the design, whose sequences it compares: parse_args refuses the flag without --design)
    Stage("seq_diversity", lambda a, recs, g, inp, sel: run_seq_diversity(a.out_dir, recs, g, mode=a.seq_align_mode),
          False, False, lambda a, done, inp, s: f"sequence identity of {done['n_sequences']} designed sequence(s), all against all, in {s:.2f} s -> "
                                                f"{a.out_dir}/{done['matrix']}, seq_diversity.json"),
)

Plan = collections.namedtuple("Plan", "stages collect ground_truth keep_selection")


def stage_plan(a, inp: bool) -> Plan:
    """What ``main()`` does after the sampling, from the namespace alone: the stages that are switched on, in their order; ``collect``: the
    ranks keep their samples on the host and gather them on rank 0 (a stage runs); ``ground_truth``: run_rank builds the ground-truth
    atom37 of every structure (an inpainting run with a stage that scores against it); ``keep_selection``: ``run_selection`` keeps its result
    (``--select`` with a stage that scores the selected structures)."""
    stages = tuple(s for s in STAGES if getattr(a, s.flag))
    return Plan(stages, bool(stages), bool(inp) and any(s.ground_truth for s in stages), bool(a.select) and any(s.selected for s in stages))


def main():
    a = parse_args()

    import torch
    import torch.distributed as dist

    from . import config, inference
    from .diffusion import SE3Diffuser
    from .model import ScoreNetwork
    from .sampler import UnconditionalSampler

    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    # FDIPT_ONE_GPU=1 (tests only): all ranks share GPU 0 and rendezvous over gloo — the multi-rank path on a one-GPU box, where
    # RCCL refuses two ranks on one device
    one_gpu = os.environ.get("FDIPT_ONE_GPU") == "1"
    if one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = f"cuda:{local_rank}"
    # one process per GPU is the contract: refuse a GPU that another compute process is using (the one-GPU test hook shares it on
    # purpose and serialises its ranks with a file lock below).  BEFORE the rendezvous: a refusing rank then never joins the group and
    # the launcher tears the job down, instead of the other ranks waiting in the final barrier for its time-out (round-5 advisor)
    from . import gpu_guard
    if one_gpu or a.allow_shared_gpu:
        os.environ["FDIPT_SHARED_GPU"] = "allow"
    else:
        gpu_guard.check(dev, policy=os.environ.get("FDIPT_SHARED_GPU") or "refuse", what="run_sharded")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo" if one_gpu else "nccl", rank=rank, world_size=world)
    inp = a.download_dir is not None
    conf = config.base_config(inpainting=inp)
    diff = SE3Diffuser(conf.diffuser, device=dev)
    net = ScoreNetwork(conf.model, diff, inpainting=inp, precision=a.precision, kernel_flags=a.kernel_flags).load_synthetic(a.weights_seed).to(dev)
    write_item, keep = None, ("prot_traj",)
    if inp:
        from .sampler import ConditionalSampler, TCRSampler
        data_conf = config.to_conf({"download_dir": a.download_dir, "data_path": a.csv, "samples": a.samples_per_structure, "seed": a.seed,
                                    "redaction": {"redact_min_len": a.redact_min_len, "redact_max_len": a.redact_max_len},
                                    "cdr_loops": ["CDR3"], "first_assembly": True})
        ds = (TCRSampler if a.tcr else ConditionalSampler)(data_conf, diff, dev)
        write_item = reference_layout_writer(a.out_dir, net, final_only=not a.full_trajectory)
        keep = ("prot_traj",) if not a.full_trajectory else ("prot_traj", "rigid_0_traj")
    else:
        ds = UnconditionalSampler(config.to_conf({"min_length": a.min_length, "max_length": a.max_length,
                                                  "length_step": a.length_step, "samples_per_length": a.samples_per_length}), diff, dev)

    inference.kept_steps(a.num_t, a.keep)  # (a bad stride fails here, before any rank allocates)
    # one session per rank: batches of a shape this rank has run before reuse that loop's device buffers and captured step graphs
    # (with --keep all a loop holds the full trajectories — 2 x 4.3 GB at B = 64, N = 300, T = 500 — so only the most recent shape stays
    #  resident, as much as a rank held at a time before sessions; kept-frame loops are small and four shapes stay)
    session = inference.Session(max_loops=1 if a.keep == "all" else 4)

    def run_batch(feats, tape):
        # (--noise device: run_rank hands over the batch's noise keys where the tape would be)
        how = dict(noise="device", noise_keys=tape) if a.noise == "device" else dict(noise_tape=tape)

        def go():
            return inference.inference_fn(net, diff, feats, num_t=a.num_t, min_t=a.min_t, aux_traj=True, noise_scale=a.noise_scale,
                                          return_device=True, **how, inpainting=inp, verify=a.verify,
                                          input_aatype=inp and not a.no_input_aatype, keep=a.keep, session=session)  # (run_rank overlaps the D2H copy with the next batch)
        if not (one_gpu and world > 1):
            return go()
        # FDIPT_ONE_GPU (tests): the ranks share one GPU.  Kernels of two processes must not be co-resident on it (DESIGN.md section 6:
        # a half-precision MFMA kernel next to another kernel's waves corrupts single residues — 1 of 12 two-rank soak runs at N = 810
        # differed in one sample), so the ranks take turns on the device: a file lock around each batch, released once its kernels are done.
        # Production runs are one process per GPU and never take this path.
        return one_gpu_turn(go)

    def one_gpu_turn(fn):
        import fcntl
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, ".one_gpu.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            try:
                res = fn()
                torch.cuda.synchronize()
                return res
            finally:
                fcntl.flock(lk, fcntl.LOCK_UN)

    if write_item is not None and one_gpu and world > 1:
        # the writer's ground-truth backbone launch (reference_layout_writer -> get_atom_positions_from_rigids) is GPU work as well
        plain_write = write_item
        write_item = lambda *args, **kw: one_gpu_turn(lambda: plain_write(*args, **kw))  # noqa: E731

    t0 = time.perf_counter()
    plan = stage_plan(a, inp)
    collected = {} if plan.collect else None
    ground_truth = None
    if plan.ground_truth:  # (the ground-truth atom37 the writer builds for <pdb>_1.pdb)
        def ground_truth(feats):
            build = lambda: inference.get_atom_positions_from_rigids(net, feats["rigids_0"], feats["torsion_angles_sin_cos"][..., 2, :], feats["aatype"])[0]  # noqa: E731
            return one_gpu_turn(build) if one_gpu and world > 1 else build()
    recs = run_rank(ds, diff, run_batch, rank, world, a.out_dir, a.seed, a.num_t, a.min_t, a.max_batch, keep=keep,
                    final_only=not a.full_trajectory, write_item=write_item, noise=a.noise, collect=collected, ground_truth=ground_truth)
    torch.cuda.synchronize()
    session.close()
    if world > 1:
        dist.barrier()
    gathered = None
    if plan.collect:  # (every rank takes part in the gather; rank 0 receives)
        from . import sharding
        gathered = sharding.gather_results(collected, len(ds), rank, world)
    if rank == 0:
        el = time.perf_counter() - t0
        allrecs = write_manifest(a.out_dir, world, len(ds), {"num_t": a.num_t, "precision": a.precision, "seed": a.seed, "noise": a.noise, "wall_s": el,
                                                                **({} if a.keep == "all" else {"keep": a.keep})})
        print(f"{sum(r['n_res'] for r in allrecs) * a.num_t / el:.0f} residue*steps/s (incl. model set-up and file output)")
        print(f"{len(ds)} samples on {world} GPU(s) in {el:.1f} s -> {a.out_dir}/manifest.json", flush=True)
        selected = {} if plan.keep_selection else None
        for stage in plan.stages:
            t1 = time.perf_counter()
            done = stage.run(a, allrecs, gathered, inp, selected)
            print(stage.report(a, done, inp, time.perf_counter() - t1), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
