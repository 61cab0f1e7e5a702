"""Wall time of the novelty search (framedipt_amd/structure_search.py): 8 queries of 300 rows against 2 048
synthetic entries of 40 .. 512 rows - a seeded mix of ideal helices, strands and random walks joined into chains, 32 of the entries
noisy windows of the queries so that something scores above 0.5 - in three calls on the same pairs:

    search(prune=False)                  every pair scored, bucketed by entry length
    search(prune=True, min_score=0.5)    the length bound on
    tm_align(queries, padded set)        what the parent offers: the set padded to 512 rows, one launch, every output of every pair

One warm-up round, then ROUNDS rounds that alternate the three calls (device tensors in, NumPy results out, a synchronise before the
clock is read).  Prints every time, the median and the range per call, the ratio of the unpruned search to the padded call with the
run-to-run spread next to it, the pruned share, and checks that the three agree on every query's best hit bit for bit.

``--inits all`` runs the three calls in the five-start mode ("The two fragment starts").  ``--inits both``
alternates ``search(prune=False)`` of the two modes instead (each between device-side events as well) and counts the pairs whose
score rose.  ``--rounds`` sets the timed rounds.

    python tools/search_wall.py [out.json] [--inits {default,all,both}] [--rounds K]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from framedipt_amd import structure_search as ss, tm_align  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=None)
ap.add_argument("--inits", choices=("default", "all", "both"), default="default")
ap.add_argument("--rounds", type=int, default=4)
opt = ap.parse_args()
ROUNDS, N_Q, ROWS, N_DB = opt.rounds, 8, 300, 2048
rng = np.random.default_rng(2048)


def segment(kind, n):
    i = np.arange(n, dtype=np.float64)
    if kind == 0:  # an ideal helix: 2.3 A radius, 100 degrees and 1.5 A per residue
        return np.stack([2.3 * np.cos(np.deg2rad(100.0) * i), 2.3 * np.sin(np.deg2rad(100.0) * i), 1.5 * i], axis=1)
    if kind == 1:  # an ideal strand: 3.3 A per residue, a zigzag of 0.9 A
        return np.stack([0.9 * (i % 2), np.zeros(n), 3.3 * i], axis=1)
    steps = rng.normal(size=(n, 3))
    return np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=1, keepdims=True), axis=0)


def chain(n):
    """Segments of 8 .. 30 rows, each turned at random and joined 3.8 A behind the last row of the one before."""
    rows, end = [], np.zeros(3)
    while sum(len(r) for r in rows) < n:
        seg = segment(int(rng.integers(3)), int(rng.integers(8, 31)))
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        seg = (seg - seg[0]) @ (q * np.sign(np.linalg.det(q))).T
        step = rng.normal(size=3)
        rows.append(seg + end + 3.8 * step / np.linalg.norm(step))
        end = rows[-1][-1]
    return np.concatenate(rows)[:n].astype(np.float32)


def five_atoms(ca):
    out = np.zeros((len(ca), 5, 3), dtype=np.float32)
    out[:] = ca[:, None]
    return out


queries = np.stack([chain(ROWS) for _ in range(N_Q)])
lengths = rng.integers(40, 513, size=N_DB)
entries = [chain(int(n)) for n in lengths]
for k in range(32):  # noisy windows of the queries, 150 .. 300 rows
    q, n = k % N_Q, int(rng.integers(150, ROWS + 1))
    s = int(rng.integers(0, ROWS - n + 1))
    entries[int(rng.integers(N_DB))] = (queries[q, s:s + n] + rng.normal(size=(n, 3)).astype(np.float32) * 0.6).astype(np.float32)
db = ss.StructureSet.from_arrays(entries)
longest = int(db.lengths.max())
padded, padded_mask = np.zeros((N_DB, longest, 5, 3), dtype=np.float32), np.zeros((N_DB, longest), dtype=np.float32)
for e, t in enumerate(entries):
    padded[e, :len(t)], padded_mask[e, :len(t)] = five_atoms(t), 1
pairs = np.array([[q, e] for q in range(N_Q) for e in range(N_DB)], dtype=np.int32)
d_queries = torch.from_numpy(np.stack([five_atoms(q) for q in queries])).cuda()
d_padded, d_padded_mask = torch.from_numpy(padded).cuda(), torch.from_numpy(padded_mask).cuda()
mode = "default" if opt.inits == "both" else opt.inits
calls = {"search": lambda: ss.search(d_queries, db, prune=False, return_scores=True, inits=mode),
         "search_pruned_0.5": lambda: ss.search(d_queries, db, prune=True, min_score=0.5, return_scores=True, inits=mode),
         "tm_align_padded": lambda: tm_align.tm_align(d_queries, d_padded, None, d_padded_mask, pairs=pairs, inits=mode)}
if opt.inits == "both":
    calls = {"search": calls["search"], "search_all": lambda: ss.search(d_queries, db, prune=False, return_scores=True, inits="all")}
walls, device_ms, results = {k: [] for k in calls}, {k: [] for k in calls}, {}
for r in range(ROUNDS + 1):  # round 0 warms every shape up
    for name, call in calls.items():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        results[name] = call()
        stop.record()
        torch.cuda.synchronize()
        if r:
            walls[name].append(time.perf_counter() - t0)
            device_ms[name].append(start.elapsed_time(stop))
        print(f"round {r} {name}: {time.perf_counter() - t0:.3f} s", flush=True)

work = ss.plan(db.lengths)
out = {"queries": N_Q, "rows": ROWS, "entries": N_DB, "pairs": len(pairs), "entry_rows": {"min": int(db.lengths.min()), "mean": float(db.lengths.mean()), "max": longest},
       "rounds": ROUNDS, "buckets": {int(c): int(e - s) for c, s, e in zip(work["bucket_cap"], work["bucket_start"][:-1], work["bucket_start"][1:])}}
for name, w in walls.items():
    out[name] = {"wall_s": w, "median_s": float(np.median(w)), "min_s": min(w), "max_s": max(w), "spread": (max(w) - min(w)) / float(np.median(w)),
                 "between_events_ms": device_ms[name]}
out["inits"] = opt.inits
if opt.inits == "both":
    plain, five = results["search"], results["search_all"]
    out["all_over_default"] = out["search_all"]["median_s"] / out["search"]["median_s"]
    out["tm_q_rose"], out["tm_q_fell"] = int((five["scores_q"] > plain["scores_q"]).sum()), int((five["scores_q"] < plain["scores_q"]).sum())
    out["tm_t_rose"], out["tm_t_fell"] = int((five["scores_t"] > plain["scores_t"]).sum()), int((five["scores_t"] < plain["scores_t"]).sum())
    out["largest_rise_tm_q"] = float(np.nanmax(five["scores_q"] - plain["scores_q"]))
    out["pdb_tm"], out["pdb_tm_all"] = plain["pdb_tm"].tolist(), five["pdb_tm"].tolist()
    out["best_hit_changed"] = int((plain["hit"][:, 0] != five["hit"][:, 0]).sum())
    for m in ("default", "all"):  # the programmes per pair and the winners: one padded tm_align call per mode (the score pass returns neither)
        dense = tm_align.tm_align(d_queries, d_padded, None, d_padded_mask, pairs=pairs, inits=m)
        out[f"dp_per_pair_{m}"] = {"mean": float(dense["init_dp"].sum(1).mean()), "min": int(dense["init_dp"].sum(1).min()), "max": int(dense["init_dp"].sum(1).max())}
        out[f"best_init_counts_{m}"] = np.bincount(dense["best_init"][dense["best_init"] >= 0], minlength=tm_align.N_INITS[m]).tolist()
        out[f"scores_equal_the_padded_call_{m}"] = bool(np.array_equal((plain if m == "default" else five)["scores_t"], dense["tm_b"].reshape(N_Q, N_DB), equal_nan=True))
    print(json.dumps(out), flush=True)
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(0)
out["search_over_padded"] = out["search"]["median_s"] / out["tm_align_padded"]["median_s"]
out["pruned_over_search"] = out["search_pruned_0.5"]["median_s"] / out["search"]["median_s"]
plain, pruned, dense = results["search"], results["search_pruned_0.5"], results["tm_align_padded"]
out["pruned_share"] = float(pruned["n_pruned"].sum()) / len(pairs)
out["hits_at_0.5"] = int((pruned["hit"] >= 0).sum())
# the three agree: every pair's scores against the padded call, the best hit of the pruned call against the unpruned one
same_scores = np.array_equal(plain["scores_q"], dense["tm_a"].reshape(N_Q, N_DB), equal_nan=True) and \
    np.array_equal(plain["scores_t"], dense["tm_b"].reshape(N_Q, N_DB), equal_nan=True)
strong = plain["tm_q"][:, 0] >= 0.5
same_hits = np.array_equal(np.where(strong, plain["hit"][:, 0], -1), pruned["hit"][:, 0]) and \
    np.array_equal(plain["tm_q"][strong, 0], pruned["tm_q"][strong, 0])
out["scores_equal_the_padded_call"], out["pruned_hits_equal_the_unpruned"] = bool(same_scores), bool(same_hits)
out["pdb_tm"] = plain["pdb_tm"].tolist()
print(json.dumps(out), flush=True)
if opt.out:
    with open(opt.out, "w") as f:
        json.dump(out, f, indent=1)
sys.exit(0 if same_scores and same_hits else 1)
