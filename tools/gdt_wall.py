"""Wall time of GDT-TS / GDT-HA for two loads of N = 300 rows - 64 samples against one ground truth, and the 2 016 pairs of an
all-against-all of 64 samples - in the three modes (none, global, search), next to ``tm_score.tm_scores`` on the same pairs in the same
process; synthetic coordinates (a CA walk, the samples perturbed copies of the ground truth).  Prints per load and entry the wall time
of the calls (device tensors in, NumPy results out; the first call on its own) and the time of the launch between device-side events,
then the ratio of the searched GDT launch to the TM-score launch (the search runs five times the TM search's items), and compares two
pairs per load with the NumPy restatement (tests/gdt_ref.py; every integer output is expected equal).

    python tools/gdt_wall.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gdt_ref as gr  # noqa: E402

from framedipt_amd import _lib, gdt, tm_score  # noqa: E402

lib = _lib.load()
events = []


def timed(launch):
    def call(args, stream):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        rc = launch(args, stream)
        stop.record()
        events.append((start, stop))
        return rc
    return call


lib.fdipt_sample_gdt, lib.fdipt_sample_tm_score = timed(lib.fdipt_sample_gdt), timed(lib.fdipt_sample_tm_score)
out, n, b = {}, 300, 64
rng = np.random.default_rng(n)
steps = rng.normal(size=(n, 3))
ca = 40.0 + np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=-1, keepdims=True), axis=0)
truth = gr.five_atoms(ca.astype(np.float32))[None]
prot = np.stack([gr.five_atoms((ca + rng.choice([0.2, 0.6, 1.5, 3.0], size=(n, 1)) * rng.normal(size=(n, 3)) / np.sqrt(3.0)).astype(np.float32)) for _ in range(b)])
d_prot, d_truth = torch.from_numpy(prot).cuda(), torch.from_numpy(truth).cuda()
torch.cuda.synchronize()
for label, second in (("b64_n300_vs_truth", d_truth), ("all_pairs_2016_n300", None)):
    entries = [("tm_score", lambda: tm_score.tm_scores(d_prot, second))] + [(f"gdt_{m}", lambda m=m: gdt.gdt_scores(d_prot, second, superpose=m)) for m in gr.MODES]
    out[label] = {}
    for name, call in entries:
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            res = call()
            walls.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        device_ms = [start.elapsed_time(stop) for start, stop in events]
        events.clear()
        rec = {"pairs": int(len(res["pairs"])), "first_call_wall_s": walls[0], "call_wall_s": walls[1:], "launch_device_ms": device_ms}
        if name.startswith("gdt_"):
            worst = 0
            for p in range(2):
                ia, ib = res["pairs"][p]
                want = gr.gdt(*gr.compact(prot[ia], truth[ib] if second is not None else prot[ib]), name[4:])
                worst = max(worst, int(np.abs(want["counts"] - res["counts"][p]).max()), int((want["res_within"] != res["res_within"][p]).sum()))
            rec.update(mean_gdt_ts=float(res["gdt_ts"].mean()), mean_gdt_ha=float(res["gdt_ha"].mean()), passes=int(res["passes"].sum()),
                       worst_integer_difference_of_two_pairs=worst)
        else:
            rec.update(mean_tm=float(res["tm"].mean()), passes=int(res["passes"].sum()))
        out[label][name] = rec
        print(label, name, json.dumps(rec), flush=True)
    tm_ms, search_ms = (min(out[label][k]["launch_device_ms"][1:]) for k in ("tm_score", "gdt_search"))
    out[label]["search_over_tm_score"] = {"launch": search_ms / tm_ms, "passes": out[label]["gdt_search"]["passes"] / out[label]["tm_score"]["passes"]}
    print(label, "search / tm_score", json.dumps(out[label]["search_over_tm_score"]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
