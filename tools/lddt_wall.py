"""Wall time of the superposition-free accuracy scores for four loads: 64 samples x N = 300 against one ground truth on the CA and on the
backbone atoms, the 64 x 63 ordered pairs of a de novo batch of N = 300 on the CA atoms, and one like BASELINE config C3 (310 samples x
N = 800 against one ground truth, both sets); synthetic coordinates (a CA walk with the other atoms scattered around it, the samples
perturbed copies of the ground truth).  Prints per load the wall time of ``lddt.local_accuracy`` calls (device tensors in, NumPy
results out; the first call on its own), the time of the two launches between device-side events, and the time of the NumPy restatement
(tests/lddt_ref.py) per pair on this host (2 pairs) with the largest difference of ``lddt`` (expected 0) and of ``fape``.

    python tools/lddt_wall.py [out.json]
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
import lddt_ref as lr  # noqa: E402

from framedipt_amd import _lib, lddt  # noqa: E402

lib = _lib.load()
launch, events = lib.fdipt_sample_lddt, []


def timed_launch(args, stream):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    rc = launch(args, stream)
    stop.record()
    events.append((start, stop))
    return rc


lib.fdipt_sample_lddt = timed_launch
out = {}
for label, b, n, mode, all_pairs in (("b64_n300_ca", 64, 300, "ca", False), ("b64_n300_backbone", 64, 300, "backbone", False),
                                     ("denovo_64x63_n300_ca", 64, 300, "ca", True), ("c3_b310_n800_ca", 310, 800, "ca", False),
                                     ("c3_b310_n800_backbone", 310, 800, "backbone", False)):
    rng = np.random.default_rng(n)
    steps = rng.normal(size=(n, 3))
    ca = 40.0 + np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=-1, keepdims=True), axis=0)
    truth = np.zeros((1, n, 37, 3), dtype=np.float32)
    truth[0, :, :5] = ca[:, None] + 0.9 * rng.normal(size=(n, 5, 3))
    prot = np.zeros((b, n, 37, 3), dtype=np.float32)
    prot[:, :, :5] = truth[:, :, :5] + rng.choice([0.1, 0.5, 1.5], size=(b, n, 1, 1)) * rng.normal(size=(b, n, 1, 3)) + 0.05 * rng.normal(size=(b, n, 5, 3))
    d_prot, d_truth = torch.from_numpy(prot).cuda(), torch.from_numpy(truth).cuda()
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        res = lddt.local_accuracy(d_prot, None if all_pairs else d_truth, atoms=mode)
        walls.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    device_ms = [start.elapsed_time(stop) for start, stop in events]
    events.clear()
    t0 = time.perf_counter()
    worst_lddt = worst_fape = 0.0
    for p in range(2):
        ia, ib = res["pairs"][p]
        want = lr.local_accuracy(prot[ia], prot[ib] if all_pairs else truth[ib], mode)
        worst_lddt = max(worst_lddt, abs(want["lddt"] - float(res["lddt"][p])))
        worst_fape = max(worst_fape, abs(want["fape"] - float(res["fape"][p])))
    numpy_s = (time.perf_counter() - t0) / 2
    out[label] = {"pairs": int(len(res["pairs"])), "first_call_wall_s": walls[0], "call_wall_s": walls[1:], "launch_pair_device_ms": device_ms,
                  "numpy_restatement_s_per_pair": numpy_s, "worst_lddt_difference": worst_lddt, "worst_fape_difference": worst_fape,
                  "mean_lddt": float(res["lddt"].mean()), "mean_drmsd": float(res["drmsd"].mean()), "mean_fape": float(res["fape"].mean())}
    print(label, json.dumps(out[label]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
