"""Wall time of the structural violations for two loads: 64 samples x N = 300, and one like BASELINE config C3 (310 samples x N = 800),
synthetic coordinates (a CA walk with the other atoms scattered around it), two undiffused-free samples in five.  Prints per load the
wall time of ``violations.structural_violations`` calls (device tensor in, NumPy results out; the first call on its own), the time of
the two launches between device-side events, and the time of the NumPy restatement (tests/violations_ref.py) per sample on this host
(8 samples) with the largest difference of ``clashes_mean_loss``.

    python tools/violations_wall.py [out.json]
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
import violations_ref as vr  # noqa: E402

from framedipt_amd import _lib, violations  # noqa: E402

lib = _lib.load()
launch, events = lib.fdipt_sample_violations, []


def timed_launch(args, stream):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    rc = launch(args, stream)
    stop.record()
    events.append((start, stop))
    return rc


lib.fdipt_sample_violations = timed_launch
out = {}
for label, b, n in (("b64_n300", 64, 300), ("c3_b310_n800", 310, 800)):
    rng = np.random.default_rng(n)
    steps = rng.normal(size=(b, n, 3))
    ca = 40.0 + np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=-1, keepdims=True), axis=1)
    prot = np.zeros((b, n, 37, 3), dtype=np.float32)
    prot[:, :, :5] = ca[:, :, None] + 0.9 * rng.normal(size=(b, n, 5, 3))
    diffuse = np.ones((b, n), dtype=np.float32)
    diffuse[::5, 40:60] = 0
    d_prot = torch.from_numpy(prot).cuda()
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        res = violations.structural_violations(d_prot, diffuse)
        walls.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    device_ms = [start.elapsed_time(stop) for start, stop in events]
    events.clear()
    t0 = time.perf_counter()
    worst = 0.0
    for s in range(8):
        want = vr.violations(prot[s], None, vr.keep_mask(prot[s], diffuse[s]))
        worst = max(worst, abs(float(want["clashes_mean_loss"]) - float(res["clashes_mean_loss"][s])))
    numpy_s = (time.perf_counter() - t0) / 8
    out[label] = {"first_call_wall_s": walls[0], "call_wall_s": walls[1:], "launch_pair_device_ms": device_ms, "numpy_restatement_s_per_sample": numpy_s,
                  "worst_clashes_mean_loss_difference": worst, "violating_residues_mean": float(res["num_residue_violations"].mean())}
    print(label, json.dumps(out[label]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
