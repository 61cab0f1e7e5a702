"""Wall time of sample selection for a load like BASELINE config C3: 62 complexes x 5 samples, two diffused regions of 12 - 16 residues,
N = 800 (synthetic coordinates).  Prints the wall time of ``selection.select_samples`` calls (device tensor in, NumPy results out), of calls
with 0 / 1000 / 10000 iterations, of 4 groups x 64 samples, and of the plain NumPy iteration (tests/selection_ref.py) for the same 62
complexes on this host, with the largest difference between the two medians.

    python tools/selection_wall.py [out.json]
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
import selection_ref as sr  # noqa: E402

from framedipt_amd import selection  # noqa: E402

rng = np.random.default_rng(0)
G, S, N = 62, 5, 800
prot = np.zeros((G * S, N, 37, 3), dtype=np.float32)
mask = np.zeros((G * S, N), dtype=np.float32)
groups = np.repeat(np.arange(G), S)
for g in range(G):
    base = 40.0 + np.cumsum(rng.normal(size=(N, 1, 3)) * 2.2, axis=0) * 0.3 + rng.normal(size=(N, 37, 3))
    prot[g * S:(g + 1) * S] = base[None] + 1.2 * rng.normal(size=(S, N, 1, 3)) + 0.3 * rng.normal(size=(S, N, 37, 3))
    a, b = int(rng.integers(90, 110)), int(rng.integers(600, 700))
    mask[g * S:(g + 1) * S, a:a + int(rng.integers(12, 17))] = 1
    mask[g * S:(g + 1) * S, b:b + int(rng.integers(12, 17))] = 1
out = {}
d_prot, d_mask = torch.from_numpy(prot).cuda(), torch.from_numpy(mask).cuda()
torch.cuda.synchronize()
walls = []
for i in range(4):
    t0 = time.perf_counter(); sel = selection.select_samples(d_prot, d_mask, groups); walls.append(time.perf_counter() - t0)
out["device_call_wall_s"] = walls
print("select_samples wall (device tensor in, NumPy out), 4 calls:", walls, flush=True)
for it in (0, 1000, 10000):
    t0 = time.perf_counter(); selection.select_samples(d_prot, d_mask, groups, max_iterations=it); out[f"wall_iters_{it}"] = time.perf_counter() - t0
print({k: v for k, v in out.items() if k.startswith("wall_iters")}, flush=True)
# larger groups: 4 x 64 samples
big = np.tile(prot[:S], (52, 1, 1, 1))[:256] + rng.normal(size=(256, N, 37, 3)).astype(np.float32)
bm = np.tile(mask[:1], (256, 1))
selection.select_samples(big, bm, np.repeat(np.arange(4), 64))
t0 = time.perf_counter(); selection.select_samples(torch.from_numpy(big).cuda(), bm, np.repeat(np.arange(4), 64)); out["wall_4x64"] = time.perf_counter() - t0
print("4 groups x 64:", out["wall_4x64"], flush=True)
t0 = time.perf_counter()
worst = 0.0
for g in range(G):
    x = sr.gather(prot, sel["residues"][g], sel["members"][g])
    med = sr.plain_median(x)
    worst = max(worst, float(np.abs(med - sel["median"][g]).max()))
out["plain_numpy_s"] = time.perf_counter() - t0
out["worst_vs_plain"] = worst
out["status_any"] = int(sel["status"].any())
print("plain NumPy iteration, 62 groups:", out["plain_numpy_s"], "s; worst |device - plain| =", worst, flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
