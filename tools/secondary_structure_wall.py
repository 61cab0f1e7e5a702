"""Wall time of the secondary structure for two loads cut from the fixture's complexes (tests/golden/dssp_cases.npz): 64 samples x
N = 300 (windows of 300 rows of 5ksa, eight rows apart) and 5 samples x N = 810 (the three complexes and two more windows, cut or
padded to 810 rows).  Prints per load the wall time of ``secondary_structure.secondary_structure`` calls (device tensor in, NumPy
results out; the first call on its own), the time of the launch between device-side events, and the time of the NumPy restatement
(tests/dssp_ref.py) per sample on this host with the number of rows whose class differs from the device's (0).

    python tools/secondary_structure_wall.py [out.json]
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
import dssp_ref as dr  # noqa: E402

from framedipt_amd import _lib, secondary_structure  # noqa: E402

lib = _lib.load()
launch, events = lib.fdipt_sample_dssp, []


def timed_launch(args, stream):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    rc = launch(args, stream)
    stop.record()
    events.append((start, stop))
    return rc


lib.fdipt_sample_dssp = timed_launch
fix = dict(np.load(os.path.join(ROOT, "tests", "golden", "dssp_cases.npz")))


def window(name, lo, n):
    """Rows lo .. lo + n of a complex as (atom37 [n,37,3], res_mask, chain_idx, aatype), padded with masked rows."""
    bb, chain, pro = fix[f"{name}.bb"][lo:lo + n], fix[f"{name}.chain_idx"][lo:lo + n], fix[f"{name}.is_proline"][lo:lo + n]
    prot, mask, ch, aa = np.zeros((n, 37, 3), dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    k = len(bb)
    prot[:k, [0, 1, 2, 4]], mask[:k], ch[:k], aa[:k] = bb, 1, chain, np.where(pro != 0, secondary_structure.PRO, 0)
    return prot, mask, ch, aa


out = {}
loads = {"b64_n300": [window("5ksa", 8 * s, 300) for s in range(64)],
         "b5_n810": [window("1fyt", 0, 810), window("5ksa", 0, 810), window("7t2d", 0, 810), window("5ksa", 10, 810), window("7t2d", 1, 810)]}
for label, samples in loads.items():
    prot, mask, chain, aatype = (np.stack(x) for x in zip(*samples))
    d_prot = torch.from_numpy(prot).cuda()
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        res = secondary_structure.secondary_structure(d_prot, mask, chain, aatype)
        walls.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    device_ms = [start.elapsed_time(stop) for start, stop in events]
    events.clear()
    t0 = time.perf_counter()
    count = min(len(samples), 5)
    differ = 0
    for s in range(count):
        want = dr.dssp(prot[s], mask[s], chain[s], aatype[s] == secondary_structure.PRO)
        differ += int((want["ss"] != res["ss"][s]).sum())
    numpy_s = (time.perf_counter() - t0) / count
    out[label] = {"first_call_wall_s": walls[0], "call_wall_s": walls[1:], "launch_device_ms": device_ms, "numpy_restatement_s_per_sample": numpy_s,
                  "rows_whose_class_differs": differ, "helix_percent_mean": float(res["helix_percent"].mean()),
                  "strand_percent_mean": float(res["strand_percent"].mean()), "ladders_mean": float(res["n_ladders"].mean())}
    print(label, json.dumps(out[label]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
