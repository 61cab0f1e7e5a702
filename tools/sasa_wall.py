"""Wall time of the solvent accessibility for two loads cut from the fixture's complexes (tests/golden/sasa_cases.npz): 64 backbone
samples x N = 300 (windows of 300 rows of 5ksa, eight rows apart, the columns N, CA, C, CB, O) and one full-atom complex (1fyt, 810
rows, about 6 500 atoms).  Prints per load the wall time of ``sasa.solvent_accessibility`` calls (device tensor in, NumPy results out;
the first call on its own), the time of the three launches between device-side events, and the time of the NumPy restatement
(tests/sasa_ref.py, filtered form) per sample on this host with the number of atoms whose count differs from the device's (0).
One run; no threshold is attached to these times.

    python tools/sasa_wall.py [out.json]
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
import sasa_ref as sr  # noqa: E402

from framedipt_amd import _lib, sasa  # noqa: E402

lib = _lib.load()
launch, events = lib.fdipt_sample_sasa, []


def timed_launch(args, stream):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    rc = launch(args, stream)
    stop.record()
    events.append((start, stop))
    return rc


lib.fdipt_sample_sasa = timed_launch
fix = dict(np.load(os.path.join(ROOT, "tests", "golden", "sasa_cases.npz")))
backbone, _, backbone_aatype = sr.case_prot(fix, "5ksa", 37)
backbone[:, 5:] = 0
whole, _, whole_aatype = sr.case_prot(fix, "1fyt", 37)

out = {}
loads = {"b64_n300_backbone": (np.stack([backbone[8 * s:8 * s + 300] for s in range(64)]), np.stack([backbone_aatype[8 * s:8 * s + 300] for s in range(64)])),
         "b1_n810_full_atom": (whole[None], whole_aatype[None])}
for label, (prot, aatype) in loads.items():
    d_prot = torch.from_numpy(prot).cuda()
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        res = sasa.solvent_accessibility(d_prot, None, None, aatype)
        walls.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    device_ms = [start.elapsed_time(stop) for start, stop in events]
    events.clear()
    t0 = time.perf_counter()
    count = min(len(prot), 3)
    differ = 0
    for s in range(count):
        want = sr.sasa(prot[s], None, None, aatype[s])
        differ += int((want["accessible"] != res["accessible"][s]).sum())
    numpy_s = (time.perf_counter() - t0) / count
    out[label] = {"first_call_wall_s": walls[0], "call_wall_s": walls[1:], "launches_device_ms": device_ms, "numpy_restatement_s_per_sample": numpy_s,
                  "atoms_whose_count_differs": differ, "atoms_per_sample": float(res["n_atoms"].mean()), "total_sasa_mean": float(res["total_sasa"].mean())}
    print(label, json.dumps(out[label]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
