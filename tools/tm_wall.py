"""Wall time of the TM-score for three loads cut from a fixture complex (tests/golden/sasa_cases.npz, 5ksa, the columns N, CA, C, CB, O):
all-against-all of 64 and of 100 backbone samples x N = 300 (windows of 300 rows, four rows apart: pairs of one fold at a shifted
correspondence, the loose end of the diversity matrix) and 64 samples against one ground truth (the window with 1 Angstrom noise: the
tm_score of protein_metrics).  Prints per load the wall time of ``tm_score.tm_scores`` calls (device tensor in, NumPy results out; the
first call on its own), the time of the launch between device-side events, the passes per seed as the device counted them, and for
three pairs the NumPy restatement (tests/tm_ref.py): its time, |device - restatement| of tm and the histogram of passes per seed.
``sclk_mhz``: the shader clock the driver reports (the marked level of the device's ``pp_dpm_sclk``, read every 20 ms by a host thread
during 30 further calls of the load; null where the file cannot be read).  One run; no threshold is attached to these times.

    python tools/tm_wall.py [out.json]
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
import tm_ref as tr  # noqa: E402

from framedipt_amd import _lib, tm_score  # noqa: E402

lib = _lib.load()
launch, events = lib.fdipt_sample_tm_score, []


def timed_launch(args, stream):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    rc = launch(args, stream)
    stop.record()
    events.append((start, stop))
    return rc


lib.fdipt_sample_tm_score = timed_launch


def sclk_path():
    """The sysfs file with the shader clock levels of device 0, or None."""
    try:
        prop = torch.cuda.get_device_properties(0)
        path = f"/sys/bus/pci/devices/{prop.pci_domain_id:04x}:{prop.pci_bus_id:02x}:{prop.pci_device_id:02x}.0/pp_dpm_sclk"
        return path if os.path.exists(path) else None
    except Exception:  # noqa: BLE001  (an older torch without the PCI ids: no clock is reported)
        return None


def sclk_while(work):
    """Run ``work()`` while a thread samples the marked clock level: (min, max) MHz over the samples, or None."""
    import re
    import threading
    path, seen, stop = sclk_path(), [], threading.Event()

    def sample():
        while not stop.is_set():
            try:
                with open(path) as f:
                    seen.extend(int(m) for m in re.findall(r"(\d+)\s*[Mm][Hh]z\s*\*", f.read()))
            except OSError:
                return
            stop.wait(0.02)

    thread = threading.Thread(target=sample) if path else None
    if thread:
        thread.start()
    work()
    torch.cuda.synchronize()
    stop.set()
    if thread:
        thread.join()
    return [min(seen), max(seen)] if seen else None


fix = dict(np.load(os.path.join(ROOT, "tests", "golden", "sasa_cases.npz")))
backbone, _, _ = sr.case_prot(fix, "5ksa", 5)
windows = np.stack([backbone[4 * s:4 * s + 300] for s in range(100)])
rng = np.random.default_rng(0)
noisy = (windows[:1] + (rng.normal(size=(64, 300, 1, 3)) / np.sqrt(3.0)).astype(np.float32)).astype(np.float32)

out = {}
loads = {"all_against_all_b64_n300": (windows[:64], None), "all_against_all_b100_n300": (windows, None), "b64_n300_against_one_ground_truth": (noisy, windows[:1])}
seeds_300 = len(tr.seeds(300)[0])
for label, (prot, truth) in loads.items():
    d_prot = torch.from_numpy(prot).cuda()
    d_truth = None if truth is None else torch.from_numpy(truth).cuda()
    torch.cuda.synchronize()
    walls = []
    for _ in range(4):
        t0 = time.perf_counter()
        res = tm_score.tm_scores(d_prot, d_truth)
        walls.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    device_ms = [start.elapsed_time(stop) for start, stop in events]
    events.clear()
    sclk = sclk_while(lambda: [tm_score.tm_scores(d_prot, d_truth) for _ in range(30)])
    events.clear()
    per_seed = res["passes"] / seeds_300
    checked = []
    for p in (0, len(res["tm"]) // 2, len(res["tm"]) - 1):
        i, j = res["pairs"][p]
        t0 = time.perf_counter()
        want = tr.tm_score(*tr.compact(prot[i], (prot if truth is None else truth)[j]))
        checked.append({"pair": [int(i), int(j)], "numpy_restatement_s": time.perf_counter() - t0, "tm": float(res["tm"][p]),
                        "abs_device_minus_restatement": abs(float(res["tm"][p]) - want["tm"]), "passes_equal": bool(res["passes"][p] == want["passes"]),
                        "passes_per_seed_histogram": np.bincount(want["seed_passes"], minlength=tr.MAX_PASSES + 1).tolist()})
    out[label] = {"pairs": int(len(res["tm"])), "first_call_wall_s": walls[0], "call_wall_s": walls[1:], "launch_device_ms": device_ms, "sclk_mhz": sclk,
                  "tm_mean": float(res["tm"].mean()), "tm_min": float(res["tm"].min()), "tm_max": float(res["tm"].max()),
                  "passes_per_seed_mean": float(per_seed.mean()), "passes_per_seed_min_pair": float(per_seed.min()), "passes_per_seed_max_pair": float(per_seed.max()),
                  "statuses": sorted(set(res["status"].tolist())), "checked": checked}
    if truth is None:
        out[label]["diversity_at_0.5"] = tm_score.diversity(res["matrix"], 0.5)["diversity"]
    print(label, json.dumps(out[label]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
