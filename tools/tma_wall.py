"""Wall time of the structural-alignment search (framedipt_amd/tm_align.py) for four loads of 300-row backbones: all-against-all of 64
and of 100 windows of a fixture complex (tests/golden/sasa_cases.npz, 5ksa, the columns N, CA, C, CB, O) taken four rows apart - one
fold at a shifted correspondence, where the fixed correspondence of ``tm_score`` scores 0.09 - 0.33 -, all-against-all of 64 unrelated
random walks (the long end: nothing is shared, the iterations run longest) and 64 noisy samples against one structure.  Prints per load
the wall time of ``tm_align`` calls (device tensor in, NumPy results out; the first call on its own), the time of the launch between
device-side events, the dynamic programmes per pair, which initial alignment won, and for two pairs the NumPy restatement
(tests/tma_ref.py): its time and |device - restatement| of tm.  ``sclk_mhz``: the shader clock the driver reports (the marked level of
the device's ``pp_dpm_sclk``, read every 20 ms by a host thread during further calls of the load; null where the file cannot be
read).  One run; no threshold is attached to these times.  ``--inits all`` runs the five-start mode ("The two
fragment starts"; the restatement is then tests/tma_inits_ref.py); ``--inits both`` alternates the two modes call by call on the same
pairs and adds, per load, the pairs whose ``tm_b`` rose, fell or whose winner is I4 or I5.  ``--loads`` picks loads by name, ``--no-check``
leaves the restatement out.

    python tools/tma_wall.py [out.json] [--inits {default,all,both}] [--loads NAME ...] [--no-check]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sasa_ref as sr  # noqa: E402
import tma_inits_ref as ti  # noqa: E402
import tma_ref as ta  # noqa: E402

from framedipt_amd import _lib, tm_align, tm_score  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=None)
ap.add_argument("--inits", choices=("default", "all", "both"), default="default")
ap.add_argument("--loads", nargs="+", default=None)
ap.add_argument("--no-check", action="store_true")
opt = ap.parse_args()
MODES = ("default", "all") if opt.inits == "both" else (opt.inits,)

lib = _lib.load()
launch, events = lib.fdipt_sample_tm_align, []


def timed_launch(args, stream):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    rc = launch(args, stream)
    stop.record()
    events.append((start, stop))
    return rc


lib.fdipt_sample_tm_align = timed_launch


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


def walk(rng, n, persist=0.7):
    d, out = rng.normal(size=3), [np.zeros(3)]
    for _ in range(n - 1):
        d = persist * d + (1.0 - persist) * 1.5 * rng.normal(size=3)
        d /= np.linalg.norm(d)
        out.append(out[-1] + 3.8 * d)
    return np.array(out) + np.array([31.0, -47.0, 58.0])


fix = dict(np.load(os.path.join(ROOT, "tests", "golden", "sasa_cases.npz")))
backbone, _, _ = sr.case_prot(fix, "5ksa", 5)
windows = np.stack([backbone[4 * s:4 * s + 300] for s in range(100)])
rng = np.random.default_rng(0)
noisy = (windows[:1] + (rng.normal(size=(64, 300, 1, 3)) / np.sqrt(3.0)).astype(np.float32)).astype(np.float32)
walks = np.stack([ta.five_atoms(walk(rng, 300).astype(np.float32)) for _ in range(64)])

out = {}
loads = {"all_against_all_b64_n300_windows": (windows[:64], None), "all_against_all_b100_n300_windows": (windows, None),
         "all_against_all_b64_n300_unrelated_walks": (walks, None), "b64_n300_against_one_structure": (noisy, windows[:1])}
for label, (prot, other) in loads.items():
    if opt.loads is not None and label not in opt.loads:
        continue
    d_prot = torch.from_numpy(prot).cuda()
    d_other = None if other is None else torch.from_numpy(other).cuda()
    torch.cuda.synchronize()
    walls, device_ms, res = {m: [] for m in MODES}, {m: [] for m in MODES}, {}
    for _ in range(3):  # (the modes alternate call by call)
        for mode in MODES:
            t0 = time.perf_counter()
            res[mode] = tm_align.tm_align(d_prot, d_other, inits=mode)
            walls[mode].append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            device_ms[mode] += [start.elapsed_time(stop) for start, stop in events]
            events.clear()
    fixed = None if other is not None else tm_score.tm_scores(d_prot)["matrix"]
    entry = {}
    for mode in MODES:
        got = res[mode]
        sclk = sclk_while(lambda: [tm_align.tm_align(d_prot, d_other, inits=mode) for _ in range(4)])
        events.clear()
        dps = got["init_dp"].sum(1)
        checked = []
        for p in () if opt.no_check else (0, len(got["tm"]) - 1):
            i, j = got["pairs"][p]
            t0 = time.perf_counter()
            want = (ta if mode == "default" else ti).align_structures(prot[i], (prot if other is None else other)[j])
            checked.append({"pair": [int(i), int(j)], "numpy_restatement_s": time.perf_counter() - t0, "tm": float(got["tm"][p]),
                            "abs_device_minus_restatement": abs(float(got["tm"][p]) - want["tm"]),
                            "alignment_equal": bool(np.array_equal(got["alignment"][p], want["alignment"])), "init_dp": got["init_dp"][p].tolist()})
        entry[mode] = {"pairs": int(len(got["tm"])), "first_call_wall_s": walls[mode][0], "call_wall_s": walls[mode][1:], "launch_device_ms": device_ms[mode],
                       "sclk_mhz": sclk, "tm_mean": float(got["tm"].mean()), "tm_min": float(got["tm"].min()), "tm_max": float(got["tm"].max()),
                       "dp_per_pair_mean": float(dps.mean()), "dp_per_pair_min": int(dps.min()), "dp_per_pair_max": int(dps.max()),
                       "best_init_counts": np.bincount(got["best_init"], minlength=tm_align.N_INITS[mode]).tolist(),
                       "n_aligned_mean": float(got["n_aligned"].mean()), "statuses": sorted(set(got["status"].tolist())), "checked": checked}
        if other is None:
            entry[mode].update({"diversity_at_0.5": tm_score.diversity(np.maximum(got["matrix"], fixed), 0.5)["diversity"],
                                "fixed_diversity_at_0.5": tm_score.diversity(fixed, 0.5)["diversity"], "fixed_won": int(np.triu(fixed > got["matrix"], 1).sum()),
                                "fixed_tm_min": float(fixed[np.triu_indices(len(fixed), 1)].min()),
                                "fixed_tm_max": float(fixed[np.triu_indices(len(fixed), 1)].max())})
    if opt.inits == "both":
        a, d = res["all"], res["default"]
        entry["all_against_default"] = {"tm_b_rose": int((a["tm_b"] > d["tm_b"]).sum()), "tm_b_fell": int((a["tm_b"] < d["tm_b"]).sum()),
                                        "largest_rise": float((a["tm_b"] - d["tm_b"]).max()), "largest_fall": float((d["tm_b"] - a["tm_b"]).max()),
                                        "won_by_i4_or_i5": int((a["best_init"] >= 3).sum()),
                                        "columns_0_to_2_equal": bool(np.array_equal(a["init_tm"][:, :3], d["init_tm"]) and np.array_equal(a["init_dp"][:, :3], d["init_dp"])),
                                        "launch_ratio": float(np.median(device_ms["all"]) / np.median(device_ms["default"]))}
    out[label] = entry[MODES[0]] if len(MODES) == 1 else entry
    print(label, json.dumps(out[label]), flush=True)
if opt.out:
    with open(opt.out, "w") as f:
        json.dump(out, f, indent=1)
