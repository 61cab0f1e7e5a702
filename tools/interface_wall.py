"""Wall time of the interface accuracy for the load the contract was sized on: 64 noisy copies (1 A per atom) of the 810-row 1fyt complex
(tests/golden/sasa_cases.npz) against it, over all ten chain pairs, for each atom set, with and without pruning, alternating the two.
Prints per atom set the wall time of ``interface.interface_accuracy`` calls (device tensors in, NumPy results out; the first call on its
own), the time of the three launches between device-side events, whether the pruned and the unpruned results are the same bits, and
the time of the same computation written in eager torch on the same GPU (float64; the reference's distances once per interface, the
models' per sample; contacts per residue pair through two membership products; both RMSDs through a batched SVD), with its counts
checked against the device's.  ``sclk_mhz``: the shader clock the driver reports (the marked level of the device's ``pp_dpm_sclk``, read
every 20 ms by a host thread during 40 further pruned calls; null where the file cannot be read).

    python tools/interface_wall.py [out.json]

``--mapped`` times the entry through a row map instead (``interface_accuracy(..., alignment=, coverage="penalise")``; DESIGN.md section
7.19) on the same load, for "cb" and "all", four variants in turn: the un-mapped call; an identity map; a map with a deleted window (rows
300 .. 339 of the reference have no model row); and what a caller without the mapped entry would do for that window - a torch gather of
the models into reference rows on the device, then the un-mapped call (its device time runs from in front of the gather to the end of
the launches).  Also says whether the identity map gave the un-mapped call's bits and the window map under "ignore" the gather's.

    python tools/interface_wall.py --mapped [out.json]
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
import interface_ref as ir  # noqa: E402

from framedipt_amd import _lib, interface  # noqa: E402

SAMPLES, REPEATS = 64, 5


def kabsch_rmsd(x, y, fit, evaluate):
    """x [S,M,3], y [M,3], fit, evaluate [M] bool -> [S]: RMSD of the atoms ``evaluate`` after the superposition of the atoms ``fit``."""
    xf, yf = x[:, fit], y[fit]
    cx, cy = xf.mean(1, keepdim=True), yf.mean(0, keepdim=True)
    u, _, vt = torch.linalg.svd((xf - cx).transpose(1, 2) @ (yf - cy))
    d = torch.sign(torch.linalg.det(u @ vt))
    u = torch.cat([u[:, :, :2], u[:, :, 2:] * d[:, None, None]], dim=2)
    moved = (x[:, evaluate] - cx) @ (u @ vt) + cy
    return ((moved - y[evaluate]) ** 2).sum(-1).mean(1).sqrt()


def torch_yardstick(models, truth, sides, mode, contact_cutoff, interface_cutoff=10.0, dev="cuda"):
    """The contract in eager torch for structures whose atoms all exist in every copy (the load of this tool).  -> n_native, n_model,
    n_shared [S,I] int64 and irmsd, lrmsd [S,I] float64 as NumPy arrays."""
    cols = ir.set_columns(mode, 37)
    has = np.any(truth[:, cols] != 0, axis=-1)
    if mode == "cb":
        has[:, 0] &= ~has[:, 1]
    row, atom = np.nonzero(has)
    y = torch.from_numpy(truth[:, cols][row, atom]).to(dev, torch.float64)
    x = torch.from_numpy(models[:, :, cols][:, row, atom]).to(dev, torch.float64)
    bb = [1] if mode == "ca" else [0, 1, 2, 4]
    brow, batom = np.nonzero(np.any(truth[:, bb] != 0, axis=-1))
    yb = torch.from_numpy(truth[:, bb][brow, batom]).to(dev, torch.float64)
    xb = torch.from_numpy(models[:, :, bb][:, brow, batom]).to(dev, torch.float64)
    n, s = truth.shape[0], models.shape[0]
    member = torch.zeros(n, len(row), device=dev)
    member[torch.from_numpy(row).to(dev), torch.arange(len(row), device=dev)] = 1.0
    out = {k: np.zeros((s, len(sides)), dtype=np.int64) for k in ("n_native", "n_model", "n_shared")}
    out.update(irmsd=np.zeros((s, len(sides))), lrmsd=np.zeros((s, len(sides))))
    for k, side in enumerate(sides):
        rec, lig = torch.from_numpy(side[row] == 1).to(dev), torch.from_numpy(side[row] == 2).to(dev)
        mr, ml = member[:, rec], member[:, lig]
        d2 = ((y[rec][:, None] - y[lig][None]) ** 2).sum(-1)
        native = (mr @ (d2 <= contact_cutoff ** 2).float() @ ml.T) > 0
        near = (mr @ (d2 <= interface_cutoff ** 2).float() @ ml.T) > 0
        at_interface = (near.any(1) | near.any(0)).cpu().numpy()
        for i in range(s):
            d2 = ((x[i, rec][:, None] - x[i, lig][None]) ** 2).sum(-1)
            model = (mr @ (d2 <= contact_cutoff ** 2).float() @ ml.T) > 0
            out["n_model"][i, k], out["n_shared"][i, k] = int(model.sum()), int((model & native).sum())
        out["n_native"][:, k] = int(native.sum())
        fit_i = torch.from_numpy(at_interface[brow]).to(dev)
        out["irmsd"][:, k] = kabsch_rmsd(xb, yb, fit_i, fit_i).cpu().numpy()
        out["lrmsd"][:, k] = kabsch_rmsd(xb, yb, torch.from_numpy(side[brow] == 1).to(dev), torch.from_numpy(side[brow] == 2).to(dev)).cpu().numpy()
    return out


def sclk_path():
    """The sysfs file with the shader clock levels of device 0, or None."""
    try:
        prop = torch.cuda.get_device_properties(0)
        path = f"/sys/bus/pci/devices/{prop.pci_domain_id:04x}:{prop.pci_bus_id:02x}:{prop.pci_device_id:02x}.0/pp_dpm_sclk"
        return path if os.path.exists(path) else None
    except Exception:  # noqa: BLE001  (an older torch without the PCI ids: no clock is reported)
        return None


def sclk_while(work):
    """Run ``work()`` while a thread samples the marked clock level: [min, max] MHz over the samples, or None (as tools/tm_wall.py)."""
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


def load(samples=SAMPLES):
    pos, chain = ir.complex_atom37("1fyt")
    rng = np.random.RandomState(810)
    noise = rng.normal(0.0, 1.0, size=(samples,) + pos.shape).astype(np.float32)
    models = np.where(np.any(pos != 0, axis=-1, keepdims=True)[None], pos[None] + noise, np.float32(0)).astype(np.float32)
    return pos, models, interface.chain_sides(chain)[0]


def main():
    lib = _lib.load()
    launch, events = lib.fdipt_sample_interface, []

    def timed_launch(args, stream):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        rc = launch(args, stream)
        stop.record()
        events.append((start, stop))
        return rc

    lib.fdipt_sample_interface = timed_launch
    pos, models, sides = load()
    d_models, d_truth, d_sides = torch.from_numpy(models).cuda(), torch.from_numpy(pos[None]).cuda(), torch.from_numpy(sides).cuda()
    torch.cuda.synchronize()
    out = {"load": {"samples": SAMPLES, "rows": int(pos.shape[0]), "interfaces": int(len(sides)), "repeats": REPEATS}}
    for mode in ("ca", "cb", "backbone", "all"):
        walls, device_ms, res = {True: [], False: []}, {True: [], False: []}, {}
        for _ in range(1 + REPEATS):  # (the first round is the warm-up of both)
            for prune in (True, False):
                t0 = time.perf_counter()
                res[prune] = interface.interface_accuracy(d_models, d_truth, d_sides, atoms=mode, prune=prune)
                walls[prune].append(time.perf_counter() - t0)
                torch.cuda.synchronize()
                device_ms[prune].append(events[-1][0].elapsed_time(events[-1][1]))
        same = all(np.array_equal(res[True][k], res[False][k], equal_nan=True) for k in ir.INT_OUTPUTS + ir.ROW_OUTPUTS + ir.FLOAT_OUTPUTS)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        yard = torch_yardstick(models, pos, sides, mode, interface.CONTACT_CUTOFF[mode])
        torch.cuda.synchronize()
        t_first = time.perf_counter() - t0
        t0 = time.perf_counter()
        yard = torch_yardstick(models, pos, sides, mode, interface.CONTACT_CUTOFF[mode])
        torch.cuda.synchronize()
        t_torch = time.perf_counter() - t0
        ok = np.isfinite(res[True]["irmsd"])
        sclk = sclk_while(lambda: [interface.interface_accuracy(d_models, d_truth, d_sides, atoms=mode) for _ in range(40)])
        out[mode] = {"pruned_first_call_wall_s": walls[True][0], "pruned_call_wall_s": walls[True][1:], "unpruned_call_wall_s": walls[False][1:],
                     "pruned_launches_device_ms": device_ms[True][1:], "unpruned_launches_device_ms": device_ms[False][1:], "pruned_equals_unpruned": bool(same), "sclk_mhz": sclk,
                     "torch_eager_first_s": t_first, "torch_eager_s": t_torch,
                     "torch_counts_equal": bool(all(np.array_equal(yard[k], res[True][k]) for k in ("n_native", "n_model", "n_shared"))),
                     "torch_worst_irmsd_difference": float(np.abs(yard["irmsd"] - res[True]["irmsd"])[ok].max()),
                     "torch_worst_lrmsd_difference": float(np.abs(yard["lrmsd"] - res[True]["lrmsd"]).max()),
                     "mean_fnat": float(res[True]["fnat"].mean()), "mean_dockq": float(np.nanmean(res[True]["dockq"]))}
        print(mode, json.dumps(out[mode]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


def main_mapped(path=None):
    lib = _lib.load()
    events = []

    def timed(launch):
        def call(*args):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            rc = launch(*args)
            stop.record()
            events.append((start, stop))
            return rc
        return call

    lib.fdipt_sample_interface, lib.fdipt_sample_interface_mapped = timed(lib.fdipt_sample_interface), timed(lib.fdipt_sample_interface_mapped)
    pos, models, sides = load()
    n = int(pos.shape[0])
    d_models, d_truth, d_sides = torch.from_numpy(models).cuda(), torch.from_numpy(pos[None]).cuda(), torch.from_numpy(sides).cuda()
    identity = torch.arange(n, dtype=torch.int32, device="cuda")
    window = identity.clone()
    window[300:340] = -1
    keys = ir.INT_OUTPUTS + ir.ROW_OUTPUTS + ir.FLOAT_OUTPUTS
    out = {"load": {"samples": SAMPLES, "rows": n, "interfaces": int(len(sides)), "repeats": REPEATS, "window": [300, 339]}}

    def gather_then_unmapped(mode):
        start = torch.cuda.Event(enable_timing=True)
        start.record()
        rows = (window >= 0).float()
        gathered = d_models[:, window.clamp(min=0).long()] * rows[None, :, None, None]
        res = interface.interface_accuracy(gathered, d_truth, d_sides, atoms=mode, res_mask=rows[None].expand(SAMPLES, n))
        events.append((start, events[-1][1]))
        return res

    for mode in ("cb", "all"):
        variants = {"unmapped": lambda: interface.interface_accuracy(d_models, d_truth, d_sides, atoms=mode),
                    "identity_map": lambda: interface.interface_accuracy(d_models, d_truth, d_sides, atoms=mode, alignment=identity, coverage="penalise"),
                    "window_map": lambda: interface.interface_accuracy(d_models, d_truth, d_sides, atoms=mode, alignment=window, coverage="penalise"),
                    "gather_then_unmapped": lambda: gather_then_unmapped(mode)}
        walls, device_ms, res = {k: [] for k in variants}, {k: [] for k in variants}, {}
        for _ in range(1 + REPEATS):  # (the first round is the warm-up of all four)
            for name, run in variants.items():
                t0 = time.perf_counter()
                res[name] = run()
                walls[name].append(time.perf_counter() - t0)
                torch.cuda.synchronize()
                device_ms[name].append(events[-1][0].elapsed_time(events[-1][1]))
        ignore = interface.interface_accuracy(d_models, d_truth, d_sides, atoms=mode, alignment=window, coverage="ignore")
        sclk = sclk_while(lambda: [variants["window_map"]() for _ in range(40)])
        out[mode] = {name: {"call_wall_s": walls[name][1:], "launches_device_ms": device_ms[name][1:]} for name in variants}
        out[mode].update(identity_equals_unmapped=bool(all(np.array_equal(res["identity_map"][k], res["unmapped"][k], equal_nan=True) for k in keys)),
                         window_ignore_equals_gather=bool(all(np.array_equal(ignore[k], res["gather_then_unmapped"][k], equal_nan=True) for k in keys)),
                         mean_fnat={name: float(res[name]["fnat"].mean()) for name in variants}, sclk_mhz=sclk)
        print(mode, json.dumps(out[mode]), flush=True)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    if "--mapped" in sys.argv[1:]:
        main_mapped(*[a for a in sys.argv[1:] if a != "--mapped"][:1])
    else:
        main()
