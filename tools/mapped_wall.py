"""Wall time of the mapped accuracy entries for two loads, synthetic coordinates as tools/lddt_wall.py builds them:

* 64 samples x N = 300 against one reference through an identity map, on the CA and on the backbone atoms, beside (a) the un-mapped
  entry on the same arrays and (b) what a user did before the mapped entries existed: a ``torch`` gather of the model rows into a
  [P, N_b, atoms, 3] copy, then the un-mapped entry - lDDT and GDT (``superpose="search"``) each;
* the 2 016 pairs i < j of 64 samples x N = 300 through ``tm_align``'s own alignments (the samples differ by a window shift, so the
  alignments are not the identity): the mapped lDDT on the CA atoms and the mapped GDT of all pairs.

Prints per load the wall time of the calls (device tensors in, NumPy results out; the first call on its own) and the time of the
launches between device-side events.

    python tools/mapped_wall.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from framedipt_amd import _call, _lib, gdt, lddt, tm_align  # noqa: E402

lib = _lib.load()
events = {}


def timed(name):
    launch = getattr(lib, name)

    def call(*args):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        rc = launch(*args)
        stop.record()
        events.setdefault(name, []).append((start, stop))
        return rc

    setattr(lib, name, call)


for entry in ("fdipt_sample_lddt", "fdipt_sample_lddt_mapped", "fdipt_sample_gdt", "fdipt_sample_gdt_mapped"):
    timed(entry)


def measure(fn, repeats=5):
    """(result, wall seconds per call, device milliseconds per entry name)."""
    events.clear()
    torch.cuda.synchronize()
    walls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = fn()
        walls.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    return res, walls, {k: [a.elapsed_time(b) for a, b in v] for k, v in events.items()}


def structures(b, n, seed):
    rng = np.random.default_rng(seed)
    steps = rng.normal(size=(n + b, 3))
    ca = 40.0 + np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=-1, keepdims=True), axis=0)
    walk = np.zeros((n + b, 37, 3), dtype=np.float32)
    walk[:, :5] = ca[:, None] + 0.9 * rng.normal(size=(n + b, 5, 3))
    truth = walk[None, :n].copy()
    prot = np.zeros((b, n, 37, 3), dtype=np.float32)
    prot[:, :, :5] = truth[:, :, :5] + rng.choice([0.1, 0.5, 1.5], size=(b, n, 1, 1)) * rng.normal(size=(b, n, 1, 3)) + 0.05 * rng.normal(size=(b, n, 5, 3))
    shifted = np.stack([walk[s % 8:s % 8 + n] for s in range(b)]).copy()  # windows of one walk, up to 7 rows apart
    shifted[:, :, :5] += 0.3 * rng.normal(size=(b, n, 1, 3)).astype(np.float32)
    return prot, truth, shifted


out = {}
b, n = 64, 300
prot, truth, shifted = structures(b, n, n)
d_prot, d_truth = torch.from_numpy(prot).cuda(), torch.from_numpy(truth).cuda()
identity = torch.arange(n, dtype=torch.int32, device="cuda")
for mode in ("ca", "backbone"):
    plain, w_plain, e_plain = measure(lambda: lddt.local_accuracy(d_prot, d_truth, atoms=mode))
    mapped, w_mapped, e_mapped = measure(lambda: lddt.local_accuracy(d_prot, d_truth, atoms=mode, alignment=identity))
    gathered, w_gather, e_gather = measure(lambda: lddt.local_accuracy(d_prot[:, identity.long()].contiguous(), d_truth, atoms=mode))
    assert all(np.array_equal(plain[k], mapped[k]) and np.array_equal(plain[k], gathered[k]) for k in ("lddt", "res_lddt", "n_scored", "fape", "drmsd"))
    out[f"identity_b64_n300_lddt_{mode}"] = {
        "pairs": b, "unmapped": {"first_call_wall_s": w_plain[0], "call_wall_s": w_plain[1:], "device_ms": e_plain["fdipt_sample_lddt"]},
        "mapped": {"first_call_wall_s": w_mapped[0], "call_wall_s": w_mapped[1:], "device_ms": e_mapped["fdipt_sample_lddt_mapped"]},
        "torch_gather_then_unmapped": {"first_call_wall_s": w_gather[0], "call_wall_s": w_gather[1:], "device_ms": e_gather["fdipt_sample_lddt"]}}
    print(mode, json.dumps(out[f"identity_b64_n300_lddt_{mode}"]), flush=True)
plain, w_plain, e_plain = measure(lambda: gdt.gdt_scores(d_prot, d_truth))
mapped, w_mapped, e_mapped = measure(lambda: gdt.gdt_scores(d_prot, d_truth, alignment=identity))
gathered, w_gather, e_gather = measure(lambda: gdt.gdt_scores(d_prot[:, identity.long()].contiguous(), d_truth))
assert all(np.array_equal(plain[k], mapped[k]) and np.array_equal(plain[k], gathered[k]) for k in ("gdt_ts", "counts", "res_within"))
out["identity_b64_n300_gdt_search"] = {
    "pairs": b, "unmapped": {"first_call_wall_s": w_plain[0], "call_wall_s": w_plain[1:], "device_ms": e_plain["fdipt_sample_gdt"]},
    "mapped": {"first_call_wall_s": w_mapped[0], "call_wall_s": w_mapped[1:], "device_ms": e_mapped["fdipt_sample_gdt_mapped"]},
    "torch_gather_then_unmapped": {"first_call_wall_s": w_gather[0], "call_wall_s": w_gather[1:], "device_ms": e_gather["fdipt_sample_gdt"]}}
print("gdt", json.dumps(out["identity_b64_n300_gdt_search"]), flush=True)

d_shift = torch.from_numpy(shifted).cuda()
pairs = _call.all_pairs(b)
t0 = time.perf_counter()
found = tm_align.tm_align(d_shift, pairs=pairs)
align_s = time.perf_counter() - t0
maps = torch.from_numpy(found["alignment"].astype(np.int32)).cuda()
res_l, w_l, e_l = measure(lambda: lddt.local_accuracy(d_shift, d_shift, atoms="ca", pairs=pairs, alignment=maps, coverage="penalise"), repeats=3)
res_g, w_g, e_g = measure(lambda: gdt.gdt_scores(d_shift, d_shift, pairs=pairs, alignment=maps, norm_length="reference"), repeats=3)
out["aligned_2016_pairs_n300"] = {
    "pairs": int(len(pairs)), "tm_align_wall_s": align_s, "mean_n_aligned": float(found["n_aligned"].mean()), "identity_maps": int((found["alignment"] == np.arange(n)).all(1).sum()),
    "lddt_ca_mapped": {"first_call_wall_s": w_l[0], "call_wall_s": w_l[1:], "device_ms": e_l["fdipt_sample_lddt_mapped"], "mean_lddt": float(res_l["lddt"].mean()),
                       "mean_coverage": float(res_l["coverage"].mean())},
    "gdt_search_mapped": {"first_call_wall_s": w_g[0], "call_wall_s": w_g[1:], "device_ms": e_g["fdipt_sample_gdt_mapped"], "mean_gdt_ts": float(np.nanmean(res_g["gdt_ts"]))}}
print("aligned", json.dumps(out["aligned_2016_pairs_n300"]), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
