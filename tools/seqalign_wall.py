"""Wall time of sequence alignment on the device for four loads of random 20-letter sequences:

* 512 sequences of 300 letters all against all (130 816 pairs), score only and with the traceback;
* 64 sequences of 300 letters against one;
* one pair of 2048 x 2048.

Prints per load the wall time of the calls (device tensors in, NumPy results out; the first call on its own), the time of the launch
between device-side events, the persistent waves the workspace cap produced (traceback), and beside it - as a yardstick, not a claim - the
wall time of the NumPy restatement (tests/seqalign_ref.py) on a sample of the same pairs, scaled to the load.  ``sclk_mhz``: the shader
clock the driver reports during further calls of the load (tools/interface_wall.py: ``sclk_while``; null where it cannot be read).

``--mode local`` / ``--mode semiglobal`` (every end gap free) time the same four loads through fdipt_seq_align_modes (DESIGN.md section
7.20; the restatement beside them is tests/seqalign_modes_ref.py); the default is the global entry.

    python tools/seqalign_wall.py [--mode {global,local,semiglobal}] [out.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import seqalign_modes_ref  # noqa: E402
import seqalign_ref  # noqa: E402
from framedipt_amd import _lib, seq_align  # noqa: E402
from interface_wall import sclk_while  # noqa: E402  (tools/: the shader clock the driver reports while a load runs)

MODE = "global"
if "--mode" in sys.argv:
    k = sys.argv.index("--mode")
    MODE = sys.argv[k + 1]
    del sys.argv[k:k + 2]
if MODE not in seq_align.MODES:
    sys.exit(f"--mode should be one of {sorted(seq_align.MODES)}")
ENTRY = "fdipt_seq_align" if MODE == "global" else "fdipt_seq_align_modes"

lib = _lib.load()
events = []
launch = getattr(lib, ENTRY)


def timed(*args):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    rc = launch(*args)
    stop.record()
    events.append((start, stop))
    return rc


setattr(lib, ENTRY, timed)


def measure(fn, repeats):
    events.clear()
    torch.cuda.synchronize()
    walls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = fn()
        walls.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    return res, walls, [a.elapsed_time(b) for a, b in events]


def restatement_wall(seqs_a, seqs_b, pairs, sample):
    """Seconds per pair of the NumPy restatement over ``sample`` of the pairs."""
    table = seq_align.table_half_units("blosum62").astype(np.int64)
    rows = pairs[np.linspace(0, len(pairs) - 1, sample).astype(int)]
    t0 = time.perf_counter()
    for i, j in rows:
        if MODE == "global":
            seqalign_ref.align(seqs_a[i], seqs_b[j], table, -20, -1)
        else:
            seqalign_modes_ref.align(seqs_a[i], seqs_b[j], table, -20, -1, seq_align.MODES[MODE], 15 if MODE == "semiglobal" else 0)
    return (time.perf_counter() - t0) / len(rows)


def load(name, xa, xb, repeats, sample, **kw):
    dev = torch.device("cuda", torch.cuda.current_device())
    da, db = torch.from_numpy(xa).to(dev), None if xb is None else torch.from_numpy(xb).to(dev)
    res, walls, device_ms = measure(lambda: seq_align.align_sequences(da, db, mode=MODE, **kw), repeats)
    n_pairs = len(res["pairs"])
    traceback = kw.get("traceback", True)
    slab = xa.shape[1] * (xa if xb is None else xb).shape[1]
    waves = int(getattr(lib, ENTRY + "_workspace_bytes")(n_pairs, xa.shape[1], (xa if xb is None else xb).shape[1], 1, 2 ** 30)) // slab if traceback else None
    sclk = sclk_while(lambda: [seq_align.align_sequences(da, db, mode=MODE, **kw) for _ in range(repeats)])
    per_pair = restatement_wall(xa, xa if xb is None else xb, res["pairs"], sample)
    out = {"mode": MODE, "pairs": n_pairs, "traceback": traceback, "first_call_wall_s": walls[0], "call_wall_s": walls[1:], "device_ms": device_ms[:repeats], "sclk_mhz": sclk,
           "persistent_waves_of_the_slabs": waves, "mean_identity_short": float(res["identity_short"].mean()),
           "restatement_s_per_pair": per_pair, "restatement_s_scaled_to_load": per_pair * n_pairs}
    print(name, json.dumps(out), flush=True)
    return out


def main():
    rng = np.random.default_rng(0)
    x512, one, x2048 = rng.integers(0, 20, (512, 300)), rng.integers(0, 20, (1, 300)), rng.integers(0, 20, (2, 2048))
    out = {"all_against_all_512x300_score_only": load("512 x 300 all against all, score only", x512, None, 4, 8, traceback=False),
           "all_against_all_512x300_traceback": load("512 x 300 all against all, traceback", x512, None, 3, 8),
           "64x300_against_one": load("64 x 300 against one", x512[:64], one, 4, 8),
           "one_pair_2048x2048": load("one pair of 2048 x 2048", x2048[:1], x2048[1:], 4, 1),
           "one_pair_2048x2048_score_only": load("one pair of 2048 x 2048, score only", x2048[:1], x2048[1:], 4, 1, traceback=False)}
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
