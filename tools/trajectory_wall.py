#!/usr/bin/env python
"""Wall time of whole trajectories from "features in hand" to "results on the host", host noise tape against device noise.

One mode per process (run it once per mode, interleaved, on one GPU): de novo, --n residues, --b samples, --t steps, aux_traj=True,
through ReverseLoop (step-graph replays, the product path).  Per trajectory: tape draw, loop set-up (with the upload of the tape),
priming + first steps + graph capture, the remaining loop, results(); and the GPU time per replayed step (HIP events around the
replays).  The first trajectory of a process also pays the lazy set-up of the kernels; the JSON line carries every trajectory.
On a tree without noise="device" only the host mode runs.  DESIGN.md section 7 quotes the table.
--keep all|last|<stride>: kept-frame trajectories; --session: the trajectories of the process run through one inference.Session (the second
and later ones reset the first one's loop and replay its graphs).  Both are ignored with a note on a tree that does not have them, so the
same command lines time a parent checkout.  peak_alloc_mb: torch's peak allocated HBM over the trajectory.

    python tools/trajectory_wall.py [--noise host|device] [--n 300] [--b 8] [--t 500] [--precision fp16] [--reps 2] [--keep last] [--session]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise", default="host", choices=["host", "device"])
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--t", type=int, default=500)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--tag", default="")
    ap.add_argument("--keep", default="all")
    ap.add_argument("--session", action="store_true")
    a = ap.parse_args()
    keep = a.keep if a.keep in ("all", "last") else int(a.keep)
    import numpy as np
    import torch
    from framedipt_amd import config, inference
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import UnconditionalSampler
    conf = config.base_config()
    d = SE3Diffuser(conf.diffuser, device="cuda")
    net = ScoreNetwork(conf.model, d, precision=a.precision).load_synthetic(7).to("cuda")
    ds = UnconditionalSampler(config.to_conf({"min_length": a.n, "max_length": a.n, "length_step": 1, "samples_per_length": a.b}), d, "cuda")
    np.random.seed(11)
    feats = {k: torch.cat([ds[i][2][k] for i in range(a.b)], 0) for k in ds[0][2]}
    min_t, T = 0.01, a.t
    n_noisy = int(np.sum(np.linspace(min_t, 1.0, T)[::-1] > min_t))
    chunk = inference.ReverseLoop.GRAPH_CHUNK
    k0 = 2 * chunk                                   # eager first step, captures and first replays stay outside the event pair
    k1 = k0 + (n_noisy - k0) // chunk * chunk        # whole chunk replays only
    sync = torch.cuda.synchronize
    rows = []
    has_keep = hasattr(inference, "kept_steps")
    if not has_keep and (keep != "all" or a.session):
        print("this tree has no keep= / Session: running the default path", file=sys.stderr)
        keep, a.session = "all", False
    n_kept = len(inference.kept_steps(T, keep)) if has_keep else T
    session = inference.Session() if a.session else None
    opts = dict(aux_traj=True, noise_scale=0.1, **({"keep": keep} if has_keep else {}))
    for rep in range(a.reps):
        sync()
        torch.cuda.reset_peak_memory_stats()
        w = {}
        t0 = time.perf_counter()
        if a.noise == "host":
            tape = inference.draw_noise_tape(d, n_noisy, a.b, a.n)
            how = dict(noise_tape=tape)
        else:
            how = dict(noise="device", noise_keys=1000 + rep * a.b)
        w["draw_s"] = time.perf_counter() - t0
        t1 = time.perf_counter()
        if session is not None:
            loop = session.loop(net, d, feats, T, min_t, noise_tape=how.get("noise_tape"), noise_keys=how.get("noise_keys"), **opts)
        else:
            loop = inference.ReverseLoop(net, d, feats, T, min_t, **opts, **how)
        captures_before = getattr(loop, "captures", 0)
        sync()
        w["setup_upload_s"] = time.perf_counter() - t1
        t2 = time.perf_counter()
        loop.prime()
        loop.run_steps(0, k0)
        sync()
        w["prime_capture_s"] = time.perf_counter() - t2
        t3 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loop.run_steps(k0, k1)
        e1.record()
        loop.run_steps(k1, T)
        sync()
        w["loop_s"] = time.perf_counter() - t3
        t4 = time.perf_counter()
        res = loop.results()
        w["results_s"] = time.perf_counter() - t4
        w["wall_s"] = time.perf_counter() - t0
        w["gpu_ms_per_step"] = e0.elapsed_time(e1) / max(1, k1 - k0)
        w["capture_s"] = loop.capture_seconds  # (cumulative over a session loop's life)
        w["captures"] = getattr(loop, "captures", 0) - captures_before
        w["peak_alloc_mb"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        w["noise_bytes_on_device"] = 0 if loop.z_rot is None else int(loop.z_rot.numel() + loop.z_trans.numel()) * 8
        assert res["prot_traj"].shape == (n_kept, a.b, a.n, 37, 3) and np.isfinite(res["prot_traj"]).all()
        if a.noise == "host":  # the upload alone, outside the wall time above
            sync()
            t5 = time.perf_counter()
            up = [torch.as_tensor(np.ascontiguousarray(z, dtype=np.float64), device="cuda") for z in tape]
            sync()
            w["upload_alone_s"] = time.perf_counter() - t5
            del up, tape
        del loop, res
        rows.append({k: round(v, 5) if isinstance(v, float) else v for k, v in w.items()})
    print(json.dumps({"tool": "trajectory_wall", "tag": a.tag, "noise": a.noise, "n": a.n, "b": a.b, "t": T, "precision": a.precision,
                      "event_steps": k1 - k0, "keep": keep, "session": bool(a.session), "trajectories": rows}), flush=True)


if __name__ == "__main__":
    main()
