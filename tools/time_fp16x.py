#!/usr/bin/env python
"""fp16 and fp16x side by side on one GPU (the c4 workload: de novo, N = 300, 8 samples): whole trajectories of T steps through
inference_fn (step-graph replays, the product path), the two modes interleaved, wall time per step.  DESIGN.md section 5 quotes it.

    python tools/time_fp16x.py [--n 300] [--b 8] [--t 20] [--rounds 3]
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
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--b", type=int, default=8)
    ap.add_argument("--t", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from framedipt_amd import config, sharding
    from framedipt_amd.diffusion import SE3Diffuser
    from framedipt_amd.inference import inference_fn
    from framedipt_amd.model import ScoreNetwork
    from framedipt_amd.sampler import UnconditionalSampler
    conf = config.base_config()
    d = SE3Diffuser(conf.diffuser, device="cuda")
    ds = UnconditionalSampler(config.to_conf({"min_length": a.n, "max_length": a.n, "length_step": 1, "samples_per_length": a.b}), d, "cuda")
    feats, tape = sharding.stack_items([sharding.seeded_item(ds, i, 5, d, a.t, 0.01) for i in range(a.b)])
    nets = {p: ScoreNetwork(conf.model, d, precision=p).load_synthetic(7).to("cuda") for p in ("fp16", "fp16x")}
    kw = dict(num_t=a.t, min_t=0.01, aux_traj=False, noise_scale=0.1, noise_tape=tape)
    for net in nets.values():  # warm-up: lazy set-up, graph capture
        inference_fn(net, d, feats, **kw)
    torch.cuda.synchronize()
    ms = {p: [] for p in nets}
    for _ in range(a.rounds):
        for p, net in nets.items():
            t0 = time.perf_counter()
            inference_fn(net, d, feats, **kw)
            torch.cuda.synchronize()
            ms[p].append((time.perf_counter() - t0) * 1e3 / a.t)
    med = {p: float(np.median(v)) for p, v in ms.items()}
    print(json.dumps({"n": a.n, "b": a.b, "t": a.t, "ms_per_step": {p: [round(x, 3) for x in v] for p, v in ms.items()},
                      "median_ms_per_step": med, "fp16x_over_fp16": med["fp16x"] / med["fp16"],
                      "residue_steps_per_s": {p: a.n * a.b / (m * 1e-3) for p, m in med.items()}}))


if __name__ == "__main__":
    main()
