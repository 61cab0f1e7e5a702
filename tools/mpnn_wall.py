"""Wall time of inverse folding (framedipt_amd/inverse_folding.py) for the load of one sharded batch: 8 backbones of 300 rows (random-walk
CA traces, tests/mpnn_ref.py:backbone), 8 sequences each at T = 0.1, synthetic parameters, K = 48.  Prints the wall time of ``design``
calls (device tensor in, NumPy results out, the rescoring included; the first call on its own) and of ``score`` calls for the same 64
sequences, the time between device-side events around each C entry, and the time of the torch restatement (tests/mpnn_ref.py) of the same
work in eager mode, float32, on the same GPU - the stand-in for what the reference's subprocess computes, without its PDB parsing - with
the number of letters in which the two disagree (float32 rounding next to a boundary of a cumulative distribution; not a parity claim).
One run; no threshold is attached to these times.  ``--tied``: the same load as a 3 x 100 homo-trimer, row r of the three chains tied
(DESIGN.md section 7.11); the restatement is then not run.  ``--ca-only``: the CA-only model on the same traces,
given as [B,N,3], and the vanilla model's design and score calls next to it in the same run (``vanilla``); the restatement is that of
tests/mpnn_ca_ref.py.

    python tools/mpnn_wall.py [out.json] [--restatement-sequences K] [--tied] [--ca-only]
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
import mpnn_ca_ref as mc  # noqa: E402
import mpnn_ref as mr  # noqa: E402

from framedipt_amd import _lib  # noqa: E402
from framedipt_amd import inverse_folding as inv  # noqa: E402

B, N, M, K, T = 8, 300, 8, 48, 0.1
ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=None)
ap.add_argument("--restatement-sequences", type=int, default=B * M, help="time the restatement on the first K sequences and scale")
ap.add_argument("--tied", action="store_true", help="three chains of 100 rows, row r of every chain tied")
ap.add_argument("--ca-only", action="store_true", help="the CA-only model on the CA traces, the vanilla model beside it")
cli = ap.parse_args()
n_restatement = 0 if cli.tied else cli.restatement_sequences

lib = _lib.load()
events = {"fdipt_mpnn_design": [], "fdipt_mpnn_score": []}


def timed(name):
    launch = getattr(lib, name)

    def call(dims, args, stream):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        rc = launch(dims, args, stream)
        stop.record()
        events[name].append((start, stop))
        return rc

    return call


lib.fdipt_mpnn_design, lib.fdipt_mpnn_score = timed("fdipt_mpnn_design"), timed("fdipt_mpnn_score")

rng = np.random.default_rng(0)
prot = np.stack([mr.backbone(rng, N) for _ in range(B)])
d_prot = torch.from_numpy(np.ascontiguousarray(prot[:, :, 1]) if cli.ca_only else prot).cuda()
model = inv.ProteinMPNN(K, ca_only=cli.ca_only).load_synthetic(mr.WEIGHT_SEED)
torch.cuda.synchronize()

out = {"backbones": B, "rows": N, "sequences_per_backbone": M, "k_neighbors": K, "temperature": T, "tied": cli.tied, "ca_only": cli.ca_only}
chains = {}
if cli.tied:
    chains = {"chain_idx": np.tile(np.repeat([1, 2, 3], N // 3), (B, 1)), "residue_index": np.tile(np.arange(N // 3), (B, 3))}
    chains["tied_positions"] = inv.tied_positions_from_chains(chains["chain_idx"][0])  # one list of groups serves every backbone
walls = []
for _ in range(3):
    t0 = time.perf_counter()
    des = model.design(d_prot, num_seq=M, temperature=T, seed=38, **chains)
    walls.append(time.perf_counter() - t0)
out["design"] = {"first_call_wall_s": walls[0], "call_wall_s": walls[1:], "letters_used": int(len(np.unique(des["S"]))),
                 "score_mean": float(des["score"].mean()), "statuses": sorted(set(des["status"].tolist()))}
walls = []
for _ in range(3):
    t0 = time.perf_counter()
    sc = model.score(d_prot, des["S"], decoding_order=des["decoding_order"], **{k: v for k, v in chains.items() if k != "tied_positions"})
    walls.append(time.perf_counter() - t0)
torch.cuda.synchronize()
out["score"] = {"first_call_wall_s": walls[0], "call_wall_s": walls[1:], "equals_design_rescoring": bool(np.array_equal(sc["log_probs"], des["log_probs"]))}
# design() launches the design entry and then the score entry (its rescoring); score() the score entry alone
out["device_ms"] = {name: [start.elapsed_time(stop) for start, stop in evs] for name, evs in events.items()}
if cli.ca_only:  # the vanilla model on the full backbones of the same traces, after the CA-only calls, for the comparison of section 7.12
    for evs in events.values():
        evs.clear()
    vanilla, d_full, walls = inv.ProteinMPNN(K).load_synthetic(mr.WEIGHT_SEED), torch.from_numpy(prot).cuda(), {"design": [], "score": []}
    for _ in range(3):
        t0 = time.perf_counter()
        vdes = vanilla.design(d_full, num_seq=M, temperature=T, seed=38, **chains)
        walls["design"].append(time.perf_counter() - t0)
    for _ in range(3):
        t0 = time.perf_counter()
        vanilla.score(d_full, vdes["S"], decoding_order=vdes["decoding_order"], **{k: v for k, v in chains.items() if k != "tied_positions"})
        walls["score"].append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    out["vanilla"] = {"design_call_wall_s": walls["design"][1:], "score_call_wall_s": walls["score"][1:],
                      "device_ms": {name: [start.elapsed_time(stop) for start, stop in evs] for name, evs in events.items()}}
print(json.dumps(out), flush=True)

# the torch restatement, eager, float32, on the same GPU: encoder once per backbone, then per sequence the design loop and its rescoring
sd = inv.synthetic_state_dict(mr.WEIGHT_SEED, K, ca_only=cli.ca_only)
ref = mr.Model(sd, K, torch.float32, "cuda")
ones, index = np.ones(N, np.float32), np.arange(N)
omit = np.array([0.0] * 20 + [1.0], np.float32)
bias = np.zeros(21, np.float32)
done, differ, t_enc, t_design, t_score = 0, 0, 0.0, 0.0, 0.0
with torch.no_grad():
    for b in range(B):
        if done >= n_restatement:
            break
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc = mc.encode_ca(ref, prot[b][:, 1], ones, index, ones) if cli.ca_only else mr.encode(ref, prot[b], ones, index, ones)
        torch.cuda.synchronize()
        t_enc += time.perf_counter() - t0
        for m in range(M):
            if done >= n_restatement:
                break
            t0 = time.perf_counter()
            S, _, _ = mr.design(ref, enc, ones, ones, des["S_input"][b], des["decoding_order"][b, m], des["u"][b, m], T, omit, bias)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            mr.score(ref, enc, ones, S, des["decoding_order"][b, m]).cpu()
            t2 = time.perf_counter()
            t_design, t_score = t_design + t1 - t0, t_score + t2 - t1
            differ += int((S.cpu().numpy() != des["S"][b, m]).sum())
            done += 1
scale = B * M / max(done, 1)
out["torch_eager_restatement"] = {"sequences_timed": done, "encode_s": t_enc, "design_s": t_design, "score_s": t_score,
                                  "design_and_rescoring_s_for_all": (t_enc + t_design + t_score) * scale, "letters_differing_from_device": differ,
                                  "letters_compared": done * N}
print(json.dumps(out["torch_eager_restatement"]), flush=True)
if cli.out:
    with open(cli.out, "w") as f:
        json.dump(out, f, indent=1)
