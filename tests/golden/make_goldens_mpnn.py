"""Fixtures of the inverse-folding tests, captured from the reference's ProteinMPNN (this container only):

    python tests/golden/make_goldens_mpnn.py      # -> tests/golden/mpnn_<case>.npz

Per case of tests/mpnn_ref.py (CASES: a to d) the reference model (ProteinMPNN/protein_mpnn_utils.py:ProteinMPNN, float32 on the CPU,
eval mode, augment_eps 0) is loaded with ``inverse_folding.synthetic_state_dict(WEIGHT_SEED, K)`` and run on ``mpnn_ref.make_case``:

* ``forward(..., use_input_decoding_order=True)`` per sequence -> ``log_probs`` [B,M,N,21];
* ``features`` -> ``E_idx`` [B,N,K_eff] (torch.topk: compared as sets per row);
* ``sample`` per sequence and temperature with ``torch.multinomial`` replaced by the contract's inverse-CDF rule on the recorded
  uniforms -> ``S_T<t>`` [B,M,N], ``probs_T<t>`` [B,M,N,21].

No weights are stored: they come back from the seed.  The input seed of a case is searched upward from 0 until the float64 restatement
says that (1) every row with res_mask and N > K has at least 1e-3 A between its K-th and (K+1)-th distance and (2) every draw lies at
least 1e-4 from every boundary of its row's cumulative distribution; both are asserted again on the recorded case.  The script prints
the largest deviation of the reference's float32 outputs from the float64 restatement over the rows with res_mask: the yardstick of
the tests' tolerance (mpnn_ref.DEVIATION).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import refharness as rh  # noqa: E402

sys.path.insert(0, os.path.join(rh.REF, "ProteinMPNN"))
import protein_mpnn_utils as pmu  # noqa: E402

import mpnn_ref as mr  # noqa: E402
from framedipt_amd import inverse_folding as inv  # noqa: E402

MIN_GAP, MIN_MARGIN = 1e-3, 1e-4


def conditions(name, case, res):
    valid = case["res_mask"] != 0
    return float(res["gap"][valid].min()), min(d["margin"] for d in res["design"].values())


def reference_model(sd, k):
    model = pmu.ProteinMPNN(num_letters=21, node_features=128, edge_features=128, hidden_dim=128, num_encoder_layers=3, num_decoder_layers=3,
                            augment_eps=0.0, k_neighbors=k)
    model.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    return model.eval()


def inverse_cdf(u_rows):
    """A stand-in for torch.multinomial inside ``sample`` (batch 1): the rows arrive in decoding order, masked rows skipped."""
    rows = iter(u_rows)

    def draw(probs, num_samples):
        p = probs[0].float()
        cum = torch.cumsum(p, dim=-1)
        hit = torch.nonzero(cum > next(rows) * cum[-1])
        return torch.tensor([[int(hit[0]) if len(hit) else int(torch.nonzero(p > 0)[-1])]])

    return draw


def reference_outputs(name, case, sd):
    b, n, k = mr.CASES[name]
    model = reference_model(sd, k)
    omit, bias = mr.omit_bias()
    out = {"E_idx": [], "log_probs": []}
    out.update({f"{key}_T{t}": [] for t in mr.TEMPERATURES[name] for key in ("S", "probs")})
    multinomial = torch.multinomial
    with torch.no_grad():
        for i in range(b):
            X = torch.from_numpy(case["prot"][i][None, :, [0, 1, 2, 4]])
            mask, chain = torch.from_numpy(case["res_mask"][i][None]), torch.from_numpy(case["chain_mask"][i][None])
            ridx, chains = torch.from_numpy(case["residue_index"][i][None]).long(), torch.from_numpy(case["chain_idx"][i][None]).long()
            S = torch.from_numpy(case["S"][i][None])
            out["E_idx"].append(model.features(X, mask, ridx, chains)[1][0].numpy())
            lps = []
            for m in range(mr.M):
                order = torch.from_numpy(case["decoding_order"][i, m][None])
                lps.append(model(X, S, mask, chain, ridx, chains, None, use_input_decoding_order=True, decoding_order=order)[0].numpy())
            out["log_probs"].append(np.stack(lps))
            for t in mr.TEMPERATURES[name]:
                Ss, Ps = [], []
                for m in range(mr.M):
                    order = case["decoding_order"][i, m]
                    torch.multinomial = inverse_cdf([float(case["u"][i, m, r]) for r in order if case["res_mask"][i, r] != 0])
                    try:
                        d = model.sample(X, torch.from_numpy(case["randn"][i, m][None]), S, chain, chains, ridx, mask=mask, temperature=t,
                                         omit_AAs_np=omit, bias_AAs_np=bias, chain_M_pos=torch.ones_like(mask), bias_by_res=torch.zeros((1, n, 21)))
                    finally:
                        torch.multinomial = multinomial
                    assert np.array_equal(d["decoding_order"][0].numpy(), order)
                    Ss.append(d["S"][0].numpy()), Ps.append(d["probs"][0].numpy())
                out[f"S_T{t}"].append(np.stack(Ss)), out[f"probs_T{t}"].append(np.stack(Ps))
    return {k_: np.stack(v) for k_, v in out.items()}


def main():
    worst = {"log_probs": 0.0, "probs": 0.0}
    for name, (b, n, k) in mr.CASES.items():
        sd = inv.synthetic_state_dict(mr.WEIGHT_SEED, k)
        for seed in range(200):
            case = mr.make_case(name, seed)
            res = mr.run_case(sd, name, case)
            gap, margin = conditions(name, case, res)
            if gap >= MIN_GAP and margin >= MIN_MARGIN:
                break
        else:
            raise SystemExit(f"case {name}: no input seed below 200 meets the fixture conditions")
        ref = reference_outputs(name, case, sd)
        valid = case["res_mask"] != 0
        assert all(set(ref["E_idx"][i, r]) == set(res["E_idx"][i, r]) for i in range(b) for r in range(n) if valid[i, r]), name
        dev_lp = float(np.abs(ref["log_probs"] - res["log_probs"])[np.broadcast_to(valid[:, None], (b, mr.M, n))].max())
        worst["log_probs"] = max(worst["log_probs"], dev_lp)
        for t, d in res["design"].items():
            assert np.array_equal(ref[f"S_T{t}"], d["S"]), (name, t)
            dev_p = float(np.abs(ref[f"probs_T{t}"] - d["probs"])[np.broadcast_to(valid[:, None], (b, mr.M, n))].max())
            worst["probs"] = max(worst["probs"], dev_p)
            print(f"case {name} T={t}: probs deviation {dev_p:.3e}, letters used {len(np.unique(d['S']))}")
        print(f"case {name}: input seed {seed}, gap {gap:.3e} A, margin {margin:.3e}, log_probs deviation {dev_lp:.3e}")
        np.savez_compressed(os.path.join(HERE, f"mpnn_{name}.npz"), input_seed=np.int64(seed), **{k_: v for k_, v in case.items() if k_ != "randn"}, **ref)
    print("largest deviation of the reference (float32) from the restatement (float64):", worst)


if __name__ == "__main__":
    main()
