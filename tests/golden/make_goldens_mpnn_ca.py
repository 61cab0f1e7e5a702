"""Fixtures of the CA-only inverse-folding tests, captured from the reference's ProteinMPNN(ca_only=True) (this container only):

    python tests/golden/make_goldens_mpnn_ca.py      # -> tests/golden/mpnn_ca_<case>.npz, tests/golden/mpnn_ca_state_dict.json

Modelled on make_goldens_mpnn.py.  Per case of tests/mpnn_ca_ref.py (CASES: ca_a to ca_f) the reference model (float32 on the CPU, eval
mode, augment_eps 0, one backbone at a time: the reference's ``torch.cross`` without ``dim`` goes wrong for a batch of 3 and for N = 6,
DESIGN.md section 7.12) is loaded - strictly - with ``inverse_folding.synthetic_state_dict(WEIGHT_SEED, K, ca_only=True)`` and run on
``mpnn_ca_ref.make_case``: ``forward`` per sequence -> ``log_probs``; ``features`` -> ``E_idx`` (compared as sets per row); ``sample``
per sequence and temperature with ``torch.multinomial`` replaced by the inverse-CDF rule on the recorded uniforms -> ``S_T<t>``,
``probs_T<t>``.  No weights are stored.  ``mpnn_ca_state_dict.json`` lists the reference's parameter names and shapes.

The input seed of a case is searched upward from 0 until the float64 restatement says that (1) every row with res_mask and N > K has at
least 1e-3 A between its K-th and (K+1)-th distance, (2) every draw lies at least 1e-4 from every boundary of its row's cumulative
distribution, (3) no CA step lies within 1e-3 A of 3.6 or 4.0 and (4) on every edge other than a self edge whose R is not zero each
antisymmetric component of R is at least 1e-5 in magnitude (100 float32 roundings of an O(1) entry: no sign in the quaternions hangs on
rounding); all four are asserted again on the recorded case.  Were no seed below 200 to meet (4) for a case, that case's N would have
to be lowered, not the margin; every case found its seed at the N of the table.

The script asserts that the reference's Q on every self edge of a row with res_mask whose R is not zero is exactly (0, 0, 0, 1) (a
row without res_mask need not have its self edge: all its adjusted distances tie), and prints the largest deviation of the reference's
float32 outputs from the float64 restatement over the rows with res_mask: the yardstick of the tests' tolerance
(mpnn_ca_ref.DEVIATION).
"""
from __future__ import annotations

import json
import os
import warnings

import numpy as np
import torch

import make_goldens_mpnn as base  # (sets the import paths up; the reference's module, the inverse-CDF stand-in)
import mpnn_ca_ref as mc
import mpnn_ref as mr
from framedipt_amd import inverse_folding as inv

HERE = base.HERE
MIN_GAP, MIN_MARGIN, MIN_STEP, MIN_ANTI = 1e-3, 1e-4, 1e-3, 1e-5
pmu = base.pmu


def conditions(case, res):
    valid = case["res_mask"] != 0
    return float(res["gap"][valid].min()), min(d["margin"] for d in res["design"].values()), res["step_margin"], res["min_anti"]


def met(cond):
    return cond[0] >= MIN_GAP and cond[1] >= MIN_MARGIN and cond[2] >= MIN_STEP and cond[3] >= MIN_ANTI


def reference_model(sd, k):
    model = pmu.ProteinMPNN(num_letters=21, node_features=128, edge_features=128, hidden_dim=128, num_encoder_layers=3, num_decoder_layers=3,
                            augment_eps=0.0, k_neighbors=k, ca_only=True)
    model.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()}, strict=True)
    return model.eval()


def reference_outputs(name, case, sd):
    b, n, k = mc.CASES[name]
    model = reference_model(sd, k)
    omit, bias = mr.omit_bias()
    out = {"E_idx": [], "log_probs": []}
    out.update({f"{key}_T{t}": [] for t in mc.TEMPERATURES[name] for key in ("S", "probs")})
    self_q = []
    multinomial = torch.multinomial
    with torch.no_grad():
        for i in range(b):
            X = torch.from_numpy(case["ca"][i][None])
            mask, chain = torch.from_numpy(case["res_mask"][i][None]), torch.from_numpy(case["chain_mask"][i][None])
            ridx, chains = torch.from_numpy(case["residue_index"][i][None]).long(), torch.from_numpy(case["chain_idx"][i][None]).long()
            S = torch.from_numpy(case["S"][i][None])
            e_idx = model.features(X, mask, ridx, chains)[1]
            out["E_idx"].append(e_idx[0].numpy())
            # Q of the self edges whose R is not zero: the last four of the orientation features
            o_feat = model.features._orientations_coarse(X, e_idx)[1][0]
            r = mc.edge_inputs(mr.Model(sd, k), case["ca"][i], case["res_mask"][i], case["residue_index"][i], case["chain_idx"][i])[3]
            framed = (e_idx[0] == torch.arange(n)[:, None]) & (r.abs().amax((-1, -2)) > 0) & (mask[0][:, None] != 0)
            self_q.append(o_feat[..., 3:][framed].numpy())
            lps = []
            for m in range(mc.M):
                order = torch.from_numpy(case["decoding_order"][i, m][None])
                lps.append(model(X, S, mask, chain, ridx, chains, None, use_input_decoding_order=True, decoding_order=order)[0].numpy())
            out["log_probs"].append(np.stack(lps))
            for t in mc.TEMPERATURES[name]:
                Ss, Ps = [], []
                for m in range(mc.M):
                    order = case["decoding_order"][i, m]
                    torch.multinomial = base.inverse_cdf([float(case["u"][i, m, r_]) for r_ in order if case["res_mask"][i, r_] != 0])
                    try:
                        d = model.sample(X, torch.from_numpy(case["randn"][i, m][None]), S, chain, chains, ridx, mask=mask, temperature=t,
                                         omit_AAs_np=omit, bias_AAs_np=bias, chain_M_pos=torch.ones_like(mask), bias_by_res=torch.zeros((1, n, 21)))
                    finally:
                        torch.multinomial = multinomial
                    assert np.array_equal(d["decoding_order"][0].numpy(), order)
                    Ss.append(d["S"][0].numpy()), Ps.append(d["probs"][0].numpy())
                out[f"S_T{t}"].append(np.stack(Ss)), out[f"probs_T{t}"].append(np.stack(Ps))
    return {k_: np.stack(v) for k_, v in out.items()}, np.concatenate(self_q)


def main():
    warnings.filterwarnings("ignore", message=".*torch.cross.*")  # the reference's call without dim: the right axis for B = 1, N != 6
    worst = {"log_probs": 0.0, "probs": 0.0}
    largest = max(os.path.getsize(os.path.join(HERE, f"mpnn_{c}.npz")) for c in mr.CASES)
    for name, (b, n, k) in mc.CASES.items():
        assert n != 6 and n >= 3
        sd = inv.synthetic_state_dict(mr.WEIGHT_SEED, k, ca_only=True)
        for seed in range(200):
            case = mc.make_case(name, seed)
            res = mc.run_case(sd, name, case)
            cond = conditions(case, res)
            if met(cond):
                break
        else:
            raise SystemExit(f"case {name}: no input seed below 200 meets the fixture conditions: lower its N, not a margin")
        ref, self_q = reference_outputs(name, case, sd)
        valid = case["res_mask"] != 0
        assert all(set(ref["E_idx"][i, r]) == set(res["E_idx"][i, r]) for i in range(b) for r in range(n) if valid[i, r]), name
        # the self edge: R is symmetric to the bit on the reference's CPU path, so sign gives 0 and Q is the identity
        assert self_q.shape == res["self_q"].shape and (self_q == np.array([0, 0, 0, 1], np.float32)).all(), (name, self_q)
        assert (res["self_q"] == np.array([0.0, 0.0, 0.0, 1.0])).all(), name
        rows = np.broadcast_to(valid[:, None], (b, mc.M, n))
        dev_lp = float(np.abs(ref["log_probs"] - res["log_probs"])[rows].max())
        worst["log_probs"] = max(worst["log_probs"], dev_lp)
        for t, d in res["design"].items():
            assert np.array_equal(ref[f"S_T{t}"], d["S"]), (name, t)
            dev_p = float(np.abs(ref[f"probs_T{t}"] - d["probs"])[rows].max())
            worst["probs"] = max(worst["probs"], dev_p)
            print(f"case {name} T={t}: probs deviation {dev_p:.3e}, letters used {len(np.unique(d['S']))}")
        print(f"case {name}: input seed {seed}, gap {cond[0]:.3e} A, margin {cond[1]:.3e}, step margin {cond[2]:.3e} A, smallest antisymmetric "
              f"component {cond[3]:.3e}, framed self edges {len(self_q)}, log_probs deviation {dev_lp:.3e}")
        path = os.path.join(HERE, f"mpnn_{name}.npz")
        np.savez_compressed(path, input_seed=np.int64(seed), **{k_: v for k_, v in case.items() if k_ != "randn"}, **ref)
        assert os.path.getsize(path) <= largest, (name, os.path.getsize(path), largest)
    print("largest deviation of the reference (float32) from the restatement (float64):", worst)
    model = reference_model(inv.synthetic_state_dict(mr.WEIGHT_SEED, 48, ca_only=True), 48)
    with open(os.path.join(HERE, "mpnn_ca_state_dict.json"), "w") as f:
        json.dump([[n_, list(v.shape)] for n_, v in model.state_dict().items()], f, indent=0)


if __name__ == "__main__":
    main()
