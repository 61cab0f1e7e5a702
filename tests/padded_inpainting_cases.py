"""Inputs shared by tests/test_padded_inpainting_host.py and tests/test_gpu_padded_inpainting.py: the four reference trajectories of
tests/golden/make_goldens_padded.py (inpainting, two chains, lengths that are no multiple of four) and a hand-made feature dict with
the conditional sampler's complete key set."""
import numpy as np
import torch

# fixture -> (N, chain gap in seq_idx, length inference_fn pads it to alone, n_rel = 2 * (N - 1 + gap) + 1)
FIXTURES = {
    "full_inpaint_n45_T4_aatype": (45, 200, 48, 489),
    "full_inpaint_n42_T4_aatype": (42, 200, 44, 483),
    "full_inpaint_n126_T4_aatype": (126, 20, 128, 291),
    "full_inpaint_n122_T4_aatype": (122, 20, 124, 283),
}
# mixed-length batches: (longer sample, its batch mate, common padded length)
PAIRS = {"n45_n42": ("full_inpaint_n45_T4_aatype", "full_inpaint_n42_T4_aatype", 48),
         "n126_n122": ("full_inpaint_n126_T4_aatype", "full_inpaint_n122_T4_aatype", 128)}

# what ConditionalSampler.__getitem__ hands over (framedipt_amd/sampler.py; tests/test_gpu_padded_inpainting.py compares the two on the GPU)
SAMPLER_KEYS = ("aatype", "seq_idx", "chain_idx", "res_mask", "fixed_mask", "rigids_0", "rigids_t", "sc_ca_t", "t",
                "torsion_angles_sin_cos")
PER_RESIDUE = tuple(k for k in SAMPLER_KEYS if k != "t")


def tape_of(G):
    """The fixture's recorded draws ([2 (T - 1), 1, N, 3]: SO(3) then R^3 per step) as inference_fn's (z_rot, z_trans)."""
    n = len(G["noise_tape"]) // 2
    return (np.stack([G["noise_tape"][2 * i] for i in range(n)]), np.stack([G["noise_tape"][2 * i + 1] for i in range(n)]))


def hand_item(n, seed, gap=200, n_noisy=3):
    """(feature dict [1, n, ...] with the conditional sampler's keys and a non-tensor entry, noise tape [n_noisy, 1, n, 3]) of a two-chain
    complex with one diffused window per chain; CPU tensors of the sampler's dtypes, no value that padding writes (0, the unit
    quaternion) on a real row."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((2, n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    tr = rng.standard_normal((2, n, 3)) * 5 + 0.5
    n1 = n // 2
    dm = np.zeros(n)
    dm[1:3] = 1
    dm[n - 3:n - 1] = 1
    tors = rng.standard_normal((n, 7, 2))
    tors /= np.linalg.norm(tors, axis=-1, keepdims=True)
    feats = {
        "aatype": torch.tensor(rng.integers(1, 20, size=n))[None],
        "seq_idx": torch.tensor(np.concatenate([np.arange(n1) + 1, np.arange(n - n1) + 1 + n1 + gap]))[None],
        "chain_idx": torch.tensor(np.concatenate([np.ones(n1), np.full(n - n1, 2)]).astype(np.int64))[None],
        "res_mask": torch.ones(1, n, dtype=torch.float64),
        "fixed_mask": torch.tensor(1 - dm)[None],
        "rigids_0": torch.tensor(np.concatenate([q[0], tr[0]], -1).astype(np.float32))[None],
        "rigids_t": torch.tensor(np.concatenate([q[1], tr[1]], -1).astype(np.float32))[None],
        "sc_ca_t": torch.tensor(tr[1].astype(np.float32) + 0.25)[None],
        "t": torch.tensor([1.0]),
        "torsion_angles_sin_cos": torch.tensor(tors)[None],
        "pdb_name": "hand-made",
    }
    tape = tuple(rng.standard_normal((n_noisy, 1, n, 3)) for _ in range(2))
    return feats, tape
