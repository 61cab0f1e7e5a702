"""Golden fixtures for the padded inpainting path (same harness as make_goldens.py / make_goldens_r3.py: the reference is imported in
the build container, only inputs and outputs are stored).  Four inpainting trajectories of the full model in the reference's default
inpainting configuration (inference.input_aatype=True / model.input_aatype=False), T = 4, noise scale 0.1, min_t = 0.01, two chains
and one diffused window per chain (make_goldens.make_feats) — at lengths that are NO multiple of four, so that inference_fn pads them
(sharding.pad_item) and pairs of them make mixed-length batches (sharding.stack_items_padded):

  traj_full_inpaint_n45_T4_aatype    N = 45, chain gap 200: pads to 48, below the edge embedder's row-table predicate
  traj_full_inpaint_n42_T4_aatype    N = 42, chain gap 200: its batch mate (44 alone, 48 in the batch)
  traj_full_inpaint_n126_T4_aatype   N = 126, chain gap 20: pads to 128, n_rel = 291, the row table is taken
  traj_full_inpaint_n122_T4_aatype   N = 122, chain gap 20: its batch mate (124 alone with n_rel = 283, 128 in the batch)

    python tests/golden/make_goldens_padded.py [job ...]
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refharness as rh  # noqa: E402,F401  (stubs + sys.path for the reference)
import make_goldens as mg  # noqa: E402
import make_goldens_r3 as r3  # noqa: E402

# name -> (N, gap in seq_idx between the two chains)
FIXTURES = {
    "full_inpaint_n45_T4_aatype": (45, 200),
    "full_inpaint_n42_T4_aatype": (42, 200),
    "full_inpaint_n126_T4_aatype": (126, 20),
    "full_inpaint_n122_T4_aatype": (122, 20),
}
PAIRS = (("full_inpaint_n45_T4_aatype", "full_inpaint_n42_T4_aatype"), ("full_inpaint_n126_T4_aatype", "full_inpaint_n122_T4_aatype"))
NUM_T = 4
_MG_MAKE_FEATS = mg.make_feats  # (traj_padded swaps the module's name for the builder below while a fixture is recorded)


def seed_of(name):
    """The name-derived seed mg.traj_golden draws the features from."""
    return zlib.crc32(name.encode()) % 1000 + 1


def make_feats(n, rng, inpainting, diff, gap=200):
    """mg.make_feats with the second chain ``gap`` positions behind the first in ``seq_idx`` (200 there).  seq_idx takes no draw and
    sample_ref does not read it, so every other feature — and the random stream — is that of mg.make_feats."""
    import torch
    f = _MG_MAKE_FEATS(n, rng, inpainting, diff)
    if inpainting and gap != 200:
        n1 = n // 2
        f["seq_idx"] = torch.tensor(np.concatenate([np.arange(n1), np.arange(n - n1) + n1 + gap]))[None]
    return f


def traj_padded(name):
    n, gap = FIXTURES[name]
    mg.make_feats = lambda *a: make_feats(*a, gap=gap)
    try:
        r3.traj_inpaint_aatype(name, n, NUM_T)
    finally:
        mg.make_feats = _MG_MAKE_FEATS
    g = dict(np.load(os.path.join(HERE, f"traj_{name}.npz")))
    n1 = n // 2
    assert g["in_seq_idx"].shape == (1, n) and int(g["in_seq_idx"][0, n1] - g["in_seq_idx"][0, n1 - 1]) == gap + 1
    assert int(g["in_seq_idx"].max() - g["in_seq_idx"].min()) == n - 1 + gap
    assert int(g["input_aatype"]) == 1 and g["res_prot_traj"].shape == (NUM_T, 1, n, 37, 3)
    size = os.path.getsize(os.path.join(HERE, f"traj_{name}.npz"))
    assert size < 1 << 20, size
    print(name, "N", n, "gap", gap, "seed", seed_of(name), "bytes", size)


for _a, _b in PAIRS:  # the two samples of a mixed batch are different complexes
    assert seed_of(_a) != seed_of(_b) and FIXTURES[_a][0] // 2 != FIXTURES[_b][0] // 2

JOBS = {"traj_" + name: (lambda name=name: traj_padded(name)) for name in FIXTURES}

if __name__ == "__main__":
    for job in (sys.argv[1:] or list(JOBS)):
        JOBS[job]()
