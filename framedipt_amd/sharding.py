"""Sample sharding over the GPUs of one node.

Each (structure, sample index) item of a sampler dataset is an independent trajectory, so ranks take disjoint item
indices and never exchange data on the hot path; results are gathered on the host at the end.  One process per GPU
(``torch.distributed`` env contract); the only collective is the end-of-run gather / timing reduction.
"""
from __future__ import annotations

from typing import List


def shard_indices(n_items: int, rank: int, world: int) -> List[int]:
    """Round-robin partition of ``range(n_items)``; ranks differ by at most one item."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside world of size {world}")
    return list(range(rank, n_items, world))


def gather_results(local: dict, n_items: int, rank: int, world: int):
    """Host-side gather of ``{item_index: ndarray}`` to rank 0 (any backend; object gather)."""
    import torch.distributed as dist
    if world == 1:
        return dict(local)
    bucket = [None] * world if rank == 0 else None
    dist.gather_object(local, bucket, dst=0)
    if rank != 0:
        return None
    merged = {}
    for part in bucket:
        merged.update(part)
    if sorted(merged) != list(range(n_items)):
        raise RuntimeError("sample gather is incomplete")
    return merged


def max_over_ranks(value: float, device=None) -> float:
    """Timing reduction used by bench.py (MAX over ranks)."""
    import torch
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return float(value)
    t = torch.tensor([value], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


# ---------------------------------------------------------------------------------------------------------------------
# Per-sample random streams ("Caveat").  The reference draws x_T and every reverse step's noise from
# ONE global legacy np.random stream, sample after sample.  Sharded runs restart that stream per sample at `seed + item`,
# draw x_T (through the dataset item) and then the whole noise tape of the sample's trajectory in the reference's per-step
# order: a sample's inputs - and with batch-position-independent kernels its whole trajectory - do not depend on the world
# size, the rank that runs it or the batch it rides in.
def seeded_item(dataset, item: int, seed: int, diffuser, num_t: int, min_t: float, noise: str = "host"):
    """``dataset[item]`` and its noise tape drawn from ``np.random.seed(seed + item)``.
    Returns (name_or_length, sample_i, feats [1,N,...], (z_rot, z_trans) [n_noisy,1,N,3] float64).
    ``noise="device"``: x_T is drawn as above and the item's noise key — ``seed + item``, the per-item seed — takes the tape's place
    (the step kernel draws from it: noise.py); nothing else is drawn on the host."""
    import numpy as np

    from .inference import draw_noise_tape
    from .noise import MODES
    if noise not in MODES:
        raise ValueError(f"noise={noise!r}: expected one of {MODES}")
    np.random.seed(seed + item)
    name, sample_i, feats = dataset[item]
    if noise == "device":
        return name, sample_i, feats, int(seed + item)
    n = feats["rigids_t"].shape[1]
    n_noisy = int(np.sum(np.linspace(min_t, 1.0, num_t)[::-1] > min_t))
    return name, sample_i, feats, draw_noise_tape(diffuser, n_noisy, 1, n)


def stack_items(items):
    """Batch of equally sized samples from ``seeded_item`` tuples: (feats [B,N,...], (z_rot, z_trans) [n,B,N,3]); items that carry
    noise keys (``seeded_item(noise="device")``) give the batch's keys [B] (int64) in the tape's place."""
    import numpy as np
    import torch
    feats = {k: torch.cat([it[2][k] for it in items], dim=0) for k in items[0][2]}
    if not isinstance(items[0][3], tuple):
        return feats, np.array([int(it[3]) for it in items], dtype=np.int64)
    tape = tuple(np.concatenate([it[3][j] for it in items], axis=1) for j in range(2))
    return feats, tape


# ---------------------------------------------------------------------------------------------------------------------
# Mixed-length batches.  The reference pads feature dicts to a common length with zeros — res_mask = 0 on the padded rows —
# and identity frames (framedipt/data/utils.py:311-339 pad_feats / pad_rigid); its inference entry point only ever sees
# B = 1, so padding there is a no-op.  Here it is what lets DIFFERENT complexes (config 3: 62 TCR-pMHC complexes of 700 - 850
# residues, all different) share a batch: every kernel treats res_mask = 0 rows as absent (masked keys get exactly zero attention
# weight, masked pair rows are zero, the reverse step leaves them where they are and they add exactly 0 to the centre of mass),
# so a sample's trajectory on its real residues does not depend on how far it was padded
# (tests/test_gpu_round3.py::test_padded_sample_matches_its_unpadded_run).
_PAD_ONE = ("rigids_t",)  # padded with identity frames (quaternion 1, 0, 0, 0; translation 0)


def pad_item(feats: dict, tape, n_pad: int):
    """One ``[1, N, ...]`` feature dict and its noise tape ``[n, 1, N, 3]`` padded to ``n_pad`` residues.  A noise key (or None) in
    the tape's place passes through: a key's draws depend on the residue index, not on the padded length."""
    import numpy as np
    import torch
    n = int(feats["rigids_t"].shape[1])
    if n_pad < n:
        raise ValueError(f"cannot pad {n} residues to {n_pad}")
    if n_pad == n:
        return feats, tape
    out = {}
    for k, v in feats.items():
        if not torch.is_tensor(v) or v.dim() < 2 or v.shape[1] != n:
            out[k] = v
            continue
        pad = torch.zeros((v.shape[0], n_pad - n) + tuple(v.shape[2:]), dtype=v.dtype, device=v.device)
        if k in _PAD_ONE:
            pad[..., 0] = 1
        elif k == "seq_idx":  # any value works (the rows are masked); the last real index keeps the relative-position table small
            pad += v[:, -1:]
        out[k] = torch.cat([v, pad], dim=1)
    if isinstance(tape, tuple):
        tape = tuple(np.concatenate([z, np.zeros(z.shape[:2] + (n_pad - n, 3), dtype=z.dtype)], axis=2) for z in tape)
    return out, tape


def stack_items_padded(items, multiple: int = 4):
    """Batch of samples of different lengths from ``seeded_item`` tuples, padded to the longest one rounded up to ``multiple``
    (4: the fast EdgeTransition / projection kernels want N % 4 == 0).  Returns (feats, tape, lengths)."""
    lengths = [int(it[2]["rigids_t"].shape[1]) for it in items]
    n_pad = -(-max(lengths) // multiple) * multiple
    padded = [pad_item(it[2], it[3], n_pad) for it in items]
    feats, tape = stack_items([(None, None, f, t) for f, t in padded])
    return feats, tape, lengths


# Lengths at which the library switches kernels (csrc: the o_pair key passes at 320 / 640 / 960, the attention / sequence-attention key-tile
# variants at 384 / 512 / 768, the 16-row node-path kernels up to 512, the register-attention limit 1024).  Inside one class a sample's
# real residues are bit-identical however far it is padded; across a boundary they agree to tolerance only (different summation orders).
# The library exports the same list (fdipt_kernel_class_bounds, next to the dispatch code); tests/test_host_cpu.py compares the two.
KERNEL_CLASS_BOUNDS = (320, 384, 512, 640, 768, 960, 1024)


def kernel_class(n: int, multiple: int = 4) -> int:
    """Kernel-selection class of a sample of ``n`` residues once padded to a multiple of ``multiple`` (stack_items_padded)."""
    n_pad = -(-int(n) // multiple) * multiple
    return sum(n_pad > b for b in KERNEL_CLASS_BOUNDS)


def batches_mixed(lengths, max_batch: int, max_waste: float = 0.15):
    """Group local item positions into batches of at most ``max_batch`` samples of SIMILAR length: positions sorted by length,
    a batch is closed when it is full, when padding its shortest member to its longest would waste more than ``max_waste`` of
    the pair work (1 - (n_min / n_max)^2), or when the next sample belongs to another kernel-selection class (``kernel_class``): a
    sample then runs on the kernels its own (4-padded) length selects whatever batch / shard / world size it rides in, which keeps
    sharded runs bit-reproducible.  Equal lengths always share a batch."""
    order = sorted(range(len(lengths)), key=lambda p: (lengths[p], p))
    out, cur = [], []
    for p in order:
        if cur and (len(cur) == max_batch or 1.0 - (lengths[cur[0]] / lengths[p]) ** 2 > max_waste
                    or kernel_class(lengths[cur[0]]) != kernel_class(lengths[p])):
            out.append(cur)
            cur = []
        cur.append(p)
    if cur:
        out.append(cur)
    return out


def batches_by_length(lengths, max_batch: int):
    """Group local item positions into batches of equal N (at most ``max_batch`` samples each), in item order."""
    out, cur = [], []
    for pos, n in enumerate(lengths):
        if cur and (lengths[cur[0]] != n or len(cur) == max_batch):
            out.append(cur)
            cur = []
        cur.append(pos)
    if cur:
        out.append(cur)
    return out
