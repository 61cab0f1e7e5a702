"""Opt-in device noise (``noise="device"``): the step kernels draw their own N(0,1) values from per-sample 64-bit keys.

The generator is counter-based (Philox4x32-10 + Box-Muller in float64, ``csrc/philox.hpp``; contract in ``include/fdipt.h``): a draw is
a function of (key, purpose, step index, residue index within the sample, component) and of nothing else — not of the batch a sample
rides in, its padded length, the precision mode, graph or eager execution, or the number of ranks.  ``fill`` writes the values the step
kernels draw, through the same device function: a run on the filled tape reproduces the ``noise="device"`` run bit for bit.
"""
from __future__ import annotations

import numpy as np

# purposes (the third counter word): separate streams, so that diffuse_rot = False does not shift the translation draws
REVERSE_ROT, REVERSE_TRANS, FORWARD_ROT, FORWARD_TRANS = 0, 1, 2, 3
MODES = ("host", "device")


def as_keys(noise_keys, B: int) -> np.ndarray:
    """``noise_keys`` as a uint64 array [B]: an int ``s`` means keys ``s, s + 1, ...``; a sequence / int64 tensor gives one key per
    sample (negative values stand for their 64-bit two's complement)."""
    if hasattr(noise_keys, "detach"):
        noise_keys = noise_keys.detach().cpu().numpy()
    if np.ndim(noise_keys) == 0:
        vals = [int(noise_keys) + b for b in range(B)]
    else:
        vals = [int(k) for k in np.asarray(noise_keys, dtype=object).reshape(-1)]
        if len(vals) != B:
            raise ValueError(f"noise_keys: {len(vals)} keys for a batch of {B} samples")
    return np.array([v & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)


def resolve(noise: str, noise_keys, noise_tape, B: int):
    """Argument check shared by every entry point, before anything touches a device.  -> uint64 keys [B], or None for ``"host"``."""
    if noise not in MODES:
        raise ValueError(f"noise={noise!r}: expected one of {MODES}")
    if noise == "host":
        if noise_keys is not None:
            raise ValueError('noise_keys are the keys of noise="device"; the host path takes a noise_tape (or the global np.random stream)')
        return None
    if noise_tape is not None:
        raise ValueError('noise="device" draws inside the step kernel: it takes noise_keys, not a noise_tape')
    if noise_keys is None:
        raise ValueError('noise="device" needs noise_keys (one 64-bit key per sample, or an int s for keys s, s + 1, ...)')
    return as_keys(noise_keys, B)


def keys_tensor(keys: np.ndarray, device):
    """The keys on the device (int64 tensor holding the uint64 bit patterns: what the ``*_gen`` entries read)."""
    import torch
    return torch.as_tensor(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64), device=device)


def fill(noise_keys, purpose: int, n_steps: int, N: int, device, k_begin: int = 0):
    """[n_steps, B, N, 3] float64 on ``device``: the draws of steps ``k_begin .. k_begin + n_steps - 1`` (``fdipt_noise_fill``)."""
    import torch

    from . import _lib
    lib = _lib.load()
    on_device = hasattr(noise_keys, "is_cuda") and noise_keys.is_cuda
    keys = noise_keys if on_device else keys_tensor(as_keys(noise_keys, max(1, int(np.size(noise_keys)))), device)
    B = int(keys.shape[0])
    out = torch.empty(n_steps, B, N, 3, dtype=torch.float64, device=keys.device)
    _lib.require_cuda(keys, "noise_fill")
    with torch.cuda.device(keys.device):
        _lib.check(lib.fdipt_noise_fill(B, N, _lib.ptr(keys), int(purpose), int(k_begin), int(n_steps), _lib.ptr(out),
                                        _lib.stream_ptr()), "noise_fill")
    return out


def filled_tape(noise_keys, n_steps: int, N: int, device, forward: bool = False):
    """(z_rot, z_trans) NumPy arrays [n_steps, B, N, 3]: the ``noise_tape`` that reproduces a ``noise="device"`` run of these keys
    (``forward``: the confidence score's forward-noising purposes)."""
    purposes = (FORWARD_ROT, FORWARD_TRANS) if forward else (REVERSE_ROT, REVERSE_TRANS)
    return tuple(fill(noise_keys, p, n_steps, N, device).cpu().numpy() for p in purposes)
