"""The one call path of the sample-analysis entries (selection, evaluation, violations, secondary_structure, sasa, tm_score, tm_align,
inverse_folding, seq_align): shape checks, device choice and upload, optional per-row inputs, output buffers, the C call and the read-back.

``structure_shape``, ``check_shapes``, ``per_row`` on the host (``dev`` None), ``plan_pairs``, ``check_map``, ``add_coverage`` and ``square_matrix`` need neither torch nor the built
library: an entry raises its shape errors before either is touched.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def host(x):
    """A tensor or an array as a NumPy array."""
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def structure_shape(x, what: str = "prot", atoms=(37, 5), lead: str = "B", items: str = "samples"):
    """(count, rows, atoms) of a structure array [count, rows, atoms, 3]; ValueError for any other shape, for an atom count outside
    ``atoms``, and for no structures or no rows.  Reads ``x.shape`` only."""
    shape = tuple(x.shape)
    if len(shape) != 4 or shape[2:] not in [(a, 3) for a in atoms]:
        raise ValueError(f"{what} should be " + " or ".join(f"[{lead}, N, {a}, 3]" for a in atoms) + f", got {shape}")
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{what} {shape}: no {items} or no residues")
    return int(shape[0]), int(shape[1]), int(shape[2])


def upload(entry: str, **structures):
    """(device, tensors): the structure arrays of a call as contiguous float32 device tensors, in the order given (None stays None).
    Tensors are used in place and name the device - they must be float32, on the GPU and on one device; with NumPy arrays only, the
    current device is used."""
    import torch
    tensors = {k: x for k, x in structures.items() if torch.is_tensor(x)}
    first = next(iter(tensors), None)
    for k, x in tensors.items():
        _lib.require_cuda(x, entry)
        if x.dtype != torch.float32:
            raise ValueError(f"{k} should be float32, got {x.dtype}")
        if x.device != tensors[first].device:
            raise ValueError(f"{first} on {tensors[first].device}, {k} on {x.device}")
    dev = tensors[first].device if tensors else torch.device("cuda", torch.cuda.current_device())
    return dev, [None if x is None else x.contiguous() if torch.is_tensor(x) else
                 torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in structures.values()]


def per_row(x, shape, what: str, kind: str = "raw", default=None, dev=None):
    """An optional input that holds one value per row of prot (or per atom: ``shape`` says), as a contiguous array of that shape: a
    NumPy array where ``dev`` is None, else a tensor on ``dev`` (a tensor given stays on the device).  ``kind``: "mask" -> (x != 0) as
    float32; "int" -> int32, a floating input rounded first; "raw" -> as given.  None -> filled with the number ``default`` in the
    kind's dtype (None where that is None too).  ValueError, naming the input, for another shape."""
    shape = tuple(shape)
    if x is not None:
        x = x if hasattr(x, "detach") else np.asarray(x)
        if tuple(x.shape) != shape:
            raise ValueError(f"{what} {tuple(x.shape)} does not match prot: expected {shape}")
    dtype = {"mask": "float32", "int": "int32"}.get(kind)
    if dev is None:
        if x is None:
            return None if default is None else np.full(shape, default, dtype=dtype)
        x = host(x)
        if kind == "mask":
            x = x != 0
        elif kind == "int" and np.issubdtype(x.dtype, np.floating):
            x = np.rint(x)
        return np.ascontiguousarray(x, dtype=dtype)
    import torch
    if x is None:
        return None if default is None else torch.full(shape, default, dtype=dtype and getattr(torch, dtype), device=dev)
    x = x.to(dev) if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if kind == "mask":
        x = x != 0
    elif kind == "int" and x.is_floating_point():
        x = torch.round(x)
    return (x if dtype is None else x.to(getattr(torch, dtype))).contiguous()


def check_shapes(checks, mapped: bool = False):
    """The shapes of the optional inputs of a call, before torch or the library is touched: ``checks`` holds (name, the input or None,
    the shape it should have).  ValueError, naming the input: it "does not match prot", or - ``mapped``: the two structures of an
    entry with a row map have rows of their own - "does not match its structure"."""
    for what, x, shape in checks:
        got = None if x is None else tuple(x.shape if hasattr(x, "shape") else np.shape(x))
        if x is not None and got != tuple(shape):
            raise ValueError(f"{what} {got} does not match {'its structure' if mapped else 'prot'}: expected {tuple(shape)}")


def atom_mask(x, shape, what: str, dev):
    """An optional atom mask as the entries read it: contiguous uint8 on ``dev`` (non-zero: the atom exists), or None."""
    import torch
    m = per_row(x, shape, what, "mask", dev=dev)
    return None if m is None else m.to(torch.uint8).contiguous()


def add_coverage(out: dict, n_pairs: int) -> dict:
    """The result of a mapped entry with ``coverage`` [P] = n_covered / n_reference (0 for no reference row); a result without a call
    (``empty_outputs``: P = 0) gains the two zero-length counts first."""
    if n_pairs == 0:
        out.update(n_covered=np.zeros(0, dtype=np.int64), n_reference=np.zeros(0, dtype=np.int64))
    out["coverage"] = np.divide(out["n_covered"], out["n_reference"], out=np.zeros(n_pairs), where=out["n_reference"] > 0)
    return out


def zeros_on(dev, spec: dict) -> dict:
    """Zeroed device tensors from {name: (dtype name, shape)}."""
    import torch
    return {k: torch.zeros(tuple(shape), dtype=getattr(torch, dtype), device=dev) for k, (dtype, shape) in spec.items()}


def to_numpy(out: dict, widen=()) -> dict:
    """Device tensors read back as NumPy arrays; the int32 ones named in ``widen`` become int64."""
    return {k: v.cpu().numpy().astype(np.int64) if k in widen else v.cpu().numpy() for k, v in out.items()}


def empty_outputs(spec: dict, widen=()) -> dict:
    """What ``run`` returns for ``spec`` without a call: for an entry whose leading dimension is 0."""
    return {k: np.zeros(tuple(shape), dtype=np.int64 if k in widen else dtype) for k, (dtype, shape) in spec.items()}


def run(name: str, struct, dev, scalars: dict, inputs: dict, outputs: dict, widen=(), workspace=None, dims=None, extra=()) -> dict:
    """One call of the C entry ``name`` on the current stream of ``dev``.  ``struct``: its args struct, filled from ``scalars`` (plain
    fields: sizes, numbers, host pointers), ``inputs`` (device tensors or None, by field name) and zeroed outputs allocated from
    ``outputs`` ({name: (dtype name, shape)}).  ``workspace``: (size function, *its arguments), sized and allocated here, or None for an
    entry that takes none.  ``dims``: a struct both functions take by reference as their first argument (the inverse-folding model).
    ``extra``: plain arguments the entry takes between its args struct and the stream.
    Returns the outputs as NumPy arrays, those named in ``widen`` as int64."""
    import torch
    lib = _lib.load()
    lead = () if dims is None else (C.byref(dims),)
    with torch.cuda.device(dev):
        out = zeros_on(dev, outputs)
        nbytes = 0 if workspace is None else int(getattr(lib, workspace[0])(*lead, *workspace[1:]))
        work = None if workspace is None else torch.empty(nbytes, dtype=torch.uint8, device=dev)
        args = struct(workspace=_lib.ptr(work), workspace_bytes=nbytes, **scalars, **{k: _lib.ptr(v) for k, v in inputs.items()},
                      **{k: _lib.ptr(v) for k, v in out.items()})
        _lib.check(getattr(lib, name)(*lead, C.byref(args), *extra, _lib.stream_ptr()), name)
        return to_numpy(out, widen)


def all_pairs(b: int) -> np.ndarray:
    """[b (b - 1) / 2, 2] int32: every i < j, i-major."""
    i, j = np.triu_indices(b, 1)
    return np.stack([i, j], axis=1).astype(np.int32)


def plan_pairs(s_a: int, s_b: int, has_b: bool, pairs, ref_index):
    """(pair_list int32 [P,2], square) of a pairwise entry over ``s_a`` structures and ``s_b`` second structures (``has_b``: a second
    array was given): ``pairs`` as listed; without a second array and a ``ref_index``, every i < j (``square``: the result carries the
    mirrored matrix); else structure i against ``ref_index[i]`` - by default row i where s_b = s_a, row 0 where s_b = 1."""
    if pairs is not None:
        return np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2), False
    if not has_b and ref_index is None:
        return all_pairs(s_a), True
    if ref_index is None:
        if s_b not in (1, s_a):
            raise ValueError(f"prot_b holds {s_b} structures for {s_a} samples: give ref_index or pairs")
        ref_index = np.arange(s_a) if s_b == s_a and s_b > 1 else np.zeros(s_a)
    return np.stack([np.arange(s_a), np.asarray(ref_index).reshape(s_a)], axis=1).astype(np.int32), False


def check_map(alignment, n_pairs: int, n_b: int, n_a: int):
    """The row map of a mapped entry, ``[N_b]`` (one map for every pair) or ``[P, N_b]``, checked without torch or the library: a NumPy
    array (or a list) comes back as int32 ``[P, N_b]`` after ``row_map.validate`` - a bad map raises here; a device tensor is checked
    for its shape and integer dtype only and comes back as it is: the device judges it (the ``MAP_*`` status bits)."""
    from . import row_map
    if hasattr(alignment, "detach"):
        shape, integer = tuple(alignment.shape), not (alignment.is_floating_point() or alignment.is_complex())
    else:
        alignment = np.asarray(alignment)
        shape, integer = alignment.shape, np.issubdtype(alignment.dtype, np.integer)
    if shape not in ((n_b,), (n_pairs, n_b)) or not integer:
        raise ValueError(f"alignment should be integers [{n_b}] (the reference's rows) or [{n_pairs}, {n_b}] (per pair), got "
                         f"{'integers' if integer else 'non-integers'} {tuple(shape)}")
    if hasattr(alignment, "detach"):
        return alignment
    return np.broadcast_to(row_map.validate(alignment, n_a), (n_pairs, n_b)).copy()


def upload_map(alignment, n_pairs: int, n_b: int, dev):
    """What ``check_map`` returned as a contiguous int32 tensor [P, N_b] on ``dev``."""
    import torch
    x = alignment.to(dev) if torch.is_tensor(alignment) else torch.from_numpy(alignment).to(dev)
    return x.to(torch.int32).expand(n_pairs, n_b).contiguous()


def run_mapped(name: str, struct, dev, scalars: dict, inputs: dict, outputs: dict, row_map: dict, widen=(), workspace=None) -> dict:
    """``run`` for an entry that takes a ``RowMap`` behind its args struct: ``row_map`` holds the struct's plain fields and its device
    inputs; ``n_covered`` and ``n_reference`` [P] are allocated here and come back with the outputs (int64)."""
    import torch
    n_pairs = int(row_map["map"].shape[0])
    with torch.cuda.device(dev):
        counts = zeros_on(dev, {"n_covered": ("int32", (n_pairs,)), "n_reference": ("int32", (n_pairs,))})
        rm = _lib.RowMap(**{k: _lib.ptr(v) if torch.is_tensor(v) or v is None else v for k, v in row_map.items()}, **{k: _lib.ptr(v) for k, v in counts.items()})
        out = run(name, struct, dev, scalars, inputs, outputs, widen=widen, workspace=workspace, extra=(C.byref(rm),))
        out.update(to_numpy(counts, widen=tuple(counts)))
    return out


def square_matrix(s: int, pair_list, values) -> np.ndarray:
    """[s,s] float64 with a unit diagonal and ``values`` at the pairs of ``pair_list``, mirrored."""
    matrix = np.ones((s, s), dtype=np.float64)
    matrix[pair_list[:, 0], pair_list[:, 1]] = matrix[pair_list[:, 1], pair_list[:, 0]] = values
    return matrix
