"""Row maps for the mapped accuracy entries (``lddt.local_accuracy(..., alignment=)``, ``gdt.gdt_scores(..., alignment=)``; DESIGN.md
section 7.16), in NumPy on the host.  A map is int32 ``[N_b]``: entry j is the row of the model (structure a) that corresponds to row j
of the reference (structure b), or -1 - the layout of ``tm_align(...)["alignment"]`` and of ``structure_search``'s.  A map need not be
monotone; it must be injective on its non-negative entries.

``from_residue_numbers`` is this project's counterpart of the reference's ``framedipt/protein/align.py`` by numbering: correspondence
by residue identity, before any superposition.  It is that file's counterpart only while the two structures number their residues alike;
``seq_align.chain_row_map`` is the counterpart by sequence (a global alignment per chain on the device, what that file itself does) and
returns a map of the same layout.  This module stays pure NumPy.
"""
from __future__ import annotations

import numpy as np

OUT_OF_RANGE, DUPLICATE = 8, 16  # FDIPT_MAP_OUT_OF_RANGE, FDIPT_MAP_DUPLICATE (pinned against the header by the tests)


def _as_map(m, what: str = "map") -> np.ndarray:
    m = np.asarray(m)
    if m.ndim < 1 or not (np.issubdtype(m.dtype, np.integer) or m.size == 0):
        raise ValueError(f"{what} should be an integer array [N_b] or [P, N_b], got {m.dtype} {m.shape}")
    return m.astype(np.int64)


def flags(m, n_a: int) -> np.ndarray:
    """The status bits the device would set, per map row: ``[P]`` for ``[P, N_b]``, a 0-d array for ``[N_b]``."""
    m = _as_map(m)
    rows = m.reshape(-1, m.shape[-1])
    out = np.zeros(len(rows), dtype=np.int64)
    for p, row in enumerate(rows):
        if np.any((row < -1) | (row >= n_a)):
            out[p] |= OUT_OF_RANGE
        used = row[row >= 0]
        if len(np.unique(used)) != len(used):
            out[p] |= DUPLICATE
    return out.reshape(m.shape[:-1])


def validate(m, n_a: int) -> np.ndarray:
    """The map as int32, or ValueError for what the device would flag: an entry < -1 or >= ``n_a``, two rows with the same entry >= 0."""
    bits = np.atleast_1d(flags(m, n_a))
    bad = np.flatnonzero(bits)
    if len(bad):
        what = [name for bit, name in ((OUT_OF_RANGE, f"an entry outside -1 .. {n_a - 1}"), (DUPLICATE, "a model row used twice")) if bits[bad[0]] & bit]
        raise ValueError(f"row map {int(bad[0])} of {len(bits)}: " + " and ".join(what))
    return np.ascontiguousarray(m, dtype=np.int32)


def identity(n: int) -> np.ndarray:
    """Row j corresponds to row j."""
    return np.arange(n, dtype=np.int32)


def from_residue_numbers(chain_a, number_a, chain_b, number_b) -> np.ndarray:
    """The map [N_b] that joins the rows with equal (chain, residue number) keys: ``chain_*`` [N] (any hashable labels, or one label for
    all rows), ``number_*`` [N] (numbers, or strings that carry an insertion code).  A key that occurs twice in one structure is refused:
    the correspondence would not be a map."""
    def keys(chain, number, what):
        number = np.asarray(number).reshape(-1)
        chain = np.asarray(chain)
        chain = np.broadcast_to(chain.reshape(-1) if chain.ndim else chain, number.shape)
        out = [(c.item() if hasattr(c, "item") else c, x.item() if hasattr(x, "item") else x) for c, x in zip(chain, number)]
        if len(set(out)) != len(out):
            seen, twice = set(), None
            for k in out:
                if k in seen:
                    twice = k
                    break
                seen.add(k)
            raise ValueError(f"{what}: the residue {twice} occurs more than once")
        return out

    row_of = {k: i for i, k in enumerate(keys(chain_a, number_a, "structure a"))}
    return np.array([row_of.get(k, -1) for k in keys(chain_b, number_b, "structure b")], dtype=np.int32)


def invert(m, n_a: int) -> np.ndarray:
    """[n_a]: the reference row of every model row, or -1.  ``invert(invert(m, n_a), len(m))`` is ``m`` again."""
    m = validate(np.asarray(m).reshape(-1), n_a)
    out = np.full(n_a, -1, dtype=np.int32)
    rows = np.flatnonzero(m >= 0)
    out[m[rows]] = rows
    return out


def compose(map_bc, map_ab) -> np.ndarray:
    """``map_ab`` [N_b] sends rows of b to rows of a, ``map_bc`` [N_c] rows of c to rows of b: the map [N_c] from rows of c to rows of
    a, -1 where either leaves the row open."""
    map_ab, map_bc = _as_map(map_ab, "map_ab").reshape(-1), validate(np.asarray(map_bc).reshape(-1), len(np.asarray(map_ab).reshape(-1)))
    out = np.full(len(map_bc), -1, dtype=np.int32)
    rows = np.flatnonzero(map_bc >= 0)
    out[rows] = map_ab[map_bc[rows]]
    return out


def push_mask(mask_a, m) -> np.ndarray:
    """A mask over the model's rows (the diffuse mask of an inpainting run, say) in the reference's rows: [N_b] float32, the model's
    value where the row has a partner, 0 elsewhere."""
    mask_a = np.asarray(mask_a).reshape(-1)
    m = validate(np.asarray(m).reshape(-1), len(mask_a))
    out = np.zeros(len(m), dtype=np.float32)
    rows = np.flatnonzero(m >= 0)
    out[rows] = mask_a[m[rows]]
    return out


def gather(x, m, fill=0):
    """Rows of the model in the reference's order: ``x`` [N_a, ...] -> [N_b, ...] with ``fill`` where the map is -1 (the gathered model of
    the contract, on the host: what the tests compare the device's gather against)."""
    x = np.asarray(x)
    m = validate(np.asarray(m).reshape(-1), len(x))
    out = np.full((len(m),) + x.shape[1:], fill, dtype=x.dtype)
    rows = np.flatnonzero(m >= 0)
    out[rows] = x[m[rows]]
    return out
