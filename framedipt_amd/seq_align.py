"""Sequence alignment on the device: global alignment with affine gaps (Gotoh, three states) as a producer of row maps and as the
sequence identity of sequences of different lengths.

``align_sequences`` is one call of ``fdipt_seq_align`` (csrc/seqalign.hip, ABI in include/fdipt.h) for any number of pairs; DESIGN.md
section 7.17 is the contract.  It restates what the reference's ``framedipt/protein/align.py`` asks of ``Bio.Align.PairwiseAligner``
(mode ``global``, BLOSUM62, open -10, extend -0.5, end gaps as inner gaps) in exact integer arithmetic in half units.  Biopython was not
at hand: parity with ``PairwiseAligner`` is claimed for the SCORE only - the score of an optimal alignment is unique - and as far as the
NumPy restatement and a brute-force enumeration pin it; which co-optimal alignment ``aligner.align(...)[0]`` returns is not reproduced.
Among equal candidates the first of M, X, Y wins (this project's own rule).  The BLOSUM62 table below was entered by hand.

``chain_row_map`` is the reference's per-chain procedure: chains with equal labels are aligned, one pair each in one launch, and their
maps are offset into whole-structure rows - the layout ``lddt.local_accuracy(..., alignment=)`` and ``gdt.gdt_scores(..., alignment=)``
read (``compare.sequence_aligned_accuracy`` does the three calls).  ``row_map.from_residue_numbers`` is the counterpart by numbering.

``mode="semiglobal"`` (chosen end gaps free: ``free_ends``) and ``mode="local"`` go through ``fdipt_seq_align_modes``
(csrc/seqalign_modes.hip) and say where the charged path lies: ``begin_a``, ``end_a``, ``begin_b``, ``end_b``.  The
same claim holds for them - the score only, against ``PairwiseAligner`` with ``mode = "local"`` or with its end-gap scores set to 0 on the
matching sides; the rules that choose among equal end cells are this project's own.  ``chain_row_map(exclude_a=, exclude_b=)`` is the
reference's ``exclude_region``, on the host.

Not built: other built-in tables, per-pair modes in one launch, distinct end-gap penalties other than 0.
"""
from __future__ import annotations

import numpy as np

from . import _call, _lib
from .output import RESTYPES

MAX_ROWS = _lib.SEQ_MAX_ROWS
LETTERS = RESTYPES + "X"  # aatype 0 .. 20
X = 20
EMPTY, BAD_LETTER, SKIPPED, NO_ALIGNED = _lib.SEQ_EMPTY, _lib.SEQ_BAD_LETTER, _lib.SEQ_SKIPPED, _lib.SEQ_NO_ALIGNED
MODES = {"global": _lib.SEQ_MODE_GLOBAL, "semiglobal": _lib.SEQ_MODE_SEMIGLOBAL, "local": _lib.SEQ_MODE_LOCAL}
FREE_ENDS = {"a_left": _lib.SEQ_FREE_A_LEFT, "a_right": _lib.SEQ_FREE_A_RIGHT, "b_left": _lib.SEQ_FREE_B_LEFT, "b_right": _lib.SEQ_FREE_B_RIGHT}
_FREE_SHORTHANDS = {"a": ("a_left", "a_right"), "b": ("b_left", "b_right"), "all": tuple(FREE_ENDS)}
_COUNTS = ("n_aligned", "n_identical", "n_gaps_a", "n_gaps_b", "n_gap_runs")
_SPAN = ("begin_a", "end_a", "begin_b", "end_b")
_INTS = ("score",) + _COUNTS + ("alignment", "status")
_MAX_WHOLE = _lib.SEQ_MAX_HALF_UNITS // 2

# BLOSUM62 in restype order ARNDCQEGHILKMFPSTWYV, whole units; entered by hand (tests/test_seq_align_host.py holds its invariants)
_B62 = """
 4 -1 -2 -2  0 -1 -1  0 -2 -1 -1 -1 -1 -2 -1  1  0 -3 -2  0
-1  5  0 -2 -3  1  0 -2  0 -3 -2  2 -1 -3 -2 -1 -1 -3 -2 -3
-2  0  6  1 -3  0  0  0  1 -3 -3  0 -2 -3 -2  1  0 -4 -2 -3
-2 -2  1  6 -3  0  2 -1 -1 -3 -4 -1 -3 -3 -1  0 -1 -4 -3 -3
 0 -3 -3 -3  9 -3 -4 -3 -3 -1 -1 -3 -1 -2 -3 -1 -1 -2 -2 -1
-1  1  0  0 -3  5  2 -2  0 -3 -2  1  0 -3 -1  0 -1 -2 -1 -2
-1  0  0  2 -4  2  5 -2  0 -3 -3  1 -2 -3 -1  0 -1 -3 -2 -2
 0 -2  0 -1 -3 -2 -2  6 -2 -4 -4 -2 -3 -3 -2  0 -2 -2 -3 -3
-2  0  1 -1 -3  0  0 -2  8 -3 -3 -1 -2 -1 -2 -1 -2 -2  2 -3
-1 -3 -3 -3 -1 -3 -3 -4 -3  4  2 -3  1  0 -3 -2 -1 -3 -1  3
-1 -2 -3 -4 -1 -2 -3 -4 -3  2  4 -2  2  0 -3 -2 -1 -2 -1  1
-1  2  0 -1 -3  1  1 -2 -1 -3 -2  5 -1 -3 -1  0 -1 -3 -2 -2
-1 -1 -2 -3 -1  0 -2 -3 -2  1  2 -1  5  0 -2 -1 -1 -1 -1  1
-2 -3 -3 -3 -2 -3 -3 -3 -1  0  0 -3  0  6 -4 -2 -2  1  3 -1
-1 -2 -2 -1 -3 -1 -1 -2 -2 -3 -3 -1 -2 -4  7 -1 -1 -4 -3 -2
 1 -1  1  0 -1  0  0  0 -1 -2 -2  0 -1 -2 -1  4  1 -3 -2 -2
 0 -1  0 -1 -1 -1 -1 -2 -2 -1 -1 -1 -1 -2 -1  1  5 -2 -2  0
-3 -3 -4 -4 -2 -2 -3 -2 -2 -3 -2 -3 -1  1 -4 -3 -2 11  2 -3
-2 -2 -2 -3 -2 -1 -2 -3  2 -1 -1 -2 -1  3 -3 -2 -2  2  7 -1
 0 -3 -3 -3 -1 -2 -2 -3 -3  3  1 -2  1 -1 -2 -2  0 -3 -1  4
"""


def _blosum62() -> np.ndarray:
    t = np.full((21, 21), -1, dtype=np.int32)
    t[:20, :20] = np.array(_B62.split(), dtype=np.int32).reshape(20, 20)
    for letters, value in (("AST", 0), ("CPW", -2)):  # the X row and column of the NCBI table: 0 / -2 against these, -1 elsewhere
        for c in letters:
            t[X, RESTYPES.index(c)] = t[RESTYPES.index(c), X] = value
    return t


def _identity() -> np.ndarray:
    t = np.where(np.eye(21, dtype=bool), 1, -1).astype(np.int32)
    t[X, X] = -1  # X never matches
    return t


BLOSUM62 = _blosum62()
IDENTITY = _identity()
_TABLES = {"blosum62": BLOSUM62, "identity": IDENTITY}


def half_units(value, what: str) -> int:
    """A gap penalty in half units; ValueError unless it is a multiple of 0.5 in -4096 .. 0."""
    twice = 2.0 * float(value)
    if twice != round(twice) or not -_lib.SEQ_MAX_HALF_UNITS <= twice <= 0:
        raise ValueError(f"{what} should be a multiple of 0.5 in {-_MAX_WHOLE} .. 0, got {value!r}")
    return int(round(twice))


def table_half_units(matrix) -> np.ndarray:
    """``matrix`` (a built-in table's name or integers [21,21] in whole units) as the device's int32 table of twice the score."""
    if isinstance(matrix, str):
        if matrix not in _TABLES:
            raise ValueError(f"matrix should be one of {sorted(_TABLES)} or an integer [21, 21] array, got {matrix!r}")
        return np.ascontiguousarray(2 * _TABLES[matrix], dtype=np.int32)
    t = _call.host(matrix)
    if t.shape != (21, 21) or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"matrix should be integers [21, 21] in whole units, got {t.dtype} {t.shape}")
    if np.abs(t).max() > _MAX_WHOLE:
        raise ValueError(f"matrix entries should lie within +-{_MAX_WHOLE}")
    return np.ascontiguousarray(2 * t.astype(np.int64), dtype=np.int32)


def encode(sequence: str) -> np.ndarray:
    """One-letter codes as aatype; a letter outside ``ARNDCQEGHILKMFPSTWYV`` becomes X (20)."""
    return np.array([LETTERS.find(c) if c in RESTYPES else X for c in sequence.upper()], dtype=np.int32)


def _sequences(seq, lengths, what: str):
    """(letters, lengths [S] int32): ``letters`` a device tensor [S,N] as given, or int32 NumPy [S,N] padded with X from strings, ragged
    lists or an array.  Every check that needs no device is made here."""
    if hasattr(seq, "detach"):
        if seq.is_floating_point() or seq.is_complex() or seq.dim() not in (1, 2):
            raise ValueError(f"{what} should be an integer tensor [S, N] or [N], got {seq.dtype} {tuple(seq.shape)}")
        letters = seq.reshape(1, -1) if seq.dim() == 1 else seq
    else:
        rows = [seq] if isinstance(seq, str) else seq
        if isinstance(rows, np.ndarray):
            if rows.ndim not in (1, 2) or not (np.issubdtype(rows.dtype, np.integer) or rows.size == 0):
                raise ValueError(f"{what} should be an integer array [S, N] or [N], got {rows.dtype} {rows.shape}")
            letters = np.ascontiguousarray(rows.reshape(1, -1) if rows.ndim == 1 else rows, dtype=np.int32)
        else:
            rows = list(rows)
            if rows and not isinstance(rows[0], str) and np.ndim(rows[0]) == 0:
                rows = [rows]  # one sequence as a list of letters
            rows = [encode(r) if isinstance(r, str) else np.asarray(r) for r in rows]
            for r in rows:
                if r.ndim != 1 or not (np.issubdtype(r.dtype, np.integer) or r.size == 0):
                    raise ValueError(f"{what} should hold one-letter strings or integer rows, got {r.dtype} {r.shape}")
            if lengths is not None and len({len(r) for r in rows}) > 1:
                raise ValueError(f"{what} is ragged: its rows carry their lengths")
            if lengths is None:
                lengths = [len(r) for r in rows]
            letters = np.full((len(rows), max([len(r) for r in rows] + [1])), X, dtype=np.int32)
            for k, r in enumerate(rows):
                letters[k, :len(r)] = r
    s, n = int(letters.shape[0]), int(letters.shape[1])
    if s < 1 or n < 1:
        raise ValueError(f"{what} {(s, n)}: no sequences or no columns")
    lens = np.full(s, n, dtype=np.int32) if lengths is None else np.asarray(_call.host(lengths)).reshape(-1).astype(np.int64)
    if lens.shape != (s,) or lens.min() < 0 or lens.max() > n:
        raise ValueError(f"lengths of {what} should be [{s}] within 0 .. {n} (the padded width), got {lens.shape} within {lens.min()} .. {lens.max()}")
    if isinstance(letters, np.ndarray):
        inside = np.arange(n)[None, :] < lens[:, None]
        if np.any(inside & ((letters < 0) | (letters > X))):
            raise ValueError(f"{what} holds a letter outside 0 .. {X}")
    return letters, lens.astype(np.int32)


def _upload(dev, x):
    import torch
    return (x.to(dev) if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)).to(torch.int32).contiguous()


def free_end_bits(mode: str, free_ends) -> int:
    """The ``FDIPT_SEQ_FREE_*`` bits of ``free_ends`` under ``mode``: names out of ``FREE_ENDS`` (an iterable), or the shorthands "a"
    (both ends of a free: b is fitted into a), "b" and "all" (an overlap alignment; the default of ``semiglobal``).  ValueError for an
    unknown mode or name, and for ``free_ends`` with another mode than "semiglobal"."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode should be one of {sorted(MODES)}, got {mode!r}")
    if mode != "semiglobal":
        if free_ends is not None:
            raise ValueError(f"free_ends belongs to mode='semiglobal', got mode={mode!r}")
        return 0
    if free_ends is None:
        free_ends = "all"
    names = _FREE_SHORTHANDS.get(free_ends, (free_ends,)) if isinstance(free_ends, str) else tuple(free_ends)
    unknown = [n for n in names if not isinstance(n, str) or n not in FREE_ENDS]
    if unknown:
        raise ValueError(f"free_ends should be 'a', 'b', 'all' or names out of {sorted(FREE_ENDS)}, got {unknown}")
    bits = 0
    for n in names:
        bits |= FREE_ENDS[n]
    return bits


def align_sequences(seq_a, seq_b=None, len_a=None, len_b=None, pairs=None, ref_index=None, matrix="blosum62", open_gap: float = -10.0,
                    extend_gap: float = -0.5, traceback: bool = True, max_workspace_bytes: int = 2 ** 30, mode: str = "global",
                    free_ends=None) -> dict:
    """seq_a: sequences as an integer array or device tensor [S,N_a] (aatype, 20 = X; ``len_a`` [S]: their lengths, default N_a), a list of
    one-letter strings (a letter outside the twenty becomes X) or a ragged list of integer rows (padded here).  seq_b, len_b: the second
    side likewise, or None.  Pairs as ``tm_align`` plans them: ``pairs`` [P,2]; no seq_b and no ref_index: all i < j of seq_a (the result
    carries ``matrix``, the mirrored ``identity_short``); else sequence i against ``ref_index[i]`` (default: row i, or the one row).

    ``matrix``: "blosum62", "identity" (+1 / -1, X never matches) or integers [21,21] in whole units; ``open_gap``, ``extend_gap``:
    multiples of 0.5, <= 0; a gap of k positions costs open + (k - 1) extend.  ``traceback=False``: no ``alignment`` and no workspace -
    every other output is the same number.  ``max_workspace_bytes`` caps the direction slabs (fewer persistent waves; same result).

    Returns per pair ``score`` (float64, whole units), ``n_aligned``, ``n_identical`` (equal letters, X excluded), ``n_gaps_a`` /
    ``n_gaps_b`` (gap positions in a / in b), ``n_gap_runs``, ``alignment`` [P,N_b] (the row of a aligned with each row of b, or -1),
    ``status`` (EMPTY, BAD_LETTER, SKIPPED), ``identity`` = n_identical / n_aligned, ``identity_b`` = n_identical / len_b,
    ``identity_short`` = n_identical / min(len_a, len_b) (0 where the divisor is 0), ``len_a``, ``len_b`` and ``pairs`` [P,2].

    ``mode``: "global" (end gaps charged like inner gaps; ``fdipt_seq_align``), "semiglobal" or "local" (``fdipt_seq_align_modes``,
    DESIGN.md section 7.20).  ``free_ends`` (semiglobal only; ``free_end_bits``): which end gaps cost nothing - names out of
    ``FREE_ENDS``, "a" (b is fitted into a), "b", or "all" (the default: an overlap alignment).  Every mode adds the span of the charged
    path, ``begin_a``, ``end_a``, ``begin_b``, ``end_b`` (global: 0, len_a, 0, len_b, formed here) - it aligns a[begin_a:end_a] with
    b[begin_b:end_b] globally, the counts are those of the span and ``alignment`` is -1 outside it -, ``mode``, ``identity_span_b`` =
    n_identical / (end_b - begin_b) and ``coverage_b`` = (end_b - begin_b) / len_b.  The two new modes set NO_ALIGNED in ``status`` where
    the result has no aligned column (an empty local result, a semi-global optimum of free runs only)."""
    bits = free_end_bits(mode, free_ends)
    table = table_half_units(matrix)
    o, e = half_units(open_gap, "open_gap"), half_units(extend_gap, "extend_gap")
    if int(max_workspace_bytes) < 0:
        raise ValueError(f"max_workspace_bytes should not be negative, got {max_workspace_bytes}")
    if seq_b is None and len_b is not None:
        raise ValueError("len_b without seq_b: the sequences of seq_a carry len_a")
    xa, la = _sequences(seq_a, len_a, "seq_a")
    xb, lb = (xa, la) if seq_b is None else _sequences(seq_b, len_b, "seq_b")
    s_a, n_a, s_b, n_b = int(xa.shape[0]), int(xa.shape[1]), int(xb.shape[0]), int(xb.shape[1])
    pair_list, square = _call.plan_pairs(s_a, s_b, seq_b is not None, pairs, ref_index)
    n_pairs = len(pair_list)
    if n_pairs and (pair_list.min() < 0 or pair_list[:, 0].max() >= s_a or pair_list[:, 1].max() >= s_b):
        raise ValueError(f"pairs should index {s_a} and {s_b} sequences")
    ints = _INTS if mode == "global" else _INTS + _SPAN
    outputs = {k: ("int32", (n_pairs, n_b) if k == "alignment" else (n_pairs,)) for k in ints if traceback or k != "alignment"}
    if n_pairs == 0:
        out = _call.empty_outputs(outputs, ints)
    else:
        import torch
        tensors = [x for x in (xa, xb) if torch.is_tensor(x)]
        for x in tensors:
            _lib.require_cuda(x, "align_sequences")
            if x.device != tensors[0].device:
                raise ValueError(f"seq_a on {xa.device}, seq_b on {xb.device}")
        dev = tensors[0].device if tensors else torch.device("cuda", torch.cuda.current_device())
        max_a, max_b = int(la.max()), int(lb.max())
        da = _upload(dev, xa)
        scalars = dict(S_a=s_a, N_a=n_a, S_b=s_b, N_b=n_b, P=n_pairs, max_len_a=max_a, max_len_b=max_b, open_gap=o, extend_gap=e, traceback=int(bool(traceback)))
        entry, struct = ("fdipt_seq_align", _lib.SeqAlignArgs) if mode == "global" else ("fdipt_seq_align_modes", _lib.SeqAlignModeArgs)
        if mode != "global":
            scalars.update(mode=MODES[mode], free_ends=bits)
        out = _call.run(entry, struct, dev, scalars,
                        dict(seq_a=da, len_a=_upload(dev, la), seq_b=None if seq_b is None else _upload(dev, xb), len_b=None if seq_b is None else _upload(dev, lb),
                             pairs=torch.from_numpy(pair_list).to(dev), table=_upload(dev, table)),
                        outputs, widen=ints,
                        workspace=(entry + "_workspace_bytes", n_pairs, max_a, max_b, int(bool(traceback)), int(max_workspace_bytes)))
    out["score"] = out["score"].astype(np.float64) / 2.0
    out["len_a"], out["len_b"] = la[pair_list[:, 0]].astype(np.int64), lb[pair_list[:, 1]].astype(np.int64)
    if mode == "global":  # the whole of both sequences, for every pair the device served
        served = (out["status"] & (EMPTY | SKIPPED)) == 0
        out.update(begin_a=np.zeros(n_pairs, dtype=np.int64), end_a=np.where(served, out["len_a"], 0), begin_b=np.zeros(n_pairs, dtype=np.int64),
                   end_b=np.where(served, out["len_b"], 0))
    out["mode"] = mode
    out.update(identities(out["n_identical"], out["n_aligned"], out["len_a"], out["len_b"]))
    span_b = (out["end_b"] - out["begin_b"]).astype(np.float64)
    out["identity_span_b"] = np.divide(out["n_identical"], span_b, out=np.zeros(n_pairs), where=span_b > 0)
    out["coverage_b"] = np.divide(span_b, out["len_b"], out=np.zeros(n_pairs), where=out["len_b"] > 0)
    out["pairs"] = pair_list.astype(np.int64)
    if square:
        out["matrix"] = _call.square_matrix(s_a, pair_list, out["identity_short"])
    return out


def identities(n_identical, n_aligned, len_a, len_b) -> dict:
    """The three identities from the integer counts (float64; 0 where the divisor is 0)."""
    n_identical = np.asarray(n_identical, dtype=np.float64)

    def over(d):
        d = np.asarray(d, dtype=np.float64)
        return np.divide(n_identical, d, out=np.zeros_like(n_identical), where=d > 0)

    return {"identity": over(n_aligned), "identity_b": over(len_b), "identity_short": over(np.minimum(len_a, len_b))}


# ---- chains (host)
def chain_runs(chain, n: int, what: str = "chain"):
    """[(label, start, stop)]: the chains of ``chain`` [n] (None or one label: one chain), each a run of consecutive rows with one label;
    a label that returns later is refused, as evaluation.py refuses it."""
    if chain is None or np.ndim(chain) == 0:
        return [(None if chain is None else (chain.item() if hasattr(chain, "item") else chain), 0, n)]
    labels = [c.item() if hasattr(c, "item") else c for c in np.asarray(_call.host(chain)).reshape(-1)]
    if len(labels) != n:
        raise ValueError(f"{what} holds {len(labels)} labels for {n} rows")
    runs = []
    for k, c in enumerate(labels):
        if runs and runs[-1][0] == c:
            runs[-1][2] = k + 1
        else:
            if any(r[0] == c for r in runs):
                raise ValueError(f"{what}: the label {c!r} returns at row {k}; a chain is one run of consecutive rows")
            runs.append([c, k, k + 1])
    return [tuple(r) for r in runs]


def plan_chains(chain_a, n_a: int, chain_b, n_b: int, chain_pairs=None):
    """[(label_a, label_b, (start_a, stop_a), (start_b, stop_b))]: the chain pairs to align - equal labels (in the order of b's chains), or
    the listed ``chain_pairs`` [(label_a, label_b)].  A listed label that no chain carries, or one listed twice, is refused."""
    runs_a = {r[0]: r[1:] for r in chain_runs(chain_a, n_a, "chain_a")}
    runs_b = {r[0]: r[1:] for r in chain_runs(chain_b, n_b, "chain_b")}
    if chain_pairs is None:
        chain_pairs = [(c, c) for c in runs_b if c in runs_a]
    chain_pairs = [tuple(p) for p in chain_pairs]
    for side, runs, what in ((0, runs_a, "chain_a"), (1, runs_b, "chain_b")):
        named = [p[side] for p in chain_pairs]
        if len(set(named)) != len(named) or any(c not in runs for c in named):
            raise ValueError(f"chain_pairs should name each chain of {what} at most once, from {sorted(runs, key=str)}; got {named}")
    return [(ca, cb, runs_a[ca], runs_b[cb]) for ca, cb in chain_pairs]


def assemble_map(plan, alignments, n_b: int) -> np.ndarray:
    """The whole-structure map [n_b] from the per-chain maps: ``alignments[k]`` (entries relative to chain a's first row, at least
    stop_b - start_b of them) is offset by the chains' first rows; the rows of an unpaired chain of b stay -1."""
    out = np.full(n_b, -1, dtype=np.int32)
    for (_, _, (sa, _), (sb, eb)), m in zip(plan, alignments):
        m = np.asarray(m)[:eb - sb]
        out[sb:eb] = np.where(m >= 0, m + sa, -1)
    return out


def _regions(exclude, n: int, what: str):
    """``exclude`` as one inclusive (start, end) per chain pair, (-1, -1) for None - the reference's default, which holds no row."""
    if exclude is None:
        return [(-1, -1)] * n
    regions = [(-1, -1) if r is None else tuple(int(v) for v in r) for r in exclude]
    if len(regions) != n or any(len(r) != 2 for r in regions):
        raise ValueError(f"{what} should hold one inclusive (start, end) or None for each of the {n} chain pairs, got {exclude!r}")
    return regions


def drop_excluded(alignments, exclude_a, exclude_b):
    """The reference's ``exclude_region`` on per-chain maps (rows relative to each chain): an aligned column whose row of a lies inside the
    pair's region of a is dropped from the map; its row of b must then lie inside the region of b - ValueError otherwise, as
    get_shared_residues_info raises.  The converse is not checked, as there.  Returns (maps, n_excluded [pairs])."""
    maps, dropped = [], np.zeros(len(alignments), dtype=np.int64)
    for k, (m, (sa, ea), (sb, eb)) in enumerate(zip(alignments, exclude_a, exclude_b)):
        m = np.array(m, dtype=np.int64)
        inside = (m >= 0) & (sa <= m) & (m <= ea)
        rows_b = np.flatnonzero(inside)
        if np.any((rows_b < sb) | (rows_b > eb)):
            raise ValueError(f"chain pair {k}: a row of a inside its excluded region {(sa, ea)} is aligned with a row of b outside {(sb, eb)}; "
                             "both chains should have the same excluded region")
        m[inside] = -1
        maps.append(m)
        dropped[k] = int(inside.sum())
    return maps, dropped


def chain_row_map(aatype_a, chain_a, aatype_b, chain_b, chain_pairs=None, exclude_a=None, exclude_b=None, **scoring) -> dict:
    """The reference's per-chain procedure (framedipt/protein/align.py:get_shared_residues_info): aatype_a [N_a] and aatype_b [N_b] (integers,
    or one-letter strings) with chain labels chain_a [N_a], chain_b [N_b] (None: one chain).  The chains with equal labels, or the listed
    ``chain_pairs`` [(label_a, label_b)], are aligned in one launch; ``scoring``: ``matrix``, ``open_gap``, ``extend_gap``,
    ``max_workspace_bytes``, ``mode`` and ``free_ends`` of ``align_sequences`` (``mode="semiglobal", free_ends="a"`` fits a reference chain
    that lacks termini into the model's; a chain pair without an aligned column, NO_ALIGNED, leaves its rows at -1).
    ``exclude_a``, ``exclude_b``: the reference's ``exclude_region`` - per chain pair one inclusive (start, end) in rows relative to the
    chain, or None; ``drop_excluded`` applies them to the maps, the per-pair counts stay those of the alignment before.

    Returns ``alignment`` [N_b] (the row of a for each row of b, -1 for a gap and for every row of an unpaired chain), ``chains`` (the label
    pairs) and per chain pair ``score``, ``identity``, ``identity_b``, ``identity_short``, ``identity_span_b``, ``coverage_b``,
    ``n_aligned``, ``n_identical``, ``n_gaps_a``, ``n_gaps_b``, ``n_gap_runs``, ``begin_a``, ``end_a``, ``begin_b``, ``end_b`` (relative to the
    chains), ``n_excluded``, ``status``."""
    a = encode(aatype_a) if isinstance(aatype_a, str) else np.asarray(_call.host(aatype_a)).reshape(-1)
    b = encode(aatype_b) if isinstance(aatype_b, str) else np.asarray(_call.host(aatype_b)).reshape(-1)
    free_end_bits(scoring.get("mode", "global"), scoring.get("free_ends"))
    plan = plan_chains(chain_a, len(a), chain_b, len(b), chain_pairs)
    regions_a, regions_b = _regions(exclude_a, len(plan), "exclude_a"), _regions(exclude_b, len(plan), "exclude_b")
    floats = ("score", "identity", "identity_b", "identity_short", "identity_span_b", "coverage_b")
    keys = floats + ("status",) + _COUNTS + _SPAN
    if not plan:
        out = {k: np.zeros(0, dtype=np.float64 if k in floats else np.int64) for k in keys}
        return dict(out, n_excluded=np.zeros(0, dtype=np.int64), alignment=np.full(len(b), -1, dtype=np.int32), chains=[])
    found = align_sequences([a[s:e] for _, _, (s, e), _ in plan], [b[s:e] for _, _, _, (s, e) in plan], traceback=True, **scoring)
    out = {k: found[k] for k in keys}
    maps, out["n_excluded"] = drop_excluded([m[:e - s] for m, (_, _, _, (s, e)) in zip(found["alignment"], plan)], regions_a, regions_b)
    return dict(out, alignment=assemble_map(plan, maps, len(b)), chains=[(ca, cb) for ca, cb, _, _ in plan])
