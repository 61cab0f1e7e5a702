"""Novelty of samples on the device: search a set of structures with the alignment search of ``tm_align``.

``evaluation/eval_denovo.py:plot_novelty`` runs ``foldseek easy-search`` of every sample against a target database and keeps the largest
TM-score of the hits (``pdbTM``).  ``search`` is that quantity under this project's own alignment search (DESIGN.md sections 7.9 and
7.15): for every query the ``top_k`` entries of a ``StructureSet`` by TM-score, exactly what a brute-force ``tm_align`` over all entries
returns, bit for bit.  **No parity with foldseek is claimed**, and there is no prefilter: every pair is scored unless its length bound
shows that it cannot enter the result.  One call of ``fdipt_structure_search_inits`` (csrc/structsearch.hip, ABI in include/fdipt.h): the
entries stay packed (no padding to the longest), the score pass is launched bucket by bucket of entry length so that every block asks
for the LDS of its bucket's cap, the top-k lists are merged on the device after every bucket, and the hits run once more for their
transforms and alignments.
"""
from __future__ import annotations

import ctypes as C
import glob
import os

import numpy as np

from . import _call, _lib
from .tm_align import INITS, check_inits
from .tm_score import CA

MAX_ROWS = _lib.TMA_MAX_ROWS
MAX_K = _lib.SEARCH_MAX_K
PRUNED, TOO_LONG = _lib.SEARCH_PRUNED, _lib.SEARCH_TOO_LONG
RANK_BY = {"query": _lib.SEARCH_RANK_QUERY, "target": _lib.SEARCH_RANK_TARGET}
# the bucket edges of the score pass: an entry is scored in the launch of the smallest cap that holds it.  Steps of 16 .. 64 rows keep
# the LDS a block asks for within a few KB of what its entry needs (DESIGN.md section 7.15 has the table) and let the floors of the
# length bound rise a dozen times per search
BUCKET_CAPS = (16, 32, 48, 64, 96, 128, 192, 256, 320, 384, 448, 512)
assert BUCKET_CAPS[-1] == MAX_ROWS

_HIT_OUTPUTS = {"hit": "int32", "tm_q": "float64", "tm_t": "float64", "n_aligned": "int32", "rmsd": "float64", "status": "int32"}
_QUERY_OUTPUTS = {"n_scored": "int32", "n_pruned": "int32", "n_skipped": "int32", "pdb_tm": "float64"}
_PAIR_OUTPUTS = {"scores_q": "float64", "scores_t": "float64", "pair_n_aligned": "int32", "pair_rmsd": "float64", "pair_status": "int32"}
_INTS = ("hit", "n_aligned", "status", "n_scored", "n_pruned", "n_skipped", "pair_n_aligned", "pair_status", "alignment", "best_init")


class StructureSet:
    """A set of CA traces on the host, packed: ``ca`` [R,3] float32 (the CA atoms of all entries, one after the other), ``offsets``
    [D+1] int64 (entry e is rows offsets[e] .. offsets[e+1]) and ``names`` (D strings).  Entries of any length may be stored; ``search``
    skips those beyond ``MAX_ROWS`` rows and says so (``TOO_LONG``, ``n_skipped``)."""

    def __init__(self, ca, offsets, names=None):
        self.ca = np.ascontiguousarray(ca, dtype=np.float32).reshape(-1, 3)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(self.offsets) < 1 or self.offsets[0] != 0 or self.offsets[-1] != len(self.ca) or (np.diff(self.offsets) < 0).any():
            raise ValueError(f"offsets should ascend from 0 to the {len(self.ca)} rows of ca")
        self.names = [str(e) for e in range(len(self))] if names is None else [str(n) for n in names]
        if len(self.names) != len(self):
            raise ValueError(f"{len(self.names)} names for {len(self)} entries")
        self._on_device = {}  # device -> (ca, offsets) tensors, uploaded by the first search there

    def __len__(self):
        return len(self.offsets) - 1

    @property
    def lengths(self):
        return np.diff(self.offsets)

    def entry(self, e: int):
        return self.ca[self.offsets[e]:self.offsets[e + 1]]

    @classmethod
    def from_arrays(cls, traces, names=None):
        """``traces``: a list of [n_i,3] arrays, one per entry."""
        traces = [np.asarray(t, dtype=np.float32).reshape(-1, 3) for t in traces]
        ca = np.concatenate(traces) if traces else np.zeros((0, 3), dtype=np.float32)
        return cls(ca, np.concatenate([[0], np.cumsum([len(t) for t in traces])]), names)

    @classmethod
    def from_structures(cls, prot, mask=None, names=None):
        """``prot`` [S,N,37,3], [S,N,5,3] or a CA trace [S,N,3] (NumPy or a tensor); ``mask`` [S,N]: the rows of each entry, default all."""
        prot = _call.host(prot)
        if prot.ndim == 3 and prot.shape[2] == 3:
            ca = prot
        else:
            _call.structure_shape(prot, "prot", lead="S", items="structures")
            ca = prot[:, :, CA]
        keep = np.ones(ca.shape[:2], dtype=bool) if mask is None else _call.per_row(mask, ca.shape[:2], "mask", "mask") != 0
        return cls.from_arrays([ca[s][keep[s]] for s in range(ca.shape[0])], names)

    @classmethod
    def from_directory(cls, path, pattern="*"):
        """One entry per chain of every file of ``path`` that matches ``pattern`` (sorted by name), named ``file:chain``: ``.cif`` /
        ``.mmcif`` through ``data/mmcif.py`` (first model, the alternate location of highest occupancy), anything else as a PDB file
        (``read_pdb_ca``).  Rows without a CA atom are dropped."""
        traces, names = [], []
        for f in sorted(glob.glob(os.path.join(str(path), pattern))):
            if not os.path.isfile(f):
                continue
            for chain, ca in (read_mmcif_ca(f) if f.lower().endswith((".cif", ".mmcif")) else read_pdb_ca(f)).items():
                traces.append(ca)
                names.append(f"{os.path.basename(f)}:{chain}")
        return cls.from_arrays(traces, names)

    def save(self, path):
        """One ``.npz`` that holds arrays and names only."""
        with open(path, "wb") as f:  # (a file object: np.savez would append .npz to another suffix)
            np.savez(f, ca=self.ca, offsets=self.offsets, names=np.array(self.names, dtype=np.str_))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["ca"], z["offsets"], [str(n) for n in z["names"]])

    def on_device(self, dev):
        import torch
        if dev not in self._on_device:
            self._on_device[dev] = (torch.from_numpy(self.ca).to(dev), torch.from_numpy(self.offsets).to(dev))
        return self._on_device[dev]


def read_mmcif_ca(path) -> dict:
    """{chain: [n,3] float32} of an mmCIF file: the CA atoms of the rows ``data/mmcif.py:chain_features`` builds, file order."""
    from .data import features, mmcif
    rows, _ = mmcif.read_atom_site(path)
    ca = features.ATOM_ORDER["CA"]
    return {chain: f["atom_positions"][f["atom_mask"][:, ca] != 0, ca].astype(np.float32) for chain, f in mmcif.chain_features(rows).items()}


def read_pdb_ca(path) -> dict:
    """{chain: [n,3] float32} of a PDB file: the CA atoms of the ATOM and HETATM records of the first model, one per residue (chain,
    number, insertion code) in file order, the alternate location of highest occupancy (the first among equals)."""
    chains: dict = {}
    with open(path, encoding="utf-8", errors="replace") as f:
        for line in f:
            if line.startswith("ENDMDL"):
                break
            if not line.startswith(("ATOM", "HETATM")) or line[12:16].strip() != "CA" or len(line) < 54:
                continue
            occupancy = float(line[54:60]) if line[54:60].strip() else 1.0
            residues = chains.setdefault(line[21].strip() or "A", {})
            key = (line[22:27], line[17:20])
            if key not in residues or occupancy > residues[key][0]:
                residues[key] = (occupancy, (float(line[30:38]), float(line[38:46]), float(line[46:54])))
    return {chain: np.array([xyz for _, xyz in residues.values()], dtype=np.float32).reshape(-1, 3) for chain, residues in chains.items()}


def plan(lengths, rank_by: str = "query") -> dict:
    """The work plan of the score pass over entries of ``lengths`` rows.  Every entry of at most ``MAX_ROWS`` rows falls into the
    smallest cap of ``BUCKET_CAPS`` that holds it; the others are ``too_long``.  The buckets are ordered so that the length bound
    falls from launch to launch - ``tm_q <= min(n1, n2) / n1`` falls with shorter entries, so ``"query"`` starts with the longest;
    ``tm_t <= min(n1, n2) / n2`` falls with longer ones, so ``"target"`` starts with the shortest - and hold their entries in ascending
    index order.  Returns ``entries`` int32 (bucket by bucket), ``bucket_start`` int32 [B+1], ``bucket_cap`` int32 [B] (empty buckets
    left out), ``bucket_of`` int64 [D] (the index into ``BUCKET_CAPS``, -1 for too long), ``too_long`` bool [D], ``detail_cap``."""
    if rank_by not in RANK_BY:
        raise ValueError(f"rank_by should be one of {sorted(RANK_BY)}, got {rank_by!r}")
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    too_long = lengths > MAX_ROWS
    bucket_of = np.where(too_long, -1, np.searchsorted(np.asarray(BUCKET_CAPS), lengths, side="left"))
    order = range(len(BUCKET_CAPS))[::-1] if rank_by == "query" else range(len(BUCKET_CAPS))
    entries, start, caps = [], [0], []
    for b in order:
        members = np.flatnonzero(bucket_of == b)
        if len(members):
            entries.append(members)
            start.append(start[-1] + len(members))
            caps.append(BUCKET_CAPS[b])
    longest = int(lengths[~too_long].max()) if (~too_long).any() else 0
    return {"entries": np.concatenate(entries).astype(np.int32) if entries else np.zeros(0, dtype=np.int32), "bucket_start": np.array(start, dtype=np.int32),
            "bucket_cap": np.array(caps, dtype=np.int32), "bucket_of": bucket_of.astype(np.int64), "too_long": too_long,
            "detail_cap": BUCKET_CAPS[int(np.searchsorted(np.asarray(BUCKET_CAPS), max(longest, 1), side="left"))]}


def bound(n1, n2, rank_by: str = "query"):
    """The largest ranked score a pair of ``n1`` query rows and ``n2`` entry rows can reach: a score is a sum of at most min(n1, n2)
    terms, each at most 1, over the normalisation length."""
    n1, n2 = np.asarray(n1, dtype=np.float64), np.asarray(n2, dtype=np.float64)
    return np.minimum(n1, n2) / (n2 if rank_by == "target" else n1)


def search(prot, db: StructureSet, mask=None, top_k: int = 1, rank_by: str = "query", min_score: float = 0.0, prune: bool = True, details: bool = True,
           return_scores: bool = False, inits: str = "default") -> dict:
    """prot [Q,N_q,37,3] or [Q,N_q,5,3] float32, a device tensor (used in place) or a NumPy array (uploaded); ``mask`` [Q,N_q] (default:
    ones): the rows of each query.  The pair is (query, entry): ``tm_q`` is ``tm_a`` of ``tm_align``, normalised by the query's rows -
    the usual ``pdbTM`` - and ``tm_t`` is ``tm_b``, normalised by the entry's.  ``rank_by``: ``"query"`` or ``"target"``, the score the
    hits are ordered by: ranked score descending, then entry index ascending; NaN never ranks; hits below ``min_score`` are not returned.
    ``prune``: skip a pair whose length bound lies strictly below what the query's list already holds - the result is the same.
    ``inits``: the initial alignments of every pair's search, ``"default"`` or ``"all"`` as in ``tm_align``.

    Returns NumPy arrays: ``hit`` [Q,k] (entry index, -1 where fewer than k entries qualify), ``tm_q``, ``tm_t`` (NaN there),
    ``n_aligned``, ``rmsd``, ``status`` [Q,k] as in ``tm_align``; ``n_scored``, ``n_pruned``, ``n_skipped`` [Q] (pairs a block scored or
    refused with a status, pairs pruned, entries beyond ``MAX_ROWS`` rows); ``pdb_tm`` [Q], the ranked score of hit 0 (NaN without a
    hit).  With ``details``: ``rotation`` [Q,k,3,3], ``translation`` [Q,k,3] (R x + t ~ y, x the query), ``alignment`` [Q,k,L] (L the
    longest entry among the hits; the query row of each entry row, or -1), ``best_init``, ``names`` (the hits' names, None without a
    hit) and ``detail_tm_q`` / ``detail_tm_t``, the detail pass's own scores.  With ``return_scores``: ``scores_q`` / ``scores_t`` [Q,D]
    (NaN where pruned or skipped) and ``pair_status`` [Q,D] (``PRUNED``, ``TOO_LONG`` and the ``tm_align`` bits)."""
    n_q, rows, atoms = _call.structure_shape(prot, "prot", lead="Q", items="queries")
    check_inits(inits)
    if not isinstance(db, StructureSet):
        raise ValueError("db should be a StructureSet")
    if len(db) < 1:
        raise ValueError("the structure set is empty")
    top_k = int(top_k)
    if not 1 <= top_k <= MAX_K:
        raise ValueError(f"top_k should be 1 .. {MAX_K}, got {top_k}")
    work = plan(db.lengths, rank_by)
    if not np.isfinite(min_score):
        raise ValueError(f"min_score should be finite, got {min_score}")
    n_db, cap = len(db), int(work["detail_cap"])
    dev, (x,) = _call.upload("search", prot=prot)
    import torch
    ca, offsets = db.on_device(dev)
    outputs = {k: (t, (n_q, top_k)) for k, t in _HIT_OUTPUTS.items()}
    outputs.update({k: (t, (n_q,)) for k, t in _QUERY_OUTPUTS.items()})
    outputs.update({k: (t, (n_q, n_db)) for k, t in _PAIR_OUTPUTS.items()})
    detail = {"detail_tm_q": ("float64", (n_q, top_k)), "detail_tm_t": ("float64", (n_q, top_k)), "rotation": ("float64", (n_q, top_k, 3, 3)),
              "translation": ("float64", (n_q, top_k, 3)), "alignment": ("int32", (n_q, top_k, cap)), "best_init": ("int32", (n_q, top_k))}
    if details:
        outputs.update(detail)
    scalars = dict(Q=n_q, N_q=rows, atoms=atoms, ca=CA, D=n_db, top_k=top_k, rank_by=RANK_BY[rank_by], prune=int(bool(prune)), details=int(bool(details)),
                   n_buckets=len(work["bucket_cap"]), detail_cap=cap, R=len(db.ca), min_score=float(min_score),
                   bucket_start=work["bucket_start"].ctypes.data_as(C.c_void_p), bucket_cap=work["bucket_cap"].ctypes.data_as(C.c_void_p))
    if not details:
        scalars.update({k: None for k in detail})
    out = _call.run("fdipt_structure_search_inits", _lib.SearchArgs, dev, scalars,
                    dict(prot=x, mask=_call.per_row(mask, (n_q, rows), "mask", "mask", default=1, dev=dev), db_ca=ca, db_offsets=offsets,
                         plan_entries=torch.from_numpy(work["entries"]).to(dev) if len(work["entries"]) else None),
                    outputs, widen=_INTS, workspace=("fdipt_structure_search_workspace", n_q, top_k, int(bool(details))), extra=(INITS[inits],))
    if details:
        hits = out["hit"]
        longest = int(db.lengths[hits[hits >= 0]].max()) if (hits >= 0).any() else 0
        out["alignment"] = np.ascontiguousarray(out["alignment"][:, :, :longest])
        out["names"] = [[db.names[e] if e >= 0 else None for e in row] for row in hits]
    if not return_scores:
        for k in _PAIR_OUTPUTS:
            del out[k]
    else:
        del out["pair_n_aligned"], out["pair_rmsd"]
    out["rank_by"], out["inits"] = rank_by, inits
    return out


def novelty_metrics(result: dict, q: int, db: StructureSet = None) -> dict:
    """The reference's novelty entry of query ``q`` of a ``search`` result: ``pdbTM`` (the ranked score of the best hit, NaN without
    one), the hit's name (from the result's ``names``, else from ``db``, else its index), ``tm_t`` and ``n_aligned``."""
    e = int(result["hit"][q, 0])
    name = None if e < 0 else result["names"][q][0] if "names" in result else db.names[e] if db is not None else str(e)
    return {"pdbTM": float(result["pdb_tm"][q]), "hit": name, "tm_t": float(result["tm_t"][q, 0]), "n_aligned": int(result["n_aligned"][q, 0])}


def hit_accuracy(result: dict, prot, db: StructureSet, mask=None, atoms: str = "ca", coverage: str = "penalise", superpose: str = "search") -> dict:
    """Is a query locally the same fold as its hits?  lDDT-CA and GDT of every query of a ``search`` result (``details=True``) against
    each of its hits, through the hit's ``alignment`` (``lddt.local_accuracy`` and ``gdt.gdt_scores`` with ``alignment=``; DESIGN.md
    section 7.16): the hit is the reference, so ``coverage="penalise"`` charges the entry rows the query has no partner for, and GDT is
    normalised by the hit's rows.  ``prot`` / ``mask``: what ``search`` was given.  The hits' traces are gathered from the set into one
    padded [Q * top_k, L, 3] array.  A structure set holds CA traces: ``atoms`` is "ca".

    Returns [Q,k] arrays - ``lddt``, ``gdt_ts``, ``gdt_ha`` float64 (NaN without a hit), ``n_covered``, ``n_reference`` int64,
    ``coverage`` - and ``res_lddt`` [Q,k,L] float64, ``res_within`` [Q,k,L] int32, ``lddt_status``, ``gdt_status`` [Q,k]."""
    if atoms != "ca":
        raise ValueError(f"a structure set holds CA traces: atoms should be 'ca', got {atoms!r}")
    if "alignment" not in result:
        raise ValueError("hit_accuracy needs the alignments of the hits: search(..., details=True)")
    from . import gdt, lddt
    hits, alignment = np.asarray(result["hit"]), np.asarray(result["alignment"])
    n_q, top_k, rows = alignment.shape
    if rows == 0:  # (no query has a hit)
        nan, zero = np.full((n_q, top_k), np.nan), np.zeros((n_q, top_k), dtype=np.int64)
        return {"lddt": nan, "gdt_ts": nan.copy(), "gdt_ha": nan.copy(), "n_covered": zero, "n_reference": zero.copy(), "coverage": zero.astype(np.float64),
                "res_lddt": np.zeros((n_q, top_k, 0)), "res_within": np.zeros((n_q, top_k, 0), dtype=np.int32), "lddt_status": zero.copy(), "gdt_status": zero.copy()}
    ref, ref_mask = np.zeros((n_q * top_k, rows, 3), dtype=np.float32), np.zeros((n_q * top_k, rows), dtype=np.float32)
    for p, e in enumerate(hits.reshape(-1)):
        if e >= 0:
            trace = db.entry(int(e))
            ref[p, :len(trace)], ref_mask[p, :len(trace)] = trace, 1
    maps = np.where(ref_mask != 0, alignment.reshape(n_q * top_k, rows), -1).astype(np.int32)
    pairs = np.stack([np.repeat(np.arange(n_q), top_k), np.arange(n_q * top_k)], axis=1).astype(np.int32)
    ca = prot if tuple(prot.shape[2:]) == (3,) else prot[:, :, CA]  # (a trace for the GDT entry: a CA trace goes with a CA trace)
    local = lddt.local_accuracy(ca, ref, atoms="ca", res_mask=mask, res_mask_b=ref_mask, pairs=pairs, alignment=maps, coverage=coverage)
    glob = gdt.gdt_scores(ca, ref, mask_a=mask, mask_b=ref_mask, pairs=pairs, alignment=maps, norm_length="reference", superpose=superpose)
    miss = (hits < 0)
    shape = (n_q, top_k)
    out = {"lddt": np.where(miss, np.nan, local["lddt"].reshape(shape)), "gdt_ts": glob["gdt_ts"].reshape(shape), "gdt_ha": glob["gdt_ha"].reshape(shape),
           "n_covered": local["n_covered"].reshape(shape), "n_reference": local["n_reference"].reshape(shape), "coverage": local["coverage"].reshape(shape),
           "res_lddt": local["res_lddt"].reshape(shape + (rows,)), "res_within": glob["res_within"].reshape(shape + (rows,)),
           "lddt_status": local["status"].reshape(shape), "gdt_status": glob["status"].reshape(shape)}
    return out


def hit_accuracy_metrics(accuracy: dict, q: int, k: int = 0) -> dict:
    """The flat entries of hit ``k`` of query ``q`` of a ``hit_accuracy`` result, as Python numbers."""
    return {"lddt_ca": float(accuracy["lddt"][q, k]), "gdt_ts": float(accuracy["gdt_ts"][q, k]), "gdt_ha": float(accuracy["gdt_ha"][q, k]),
            "n_covered": int(accuracy["n_covered"][q, k]), "n_reference": int(accuracy["n_reference"][q, k]), "coverage": float(accuracy["coverage"][q, k])}
