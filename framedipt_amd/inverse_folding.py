"""Inverse folding on the device: ProteinMPNN scoring and sequence design for sampled backbones.

The reference's first step after sampling (experiments/inference.py:run_self_consistency -> run_protein_mpnn) is a subprocess of
ProteinMPNN/protein_mpnn_run.py per sample directory.  Here the vanilla full-backbone model (ProteinMPNN/protein_mpnn_utils.py:
ProteinFeatures, EncLayer, DecLayer, ProteinMPNN.forward and .sample) runs on the device through ``fdipt_mpnn_score`` and
``fdipt_mpnn_design`` (csrc/mpnn.hip, ABI in include/fdipt.h); DESIGN.md section 7.10 is the contract.  Inference only, float32.
Section 7.11 adds what the vendored ProteinMPNN offers beyond that subprocess: the per-row controls of ``sample`` (``bias_by_res``,
``omit_AA_mask``, the two PSSM stages), tied positions (``tied_sample``; ``tied_positions_from_chains`` for homo-oligomers) and the two
probability modes ``unconditional_probs`` and ``conditional_probs`` with ``native_scores``.  Section 7.12 is the CA-only model
(``CA_ProteinFeatures``, ``ProteinMPNN(ca_only=True)`` of the reference): ``ProteinMPNN(ca_only=True)`` here reads only the CA trace, and
everything after the features - encoder, decoder, controls, ties, probability modes - is the same code.  No trained CA checkpoint was
available when this was built: parity is claimed against the reference's code with synthetic parameters.  Not built: tied groups with a
masked or fixed member (``tie_groups`` refuses them).

Two alphabets meet here.  ``S`` arrays, ``probs`` and ``log_probs`` are in the MODEL's alphabet ``ACDEFGHIKLMNPQRSTVWYX``, as in the
reference; ``aatype`` arrays are in this project's restype order (``output.RESTYPES``, 20 = unknown).  ``aatype_to_mpnn`` and
``mpnn_to_aatype`` convert.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from . import _call, _lib
from .output import RESTYPES

ALPHABET = "ACDEFGHIKLMNPQRSTVWYX"
VOCAB, HIDDEN, LAYERS = 21, 128, 3
EDGE_IN, EDGE_IN_CA = 416, 167   # the inputs of features.edge_embedding: 16 + 25 x 16, and 16 + 9 x 16 + 7 for the CA-only model
MAX_ROWS, MAX_SEQ, MAX_NEIGHBORS = _lib.MPNN_MAX_ROWS, _lib.MPNN_MAX_SEQ, _lib.MPNN_MAX_NEIGHBORS
MASKED_NEIGHBOR, NO_LETTER = _lib.MPNN_MASKED_NEIGHBOR, _lib.MPNN_NO_LETTER
_TO_MPNN = np.array([ALPHABET.index(c) for c in RESTYPES] + [20], dtype=np.int64)       # restype index -> model letter
_TO_AATYPE = np.array([(RESTYPES + "X").index(c) for c in ALPHABET], dtype=np.int64)    # model letter -> restype index


def aatype_to_mpnn(aatype):
    """Restype-order indices (0 .. 19, 20 = unknown) as letters of the model's alphabet."""
    a = np.asarray(aatype, dtype=np.int64)
    if a.size and (a.min() < 0 or a.max() > 20):
        raise ValueError("aatype outside 0 .. 20")
    return _TO_MPNN[a]


def mpnn_to_aatype(S):
    s = np.asarray(S, dtype=np.int64)
    if s.size and (s.min() < 0 or s.max() > 20):
        raise ValueError("letters outside 0 .. 20")
    return _TO_AATYPE[s]


def seq_to_mpnn(seq: str):
    """A one-letter string as model letters; anything outside the 20 standard letters is X."""
    return np.array([ALPHABET.index(c) if c in ALPHABET else 20 for c in seq], dtype=np.int64)


def mpnn_to_seq(S, mask=None) -> str:
    """The letters of the rows where ``mask`` is set (ProteinMPNN/protein_mpnn_utils.py:_S_to_seq)."""
    s = np.asarray(S, dtype=np.int64)
    keep = np.ones(s.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    return "".join(ALPHABET[int(c)] for c in s[keep])


# ------------------------------------------------------------------------------------------------ parameters
def _layer_shapes(prefix, w1_in, edge_update):
    out = OrderedDict()
    for n in ("norm1", "norm2") + (("norm3",) if edge_update else ()):
        out[f"{prefix}.{n}.weight"], out[f"{prefix}.{n}.bias"] = (HIDDEN,), (HIDDEN,)
    mats = [("W1", w1_in), ("W2", HIDDEN), ("W3", HIDDEN)] + ([("W11", w1_in), ("W12", HIDDEN), ("W13", HIDDEN)] if edge_update else [])
    for n, fan_in in mats:
        out[f"{prefix}.{n}.weight"], out[f"{prefix}.{n}.bias"] = (HIDDEN, fan_in), (HIDDEN,)
    out[f"{prefix}.dense.W_in.weight"], out[f"{prefix}.dense.W_in.bias"] = (4 * HIDDEN, HIDDEN), (4 * HIDDEN,)
    out[f"{prefix}.dense.W_out.weight"], out[f"{prefix}.dense.W_out.bias"] = (HIDDEN, 4 * HIDDEN), (HIDDEN,)
    return out


# the parameters of a CA-only state dict that the reference's forward never reads (departure c)
CA_UNREAD = ("features.node_embedding.weight", "features.norm_nodes.weight", "features.norm_nodes.bias", "W_v.weight", "W_v.bias")


def param_shapes(ca_only: bool = False) -> "OrderedDict[str, tuple]":
    """The reference's parameter names and shapes (hidden 128, 3 + 3 layers), in a fixed order: the vanilla model, or with ``ca_only``
    the CA-only one - 167 edge inputs and the five parameters of ``CA_UNREAD``."""
    s = OrderedDict()
    s["features.embeddings.linear.weight"], s["features.embeddings.linear.bias"] = (16, 66), (16,)
    if ca_only:
        s["features.node_embedding.weight"] = (HIDDEN, 3)
    s["features.edge_embedding.weight"] = (HIDDEN, EDGE_IN_CA if ca_only else EDGE_IN)
    if ca_only:
        s["features.norm_nodes.weight"], s["features.norm_nodes.bias"] = (HIDDEN,), (HIDDEN,)
    s["features.norm_edges.weight"], s["features.norm_edges.bias"] = (HIDDEN,), (HIDDEN,)
    if ca_only:
        s["W_v.weight"], s["W_v.bias"] = (HIDDEN, HIDDEN), (HIDDEN,)
    s["W_e.weight"], s["W_e.bias"] = (HIDDEN, HIDDEN), (HIDDEN,)
    s["W_s.weight"] = (VOCAB, HIDDEN)
    for l in range(LAYERS):
        s.update(_layer_shapes(f"encoder_layers.{l}", 3 * HIDDEN, True))
    for l in range(LAYERS):
        s.update(_layer_shapes(f"decoder_layers.{l}", 4 * HIDDEN, False))
    s["W_out.weight"], s["W_out.bias"] = (VOCAB, HIDDEN), (VOCAB,)
    return s


def synthetic_state_dict(seed: int, k: int = 48, ca_only: bool = False) -> "OrderedDict[str, np.ndarray]":
    """Synthetic float32 parameters under the reference's names from ``np.random.default_rng((seed, k))``, drawn in the order of
    ``param_shapes``: Xavier-uniform matrices (the reference's initialisation), biases uniform in +-0.1, LayerNorm gains 1 + 0.1 n and
    shifts 0.1 n - nothing is zero or one, so that a swapped gain, shift or bias shows.  ``k`` does not change a shape; it enters the
    stream so that models of different K differ.  ``ca_only``: the CA-only model from ``np.random.default_rng((seed, k, 1))`` in the
    order of ``param_shapes(ca_only=True)``, the five unread parameters included (the reference's strict ``load_state_dict`` wants them)."""
    rng = np.random.default_rng((int(seed), int(k), 1) if ca_only else (int(seed), int(k)))
    sd = OrderedDict()
    for name, shape in param_shapes(ca_only).items():
        if len(shape) == 2:
            bound = np.sqrt(6.0 / (shape[0] + shape[1]))
            v = rng.uniform(-bound, bound, size=shape)
        elif ".norm" in name and name.endswith(".weight"):
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif ".norm" in name:
            v = 0.1 * rng.standard_normal(shape)
        else:
            v = rng.uniform(-0.1, 0.1, size=shape)
        sd[name] = v.astype(np.float32)
    return sd


def _image_order():
    """(parameter name, transposed?) in the order of the weight image (the table in include/fdipt.h)."""
    order = [("features.embeddings.linear.weight", True), ("features.embeddings.linear.bias", False), ("features.edge_embedding.weight", True),
             ("features.norm_edges.weight", False), ("features.norm_edges.bias", False), ("W_e.weight", True), ("W_e.bias", False), ("W_s.weight", False)]

    def linear(p):
        return [(p + ".weight", True), (p + ".bias", False)]

    def norm(p):
        return [(p + ".weight", False), (p + ".bias", False)]

    for kind, edge in (("encoder_layers", True), ("decoder_layers", False)):
        for l in range(LAYERS):
            p = f"{kind}.{l}"
            order += linear(p + ".W1") + linear(p + ".W2") + linear(p + ".W3") + norm(p + ".norm1") + linear(p + ".dense.W_in") + linear(p + ".dense.W_out") + norm(p + ".norm2")
            if edge:
                order += linear(p + ".W11") + linear(p + ".W12") + linear(p + ".W13") + norm(p + ".norm3")
    return order + linear("W_out")


def is_ca_state_dict(sd) -> bool:
    """Does a state dict hold the CA-only model?  It is known by the 167 columns of ``features.edge_embedding.weight``."""
    w = sd.get("features.edge_embedding.weight") if hasattr(sd, "get") else None
    return w is not None and len(w.shape) == 2 and int(w.shape[1]) == EDGE_IN_CA


def pack_image(sd, ca_only=None) -> np.ndarray:
    """The packed float32 weight image of a state dict under the reference's names (tensors or arrays).  ``ca_only``: which model the
    dict must hold; None: whichever its ``features.edge_embedding.weight`` says (``is_ca_state_dict``).  The image of a CA-only model is
    the same table with 167 rows of edge_embedding; the five parameters its forward never reads may be present and are dropped."""
    ca_only = is_ca_state_dict(sd) if ca_only is None else bool(ca_only)
    what = "CA-only" if ca_only else "vanilla"
    shapes = param_shapes(ca_only)
    missing = [n for n in shapes if n not in sd and n not in CA_UNREAD]
    if missing:
        raise ValueError(f"state dict lacks {missing[:3]}{' ...' if len(missing) > 3 else ''} of the {what} model")
    parts = []
    for name, transposed in _image_order():
        v = sd[name]
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if tuple(v.shape) != shapes[name]:
            raise ValueError(f"{name}: shape {tuple(v.shape)}, the {what} model has {shapes[name]} (other widths are not built)")
        parts.append(np.ascontiguousarray(v.T if transposed else v, dtype=np.float32).reshape(-1))
    return np.concatenate(parts)


# ------------------------------------------------------------------------------------------------ host-side helpers
def decoding_order_from(randn, chain_mask):
    """``argsort((chain_mask + 0.0001) * |randn|)`` as the reference builds it: fixed rows first.  torch tensors, any leading shape."""
    import torch
    return torch.argsort((chain_mask + 0.0001) * torch.abs(randn), dim=-1)


def scores_of(log_probs, S, mask):
    """ProteinMPNN/protein_mpnn_utils.py:_scores: the mean negative log-probability of the letters over the rows of ``mask``."""
    lp = np.take_along_axis(np.asarray(log_probs), np.asarray(S)[..., None], axis=-1)[..., 0]
    mask = np.broadcast_to(np.asarray(mask, dtype=np.float32), lp.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (-(lp * mask).sum(-1) / mask.sum(-1)).astype(np.float32)


def native_scores(cond_log_probs, S, mask):
    """The mean negative conditional log-probability of the letters ``S`` over the rows of ``mask`` (``scores_of`` on the output of
    ``conditional_probs``): how well the backbone, with every other letter given, explains the letters of those rows."""
    return scores_of(cond_log_probs, S, mask)


def log_odds_mask(pssm_log_odds, pssm_threshold=0.0):
    """``pssm_log_odds > pssm_threshold`` as float32 (protein_mpnn_run.py:309): the letters the log-odds stage keeps at full weight."""
    return (np.asarray(pssm_log_odds, dtype=np.float32) > np.float32(pssm_threshold)).astype(np.float32)


def _is_seq(v):
    return isinstance(v, (list, tuple, np.ndarray))


def tie_groups(tied_positions, b, n, res_mask, chain_mask):
    """``tie_group`` [B,N] int32 (-1 = untied, else the group's index in its backbone's list) and the lists themselves, one per backbone.
    ``tied_positions``: None, a list of groups (lists of rows) for all backbones, or one such list per backbone.  ValueError, naming the
    row, for a member without res_mask or without chain_mask, a row in two groups, a group of one and an index out of range: the
    reference's behaviour there is an accident and nothing is built for it."""
    tie = np.full((b, n), -1, np.int32)
    if tied_positions is None:
        return tie, [[] for _ in range(b)]
    tp = list(tied_positions)
    if all(_is_seq(g) and all(_is_seq(e) for e in g) for g in tp) and (len(tp) == b or not tp):
        per = [[list(g) for g in one] for one in tp] if tp else [[] for _ in range(b)]
    elif all(_is_seq(g) and not any(_is_seq(e) for e in g) for g in tp):
        per = [[list(g) for g in tp] for _ in range(b)]
    else:
        raise ValueError(f"tied_positions: a list of groups of rows, or one such list for each of the {b} backbones")
    out = []
    for i, groups in enumerate(per):
        clean = []
        for gi, g in enumerate(groups):
            rows = []
            for r in g:
                if int(r) != r or not 0 <= int(r) < n:
                    raise ValueError(f"tied_positions: backbone {i}, group {gi}: row {r} outside 0 .. {n - 1}")
                r = int(r)
                if tie[i, r] >= 0 or r in rows:
                    raise ValueError(f"tied_positions: backbone {i}: row {r} is in two groups")
                if res_mask[i, r] == 0:
                    raise ValueError(f"tied_positions: backbone {i}, group {gi}: row {r} has no res_mask")
                if chain_mask[i, r] == 0:
                    raise ValueError(f"tied_positions: backbone {i}, group {gi}: row {r} is fixed (no chain_mask)")
                rows.append(r)
            if len(rows) < 2:
                raise ValueError(f"tied_positions: backbone {i}, group {gi}: a group of one (row {rows[0] if rows else None})")
            tie[i, rows] = gi
            clean.append(rows)
        out.append(clean)
    return tie, out


def flatten_decoding_order(order, groups):
    """The reference's ``new_decoding_order`` (tied_sample) for one drawn order [N]: walk it; a row not yet emitted emits its whole group
    in the group's listed order, an untied row emits itself."""
    member = {r: g for g in groups for r in g}
    seen, flat = set(), []
    for r in (int(v) for v in order):
        if r in seen:
            continue
        rows = member.get(r, [r])
        flat.extend(rows)
        seen.update(rows)
    return np.asarray(flat, dtype=np.int64)


def tied_positions_from_chains(chain_idx, res_mask=None):
    """The ties of a homo-oligomer: row r of every chain is one group (protein_mpnn_run.py's ``--homooligomer``).  chain_idx [N] or
    [B,N]; chains are the runs of rows with res_mask that share a chain_idx, in order of first appearance, and must have equal lengths.
    Returns one list of groups per backbone (for a 1-D chain_idx: the list of groups)."""
    ch = np.asarray(chain_idx)
    single = ch.ndim == 1
    ch = ch[None] if single else ch
    mask = np.ones(ch.shape, bool) if res_mask is None else np.asarray(res_mask).reshape(ch.shape) != 0
    out = []
    for i in range(ch.shape[0]):
        chains = OrderedDict()
        for r in np.flatnonzero(mask[i]):
            chains.setdefault(int(ch[i, r]), []).append(int(r))
        lengths = {len(v) for v in chains.values()}
        if len(lengths) > 1:
            raise ValueError(f"tied_positions_from_chains: backbone {i}: chains of lengths {sorted(len(v) for v in chains.values())}")
        out.append([list(g) for g in zip(*chains.values())] if len(chains) > 1 else [])
    return out[0] if single else out


def _fmt(x):
    return np.format_float_positional(np.float32(x), unique=False, precision=4)


def fasta_records(result: dict, b: int, name: str, model_name: str = "synthetic") -> str:
    """The reference's ``seqs/<name>.fa`` for backbone ``b`` of a ``design`` result (protein_mpnn_run.py:348, 367): the input sequence
    first, then one record per designed sequence with the four-decimal score, global_score and seq_recovery.  The first record's score
    fields are those of the input sequence where the result carries them (``native_score``, ``native_global_score``), NaN otherwise.
    The result of a CA-only model (``ca_only`` set) names its model as ``CA_model_name=``, as protein_mpnn_run.py:344-348 does."""
    chain = result["chain_mask"][b] * result["res_mask"][b]
    lines = [">{}, score={}, global_score={}, fixed_chains={}, designed_chains={}, {}={}, git_hash={}, seed={}".format(
        name, _fmt(result.get("native_score", np.full(len(result["S"]), np.nan))[b]),
        _fmt(result.get("native_global_score", np.full(len(result["S"]), np.nan))[b]), [], ["A"],
        "CA_model_name" if result.get("ca_only") else "model_name", model_name, "unknown", result["seed"]),
        mpnn_to_seq(result["S_input"][b], chain)]
    for m in range(result["S"].shape[1]):
        lines.append(">T={}, sample={}, score={}, global_score={}, seq_recovery={}".format(
            result["temperature"], m + 1, _fmt(result["score"][b, m]), _fmt(result["global_score"][b, m]), _fmt(result["seq_recovery"][b, m])))
        lines.append(mpnn_to_seq(result["S"][b, m], chain))
    return "\n".join(lines) + "\n"


class ProteinMPNN:
    """ProteinMPNN (hidden 128, 3 + 3 layers, vocabulary 21) with ``k_neighbors`` neighbours per row: the vanilla full-backbone model, or
    with ``ca_only`` the CA-only one, whose features read nothing but the CA trace."""

    def __init__(self, k_neighbors: int = 48, ca_only: bool = False):
        if not 1 <= int(k_neighbors) <= MAX_NEIGHBORS:
            raise ValueError(f"k_neighbors {k_neighbors} outside 1 .. {MAX_NEIGHBORS}")
        self.k_neighbors = int(k_neighbors)
        self.ca_only = bool(ca_only)
        self.noise_level = None
        self.source = None      # "synthetic(seed)" or the checkpoint's path
        self.image = None       # the packed float32 image (NumPy)
        self._device_image = {}

    def dims(self):
        return _lib.MpnnDims(hidden=HIDDEN, enc_layers=LAYERS, dec_layers=LAYERS, vocab=VOCAB, k_neighbors=self.k_neighbors, ca_only=int(self.ca_only))

    # ---- parameters
    def load_state_dict(self, sd):
        """A state dict under the reference's names.  A CA-only model is known by its 167-column ``features.edge_embedding.weight``;
        ValueError where that disagrees with the ``ca_only`` this object was built with."""
        if is_ca_state_dict(sd) != self.ca_only:
            raise ValueError("the state dict holds the {} model (features.edge_embedding.weight has {} columns) but this is ProteinMPNN(ca_only={})".format(
                "CA-only" if not self.ca_only else "vanilla full-backbone", int(sd["features.edge_embedding.weight"].shape[1])
                if "features.edge_embedding.weight" in sd else "no", self.ca_only))
        self.image = pack_image(sd, self.ca_only)
        self._device_image = {}
        return self

    def load_synthetic(self, seed: int = 0):
        self.source = f"synthetic({seed})"
        return self.load_state_dict(synthetic_state_dict(seed, self.k_neighbors, self.ca_only))

    def load_checkpoint(self, path):
        """A ``.pt`` file in the layout of protein_mpnn_run.py:160-168: ``model_state_dict``, ``num_edges`` (K), ``noise_level``."""
        import torch
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        k = int(ckpt["num_edges"])
        if not 1 <= k <= MAX_NEIGHBORS:
            raise ValueError(f"{path}: num_edges {k} outside 1 .. {MAX_NEIGHBORS}")
        self.k_neighbors, self.noise_level, self.source = k, ckpt.get("noise_level"), str(path)
        return self.load_state_dict(ckpt["model_state_dict"])

    def _weights_on(self, dev):
        import torch
        if self.image is None:
            raise _lib.FdiptError("ProteinMPNN has no parameters: load_state_dict, load_checkpoint or load_synthetic first")
        key = str(dev)
        if key not in self._device_image:
            self._device_image[key] = torch.from_numpy(self.image).to(dev)
        return self._device_image[key]

    # ---- inputs
    def _inputs(self, prot, res_mask, chain_mask, residue_index, chain_idx):
        shape = tuple(prot.shape)
        if self.ca_only and (len(shape) == 2 or (len(shape) == 3 and shape[1] not in (37, 5, 1))) and shape[-1] == 3:
            prot = prot[None, :, None] if len(shape) == 2 else prot[:, :, None]  # a CA trace [N,3] or [B,N,3] as [B,N,1,3]
        elif len(shape) == 3:
            prot = prot[None]
        b, n, _ = _call.structure_shape(prot, atoms=(37, 5, 1) if self.ca_only else (37, 5), items="backbones")
        if n > MAX_ROWS:
            raise ValueError(f"{n} rows: at most {MAX_ROWS}")
        if self.ca_only and n < 3:
            raise ValueError(f"{n} rows: the CA-only model needs at least 3")
        dev, (x,) = _call.upload("ProteinMPNN", prot=prot)

        def rows(v, what, kind, default=None):  # (on the host: the planning of orders, ties and scores reads them; one backbone's [N] serves B = 1)
            return _call.per_row(v[None] if v is not None and len(v.shape) == 1 else v, (b, n), what, kind, default)

        residue_index = rows(residue_index, "residue_index", "int")
        if residue_index is None:
            residue_index = np.tile(np.arange(n, dtype=np.int32), (b, 1))
        return (dev, x, b, n, rows(res_mask, "res_mask", "mask", 1), rows(chain_mask, "chain_mask", "mask", 1), residue_index,
                rows(chain_idx, "chain_idx", "int", 1))

    @staticmethod
    def _per_sequence(v, b, m, n, dtype, what):
        v = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
        if v.shape == (n,):
            v = v[None]
        if v.shape == (b, n):
            v = np.repeat(v[:, None], m, axis=1)
        if v.shape != (b, m, n):
            raise ValueError(f"{what} {v.shape} should be {(b, m, n)}")
        return np.ascontiguousarray(v, dtype=dtype)

    @staticmethod
    def _per_row(v, b, n, width, what):
        """An optional per-row input as float32 [B,N] (width None) or [B,N,width]; one backbone's array serves all."""
        if v is None:
            return None
        v = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32)
        tail = () if width is None else (width,)
        if v.shape == (n,) + tail:
            v = np.broadcast_to(v, (b, n) + tail)
        if v.shape != (b, n) + tail:
            raise ValueError(f"{what} {v.shape} should be {(b, n) + tail}")
        return np.array(v, dtype=np.float32, order="C")  # (a copy: a broadcast view is read-only)

    @staticmethod
    def _check_order(order, n):
        if not np.array_equal(np.sort(order, axis=-1), np.broadcast_to(np.arange(n), order.shape)):
            raise ValueError("decoding_order: every sequence needs a permutation of 0 .. N-1")

    def _run(self, design, dev, x, b, n, m, res_mask, chain_mask, residue_index, chain_idx, S, order, u=None, omit=None, bias=None, temperature=1.0,
             controls=None, pssm_multi=0.0, unconditional=False):
        """One call of fdipt_mpnn_design or fdipt_mpnn_score; NumPy outputs, the integer ones as int64.  ``controls``: the optional arrays of FdiptMpnnArgs by field
        name (None = absent).  ``unconditional``: the score entry's mode in which S and order are not read (pass None)."""
        import torch
        if m > MAX_SEQ:
            raise ValueError(f"{m} sequences per backbone: at most {MAX_SEQ}")
        inputs = {"res_mask": res_mask, "chain_mask": chain_mask, "residue_index": residue_index, "chain_idx": chain_idx,
                  "S": None if S is None else S.astype(np.int32), "decoding_order": None if order is None else order.astype(np.int32),
                  "u": u, "omit": omit, "bias": bias, **(controls or {})}
        inputs = {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inputs.items()}
        outputs = {"E_idx": ("int32", (b, n, min(self.k_neighbors, n))), "status": ("int32", (b,))}
        if design:
            outputs.update(S_out=("int32", (b, m, n)), probs=("float32", (b, m, n, VOCAB)))
        else:
            outputs["log_probs"] = ("float32", (b, m, n, VOCAB))
        return _call.run("fdipt_mpnn_design" if design else "fdipt_mpnn_score", _lib.MpnnArgs, dev,
                         dict(B=b, N=n, M=m, atoms=int(x.shape[2]), temperature=float(temperature), pssm_multi=float(pssm_multi),
                              unconditional=int(bool(unconditional))),
                         dict(weights=self._weights_on(dev), prot=x, **inputs), outputs, widen=("E_idx", "status", "S_out"),
                         workspace=("fdipt_mpnn_workspace", b, n, m), dims=self.dims())

    # ---- the two entry points
    def score(self, prot, S, res_mask=None, chain_mask=None, residue_index=None, chain_idx=None, decoding_order=None, seed=None) -> dict:
        """Teacher-forced log-probabilities (``forward(..., use_input_decoding_order=True)``).  prot [B,N,37|5,3] float32 (device tensor
        or NumPy; a single [N,..] backbone gains B = 1; a CA-only model reads atom 1 of either layout and also takes the CA trace alone
        as [B,N,3], [N,3] or [B,N,1,3] - a 3-D array whose middle extent is 37, 5 or 1 is one backbone [N,atoms,3]); S [B,N] or [B,M,N] model letters; decoding_order [B,M,N] / [B,N] or None: drawn
        as the reference draws it from ``torch.Generator().manual_seed(seed)``.  Returns ``log_probs`` [B,M,N,21] (0 in rows without
        res_mask), ``score`` and ``global_score`` [B,M], ``E_idx`` [B,N,K_eff], ``decoding_order``, ``status`` [B]."""
        import torch
        dev, x, b, n, res_mask, chain_mask, residue_index, chain_idx = self._inputs(prot, res_mask, chain_mask, residue_index, chain_idx)
        S = np.asarray(S.detach().cpu().numpy() if hasattr(S, "detach") else S)
        given = None if decoding_order is None else np.asarray(decoding_order.detach().cpu().numpy() if hasattr(decoding_order, "detach") else decoding_order)
        m = int(S.shape[1]) if S.ndim == 3 else int(given.shape[1]) if given is not None and given.ndim == 3 else 1
        S = self._per_sequence(S, b, m, n, np.int64, "S")
        if S.min() < 0 or S.max() >= VOCAB:
            raise ValueError("S: letters outside 0 .. 20")
        if decoding_order is None:
            gen = torch.Generator().manual_seed(0 if seed is None else int(seed))
            randn = torch.randn((b, m, n), generator=gen)
            decoding_order = decoding_order_from(randn, torch.from_numpy(chain_mask * res_mask)[:, None]).numpy()
        order = self._per_sequence(decoding_order, b, m, n, np.int64, "decoding_order")
        self._check_order(order, n)
        out = self._run(False, dev, x, b, n, m, res_mask, chain_mask, residue_index, chain_idx, S, order)
        return {"log_probs": out["log_probs"], "score": scores_of(out["log_probs"], S, (res_mask * chain_mask)[:, None]),
                "global_score": scores_of(out["log_probs"], S, res_mask[:, None]), "E_idx": out["E_idx"], "decoding_order": order,
                "status": out["status"]}

    def design(self, prot, num_seq: int = 8, temperature: float = 0.1, seed: int = 38, res_mask=None, chain_mask=None, aatype=None,
               residue_index=None, chain_idx=None, omit: str = "X", bias=None, decoding_order=None, u=None, bias_by_res=None, omit_mask=None,
               pssm_coef=None, pssm_bias=None, pssm_multi: float = 0.0, pssm_log_odds=None, pssm_threshold: float = 0.0, tied_positions=None,
               tied_beta=None) -> dict:
        """``num_seq`` sequences per backbone by the autoregressive loop of ``sample``, then the reference's rescoring of each.  Rows with
        chain_mask 0 are fixed to ``aatype`` (restype order; default: all unknown), rows without res_mask keep it too.  ``omit``: letters
        never drawn; ``bias``: a dict letter -> bias or 21 floats in the model's alphabet.  decoding_order and the uniforms u [B,M,N]
        come from ``torch.Generator().manual_seed(seed)`` (a normal draw, then a uniform draw) unless passed in.  A letter is the first
        one whose cumulative probability exceeds u * sum(p).  Returns ``S`` [B,M,N] model letters, ``aatype`` [B,M,N], ``sequences``
        (strings over the rows with res_mask), ``probs`` [B,M,N,21], ``log_probs``, ``decoding_order``, ``u``, ``score``,
        ``global_score``, ``seq_recovery`` [B,M] (NaN without aatype), ``E_idx``, ``status`` [B].

        Per-row controls (each [B,N,..] or [N,..] for all backbones, None = absent, and with none given every
        output keeps its bits): ``bias_by_res`` [.,N,21] joins the logits as bias / T; ``pssm_bias`` [.,N,21] with ``pssm_coef`` [.,N] and
        ``pssm_multi`` mixes a profile in; ``pssm_log_odds`` [.,N,21] keeps the letters above ``pssm_threshold`` at full weight and the
        others at 0.001 (needs ``pssm_coef`` too, as the C entry does); ``omit_mask`` [.,N,21] forbids letters per row.  A row left
        without a letter keeps its input letter, has probs 0 and sets ``NO_LETTER`` in its backbone's status.
        ``tied_positions`` (``tie_groups``; ``tied_positions_from_chains`` builds a homo-oligomer's) with ``tied_beta`` [.,N] (default 1):
        the rows of a group get one letter from the weighted sum of their logits, as ``tied_sample`` does; the controls and u of a group
        are read at its LAST listed member.  The result gains ``tie_group`` [B,N] and ``decoding_order`` is the flattened one (every
        group emitted whole at its first drawn member), which the rescoring uses too: it is teacher-forced, so the members of a group
        see each other's letters there and ``log_probs`` of tied rows do not agree with ``probs``."""
        import torch
        if not temperature > 0:
            raise ValueError("temperature must be positive")
        dev, x, b, n, res_mask, chain_mask, residue_index, chain_idx = self._inputs(prot, res_mask, chain_mask, residue_index, chain_idx)
        m = int(num_seq)
        if m < 1:
            raise ValueError("num_seq < 1")
        s_in = np.full((b, n), 20, np.int64) if aatype is None else aatype_to_mpnn(self._per_sequence(aatype, b, 1, n, np.int64, "aatype")[:, 0])
        omit_v = np.array([1.0 if c in omit else 0.0 for c in ALPHABET], dtype=np.float32)
        if omit_v.all():
            raise ValueError("omit leaves no letter")
        if isinstance(bias, dict):
            bias = [float(bias.get(c, 0.0)) for c in ALPHABET]
        bias_v = np.zeros(VOCAB, np.float32) if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        if bias_v.shape != (VOCAB,):
            raise ValueError("bias: 21 values in the model's alphabet, or a dict by letter")
        gen = torch.Generator().manual_seed(int(seed))
        randn = torch.randn((b, m, n), generator=gen)
        drawn_u = torch.rand((b, m, n), generator=gen, dtype=torch.float32).numpy()
        designed = chain_mask * res_mask
        if decoding_order is None:
            decoding_order = decoding_order_from(randn, torch.from_numpy(designed)[:, None]).numpy()
        order = self._per_sequence(decoding_order, b, m, n, np.int64, "decoding_order")
        self._check_order(order, n)
        u = self._per_sequence(drawn_u if u is None else u, b, m, n, np.float32, "u")
        if u.min() < 0 or u.max() >= 1:
            raise ValueError("u outside [0, 1)")
        S_in = self._per_sequence(s_in, b, m, n, np.int64, "aatype")
        controls = {"bias_by_res": self._per_row(bias_by_res, b, n, VOCAB, "bias_by_res"), "omit_mask": self._per_row(omit_mask, b, n, VOCAB, "omit_mask"),
                    "pssm_coef": self._per_row(pssm_coef, b, n, None, "pssm_coef"), "pssm_bias": self._per_row(pssm_bias, b, n, VOCAB, "pssm_bias"),
                    "pssm_log_odds_mask": None if pssm_log_odds is None else log_odds_mask(self._per_row(pssm_log_odds, b, n, VOCAB, "pssm_log_odds"), pssm_threshold)}
        if (controls["pssm_bias"] is not None or controls["pssm_log_odds_mask"] is not None) and controls["pssm_coef"] is None:
            raise ValueError("pssm_bias and pssm_log_odds need pssm_coef")
        tie_group, groups = tie_groups(tied_positions, b, n, res_mask, chain_mask)
        if tied_positions is not None:
            beta = self._per_row(tied_beta, b, n, None, "tied_beta")
            controls["tie_group"], controls["tied_beta"] = tie_group, np.ones((b, n), np.float32) if beta is None else beta
            order = np.stack([np.stack([flatten_decoding_order(order[i, j], groups[i]) for j in range(m)]) for i in range(b)])
        elif tied_beta is not None:
            raise ValueError("tied_beta without tied_positions")
        common = (dev, x, b, n, m, res_mask, chain_mask, residue_index, chain_idx)
        des = self._run(True, *common, S_in, order, u=u, omit=omit_v, bias=bias_v, temperature=temperature, controls=controls, pssm_multi=pssm_multi)
        S = des["S_out"]
        rescored = self._run(False, *common, S, order)
        with np.errstate(invalid="ignore", divide="ignore"):
            recovery = (((S == S_in) * designed[:, None]).sum(-1) / designed.sum(-1)[:, None]).astype(np.float32)
        if aatype is None:
            recovery = np.full((b, m), np.nan, np.float32)
        return {"S": S, "aatype": mpnn_to_aatype(S), "sequences": [[mpnn_to_seq(S[i, j], res_mask[i]) for j in range(m)] for i in range(b)],
                "probs": des["probs"], "log_probs": rescored["log_probs"], "decoding_order": order, "u": u,
                "score": scores_of(rescored["log_probs"], S, designed[:, None]), "global_score": scores_of(rescored["log_probs"], S, res_mask[:, None]),
                "seq_recovery": recovery, "E_idx": des["E_idx"], "status": des["status"] | rescored["status"],
                "S_input": s_in, "res_mask": res_mask, "chain_mask": chain_mask, "temperature": temperature, "seed": seed, "tie_group": tie_group.astype(np.int64),
                "ca_only": self.ca_only}

    def unconditional_probs(self, prot, res_mask=None, residue_index=None, chain_idx=None) -> dict:
        """``unconditional_probs`` of the reference: the decoder with no neighbour counted as decoded, what the backbone alone says.
        Returns ``log_probs`` [B,N,21] (0 in rows without res_mask), ``E_idx``, ``status`` [B]."""
        dev, x, b, n, res_mask, chain_mask, residue_index, chain_idx = self._inputs(prot, res_mask, None, residue_index, chain_idx)
        out = self._run(False, dev, x, b, n, 1, res_mask, chain_mask, residue_index, chain_idx, None, None, unconditional=True)
        return {"log_probs": out["log_probs"][:, 0], "E_idx": out["E_idx"], "status": out["status"]}

    def conditional_probs(self, prot, S, res_mask=None, chain_mask=None, residue_index=None, chain_idx=None, backbone_only: bool = False, seed=None,
                          randn=None) -> dict:
        """``conditional_probs`` of the reference.  For every row i with chain_mask and res_mask, row i of the teacher-forced
        log-probabilities of ``S`` [B,N] under the order ``argsort((onehot_i + 0.0001) * |randn|)``: i decoded last, every other letter
        given.  ``backbone_only``: ``argsort((1 - onehot_i + 0.0001) * |randn|)``, i decoded first, no letter given.  ``randn`` [B,N]:
        one normal draw per backbone, from ``torch.Generator().manual_seed(seed)`` (0 for None) unless passed in.  Built as host-side
        chunks of at most MAX_SEQ orders through ``fdipt_mpnn_score`` (each chunk runs the encoder again).
        Returns ``log_probs`` [B,N,21] (0 in every other row), the ``randn`` used, ``status`` [B]."""
        import torch
        dev, x, b, n, res_mask, chain_mask, residue_index, chain_idx = self._inputs(prot, res_mask, chain_mask, residue_index, chain_idx)
        S = self._per_sequence(S, b, 1, n, np.int64, "S")[:, 0]
        if S.min() < 0 or S.max() >= VOCAB:
            raise ValueError("S: letters outside 0 .. 20")
        if randn is None:
            randn = torch.randn((b, n), generator=torch.Generator().manual_seed(0 if seed is None else int(seed))).numpy()
        randn = np.asarray(randn.detach().cpu().numpy() if hasattr(randn, "detach") else randn, dtype=np.float32)
        randn = randn[None] if randn.ndim == 1 else randn
        if randn.shape != (b, n):
            raise ValueError(f"randn {randn.shape} should be {(b, n)}")
        rows = [np.flatnonzero(chain_mask[i] * res_mask[i]) for i in range(b)]
        out, status = np.zeros((b, n, VOCAB), np.float32), np.zeros((b,), np.int64)
        for start in range(0, max(len(r) for r in rows), MAX_SEQ):
            chunk = [r[start:start + MAX_SEQ] for r in rows]
            m = max(len(c) for c in chunk)
            order = np.tile(np.arange(n, dtype=np.int64), (b, m, 1))  # (sequences past a backbone's rows: any order; not read back)
            for i, c in enumerate(chunk):
                if len(c):
                    hot = torch.zeros((len(c), n))
                    hot[torch.arange(len(c)), torch.from_numpy(c)] = 1.0
                    order[i, :len(c)] = torch.argsort(((1.0 - hot if backbone_only else hot) + 0.0001) * torch.abs(torch.from_numpy(randn[i]))[None], dim=-1).numpy()
            res = self._run(False, dev, x, b, n, m, res_mask, chain_mask, residue_index, chain_idx, np.repeat(S[:, None], m, axis=1), order)
            status |= res["status"]
            for i, c in enumerate(chunk):
                out[i, c] = res["log_probs"][i, np.arange(len(c)), c]
        return {"log_probs": out, "randn": randn, "status": status}
