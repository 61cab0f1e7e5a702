"""Inverse folding on the device: ProteinMPNN scoring and sequence design for sampled backbones.

The reference's first step after sampling (experiments/inference.py:run_self_consistency -> run_protein_mpnn) is a subprocess of
ProteinMPNN/protein_mpnn_run.py per sample directory.  Here the vanilla full-backbone model (ProteinMPNN/protein_mpnn_utils.py:
ProteinFeatures, EncLayer, DecLayer, ProteinMPNN.forward and .sample) runs on the device through ``fdipt_mpnn_score`` and
``fdipt_mpnn_design`` (csrc/mpnn.hip, ABI in include/fdipt.h); DESIGN.md section 7.10 is the contract.  Inference only, float32;
``ca_only``, tied positions, PSSM, ``omit_AA_mask`` and ``bias_by_res`` are not built.

Two alphabets meet here.  ``S`` arrays, ``probs`` and ``log_probs`` are in the MODEL's alphabet ``ACDEFGHIKLMNPQRSTVWYX``, as in the
reference; ``aatype`` arrays are in this project's restype order (``output.RESTYPES``, 20 = unknown).  ``aatype_to_mpnn`` and
``mpnn_to_aatype`` convert.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict

import numpy as np

from . import _lib
from .output import RESTYPES

ALPHABET = "ACDEFGHIKLMNPQRSTVWYX"
VOCAB, HIDDEN, LAYERS = 21, 128, 3
MAX_ROWS, MAX_SEQ, MAX_NEIGHBORS = _lib.MPNN_MAX_ROWS, _lib.MPNN_MAX_SEQ, _lib.MPNN_MAX_NEIGHBORS
MASKED_NEIGHBOR = _lib.MPNN_MASKED_NEIGHBOR
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


def param_shapes() -> "OrderedDict[str, tuple]":
    """The reference's parameter names and shapes (vanilla model: hidden 128, 3 + 3 layers), in a fixed order."""
    s = OrderedDict()
    s["features.embeddings.linear.weight"], s["features.embeddings.linear.bias"] = (16, 66), (16,)
    s["features.edge_embedding.weight"] = (HIDDEN, 416)
    s["features.norm_edges.weight"], s["features.norm_edges.bias"] = (HIDDEN,), (HIDDEN,)
    s["W_e.weight"], s["W_e.bias"] = (HIDDEN, HIDDEN), (HIDDEN,)
    s["W_s.weight"] = (VOCAB, HIDDEN)
    for l in range(LAYERS):
        s.update(_layer_shapes(f"encoder_layers.{l}", 3 * HIDDEN, True))
    for l in range(LAYERS):
        s.update(_layer_shapes(f"decoder_layers.{l}", 4 * HIDDEN, False))
    s["W_out.weight"], s["W_out.bias"] = (VOCAB, HIDDEN), (VOCAB,)
    return s


def synthetic_state_dict(seed: int, k: int = 48) -> "OrderedDict[str, np.ndarray]":
    """Synthetic float32 parameters under the reference's names from ``np.random.default_rng((seed, k))``, drawn in the order of
    ``param_shapes``: Xavier-uniform matrices (the reference's initialisation), biases uniform in +-0.1, LayerNorm gains 1 + 0.1 n and
    shifts 0.1 n - nothing is zero or one, so that a swapped gain, shift or bias shows.  ``k`` does not change a shape; it enters the
    stream so that models of different K differ."""
    rng = np.random.default_rng((int(seed), int(k)))
    sd = OrderedDict()
    for name, shape in param_shapes().items():
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


def pack_image(sd) -> np.ndarray:
    """The packed float32 weight image of a state dict under the reference's names (tensors or arrays)."""
    shapes = param_shapes()
    missing = [n for n in shapes if n not in sd]
    if missing:
        raise ValueError(f"state dict lacks {missing[:3]}{' ...' if len(missing) > 3 else ''}: the vanilla full-backbone model is the one built")
    parts = []
    for name, transposed in _image_order():
        v = sd[name]
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if tuple(v.shape) != shapes[name]:
            raise ValueError(f"{name}: shape {tuple(v.shape)}, the vanilla model has {shapes[name]} (ca_only and other widths are not built)")
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


def _fmt(x):
    return np.format_float_positional(np.float32(x), unique=False, precision=4)


def fasta_records(result: dict, b: int, name: str, model_name: str = "synthetic") -> str:
    """The reference's ``seqs/<name>.fa`` for backbone ``b`` of a ``design`` result (protein_mpnn_run.py:348, 367): the input sequence
    first, then one record per designed sequence with the four-decimal score, global_score and seq_recovery.  The first record's score
    fields are those of the input sequence where the result carries them (``native_score``, ``native_global_score``), NaN otherwise."""
    chain = result["chain_mask"][b] * result["res_mask"][b]
    lines = [">{}, score={}, global_score={}, fixed_chains={}, designed_chains={}, model_name={}, git_hash={}, seed={}".format(
        name, _fmt(result.get("native_score", np.full(len(result["S"]), np.nan))[b]),
        _fmt(result.get("native_global_score", np.full(len(result["S"]), np.nan))[b]), [], ["A"], model_name, "unknown", result["seed"]),
        mpnn_to_seq(result["S_input"][b], chain)]
    for m in range(result["S"].shape[1]):
        lines.append(">T={}, sample={}, score={}, global_score={}, seq_recovery={}".format(
            result["temperature"], m + 1, _fmt(result["score"][b, m]), _fmt(result["global_score"][b, m]), _fmt(result["seq_recovery"][b, m])))
        lines.append(mpnn_to_seq(result["S"][b, m], chain))
    return "\n".join(lines) + "\n"


class ProteinMPNN:
    """The vanilla ProteinMPNN (hidden 128, 3 + 3 layers, vocabulary 21) with ``k_neighbors`` neighbours per row."""

    def __init__(self, k_neighbors: int = 48):
        if not 1 <= int(k_neighbors) <= MAX_NEIGHBORS:
            raise ValueError(f"k_neighbors {k_neighbors} outside 1 .. {MAX_NEIGHBORS}")
        self.k_neighbors = int(k_neighbors)
        self.noise_level = None
        self.source = None      # "synthetic(seed)" or the checkpoint's path
        self.image = None       # the packed float32 image (NumPy)
        self._device_image = {}

    def dims(self):
        return _lib.MpnnDims(hidden=HIDDEN, enc_layers=LAYERS, dec_layers=LAYERS, vocab=VOCAB, k_neighbors=self.k_neighbors)

    # ---- parameters
    def load_state_dict(self, sd):
        self.image = pack_image(sd)
        self._device_image = {}
        return self

    def load_synthetic(self, seed: int = 0):
        self.source = f"synthetic({seed})"
        return self.load_state_dict(synthetic_state_dict(seed, self.k_neighbors))

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
    @staticmethod
    def _inputs(prot, res_mask, chain_mask, residue_index, chain_idx):
        import torch
        if len(prot.shape) == 3:
            prot = prot[None]
        if len(prot.shape) != 4 or tuple(prot.shape[2:]) not in ((37, 3), (5, 3)):
            raise ValueError(f"prot should be [B, N, 37, 3] or [B, N, 5, 3], got {tuple(prot.shape)}")
        b, n = int(prot.shape[0]), int(prot.shape[1])
        if b < 1 or n < 1:
            raise ValueError(f"prot {tuple(prot.shape)}: no backbones or no residues")
        if n > MAX_ROWS:
            raise ValueError(f"{n} rows: at most {MAX_ROWS}")
        if torch.is_tensor(prot):
            _lib.require_cuda(prot, "ProteinMPNN")
            if prot.dtype != torch.float32:
                raise ValueError(f"prot should be float32, got {prot.dtype}")
            dev, x = prot.device, prot.contiguous()
        else:
            dev = torch.device("cuda", torch.cuda.current_device())
            x = torch.from_numpy(np.ascontiguousarray(prot, dtype=np.float32)).to(dev)

        def rows(v, default, dtype, what):
            if v is None:
                return default
            v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            v = v[None] if v.ndim == 1 else v
            if v.shape != (b, n):
                raise ValueError(f"{what} {v.shape} should be {(b, n)}")
            return np.ascontiguousarray(v, dtype=dtype)

        res_mask = (rows(res_mask, np.ones((b, n), np.float32), np.float32, "res_mask") != 0).astype(np.float32)
        chain_mask = (rows(chain_mask, np.ones((b, n), np.float32), np.float32, "chain_mask") != 0).astype(np.float32)
        residue_index = rows(residue_index, np.tile(np.arange(n, dtype=np.int32), (b, 1)), np.int32, "residue_index")
        chain_idx = rows(chain_idx, np.ones((b, n), np.int32), np.int32, "chain_idx")
        return dev, x, b, n, res_mask, chain_mask, residue_index, chain_idx

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
    def _check_order(order, n):
        if not np.array_equal(np.sort(order, axis=-1), np.broadcast_to(np.arange(n), order.shape)):
            raise ValueError("decoding_order: every sequence needs a permutation of 0 .. N-1")

    def _run(self, design, dev, x, b, n, m, res_mask, chain_mask, residue_index, chain_idx, S, order, u=None, omit=None, bias=None, temperature=1.0):
        """One call of fdipt_mpnn_design or fdipt_mpnn_score; NumPy outputs."""
        import torch
        lib = _lib.load()
        if m > MAX_SEQ:
            raise ValueError(f"{m} sequences per backbone: at most {MAX_SEQ}")
        with torch.cuda.device(dev):
            dims, k_eff = self.dims(), min(self.k_neighbors, n)

            def up(v):
                return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dev)

            t = {k: up(v) for k, v in (("res_mask", res_mask), ("chain_mask", chain_mask), ("residue_index", residue_index), ("chain_idx", chain_idx),
                                       ("S", S.astype(np.int32)), ("decoding_order", order.astype(np.int32)), ("u", u), ("omit", omit), ("bias", bias))}
            out = {"E_idx": torch.zeros((b, n, k_eff), dtype=torch.int32, device=dev), "status": torch.zeros((b,), dtype=torch.int32, device=dev)}
            if design:
                out["S_out"] = torch.zeros((b, m, n), dtype=torch.int32, device=dev)
                out["probs"] = torch.zeros((b, m, n, VOCAB), dtype=torch.float32, device=dev)
            else:
                out["log_probs"] = torch.zeros((b, m, n, VOCAB), dtype=torch.float32, device=dev)
            nbytes = int(lib.fdipt_mpnn_workspace(C.byref(dims), b, n, m))
            work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            p = _lib.ptr
            args = _lib.MpnnArgs(B=b, N=n, M=m, atoms=int(x.shape[2]), weights=p(self._weights_on(dev)), prot=p(x), temperature=float(temperature),
                                 workspace=p(work), workspace_bytes=nbytes, **{k: p(v) for k, v in t.items()}, **{k: p(v) for k, v in out.items()})
            fn = lib.fdipt_mpnn_design if design else lib.fdipt_mpnn_score
            _lib.check(fn(C.byref(dims), C.byref(args), _lib.stream_ptr()), "fdipt_mpnn_design" if design else "fdipt_mpnn_score")
            return {k: v.cpu().numpy() for k, v in out.items()}

    # ---- the two entry points
    def score(self, prot, S, res_mask=None, chain_mask=None, residue_index=None, chain_idx=None, decoding_order=None, seed=None) -> dict:
        """Teacher-forced log-probabilities (``forward(..., use_input_decoding_order=True)``).  prot [B,N,37|5,3] float32 (device tensor
        or NumPy; a single [N,..] backbone gains B = 1); S [B,N] or [B,M,N] model letters; decoding_order [B,M,N] / [B,N] or None: drawn
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
                "global_score": scores_of(out["log_probs"], S, res_mask[:, None]), "E_idx": out["E_idx"].astype(np.int64), "decoding_order": order,
                "status": out["status"].astype(np.int64)}

    def design(self, prot, num_seq: int = 8, temperature: float = 0.1, seed: int = 38, res_mask=None, chain_mask=None, aatype=None,
               residue_index=None, chain_idx=None, omit: str = "X", bias=None, decoding_order=None, u=None) -> dict:
        """``num_seq`` sequences per backbone by the autoregressive loop of ``sample``, then the reference's rescoring of each.  Rows with
        chain_mask 0 are fixed to ``aatype`` (restype order; default: all unknown), rows without res_mask keep it too.  ``omit``: letters
        never drawn; ``bias``: a dict letter -> bias or 21 floats in the model's alphabet.  decoding_order and the uniforms u [B,M,N]
        come from ``torch.Generator().manual_seed(seed)`` (a normal draw, then a uniform draw) unless passed in.  A letter is the first
        one whose cumulative probability exceeds u * sum(p).  Returns ``S`` [B,M,N] model letters, ``aatype`` [B,M,N], ``sequences``
        (strings over the rows with res_mask), ``probs`` [B,M,N,21], ``log_probs``, ``decoding_order``, ``u``, ``score``,
        ``global_score``, ``seq_recovery`` [B,M] (NaN without aatype), ``E_idx``, ``status`` [B]."""
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
        common = (dev, x, b, n, m, res_mask, chain_mask, residue_index, chain_idx)
        des = self._run(True, *common, S_in, order, u=u, omit=omit_v, bias=bias_v, temperature=temperature)
        S = des["S_out"].astype(np.int64)
        rescored = self._run(False, *common, S, order)
        with np.errstate(invalid="ignore", divide="ignore"):
            recovery = (((S == S_in) * designed[:, None]).sum(-1) / designed.sum(-1)[:, None]).astype(np.float32)
        if aatype is None:
            recovery = np.full((b, m), np.nan, np.float32)
        return {"S": S, "aatype": mpnn_to_aatype(S), "sequences": [[mpnn_to_seq(S[i, j], res_mask[i]) for j in range(m)] for i in range(b)],
                "probs": des["probs"], "log_probs": rescored["log_probs"], "decoding_order": order, "u": u,
                "score": scores_of(rescored["log_probs"], S, designed[:, None]), "global_score": scores_of(rescored["log_probs"], S, res_mask[:, None]),
                "seq_recovery": recovery, "E_idx": des["E_idx"].astype(np.int64), "status": (des["status"] | rescored["status"]).astype(np.int64),
                "S_input": s_in, "res_mask": res_mask, "chain_mask": chain_mask, "temperature": temperature, "seed": seed}
