"""ctypes binding of ``libfdipt_hip.so``, derived from its C ABI in ``include/fdipt.h``.

The structs, the signature of every entry point and the integer constants below are read from the header at import
(``framedipt_amd/_header.py``): the header is their one source.  The product path has no CPU fallback: every arithmetic entry point goes
through this library and raises if it is missing or if a kernel reports an error.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# FDIPT_LIB: another build of the library (csrc/build.sh with FDIPT_VARIANT, e.g. the bf16 one: lib/libfdipt_hip_bf16.so)
LIB_PATH = os.environ.get("FDIPT_LIB") or os.path.join(_HERE, "lib", "libfdipt_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fdipt.h")


class FdiptError(RuntimeError):
    pass


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise FdiptError(f"{HEADER_PATH} not found: the binding of libfdipt_hip.so is derived from this header and needs it beside the package")
    with open(HEADER_PATH) as f:
        return _header.parse(f.read())


_H = _read_header()
# every FDIPT_<NAME> integer macro as <NAME>: PREC_*, KF_* (FdiptDims.kernel_flags), SELECT_* and EVAL_* (limits and status bits),
# VIOLATION_CONSTANTS, DSSP_* (class codes, the bridge slots of a row, status bits), TM_* and TMA_* (the row limits, status bits), SEARCH_* (the
# largest top_k, status bits, the ranking), MPNN_* (limits,
# status bits), LDDT_* (atom sets, tile sizes, status bits), GDT_* (modes, the number of cutoffs, status bits), MAP_* (the coverage switch and the status bits of a row map), SEQ_* (sequence alignment: limits, status bits, modes, free-end bits), IFACE_* (interface accuracy: atom sets, sides, limits, tile sizes, flags, status bits), the E* return codes
globals().update(_H.macros)
_ERR = {_H.macros["EINVAL"]: "FDIPT_EINVAL (bad argument)", _H.macros["ELAUNCH"]: "FDIPT_ELAUNCH (HIP launch error)",
        _H.macros["ESIZE"]: "FDIPT_ESIZE (workspace too small or N beyond the compiled tiling: N <= 1024, N <= 2048 with KF_STREAM_ATTN in the fp16 mode; "
                            "sample selection: a group of more than 64 samples; inverse folding: N > 2048 or more than 64 sequences; sequence alignment: a length > 2048; interface accuracy: N > 2048 or more than 64 interfaces)"}

Dims, ForwardArgs, ReverseIndexed, SelectArgs, EvalArgs, ViolationArgs, DsspArgs, SasaArgs, TmArgs, TmAlignArgs, SearchArgs, MpnnDims, MpnnArgs, LddtArgs, GdtArgs, RowMap, SeqAlignArgs, SeqAlignModeArgs, InterfaceArgs = (
    _H.structs["Fdipt" + n] for n in ("Dims", "ForwardArgs", "ReverseIndexed", "SelectArgs", "EvalArgs", "ViolationArgs", "DsspArgs", "SasaArgs", "TmArgs",
                                      "TmAlignArgs", "SearchArgs", "MpnnDims", "MpnnArgs", "LddtArgs", "GdtArgs", "RowMap", "SeqAlignArgs", "SeqAlignModeArgs", "InterfaceArgs"))
for _cls, _doc in ((ReverseIndexed, "one reverse step addressed through a device-side step cursor."),
                   (SelectArgs, "sample selection over G groups of the B samples of one atom37 array."),
                   (EvalArgs, "evaluation of B samples against R ground-truth structures."),
                   (ViolationArgs, "structural violations of B samples."),
                   (DsspArgs, "secondary structure (coil / helix / strand) of B samples."),
                   (SasaArgs, "solvent accessibility (Shrake-Rupley ASA, RSA) of B samples."),
                   (TmArgs, "TM-score of P pairs of structures under the row-by-row correspondence."),
                   (TmAlignArgs, "structural alignment search (TM-align style) for P pairs of structures."),
                   (SearchArgs, "novelty search: the top-k entries of a packed structure set per query, by the alignment search."),
                   (MpnnDims, "the sizes of the inverse-folding model (ProteinMPNN)."),
                   (MpnnArgs, "inverse folding: scoring or design of M sequences for each of B backbones."),
                   (LddtArgs, "superposition-free accuracy (lDDT, dRMSD, backbone FAPE) of P ordered pairs of structures."),
                   (GdtArgs, "GDT-TS / GDT-HA of P pairs of structures: no, one global or a searched superposition per cutoff."),
                   (RowMap, "the row map of the mapped accuracy entries: the model row of every reference row, per pair."),
                   (SeqAlignArgs, "global sequence alignment with affine gaps (Gotoh) of P pairs of sequences."),
                   (SeqAlignModeArgs, "sequence alignment with a mode (global, semi-global with free end gaps, local) of P pairs of sequences."),
                   (InterfaceArgs, "interface accuracy (contacts, fnat, iRMSD, LRMSD, DockQ) of P pairs of structures on I interfaces.")):
    _cls.__doc__ = f"Fdipt{_cls.__name__} (include/fdipt.h): {_doc}"

_lib = None

# name -> (restype, argtypes); every symbol declared in include/fdipt.h
SIGNATURES = {name: (res, args) for name, (res, args, _) in _H.functions.items()}


def load():
    """Load the shared library (once) and bind every declared symbol; raises if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FdiptError(
            f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or framedipt_amd/csrc/build.sh).  There is no CPU fallback for the sampler hot path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise FdiptError(f"libfdipt_hip: {what} failed with {_ERR.get(rc, rc)}")


def ptr(t):
    """Device (or host) pointer of a contiguous torch tensor / None."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise FdiptError("non-contiguous tensor passed to the C ABI")
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(t, what: str):
    if not t.is_cuda:
        raise FdiptError(f"{what}: tensors must live on the MI355X (got device {t.device}); no CPU fallback exists")
