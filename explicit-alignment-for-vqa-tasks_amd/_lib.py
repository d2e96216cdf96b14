"""ctypes binding of libeavqa_hip.so, derived from the C ABI's own description.

include/eavqa.h and include/eavqa_test.h are read at import (``_abi``): every prototype becomes an ``argtypes`` list and a ``restype``,
every ``typedef struct`` a ``ctypes.Structure``, every enum member and ``#define``d integer a constant of this module under its header
name.  Nothing here repeats a declaration; the two places where the binding is not what the C type says are ``OVERRIDES``.  A header
construct the reader does not know is an error at import, never a guess.  ``tests/golden/abi_signatures.txt`` is the reviewed record of
the resulting table.

The product path has NO fallback: if the shared library is missing or a call returns an error code, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _abi
from .build import INCLUDE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libeavqa_hip.so")
HEADERS = ("eavqa.h", "eavqa_test.h")

# where the ctypes type is not the mapping of the C type (_abi.bind):
OVERRIDES = {
    "eavqa_clip_state_t*": C.c_void_p,                      # the state block lives in DEVICE memory: an address, not a host struct
    "eavqa_gemm_route.split_rows": C.POINTER(C.c_int),      # a HOST out-parameter, filled through byref(c_int())
}


def _read(name: str) -> _abi.Header:
    with open(os.path.join(INCLUDE, name)) as f:
        return _abi.parse(f.read(), name)


ABI = _abi.merge(_read(h) for h in HEADERS)
STRUCTS, SIGNATURES, RESTYPES, PARAMS = _abi.bind(ABI, OVERRIDES)      # SIGNATURES: name -> argtypes, PARAMS: name -> parameter names

CONSTANTS = ABI.constants
globals().update(CONSTANTS)                                 # EAVQA_F32, EAVQA_GEMM_OUT_F32, EAVQA_E_ARG, EAVQA_ABI_VERSION, ...
F32, BF16 = CONSTANTS["EAVQA_F32"], CONSTANTS["EAVQA_BF16"]
ACT = {n[len("EAVQA_ACT_"):].lower(): v for n, v in CONSTANTS.items() if n.startswith("EAVQA_ACT_")}

GemmLn, LMLayer, LMTail, LMLayerScales, T5DecLayer, DecodeGemm, ClipState, LaunchPlan = (
    STRUCTS[f"eavqa_{n}_t"] for n in ("gemm_ln", "lm_layer", "lm_tail", "lm_layer_scales", "t5_dec_layer", "decode_gemm", "clip_state", "launch_plan"))

_lib = None


class EavqaError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the library once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EavqaError(
            f"{LIB_PATH} is missing: the HIP extension is the only compute path. "
            "Build it with `python -m eavqa_amd.build` (needs hipcc, no GPU required to compile)."
        )
    # torch ships its own libamdhip64: it must be in the process before this library asks the loader for that SONAME,
    # otherwise the system runtime gets bound first and torch later runs on a HIP runtime it was not built against
    # (seen as hipGetDevice failing when build() and smoke() share one process)
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    got = lib.eavqa_abi_version()
    if got != CONSTANTS["EAVQA_ABI_VERSION"]:
        raise EavqaError(f"libeavqa_hip.so ABI version {got}, include/eavqa.h says {CONSTANTS['EAVQA_ABI_VERSION']}")
    _lib = lib
    return lib


def call(name: str, *args) -> None:
    """Invoke an int-returning entry point and raise on a non-zero code."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise EavqaError(f"{name} failed: {lib.eavqa_strerror(rc).decode()} (code {rc})")
