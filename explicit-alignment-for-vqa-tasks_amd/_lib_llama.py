"""ctypes binding of libeavqa_llama_hip.so (include/eavqa_llama.h): the Llama family's kernels and layer driver.

Derived from the header the way ``_lib`` derives the first library's: every prototype becomes an ``argtypes`` list and a ``restype``.
The header is read on top of include/eavqa.h (whose conventions and codes it shares), and only what it declares itself is bound
here.  No fallback: a missing library or a non-zero return code raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _abi, _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libeavqa_llama_hip.so")
HEADER = "eavqa_llama.h"

_OWN = _lib._read(HEADER)
_BOUND = _abi.bind(_abi.merge([_lib.ABI, _OWN]), _lib.OVERRIDES)
STRUCTS = {n: _BOUND.structs[n] for n in _OWN.structs}
LlamaLayer = STRUCTS["eavqa_llama_layer_t"]
SIGNATURES = {n: _BOUND.argtypes[n] for n in _OWN.functions}
RESTYPES = {n: _BOUND.restypes[n] for n in _OWN.functions}
PARAMS = {n: _BOUND.params[n] for n in _OWN.functions}

_lib_llama = None


def load() -> C.CDLL:
    """Load the library once (after libeavqa_hip.so, which it links against); raise when it is absent."""
    global _lib_llama
    if _lib_llama is not None:
        return _lib_llama
    _lib.load()
    if not os.path.exists(LIB_PATH):
        raise _lib.EavqaError(f"{LIB_PATH} is missing: the Llama family has no other compute path.  Build it with `python -m eavqa_amd.build`.")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    _lib_llama = lib
    return lib


def call(name: str, *args) -> None:
    """Invoke an int-returning entry point and raise on a non-zero code."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise _lib.EavqaError(f"{name} failed: {_lib.load().eavqa_strerror(rc).decode()} (code {rc})")
