"""Generates tests/golden/abi_signatures.txt: the ctypes form of the C ABI, one line per entry point -
``restype name(ctype parameter, ...)`` with ctypes class names, ``POINTER(eavqa_x_t)`` for a host struct - followed by one block per
struct that some entry point takes by pointer, field by field.

The file was first written from the hand-kept ``SIGNATURES`` / ``_RESTYPES`` / ``_fields_`` tables of the commit BEFORE ``_lib`` derived
its bindings from the headers, so that the derived table is held to the hand one object for object:

    git show <that commit>:explicit-alignment-for-vqa-tasks_amd/_lib.py > /tmp/hand_lib.py
    python tests/golden/make_golden_abi.py --hand /tmp/hand_lib.py

The hand table knew no parameter names; they come from the headers in both modes (the C compiler holds them to the definitions).  After
a change of a prototype or struct, regenerate from the headers and review the diff, which shows the C types that moved:

    python tests/golden/make_golden_abi.py"""
import ctypes as C
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DST = os.path.join(HERE, "abi_signatures.txt")

# the Python class names of the hand table's struct mirrors
HAND_STRUCTS = {"GemmLn": "eavqa_gemm_ln_t", "LMLayer": "eavqa_lm_layer_t", "LMTail": "eavqa_lm_tail_t", "LMLayerScales": "eavqa_lm_layer_scales_t",
                "T5DecLayer": "eavqa_t5_dec_layer_t", "DecodeGemm": "eavqa_decode_gemm_t"}


FIXED_WIDTH = {C.c_int64: "c_int64", C.c_uint64: "c_uint64"}      # ctypes aliases them to c_long / c_ulong where long has 64 bits


def describe(signatures, restypes, params, struct_name=lambda cls: cls.__name__):
    """The text of the file.  ``signatures``: name -> argtypes, ``restypes``: name -> restype, ``params``: name -> parameter names,
    ``struct_name``: Structure subclass -> its typedef's name."""
    structs = {}

    def show(t):
        if issubclass(t, C.Array):
            return f"{show(t._type_)}[{t._length_}]"
        if issubclass(t, C._Pointer):
            if issubclass(t._type_, C.Structure):
                structs[struct_name(t._type_)] = t._type_
                return f"POINTER({struct_name(t._type_)})"
            return f"POINTER({show(t._type_)})"
        return FIXED_WIDTH.get(t, t.__name__)

    lines = []
    for name in sorted(signatures):
        assert len(signatures[name]) == len(params[name]), name
        lines.append(f"{show(restypes[name])} {name}({', '.join(f'{show(t)} {p}' for t, p in zip(signatures[name], params[name]))})")
    for name in sorted(structs):
        lines += ["", f"struct {name}"] + [f"    {show(t)} {field}" for field, t in structs[name]._fields_]
    return "\n".join(lines) + "\n"


def from_headers():
    sys.path.insert(0, ROOT)
    from eavqa_amd import _lib
    return describe(_lib.SIGNATURES, _lib.RESTYPES, _lib.PARAMS)


def from_hand_table(path):
    sys.path.insert(0, ROOT)
    from eavqa_amd import _lib
    spec = importlib.util.spec_from_file_location("hand_lib", path)
    hand = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hand)
    restypes = {name: hand._RESTYPES.get(name, C.c_int) for name in hand.SIGNATURES}
    return describe(hand.SIGNATURES, restypes, _lib.PARAMS, lambda cls: HAND_STRUCTS[cls.__name__])


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--hand":
        text = from_hand_table(sys.argv[2])
    elif len(sys.argv) == 1:
        text = from_headers()
    else:
        sys.exit(__doc__)
    with open(DST, "w") as f:
        f.write(text)
    print(f"{DST}: {text.count(chr(10))} lines")
