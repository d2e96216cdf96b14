"""CPU: the ctypes bindings ``_lib`` derives from include/eavqa.h and include/eavqa_test.h.

Four things are held here, none of which needs the built library or a GPU: the derived table equals the hand-kept table of the commit
before it (tests/golden/abi_signatures.txt, from then on the reviewed record of the ABI); one signature per mapping rule, written out
by hand; what the header reader accepts and what it refuses; and the struct layouts against the C compiler's, which also keeps the
two headers valid C99."""
import ctypes as C
import importlib.util
import os
import subprocess

import pytest

from eavqa_amd import _abi, _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

i32, i64, u64, f32, ptr = C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_void_p


def test_the_derived_table_is_the_recorded_one():
    spec = importlib.util.spec_from_file_location("make_golden_abi", os.path.join(GOLDEN, "make_golden_abi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "abi_signatures.txt")) as f:
        want = f.read()
    got = gen.describe(_lib.SIGNATURES, _lib.RESTYPES, _lib.PARAMS)
    assert got.splitlines() == want.splitlines()
    assert got == want


_GEMM = [i32] * 6 + [ptr, i64] * 3 + [i32, f32, ptr, i32, ptr, ptr, i64, ptr, i64]

# one entry per mapping rule, written from the prototypes by hand: (restype, argtypes)
PINNED = {
    "eavqa_gemm": (i32, _GEMM + [ptr]),                                                     # int / int64_t / float / pointer mix
    "eavqa_sample_pick": (i32, [i32, i32, ptr, i64, f32, i32, f32, u64, u64, ptr, ptr, i64, i64, ptr, ptr, i64, ptr, ptr, ptr, i64, ptr, ptr]),
    "eavqa_gemm_ln": (i32, _GEMM + [C.POINTER(_lib.GemmLn), ptr]),                          # a host struct by pointer
    "eavqa_gemm_decode": (i32, [C.POINTER(_lib.DecodeGemm), ptr]),
    "eavqa_adamw_clipped": (i32, [i64, ptr, ptr, ptr, ptr, f32, f32, f32, f32, f32, ptr, i32, ptr, ptr]),   # the device struct: an address
    "eavqa_gemm_route": (i32, [i32] * 8 + [C.POINTER(C.c_int)]),                            # the host out-parameter
    "eavqa_gemm_splitk_route": (i32, [i32] * 6 + [C.POINTER(_lib.LaunchPlan)]),             # the host out-struct of the decode plans
    "eavqa_gemm_decode_route": (i32, [i32] * 6 + [C.POINTER(_lib.LaunchPlan)]),
    "eavqa_attention_decode_route": (i32, [i32] * 5 + [C.POINTER(_lib.LaunchPlan)]),
    "eavqa_strerror": (C.c_char_p, [i32]),
    "eavqa_t5_decoder_step_workspace_bytes": (i64, [i32] * 6),
    "eavqa_abi_version": (i32, []),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_one_signature_per_mapping_rule(name):
    restype, argtypes = PINNED[name]
    assert _lib.RESTYPES[name] is restype
    assert len(_lib.SIGNATURES[name]) == len(argtypes) == len(_lib.PARAMS[name])
    for got, want, param in zip(_lib.SIGNATURES[name], argtypes, _lib.PARAMS[name]):
        assert got is want, param


def test_names_constants_and_structs():
    assert _lib.PARAMS["eavqa_gemm_route"] == ("dtype", "a_kc", "b_kc", "M", "N", "K", "has_ln", "knobs", "split_rows")
    assert _lib.PARAMS["eavqa_abi_version"] == ()
    assert (_lib.F32, _lib.BF16, _lib.EAVQA_F16, _lib.EAVQA_E_ARCH, _lib.EAVQA_ABI_VERSION) == (0, 1, 2, -6, 1)
    assert (_lib.EAVQA_GEMM_OUT_F32, _lib.EAVQA_GEMM_RESIDUAL_LOWP, _lib.EAVQA_GEMM_STREAM_F16) == (1, 2, 4)
    assert _lib.ACT == {"none": 0, "tanh": 1, "relu": 2, "gelu_new": 3, "quick_gelu": 4}
    assert _lib.DecodeGemm._fields_[:4] == [("M", i32), ("N", i32), ("K", i32), ("A", ptr)]
    assert dict(_lib.DecodeGemm._fields_)["out"] is ptr * 3 and dict(_lib.DecodeGemm._fields_)["ld_out"] is i64 * 3
    assert _lib.LMLayerScales._fields_ == [(n, f32) for n in ("s_qkv", "s_o", "s_fc1", "s_fc2")]
    assert [n for n, _ in _lib.ClipState._fields_] == ["norm", "scale_eff", "inv_bc1", "inv_sqrt_bc2", "applied_steps", "skipped_steps", "skip",
                                                       "reserved"]
    from eavqa_amd import ops
    assert ops.CLIP_STATE_WORDS == 8 and ops.F16 == 2 and ops.ENSEMBLE_MODES == {"product": 0, "mixture": 1}


# ---- the reader on synthetic snippets

def _bind(text, overrides={}):
    return _abi.bind(_abi.parse(text, "snippet.h"), overrides)


def test_the_reader_accepts_the_subset_the_headers_use():
    h = _abi.parse('''
        /* a comment with int bogus(double x); inside
           over two lines */
        #ifndef EAVQA_X_H
        #define EAVQA_X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #pragma GCC visibility push(default)
        #define EAVQA_VERSION 3     // trailing comment
        #define EAVQA_MASK 0x10
        enum { EAVQA_A = 0, EAVQA_B = -2,
               EAVQA_C = 7 };   /* comment */
        typedef struct {
            const float* g; void* out[3]; int64_t ld_out[3];
            int M, N;
            float s_a, s_b; uint64_t seed; int32_t n;
        } eavqa_thing_t;
        typedef struct { void* k; void* v; } eavqa_pair_t;
        int eavqa_none(void);
        const char* eavqa_name(int code);
        int64_t eavqa_bytes(int rows, int64_t ld);
        int eavqa_run(const eavqa_thing_t* t, eavqa_pair_t* pairs, const int32_t* idx, const uint8_t *bytes, double* acc,
                      uint64_t seed, float eps, int32_t n, void* stream);
        #ifdef __cplusplus
        }
        #endif
        #endif
    ''', "snippet.h")
    assert h.constants == {"EAVQA_VERSION": 3, "EAVQA_MASK": 16, "EAVQA_A": 0, "EAVQA_B": -2, "EAVQA_C": 7}
    assert list(h.structs) == ["eavqa_thing_t", "eavqa_pair_t"] and list(h.functions) == ["eavqa_none", "eavqa_name", "eavqa_bytes", "eavqa_run"]
    b = _abi.bind(h, {})
    thing, pair = b.structs["eavqa_thing_t"], b.structs["eavqa_pair_t"]
    assert thing._fields_ == [("g", ptr), ("out", ptr * 3), ("ld_out", i64 * 3), ("M", i32), ("N", i32), ("s_a", f32), ("s_b", f32),
                              ("seed", u64), ("n", i32)]
    assert pair._fields_ == [("k", ptr), ("v", ptr)]
    assert b.argtypes == {"eavqa_none": [], "eavqa_name": [i32], "eavqa_bytes": [i32, i64],
                          "eavqa_run": [C.POINTER(thing), C.POINTER(pair), ptr, ptr, ptr, u64, f32, i32, ptr]}
    assert b.restypes == {"eavqa_none": i32, "eavqa_name": C.c_char_p, "eavqa_bytes": i64, "eavqa_run": i32}
    assert b.params["eavqa_run"] == ("t", "pairs", "idx", "bytes", "acc", "seed", "eps", "n", "stream") and b.params["eavqa_none"] == ()


def test_overrides_replace_single_results_and_must_name_something_declared():
    text = "typedef struct { float norm; } eavqa_state_t;\nint eavqa_f(eavqa_state_t* state, int* rows);\nint eavqa_g(const eavqa_state_t* s, int* rows);"
    b = _bind(text, {"eavqa_state_t*": ptr, "eavqa_f.rows": C.POINTER(i32)})
    assert b.argtypes == {"eavqa_f": [ptr, C.POINTER(i32)], "eavqa_g": [ptr, ptr]}
    with pytest.raises(_abi.AbiError, match="eavqa_f.cols"):
        _bind(text, {"eavqa_f.cols": ptr})


REJECTED = [
    ("double", "int eavqa_f(double x);", "double x"),
    ("unsigned", "int eavqa_f(unsigned n);", "unsigned n"),
    ("unsigned_int", "int eavqa_f(unsigned int n);", "unsigned int n"),
    ("size_t", "int eavqa_f(size_t n);", "size_t n"),
    ("function_pointer", "int eavqa_f(void (*cb)(int), void* stream);", "(*cb)"),
    ("union", "typedef union { int a; float b; } eavqa_u_t;", "union"),
    ("nested_struct", "typedef struct { int a; struct { int b; } in; } eavqa_s_t;", "struct { int b; }"),
    ("by_value_struct_field", "typedef struct { int a; } eavqa_a_t;\ntypedef struct { eavqa_a_t a; } eavqa_b_t;", "eavqa_a_t a"),
    ("by_value_struct_parameter", "typedef struct { int a; } eavqa_a_t;\nint eavqa_f(eavqa_a_t a);", "eavqa_a_t a"),
    ("enum_member_without_a_value", "enum { EAVQA_A = 0, EAVQA_B };", "EAVQA_B"),
    ("enum_member_of_another_name", "enum { EAVQA_A = 0, load = 1 };", "load = 1"),
    ("named_enum", "enum eavqa_e { EAVQA_A = 0 };", "enum eavqa_e"),
    ("variadic", "int eavqa_f(int n, ...);", "..."),
    ("unnamed_parameter", "int eavqa_f(int, float x);", "'int'"),
    ("empty_parameter_list", "int eavqa_f();", "eavqa_f()"),
    ("array_parameter", "int eavqa_f(int n[3]);", "n[3]"),
    ("pointer_to_pointer", "int eavqa_f(void** p);", "void** p"),
    ("double_field", "typedef struct { double x; } eavqa_s_t;", "double x"),
    ("bit_field", "typedef struct { int x : 3; } eavqa_s_t;", "int x : 3"),
    ("void_return", "void eavqa_f(int n);", "void eavqa_f"),
    ("float_return", "float eavqa_f(int n);", "float eavqa_f"),
    ("function_body", "int eavqa_f(int n) { return n; }", "eavqa_f(int n)"),
    ("static_inline", "static inline int eavqa_f(int n);", "static inline"),
    ("foreign_name", "int other_f(int n);", "other_f"),
    ("continued_define", "#define EAVQA_X \\\n 3", "EAVQA_X"),
    ("unknown_struct_pointer", "int eavqa_f(const eavqa_missing_t* p);", None),
]


@pytest.mark.parametrize("text,quoted", [r[1:] for r in REJECTED], ids=[r[0] for r in REJECTED])
def test_the_reader_refuses_everything_else(text, quoted):
    """... with a message that names the header and carries the offending text; nothing is skipped."""
    good = "int eavqa_before(int n);\n", "\nint eavqa_after(int n);"
    with pytest.raises(_abi.AbiError) as e:
        _bind(good[0] + text + good[1])
    if quoted is None:
        assert "eavqa_missing_t" in str(e.value)
    else:
        assert str(e.value).startswith("snippet.h: ") and quoted in str(e.value), str(e.value)


def test_a_name_declared_in_both_headers_is_an_error():
    one = _abi.parse("int eavqa_f(int n);", "a.h")
    with pytest.raises(_abi.AbiError, match="eavqa_f"):
        _abi.merge([one, _abi.parse("int eavqa_f(int64_t n);", "b.h")])


# ---- struct layouts against the compiler

def _clang():
    """The toolchain's own clang, found from hipcc the way ``build._hipcc`` finds hipcc."""
    from eavqa_amd import build
    hipcc = os.path.realpath(build._hipcc())
    rocm = os.path.dirname(os.path.dirname(hipcc))
    for exe in (os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang"),
                os.path.join(os.path.dirname(hipcc), "amdclang")):
        if os.path.exists(exe):
            return exe
    raise RuntimeError(f"no clang beside {hipcc}: the library could not have been built either")


def test_struct_layouts_equal_the_compilers(tmp_path):
    """A stand-alone C99 host program prints sizeof and every offsetof of the eight structs; ctypes has to agree.  Compiling it with
    -Wall -pedantic -Werror is also what keeps both headers plain C, as their file comments promise."""
    structs = _lib.STRUCTS
    assert len(structs) == 8
    body = []
    for name, cls in structs.items():
        body.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        body += [f'    printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "eavqa.h"\n#include "eavqa_test.h"\n\nint main(void) {\n'
                   + "\n".join(body) + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    from eavqa_amd import build
    r = subprocess.run([_clang(), "-std=c99", "-Wall", "-pedantic", "-Werror", f"-I{build.INCLUDE}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    want = {}
    for name, cls in structs.items():
        want[name] = C.sizeof(cls)
        want.update({f"{name}.{f}": getattr(cls, f).offset for f, _ in cls._fields_})
    assert got == want
    assert (want["eavqa_decode_gemm_t"], want["eavqa_decode_gemm_t.out"], want["eavqa_decode_gemm_t.stats_out"]) == (200, 144, 192)
    assert want["eavqa_gemm_ln_t"] == 88 and want["eavqa_clip_state_t"] == 32
    assert (want["eavqa_launch_plan_t"], want["eavqa_launch_plan_t.grid_x"], want["eavqa_launch_plan_t.lds_bytes"]) == (32, 16, 28)
