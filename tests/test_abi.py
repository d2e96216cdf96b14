"""CPU: the C-ABI library builds, loads, and exports exactly what include/eavqa.h (the drop-in boundary) and
include/eavqa_test.h (test-only kernel selectors) declare.
No compute call is made here (there is no GPU in the build container)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(headers=("eavqa.h", "eavqa_test.h")):
    out = set()
    for h in headers:
        text = open(os.path.join(ROOT, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        out |= set(re.findall(r"\b(eavqa_[a-z0-9_]+)\s*\(", text))
    return sorted(out)


@pytest.fixture(scope="module")
def lib():
    from eavqa_amd import build, _lib
    build.build()
    return _lib.load()


def test_header_declares_the_expected_surface():
    syms = declared_symbols()
    assert "eavqa_gemm" in syms and "eavqa_attention_fwd" in syms and len(syms) >= 20
    public = declared_symbols(("eavqa.h",))
    # the drop-in boundary carries no test hooks and no process-global switches
    assert not [n for n in public if "debug" in n or n.endswith("_ex")]
    assert set(declared_symbols(("eavqa_test.h",))) - set(public) == {"eavqa_gemm_ex", "eavqa_gemm_ln_ex", "eavqa_gemm_route", "eavqa_attention_fwd_ex", "eavqa_attention_bwd_ex",
                                                                                "eavqa_gemm_splitk_ex",
                                                                                "eavqa_gemm_decode_ex", "eavqa_t5_decoder_step_ex",
                                                                                "eavqa_gemm_splitk_route", "eavqa_gemm_decode_route",
                                                                                "eavqa_attention_decode_route"}


def test_every_declared_symbol_is_exported_and_bound(lib):
    from eavqa_amd import _lib
    for name in declared_symbols():
        assert hasattr(lib, name), f"{name} declared in eavqa.h but not exported"
    # the bindings are derived from the headers (tests/test_abi_bindings_cpu.py); this name scan is a second, independent reading of them
    assert sorted(_lib.SIGNATURES) == declared_symbols()


def test_the_dynamic_symbol_table_is_exactly_the_two_headers():
    """Hidden visibility + csrc/exports.map: no C++ symbol, kernel handle or toolchain bookkeeping symbol leaves the library."""
    import subprocess
    from eavqa_amd import build
    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == declared_symbols()


def test_library_exports_no_mutable_global_switches(lib):
    """`no global mutable state` (include/eavqa.h conventions): the round-1 eavqa_debug_* setters are gone."""
    for name in ("eavqa_debug_disable_fast_gemm", "eavqa_debug_gemm_stagger", "eavqa_debug_attention_valu"):
        assert not hasattr(lib, name), name


def test_abi_version_and_strerror(lib):
    assert lib.eavqa_abi_version() == 1
    assert lib.eavqa_strerror(0) == b"ok"
    assert b"aligned" in lib.eavqa_strerror(-2)
    assert b"unknown" in lib.eavqa_strerror(-99)


def test_argument_validation_happens_before_any_launch(lib):
    """Bad arguments are rejected on the host (no GPU needed): null pointers, bad dtype, bad shapes."""
    assert lib.eavqa_gemm(1, 1, 1, 8, 8, 8, None, 8, None, 8, None, 8, 0, 1.0, None, 0, None, None, 0, None, 0, None) == -1
    assert lib.eavqa_gemm(7, 1, 1, 8, 8, 8, 16, 8, 16, 8, 16, 8, 0, 1.0, None, 0, None, None, 0, None, 0, None) == -4
    assert lib.eavqa_gemm(1, 1, 1, 8, 8, 12, 16, 16, 16, 16, 16, 8, 0, 1.0, None, 0, None, None, 0, None, 0, None) == -3
    assert lib.eavqa_gemm(1, 1, 1, 8, 8, 8, 18, 8, 16, 8, 16, 8, 0, 1.0, None, 0, None, None, 0, None, 0, None) == -2
    assert lib.eavqa_layernorm_fwd(0, 1, 4, 6, 16, 8, None, None, 1e-5, 16, 8, None, None, None) == -3
    assert lib.eavqa_attention_fwd(0, 1, 1, 4, 4, 6, 16, 8, 16, 8, 16, 8, 16, 8, 0, 0, None, 0, None, 0, 1.0, None, None) == -3
    assert lib.eavqa_adamw(0, None, None, None, None, 1, 0.1, 0.9, 0.999, 1e-8, 0.01, 1.0, 0, None, None) == -1


def _positional(entry, values, alias={}):
    """The positional arguments of ``entry`` in the order of its prototype (``_lib.PARAMS``, read from the header): ``values`` by parameter
    name, or by the shorter name ``alias`` gives a parameter in these tests."""
    from eavqa_amd import _lib
    return [values[alias.get(p, p)] for p in _lib.PARAMS[entry]]


_ATTN_ALIAS = {"cu_seqlens": "cu", "qkv_partials": "part", "partials": "part", "qkv_bias": "bias", "k_cache": "k", "v_cache": "v"}
_BLOCK_ALIAS = {"key_mask": "mask", "enc_mask": "mask", "workspace": "ws", "workspace_bytes": "ws_bytes"}


def _attn_call(lib, name, **over):
    """One attention entry point on a small valid problem (16 stands for an aligned pointer, 18 for a misaligned one; dtype 1 = bf16)
    with the named arguments replaced: the one fault of the call."""
    a = dict(dtype=1, B=1, H=1, Sq=4, Sk=4, hd=8, q=16, ldq=8, k=16, ldk=8, v=16, ldv=8, o=16, ldo=8, d_o=16, lddo=8, dq=16, lddq=8,
             dk=16, lddk=8, dv=16, lddv=8, q_batch_rows=0, kv_batch_rows=0, key_mask=None, ld_mask=0, cu=None, causal=0, scale=1.0,
             lse=16, delta=16, stream=None, k_new=16, v_new=16, ld_new=8, part=16, ks=1, bias=None, part_cols=8, rel_bias=None, rel_ld=0,
             rel_zero=0, path=0)
    assert not set(over) - set(a), over
    a.update(over)
    return getattr(lib, "eavqa_attention_" + name)(*_positional("eavqa_attention_" + name, a, _ATTN_ALIAS))


# (entry point, the one fault, error code): -1 ARG, -2 ALIGN, -3 SHAPE, -4 DTYPE.  The codes are the ones the library returned before the
# attention host layer was folded into one validation and two dispatchers; a change here is a change of the C ABI's behaviour.
ATTENTION_REJECTIONS = [
    ("fwd", dict(q=None), -1),
    ("fwd", dict(dtype=7), -4),
    ("fwd", dict(hd=6), -3),
    ("fwd", dict(B=256, H=256), -3),
    ("fwd", dict(ldq=6), -2),
    ("fwd", dict(cu=16, key_mask=16), -1),
    ("fwd", dict(cu=16, Sk=8), -1),
    ("fwd", dict(key_mask=16, ld_mask=2), -1),
    ("fwd", dict(q_batch_rows=2), -1),
    ("fwd", dict(kv_batch_rows=2), -1),
    ("fwd", dict(Sq=0), -1),
    ("fwd", dict(dtype=7, hd=6, ldq=6), -4),            # dtype before shape before leading dimensions
    ("fwd", dict(hd=6, ldq=6), -3),
    ("fwd", dict(ldq=6, q_batch_rows=2), -2),
    ("fwd_ex", dict(o=None), -1),
    ("fwd_ex", dict(dtype=7), -4),
    ("fwd_ex", dict(ldo=6), -2),
    ("fwd_ex", dict(cu=16, key_mask=16), -1),
    ("decode", dict(k_new=None), -1),
    ("decode", dict(v_new=None), -1),
    ("decode", dict(ld_new=4), -2),
    ("decode", dict(k_new=18), -2),
    ("decode", dict(dtype=0), -3),                      # fp32: the append form outside the decode kernel
    ("decode", dict(q=18), -3),                         # a misaligned q misses the decode kernel too
    ("decode", dict(hd=12, ldq=12, ldk=12, ldv=12, ldo=12), -3),
    ("decode", dict(dtype=7), -4),
    ("decode", dict(k_new=None, dtype=7), -1),          # the entry's own checks come first
    ("decode", dict(kv_batch_rows=2), -1),
    ("decode_splitk", dict(ks=0), -1),
    ("decode_splitk", dict(part=None), -1),
    ("decode_splitk", dict(part=18), -2),
    ("decode_splitk", dict(bias=18), -2),
    ("decode_splitk", dict(dtype=0), -3),
    ("decode_splitk", dict(k=None), -1),
    ("decode_splitk", dict(ldk=6), -2),
    ("decode_splitk_rel", dict(part_cols=16), -3),      # 2 H hd
    ("decode_splitk_rel", dict(rel_bias=16, rel_zero=2, rel_ld=8), -1),     # rel_zero = Sk - 2
    ("decode_splitk_rel", dict(rel_bias=16, rel_zero=3, rel_ld=3), -1),
    ("decode_splitk_rel", dict(rel_bias=16, rel_zero=2, rel_ld=8, dtype=7), -1),
    ("decode_splitk_rel", dict(part_cols=16, part=18), -3),
    ("decode_splitk_rel", dict(part=18), -2),
    ("decode_splitk_rel", dict(dtype=7), -4),
    ("decode_splitk_rel", dict(dtype=0), -3),
    ("fwd_rel", dict(rel_bias=16, rel_zero=3, rel_ld=6), -1),               # rel_ld = rel_zero + Sk - 1
    ("fwd_rel", dict(rel_bias=16, rel_zero=2, rel_ld=8), -1),
    ("fwd_rel", dict(rel_bias=16, rel_zero=3, rel_ld=6, ldq=6), -2),        # leading dimensions before the table span
    ("fwd_rel", dict(rel_bias=16, rel_zero=3, rel_ld=6, dtype=7), -4),
    ("fwd_rel", dict(v=None), -1),
    ("fwd_rel", dict(dtype=7), -4),
    ("fwd_rel", dict(hd=6), -3),
    ("fwd_rel", dict(ldv=6), -2),
    ("fwd_rel", dict(key_mask=16, ld_mask=2), -1),
    ("fwd_rel", dict(q_batch_rows=2), -1),
    ("bwd", dict(delta=None), -1),
    ("bwd", dict(lddq=6), -2),
    ("bwd", dict(dtype=7), -4),
    ("bwd", dict(hd=6), -3),
    ("bwd", dict(cu=16, key_mask=16), -1),
    ("bwd", dict(cu=16, Sk=8), -1),
    ("bwd", dict(lddq=6, cu=16, key_mask=16), -2),
    ("bwd_ex", dict(lse=None), -1),
    ("bwd_ex", dict(lddv=6), -2),
    ("bwd_ex", dict(B=256, H=256), -3),
    ("bwd_rel", dict(dk=None), -1),
    ("bwd_rel", dict(rel_bias=16, rel_zero=3, rel_ld=6), -1),
    ("bwd_rel", dict(rel_bias=16, rel_zero=3, rel_ld=6, lddk=6), -2),
    ("bwd_rel", dict(dtype=7), -4),
    ("bwd_rel", dict(hd=6), -3),
    ("bwd_rel", dict(lddo=6), -2),
]


@pytest.mark.parametrize("name,fault,code", ATTENTION_REJECTIONS, ids=[f"{n}-{'-'.join(f'{k}_{v}' for k, v in f.items())}" for n, f, _ in ATTENTION_REJECTIONS])
def test_attention_rejections_are_pinned(lib, name, fault, code):
    """Every attention entry point rejects a faulty call on the host, with the same code as ever (no GPU needed)."""
    assert _attn_call(lib, name, **fault) == code


def _gemm_call(lib, name, **over):
    """One GEMM-family entry point on a small valid problem (16 stands for an aligned pointer; dtype 1 = bf16) with the named arguments
    replaced: the fault(s) of the call.  `ln` is None (a null eavqa_gemm_ln_t*) or a dict of the struct's fields (all null by default)."""
    from eavqa_amd import _lib
    import ctypes as C
    a = dict(dtype=1, a_kc=1, b_kc=1, M=8, N=8, K=128, A=16, lda=128, B=16, ldb=128, C=16, ldc=8, out_flags=0, alpha=1.0, bias=None, act=0,
             aux_in=None, aux_out=None, ld_aux=8, residual=None, ldr=8, ln={}, stream=None, knobs=0, next_weight=None, next_weight_bytes=0,
             a_row_scale=16, b_scale=1.0, out_f32=0, tile=0, rows=8, cols=8, x=16, ldx=8, out=16, ld_out=8, row_scale=16)
    assert not set(over) - set(a), over
    a.update(over)
    a["ln"] = None if a["ln"] is None else C.byref(_lib.GemmLn(**a["ln"]))
    return getattr(lib, "eavqa_" + name)(*_positional("eavqa_" + name, a))


_LN_CONSUMER = dict(ln_stats=16, ln_parts=2, ln_ld=2, ln_cols=128, ln_c=16, ln_eps=1e-5)

# (entry point, the fault(s), error code): -1 ARG, -2 ALIGN, -3 SHAPE, -4 DTYPE.  The codes are the ones the library returned before the GEMM
# host layer became one call struct, one validation and one route function (recorded from that library); a change here is a change of the
# C ABI's behaviour.  Calls with two faults pin the ORDER of the checks.
GEMM_REJECTIONS = [
    ("gemm", dict(A=None), -1),
    ("gemm", dict(B=None), -1),
    ("gemm", dict(C=None), -1),
    ("gemm", dict(M=0), -1),
    ("gemm", dict(N=-1), -1),
    ("gemm", dict(K=0), -1),
    ("gemm", dict(dtype=7), -4),
    ("gemm", dict(dtype=2), -4),                        # half is a storage type only
    ("gemm", dict(act=5), -4),
    ("gemm", dict(act=-1), -4),
    ("gemm", dict(out_flags=8), -1),
    ("gemm", dict(dtype=0, out_flags=2), -4),           # 16-bit streams: bf16 operands only
    ("gemm", dict(dtype=0, out_flags=4), -4),
    ("gemm", dict(K=132), -3),
    ("gemm", dict(dtype=0, K=130), -3),
    ("gemm", dict(a_kc=0, M=12), -3),
    ("gemm", dict(b_kc=0, N=12, ldc=16), -3),
    ("gemm", dict(lda=132), -2),
    ("gemm", dict(ldb=132), -2),
    ("gemm", dict(A=18), -2),
    ("gemm", dict(B=24), -2),
    ("gemm", dict(lda=64), -1),
    ("gemm", dict(ldb=64), -1),
    ("gemm", dict(ldc=4), -1),
    ("gemm", dict(aux_out=16, ld_aux=4), -1),
    ("gemm", dict(aux_in=16, ld_aux=4), -1),
    ("gemm", dict(residual=16, ldr=4), -1),
    ("gemm", dict(A=None, dtype=7), -1),                # null pointers before the dtype
    ("gemm", dict(out_flags=8, A=None, B=None), -1),
    ("gemm", dict(out_flags=8, dtype=7), -1),           # the flags before everything but the eavqa_gemm_ln block
    ("gemm", dict(dtype=0, out_flags=2, A=None), -4),
    ("gemm", dict(M=0, dtype=7), -1),
    ("gemm", dict(dtype=7, K=132), -4),                 # dtype before shape
    ("gemm", dict(act=9, K=132), -4),
    ("gemm", dict(K=132, A=18), -3),                    # shape before alignment
    ("gemm", dict(lda=68), -2),                         # alignment before the leading dimensions' lower bounds
    ("gemm", dict(A=18, ldc=4), -2),
    ("gemm", dict(ldc=4, aux_out=16, ld_aux=4, residual=16, ldr=4), -1),
    ("gemm_ex", dict(A=None), -1),
    ("gemm_ex", dict(dtype=7), -4),
    ("gemm_ex", dict(K=132), -3),
    ("gemm_ex", dict(lda=132), -2),
    ("gemm_ex", dict(dtype=7, knobs=2 << 14), -4),
    ("gemm_ln", dict(ln=None), -1),
    ("gemm_ln", dict(ln=dict(copy_out=16, ld_copy=4)), -1),
    ("gemm_ln", dict(A=None), -1),
    ("gemm_ln", dict(dtype=7), -4),
    ("gemm_ln", dict(a_kc=0), -3),                      # the eavqa_gemm_ln form exists for k-contiguous operands
    ("gemm_ln_ex", dict(ln=None), -1),
    ("gemm_ln_ex", dict(ln=None, dtype=7), -1),         # the entry's own check comes first
    ("gemm_ln_ex", dict(ln=dict(copy_out=16, ld_copy=4)), -1),
    ("gemm_ln_ex", dict(ln=dict(stats_out=16, stats_ld=0)), -1),
    ("gemm_ln_ex", dict(N=72, ldc=72, ln=dict(stats_out=16, stats_ld=1)), -1),
    ("gemm_ln_ex", dict(ln=dict(_LN_CONSUMER, ln_c=None)), -1),
    ("gemm_ln_ex", dict(ln=dict(_LN_CONSUMER, ln_parts=0)), -1),
    ("gemm_ln_ex", dict(ln=dict(_LN_CONSUMER, ln_ld=1)), -1),
    ("gemm_ln_ex", dict(ln=dict(_LN_CONSUMER, ln_cols=0)), -1),
    ("gemm_ln_ex", dict(ln=dict(_LN_CONSUMER, ln_eps=-1.0)), -1),
    ("gemm_ln_ex", dict(ln=dict(_LN_CONSUMER, ln_eps=float("nan"))), -1),
    ("gemm_ln_ex", dict(ln=dict(_LN_CONSUMER, mean_out=16)), -1),
    ("gemm_ln_ex", dict(ln=dict(_LN_CONSUMER, rstd_out=16)), -1),
    ("gemm_ln_ex", dict(ln=dict(mean_out=16, rstd_out=16)), -1),            # the row statistics exist on the consumer side only
    ("gemm_ln_ex", dict(a_kc=0), -3),
    ("gemm_ln_ex", dict(b_kc=0), -3),
    ("gemm_ln_ex", dict(dtype=0, a_kc=0, M=6), -3),
    ("gemm_ln_ex", dict(ln=dict(copy_out=16, ld_copy=4), dtype=7), -1),     # the eavqa_gemm_ln block before everything else
    ("gemm_ln_ex", dict(ln=dict(copy_out=16, ld_copy=4), a_kc=0), -1),
    ("gemm_ln_ex", dict(a_kc=0, A=None), -3),
    ("gemm_ln_ex", dict(a_kc=0, out_flags=8), -3),
    ("gemm_ln_ex", dict(a_kc=0, dtype=7), -3),
    ("gemm_ln_ex", dict(ln=dict(copy_out=16, ld_copy=8), knobs=2 << 8), -3),    # a knob-only full-line tile has no eavqa_gemm_ln form
    ("gemm_ln_ex", dict(ln=dict(stats_out=16, stats_ld=1), knobs=10 << 8), -3),
    ("gemm_pf", dict(next_weight_bytes=-1), -1),
    ("gemm_pf", dict(next_weight_bytes=-1, dtype=7), -1),
    ("gemm_pf", dict(next_weight=16, next_weight_bytes=256, dtype=7), -4),
    ("gemm_pf", dict(A=None), -1),
    ("gemm_pf", dict(K=132), -3),
    ("gemm_pf", dict(B=24), -2),
    ("gemm_fp8", dict(A=None), -1),
    ("gemm_fp8", dict(B=None), -1),
    ("gemm_fp8", dict(C=None), -1),
    ("gemm_fp8", dict(a_row_scale=None), -1),
    ("gemm_fp8", dict(M=0), -1),
    ("gemm_fp8", dict(N=0), -1),
    ("gemm_fp8", dict(K=-128), -1),
    ("gemm_fp8", dict(act=5), -4),
    ("gemm_fp8", dict(K=64), -3),
    ("gemm_fp8", dict(lda=136), -2),
    ("gemm_fp8", dict(ldb=136), -2),
    ("gemm_fp8", dict(A=18), -2),
    ("gemm_fp8", dict(B=24), -2),
    ("gemm_fp8", dict(lda=64), -1),
    ("gemm_fp8", dict(ldb=64), -1),
    ("gemm_fp8", dict(ldc=4), -1),
    ("gemm_fp8", dict(aux_in=16, ld_aux=4), -1),
    ("gemm_fp8", dict(aux_out=16, ld_aux=4), -1),
    ("gemm_fp8", dict(residual=16, ldr=4), -1),
    ("gemm_fp8", dict(K=64, A=None), -1),               # null pointers, sizes, activation, then K % 128, alignment, leading dimensions
    ("gemm_fp8", dict(K=64, a_row_scale=None), -1),
    ("gemm_fp8", dict(K=64, M=0), -1),
    ("gemm_fp8", dict(K=64, act=5), -4),
    ("gemm_fp8", dict(K=64, A=18), -3),
    ("gemm_fp8", dict(K=64, lda=32), -3),
    ("gemm_fp8", dict(A=18, ldc=4), -2),
    ("gemm_fp8", dict(lda=72), -2),
    ("gemm_fp8", dict(act=5, tile=3), -4),
    ("quantize_rows_fp8", dict(x=None), -1),
    ("quantize_rows_fp8", dict(out=None), -1),
    ("quantize_rows_fp8", dict(row_scale=None), -1),
    ("quantize_rows_fp8", dict(rows=0), -1),
    ("quantize_rows_fp8", dict(cols=0), -1),
    ("quantize_rows_fp8", dict(cols=6), -3),
    ("quantize_rows_fp8", dict(ldx=6), -2),
    ("quantize_rows_fp8", dict(ldx=4), -2),
    ("quantize_rows_fp8", dict(ld_out=6), -2),
    ("quantize_rows_fp8", dict(ld_out=4), -2),
    ("quantize_rows_fp8", dict(x=20), -2),
    ("quantize_rows_fp8", dict(out=18), -2),
    ("quantize_rows_fp8", dict(dtype=7), -4),
    ("quantize_rows_fp8", dict(dtype=2), -4),
    ("quantize_rows_fp8", dict(cols=6, x=None), -1),
    ("quantize_rows_fp8", dict(cols=6, ldx=6), -3),
    ("quantize_rows_fp8", dict(dtype=7, x=20), -2),     # the dtype is looked at last
]


def _fault_id(fault):
    def one(k, v):
        if not isinstance(v, dict):
            return f"{k}_{v}"
        consumer = bool(v.get("ln_stats"))               # a consumer block is named by what it changes of _LN_CONSUMER
        own = {f: x for f, x in v.items() if not consumer or _LN_CONSUMER.get(f, object()) != x}
        return ("consumer+" if consumer else "ln+") + "+".join(f"{f}_{x}" for f, x in own.items())
    return "-".join(one(k, v) for k, v in fault.items())


@pytest.mark.parametrize("name,fault,code", GEMM_REJECTIONS, ids=[f"{n}-{_fault_id(f)}" for n, f, _ in GEMM_REJECTIONS])
def test_gemm_rejections_are_pinned(lib, name, fault, code):
    """Every GEMM entry point rejects a faulty call on the host, with the same code as ever (no GPU needed)."""
    assert _gemm_call(lib, name, **fault) == code


_DECODE_GOOD = {
    "splitk": dict(dtype=1, M=8, N=128, K=128, A=16, lda=128, B=16, ldb=128, a_row_scale=16, b_scale=1.0, partials=16, ks=1, stream=None, unroll=0),
    "finish": dict(dtype=1, M=8, N=128, F=64, partials=16, ks=2, bias=None, act=0, residual=None, ld_residual=0, out_f32=0, n_seg=1, out0=16,
                   ld0=128, out1=None, ld1=0, out2=None, ld2=0, out=16, ld=64, stream=None),
    "direct": dict(args=True, sel=0, stream=None, M=8, N=128, K=128, A=16, lda=128, a_kind=0, gamma=None, beta=None, eps=1e-5, stats_in=None,
                   n_stats_in=0, stats_in_cols=0, B=16, ldb=128, gated_rows=0, bias=None, act=0, residual=None, ld_residual=0, out_f32=0,
                   n_seg=1, out0=16, out1=None, out2=None, ld_out=128, stats_out=None),
    "shared": dict(dtype=1, B=1, G=2, H=1, S0=4, t=0, t_max=4, hd=8, q=16, ldq=8, k_prompt=16, ldk=8, v_prompt=16, ldv=8, prompt_batch_rows=4,
                   k_tail=16, v_tail=16, ld_tail=8, k_new=16, v_new=16, ld_new=8, o=16, ldo=8, key_mask=None, ld_mask=0, scale=1.0, stream=None),
}
_DECODE_FAMILY = {"gemm_splitk": "splitk", "gemm_splitk_ex": "splitk", "gemm_fp8_splitk": "splitk", "splitk_finish": "finish",
                  "splitk_finish_gated": "finish", "gemm_decode": "direct", "gemm_decode_ex": "direct", "attention_decode_shared": "shared"}
_NORM = dict(a_kind=1, gamma=16, stats_in=16, n_stats_in=2, stats_in_cols=64)      # a LayerNorm-on-load call of the direct GEMM, K = 128


def _decode_call(lib, name, **over):
    """One decode-step entry point on a small valid problem (16 stands for an aligned pointer, 18 / 24 for misaligned ones; dtype 1 = bf16)
    with the named arguments replaced: the fault(s) of the call.  eavqa_gemm_decode takes its arguments as the fields of an
    eavqa_decode_gemm_t (out0..2 = out[0..2], ld_out for all three; args=False: a null struct).  Only ever called WITH a fault: a valid
    call would go on to launch."""
    from eavqa_amd import _lib
    import ctypes as C
    a = dict(_DECODE_GOOD[_DECODE_FAMILY[name]])
    assert not set(over) - set(a), over
    a.update(over)
    if _DECODE_FAMILY[name] == "direct":
        g = _lib.DecodeGemm()
        for f, _ in _lib.DecodeGemm._fields_:
            if f not in ("out", "ld_out"):
                setattr(g, f, a[f])
        for i in range(3):
            g.out[i], g.ld_out[i] = a[f"out{i}"], a["ld_out"]
        a["args"] = C.byref(g) if a["args"] else None
    return getattr(lib, "eavqa_" + name)(*_positional("eavqa_" + name, a))


_BIG_A = dict(M=64, K=1216, lda=1216, ldb=1216)         # bf16 split-K: a 152 KiB A slice in one piece (ks = 1)

# (entry point, the fault(s), error code): -1 ARG, -2 ALIGN, -3 SHAPE, -4 DTYPE.  The codes are the ones the library returned before the
# decode-step kernels got one host layer (csrc/decode_params.h), read off those entry points; a change here is a change of the C ABI's
# behaviour.  Calls with two faults pin the ORDER of the checks.  The two stats-coverage rows of eavqa_gemm_decode at the end are the one
# new rule: every statistics partial begins inside the row.
DECODE_GEMM_REJECTIONS = [
    ("gemm_splitk", dict(dtype=0), -4),
    ("gemm_splitk", dict(A=None), -1),
    ("gemm_splitk", dict(B=None), -1),
    ("gemm_splitk", dict(partials=None), -1),
    ("gemm_splitk", dict(M=0), -1),
    ("gemm_splitk", dict(M=65), -1),
    ("gemm_splitk", dict(N=0), -1),
    ("gemm_splitk", dict(K=0), -1),
    ("gemm_splitk", dict(ks=0), -1),
    ("gemm_splitk", dict(K=96, ks=2), -3),
    ("gemm_splitk", dict(lda=64), -3),
    ("gemm_splitk", dict(ldb=64), -3),
    ("gemm_splitk", dict(lda=132), -2),
    ("gemm_splitk", dict(ldb=132), -2),
    ("gemm_splitk", dict(A=18), -2),
    ("gemm_splitk", dict(B=24), -2),
    ("gemm_splitk", _BIG_A, -3),
    ("gemm_splitk", dict(dtype=0, A=None), -4),         # dtype, arguments, shape, alignment, the staged slice
    ("gemm_splitk", dict(A=None, K=96, ks=2), -1),
    ("gemm_splitk", dict(lda=64, A=18), -3),
    ("gemm_splitk", dict(_BIG_A, A=18), -2),
    ("gemm_splitk_ex", dict(dtype=0), -4),
    ("gemm_splitk_ex", dict(A=None), -1),
    ("gemm_splitk_ex", dict(K=96, ks=2), -3),
    ("gemm_splitk_ex", dict(B=24), -2),
    ("gemm_splitk_ex", dict(unroll=4), -1),
    ("gemm_splitk_ex", dict(unroll=0x200), -1),
    ("gemm_splitk_ex", dict(unroll=0x3000), -1),
    ("gemm_splitk_ex", dict(_BIG_A, unroll=4), -3),     # ... and the selector last
    ("gemm_splitk_ex", dict(A=18, unroll=4), -2),
    ("gemm_fp8_splitk", dict(a_row_scale=None), -1),
    ("gemm_fp8_splitk", dict(A=None), -1),
    ("gemm_fp8_splitk", dict(B=None), -1),
    ("gemm_fp8_splitk", dict(partials=None), -1),
    ("gemm_fp8_splitk", dict(M=65), -1),
    ("gemm_fp8_splitk", dict(ks=0), -1),
    ("gemm_fp8_splitk", dict(K=192, lda=192, ldb=192), -3),
    ("gemm_fp8_splitk", dict(K=256, lda=256, ldb=256, ks=4), -3),
    ("gemm_fp8_splitk", dict(lda=64), -3),
    ("gemm_fp8_splitk", dict(lda=136), -2),
    ("gemm_fp8_splitk", dict(ldb=136), -2),
    ("gemm_fp8_splitk", dict(A=18), -2),
    ("gemm_fp8_splitk", dict(B=24), -2),
    ("gemm_fp8_splitk", dict(M=64, K=2432, lda=2432, ldb=2432), -3),
    ("gemm_fp8_splitk", dict(K=192, lda=192, ldb=192, a_row_scale=None), -1),
    ("gemm_fp8_splitk", dict(K=192, lda=192, ldb=192, A=18), -3),
    ("gemm_fp8_splitk", dict(M=64, K=2432, lda=2432, ldb=2432, B=24), -2),
    ("splitk_finish", dict(dtype=7), -4),
    ("splitk_finish", dict(partials=None), -1),
    ("splitk_finish", dict(out0=None), -1),
    ("splitk_finish", dict(M=0), -1),
    ("splitk_finish", dict(N=0), -1),
    ("splitk_finish", dict(ks=0), -1),
    ("splitk_finish", dict(n_seg=0), -1),
    ("splitk_finish", dict(n_seg=4), -1),
    ("splitk_finish", dict(n_seg=2), -1),               # out1 is null
    ("splitk_finish", dict(n_seg=3, out1=16), -1),
    ("splitk_finish", dict(N=130), -3),
    ("splitk_finish", dict(n_seg=3, out1=16, out2=16), -3),     # 128 columns in three segments
    ("splitk_finish", dict(ld0=130), -3),
    ("splitk_finish", dict(n_seg=2, out1=16, ld1=2), -3),
    ("splitk_finish", dict(residual=16, ld_residual=130), -3),
    ("splitk_finish", dict(act=5), -4),
    ("splitk_finish", dict(act=-1), -4),
    ("splitk_finish", dict(dtype=7, partials=None), -4),        # dtype, arguments, shape, activation
    ("splitk_finish", dict(partials=None, N=130), -1),
    ("splitk_finish", dict(n_seg=2, N=130), -1),
    ("splitk_finish", dict(N=130, act=5), -3),
    ("splitk_finish_gated", dict(dtype=7), -4),
    ("splitk_finish_gated", dict(partials=None), -1),
    ("splitk_finish_gated", dict(out=None), -1),
    ("splitk_finish_gated", dict(M=0), -1),
    ("splitk_finish_gated", dict(F=0), -1),
    ("splitk_finish_gated", dict(ks=0), -1),
    ("splitk_finish_gated", dict(F=6), -3),
    ("splitk_finish_gated", dict(ld=6), -3),
    ("splitk_finish_gated", dict(act=5), -4),
    ("splitk_finish_gated", dict(dtype=7, out=None), -4),
    ("splitk_finish_gated", dict(out=None, F=6), -1),
    ("splitk_finish_gated", dict(F=6, act=5), -3),
    ("gemm_decode", dict(args=False), -1),
    ("gemm_decode", dict(A=None), -1),
    ("gemm_decode", dict(B=None), -1),
    ("gemm_decode", dict(out0=None), -1),
    ("gemm_decode", dict(M=0), -1),
    ("gemm_decode", dict(M=65), -1),
    ("gemm_decode", dict(N=0), -1),
    ("gemm_decode", dict(K=0), -1),
    ("gemm_decode", dict(K=96), -3),
    ("gemm_decode", dict(a_kind=3), -4),
    ("gemm_decode", dict(a_kind=-1), -4),
    ("gemm_decode", dict(act=5), -4),
    ("gemm_decode", dict(_NORM, gamma=None), -1),
    ("gemm_decode", dict(_NORM, stats_in=None), -1),
    ("gemm_decode", dict(_NORM, n_stats_in=0), -1),
    ("gemm_decode", dict(_NORM, n_stats_in=257, stats_in_cols=1), -1),
    ("gemm_decode", dict(_NORM, stats_in_cols=0), -1),
    ("gemm_decode", dict(_NORM, K=16448, lda=16448, ldb=16448, n_stats_in=256, stats_in_cols=65), -1),
    ("gemm_decode", dict(_NORM, stats_in_cols=63), -1),         # 2 x 63 columns do not cover 128
    ("gemm_decode", dict(lda=64), -2),
    ("gemm_decode", dict(ldb=64), -2),
    ("gemm_decode", dict(lda=132), -2),
    ("gemm_decode", dict(ldb=132), -2),
    ("gemm_decode", dict(_NORM, lda=130), -2),                  # the fp32 stream: a multiple of 4
    ("gemm_decode", dict(A=18), -2),
    ("gemm_decode", dict(B=24), -2),
    ("gemm_decode", dict(_NORM, gamma=18), -2),
    ("gemm_decode", dict(_NORM, beta=18), -2),
    ("gemm_decode", dict(n_seg=0), -3),
    ("gemm_decode", dict(n_seg=4), -3),
    ("gemm_decode", dict(n_seg=3, out1=16, out2=16), -3),       # 128 columns in three segments
    ("gemm_decode", dict(n_seg=2), -1),                         # out[1] is null
    ("gemm_decode", dict(gated_rows=64), -1),
    ("gemm_decode", dict(ldb=1 << 24), -3),                     # B spans 2 GB and more
    ("gemm_decode", dict(A=None, K=96), -1),                    # arguments, K % 64, a_kind / act, the norm's arguments, leading dimensions and
    ("gemm_decode", dict(K=96, a_kind=3), -3),                  # alignment, segments, the gate - then the plan, then the extents
    ("gemm_decode", dict(a_kind=3, act=5, lda=132), -4),
    ("gemm_decode", dict(_NORM, gamma=None, lda=132), -1),
    ("gemm_decode", dict(lda=132, n_seg=4), -2),
    ("gemm_decode", dict(n_seg=4, gated_rows=64), -3),
    ("gemm_decode", dict(n_seg=2, gated_rows=64), -1),
    ("gemm_decode_ex", dict(args=False, sel=1), -1),
    ("gemm_decode_ex", dict(K=96, sel=5), -3),
    ("gemm_decode_ex", dict(sel=5), -3),                        # five fragments: no such kernel
    ("gemm_decode_ex", dict(M=64, sel=3), -3),
    ("gemm_decode_ex", dict(gated_rows=128, ldb=128, sel=1), -1),       # the gate needs an even fragment count
    ("gemm_decode_ex", dict(gated_rows=128, sel=3), -1),
    ("gemm_decode_ex", dict(gated_rows=64, sel=5), -1),
    ("gemm_decode_ex", dict(gated_rows=128, sel=5), -1),        # odd before missing
    ("gemm_decode_ex", dict(ldb=1 << 24, sel=5), -3),
    ("gemm_decode_ex", dict(ldb=1 << 24, gated_rows=128, sel=1), -1),
    # the new rule, just inside and just outside ((n_stats_in - 1) * stats_in_cols = 64 < 128; = 128): the misaligned lda is checked after it
    ("gemm_decode", dict(_NORM, n_stats_in=2, stats_in_cols=64, lda=130), -2),
    ("gemm_decode", dict(_NORM, n_stats_in=3, stats_in_cols=64, lda=130), -1),
    ("gemm_decode", dict(_NORM, n_stats_in=3, stats_in_cols=48, lda=130), -2),
    ("gemm_decode", dict(_NORM, n_stats_in=4, stats_in_cols=48, lda=130), -1),
    ("attention_decode_shared", dict(q=None), -1),
    ("attention_decode_shared", dict(k_prompt=None), -1),
    ("attention_decode_shared", dict(v_tail=None), -1),
    ("attention_decode_shared", dict(k_new=None), -1),
    ("attention_decode_shared", dict(o=None), -1),
    ("attention_decode_shared", dict(B=0), -1),
    ("attention_decode_shared", dict(H=0), -1),
    ("attention_decode_shared", dict(dtype=7), -4),
    ("attention_decode_shared", dict(G=0), -3),
    ("attention_decode_shared", dict(G=9), -3),
    ("attention_decode_shared", dict(hd=12), -3),
    ("attention_decode_shared", dict(hd=136), -3),
    ("attention_decode_shared", dict(S0=0), -3),
    ("attention_decode_shared", dict(S0=3585), -3),
    ("attention_decode_shared", dict(t_max=0), -3),
    ("attention_decode_shared", dict(t_max=257), -3),
    ("attention_decode_shared", dict(H=262144), -3),
    ("attention_decode_shared", dict(t=-1), -1),
    ("attention_decode_shared", dict(t=4), -1),
    ("attention_decode_shared", dict(ldq=12), -2),
    ("attention_decode_shared", dict(ld_tail=12), -2),
    ("attention_decode_shared", dict(dtype=0, ldo=10), -2),     # fp32: multiples of 4
    ("attention_decode_shared", dict(q=18), -2),
    ("attention_decode_shared", dict(v_new=24), -2),
    ("attention_decode_shared", dict(ldk=0), -1),
    ("attention_decode_shared", dict(H=2), -1),                 # every leading dimension is below H hd
    ("attention_decode_shared", dict(prompt_batch_rows=2), -1),
    ("attention_decode_shared", dict(key_mask=16, ld_mask=2), -1),
    ("attention_decode_shared", dict(q=None, dtype=7), -1),     # arguments, dtype, shape, t, alignment, extents
    ("attention_decode_shared", dict(dtype=7, G=9), -4),
    ("attention_decode_shared", dict(G=9, t=4), -3),
    ("attention_decode_shared", dict(t=4, ldq=12), -1),
    ("attention_decode_shared", dict(ldq=12, prompt_batch_rows=2), -2),
    ("attention_decode_shared", dict(q=18, prompt_batch_rows=2), -2),
]


@pytest.mark.parametrize("name,fault,code", DECODE_GEMM_REJECTIONS, ids=[f"{n}-{_fault_id(f)}-{i}" for i, (n, f, _) in enumerate(DECODE_GEMM_REJECTIONS)])
def test_decode_rejections_are_pinned(lib, name, fault, code):
    """Every decode-step entry point rejects a faulty call on the host, with the same code as ever (no GPU needed)."""
    assert code < 0
    assert _decode_call(lib, name, **fault) == code


def _block_call(lib, name, **over):
    """One decoder block driver on a small valid problem (16 stands for a device pointer; dtype 1 = bf16; the layer tables are host arrays of
    such pointers) with the named arguments replaced: the one fault of the call.  workspace_bytes is what the driver's own size function
    returns for the shape, minus `ws_short`.  Only ever called WITH a fault: a valid call would go on to enqueue kernels."""
    from eavqa_amd import _lib
    t5 = name.startswith("t5")
    a = dict(dtype=1, n_layer=2, layers=True, tails=True, null_tail=False, scales=True, ln_final=16, E=64 if t5 else 128, inner=256, H=4,
             F=128 if t5 else 512, gated=1, act=2, eps=1e-5, B=2, G=2, beams=2, Sq=1, row0=5, S0=5, S_max=16, t=3, t_max=8, S=20, x=16, out=16,
             mask=None, ld_mask=0, rel_bias=16, rel_ld=15, rel_zero=7, ws=16, ws_short=0, stream=None)
    assert not set(over) - set(a), over
    a.update(over)

    def table(kind):
        rows = (kind * a["n_layer"])()
        for r in rows:
            for f, _ in kind._fields_:
                setattr(r, f, 16)
        return rows
    a["layers"] = table(_lib.T5DecLayer if t5 else _lib.LMLayer) if a["layers"] else None
    a["tails"] = table(_lib.LMTail) if a["tails"] else None
    if a["null_tail"]:
        a["tails"][1].v_tail = None
    a["scales"] = (_lib.LMLayerScales * a["n_layer"])() if a["scales"] else None
    sizes = {
        "lm_block_forward": lambda: lib.eavqa_lm_block_workspace_bytes(a["dtype"], a["B"] * a["Sq"], a["E"], a["F"]),
        "lm_block_step_shared": lambda: lib.eavqa_lm_block_step_shared_workspace_bytes(a["dtype"], a["B"] * a["G"], a["E"], a["F"]),
        "lm_block_forward_fp8": lambda: lib.eavqa_lm_block_fp8_workspace_bytes(a["B"] * a["Sq"], a["E"], a["F"]),
        "t5_decoder_step": lambda: lib.eavqa_t5_decoder_step_workspace_bytes(a["dtype"], a["B"], a["E"], a["inner"], a["F"], a["gated"]),
        "t5_decoder_step_beams": lambda: lib.eavqa_t5_decoder_step_beams_workspace_bytes(a["dtype"], a["B"], a["beams"], a["E"], a["inner"], a["F"],
                                                                                          a["gated"]),
    }
    a["ws_bytes"] = sizes[name]() - a["ws_short"]
    return getattr(lib, "eavqa_" + name)(*_positional("eavqa_" + name, a, _BLOCK_ALIAS))


# (entry point, the one fault, error code): -1 ARG, -3 SHAPE, -4 DTYPE.  Every fault is one the drivers reject themselves, before their first
# kernel call, so no GPU is needed.  The codes are the ones the library returned before the drivers were folded onto one workspace layout and
# one layer loop per route (recorded from that library); a change here is a change of the C ABI's behaviour.
BLOCK_REJECTIONS = [
    ("lm_block_forward", dict(layers=False), -1),
    ("lm_block_forward", dict(ws=None), -1),
    ("lm_block_forward", dict(S_max=5), -1),                    # S_max < row0 + Sq
    ("lm_block_forward", dict(H=3), -3),                        # E % H
    ("lm_block_forward", dict(ws_short=1), -1),
    ("lm_block_forward", dict(ws_short=1, B=65), -1),           # ... also on the shape without a split plan
    ("lm_block_step_shared", dict(layers=False), -1),
    ("lm_block_step_shared", dict(ws=None), -1),
    ("lm_block_step_shared", dict(G=9), -3),
    ("lm_block_step_shared", dict(t=8), -1),                    # t == t_max
    ("lm_block_step_shared", dict(dtype=7), -4),
    ("lm_block_step_shared", dict(null_tail=True), -1),
    ("lm_block_step_shared", dict(H=3), -3),
    ("lm_block_step_shared", dict(ws_short=1), -1),
    ("lm_block_forward_fp8", dict(layers=False), -1),
    ("lm_block_forward_fp8", dict(ws=None), -1),
    ("lm_block_forward_fp8", dict(E=192), -3),                  # E % 128
    ("lm_block_forward_fp8", dict(S_max=5), -1),
    ("lm_block_forward_fp8", dict(ws_short=1), -1),
    ("t5_decoder_step", dict(layers=False), -1),
    ("t5_decoder_step", dict(ws=None), -1),
    ("t5_decoder_step", dict(t=0), -1),
    ("t5_decoder_step", dict(dtype=7), -4),
    ("t5_decoder_step", dict(H=3), -3),                         # inner % H
    ("t5_decoder_step", dict(ws_short=1), -1),
    ("t5_decoder_step_beams", dict(layers=False), -1),
    ("t5_decoder_step_beams", dict(ws=None), -1),
    ("t5_decoder_step_beams", dict(beams=9), -3),
    ("t5_decoder_step_beams", dict(ws_short=1), -1),
]


@pytest.mark.parametrize("name,fault,code", BLOCK_REJECTIONS, ids=[f"{n}-{_fault_id(f)}" for n, f, _ in BLOCK_REJECTIONS])
def test_block_driver_rejections_are_pinned(lib, name, fault, code):
    """Every decoder block driver rejects a faulty call on the host, with the same code as ever (no GPU needed)."""
    assert _block_call(lib, name, **fault) == code


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from eavqa_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.EavqaError, match="only compute path"):
        _lib.load()


def test_cpu_tensors_are_rejected_not_emulated():
    import torch
    from eavqa_amd import ops, _lib
    with pytest.raises(_lib.EavqaError, match="no CPU fallback"):
        ops.gemm(torch.zeros(8, 8), torch.zeros(8, 8))


def test_decode_plans_are_pure_host_arithmetic(lib):
    """eavqa_gemm_splitk_plan / eavqa_lm_block_workspace_bytes touch no device: the split of every decode GEMM of the few-shot model
    (OPT-2.7B, B = 32) is the one profiles/round2_decode.md was measured with (FFN-up since round 3: 512-deep slices, no split gives one
    workgroup per CU there), unsupported shapes give 0."""
    plan = lib.eavqa_gemm_splitk_plan
    E, F = 2560, 10240
    assert [plan(32, 3 * E, E), plan(32, E, E), plan(32, F, E), plan(32, E, F)] == [4, 10, 5, 10]
    for M, N, K in ((32, 3 * E, E), (1, 64, 32), (64, 50272, 2560), (17, 200, 96), (64, 12800, 512)):
        ks = plan(M, N, K)
        assert ks >= 1 and K % (32 * ks) == 0 and (K // ks) * (1 if M <= 16 else 2 if M <= 32 else 4) * 32 <= 64 * 1024
    assert plan(32, 8192, 2048) == 4 and plan(32, 16384, 4096) == 8        # OPT-1.3B FFN-up: one round exists; OPT-6.7B: 512-deep slices
    assert plan(65, 128, 64) == 0 and plan(8, 128, 48) == 0 and plan(0, 128, 64) == 0
    ws = lib.eavqa_lm_block_workspace_bytes
    small, big = ws(1, 32, E, F), ws(1, 4800, E, F)             # dtype 1 = bfloat16: a decode step, the 150-position prefill of 32 prompts
    assert 0 < small < big
    assert 0 < ws(0, 32, E, F) < small            # fp32 has no split-K decode route: no partial-sum buffers in its workspace
