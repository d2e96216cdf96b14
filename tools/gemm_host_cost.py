#!/usr/bin/env python3
"""Host cost of one call of a host layer: an enqueue-only loop on a decode-step shape (bf16, 32 rows).  Synchronise, start the wall clock,
issue the calls straight through ctypes, stop the clock BEFORE the final synchronise, divide.  A decode step issues hundreds of such calls
and is host-bound, so this is the number a change of a host layer must not move.

    python tools/gemm_host_cost.py [--entry gemm|splitk|attention_decode] [--calls 10000] [--repeats 5]

--entry gemm              eavqa_gemm, N = K = 2048 (csrc/gemm.hip)
        splitk            eavqa_gemm_splitk + eavqa_splitk_finish, N = K = 2560 at the planned split: two calls per round (csrc/decode.hip)
        attention_decode  eavqa_attention_decode_splitk, 32 heads x 80, 160 keys (csrc/attention_decode.hip)
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from eavqa_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--entry", choices=("gemm", "splitk", "attention_decode"), default="gemm")
ap.add_argument("--calls", type=int, default=10000)
ap.add_argument("--repeats", type=int, default=5)
a = ap.parse_args()
lib = _lib.load()
M = 32
bf16 = dict(device="cuda", dtype=torch.bfloat16)
if a.entry == "gemm":
    N = K = 2048
    A, B, out = torch.randn(M, K, **bf16), torch.randn(N, K, **bf16) * 0.02, torch.empty(M, N, **bf16)
    what = "eavqa_gemm call"
    calls = [(lib.eavqa_gemm, (1, 1, 1, M, N, K, A.data_ptr(), K, B.data_ptr(), K, out.data_ptr(), N, 0, 1.0, None, 0, None, None, 0, None, 0, None))]
elif a.entry == "splitk":
    N = K = 2560
    ks = lib.eavqa_gemm_splitk_plan(M, N, K)
    A, B, out = torch.randn(M, K, **bf16), torch.randn(N, K, **bf16) * 0.02, torch.empty(M, N, **bf16)
    part = torch.empty(ks, M, N, device="cuda", dtype=torch.float32)
    what = "eavqa_gemm_splitk + eavqa_splitk_finish pair"
    calls = [(lib.eavqa_gemm_splitk, (1, M, N, K, A.data_ptr(), K, B.data_ptr(), K, part.data_ptr(), ks, None)),
             (lib.eavqa_splitk_finish, (1, M, N, part.data_ptr(), ks, None, 0, None, 0, 0, 1, out.data_ptr(), N, None, 0, None, 0, None))]
else:
    H, hd, Sk, S_max, ks = 32, 80, 160, 192, 4
    E = H * hd
    part = torch.randn(ks, M, 3 * E, device="cuda", dtype=torch.float32) * 0.1
    kc, vc, out = torch.randn(M * S_max, E, **bf16), torch.randn(M * S_max, E, **bf16), torch.empty(M, E, **bf16)
    what = "eavqa_attention_decode_splitk call"
    calls = [(lib.eavqa_attention_decode_splitk, (1, M, H, Sk, hd, part.data_ptr(), ks, None, kc.data_ptr(), E, vc.data_ptr(), E, S_max,
                                                  out.data_ptr(), E, None, 0, hd ** -0.5, None))]
for _ in range(200):
    for fn, args in calls:
        assert fn(*args) == 0
res = []
for _ in range(a.repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        for fn, args in calls:
            fn(*args)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    res.append((t1 - t0) / a.calls * 1e6)
print(f"host us per {what} (enqueue only), per repeat:", " ".join(f"{r:.3f}" for r in res), " min", f"{min(res):.3f}", " median", f"{sorted(res)[len(res) // 2]:.3f}")
