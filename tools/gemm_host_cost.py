#!/usr/bin/env python3
"""Host cost of one eavqa_gemm call: an enqueue-only loop on a decode-step shape (M = 32, N = K = 2048, bf16).  Synchronise, start the wall
clock, issue the calls straight through ctypes, stop the clock BEFORE the final synchronise, divide.  A decode step issues hundreds of such
calls and is host-bound, so this is the number a change of the GEMM host layer (csrc/gemm.hip) must not move.

    python tools/gemm_host_cost.py [--calls 10000] [--repeats 5]
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from eavqa_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10000)
ap.add_argument("--repeats", type=int, default=5)
a = ap.parse_args()
lib = _lib.load()
M, N, K = 32, 2048, 2048
A = torch.randn(M, K, device="cuda").to(torch.bfloat16)
B = (torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16)
out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
args = (1, 1, 1, M, N, K, A.data_ptr(), K, B.data_ptr(), K, out.data_ptr(), N, 0, 1.0, None, 0, None, None, 0, None, 0, None)
fn = lib.eavqa_gemm
for _ in range(200):
    assert fn(*args) == 0
res = []
for _ in range(a.repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        fn(*args)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    res.append((t1 - t0) / a.calls * 1e6)
print("host us per eavqa_gemm call (enqueue only), per repeat:", " ".join(f"{r:.3f}" for r in res), " min", f"{min(res):.3f}", " median", f"{sorted(res)[len(res) // 2]:.3f}")
