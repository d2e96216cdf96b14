#!/usr/bin/env python3
"""One ops.gemm per row of the route table of tests/test_gemm_route_cpu.py, to be run under a kernel trace, and the comparison of two such
traces: the check that a change of the GEMM host layer (csrc/gemm.hip) launches what its parent launched.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o trace -- python tools/gemm_route_trace.py --calls OUT/calls.txt
    python tools/gemm_route_trace.py --compare OLD/trace_kernel_trace.csv NEW/trace_kernel_trace.csv [--calls NEW/calls.txt]

The driver takes the table from --table (default: the test module of this tree), so the same file can be handed to a checkout that predates
it.  A row is issued as the call its columns describe: the knobs through eavqa_gemm_ex, has_ln as an eavqa_gemm_ln producer call (second copy +
row statistics), and every bf16 row without knobs a second time through eavqa_gemm_pf (the look-ahead form).  --calls lists, per call, what
eavqa_gemm_route says it launches (where the library has that entry point); --compare checks the second trace against that list too.
"""
import argparse, csv, importlib.util, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL = ["gemm_f32_kernel", "gemm_bf16_kernel", "gemm_bf16_skinny_kernel", "gemm_bf16_fast_kernel", "gemm_bf16_shaped_kernel", "gemm_bf16_big_kernel",
          "gemm_bf16_k64s_"]
LAYOUT = ["true, true", "true, false", "false, true", "false, false"]
SHAPED = ["4, 1, 2, 5", "4, 1, 2, 6", "4, 2, 4, 4", "4, 2, 4, 5", "4, 2, 4, 6"]                    # SHAPES, csrc/gemm_r1.hip
K64 = ["4, 1, 2, 5, 3, 2", "4, 1, 2, 5, 3, 4", "2, 2, 4, 4, 2, 4", "4, 2, 4, 4, 3, 4", "4, 2, 4, 5, 3, 4", "4, 1, 2, 5, 4, 2", "4, 1, 2, 6, 3, 2",
       "4, 2, 4, 6, 2, 4", "2, 4, 8, 4, 2, 4", "2, 2, 4, 4, 3, 2", "2, 4, 4, 4, 3, 4"]             # K64_SHAPES, csrc/gemm_k64.hip


def load_table(path):
    spec = importlib.util.spec_from_file_location("route_table", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [row for row, _ in mod.ROUTES]


def expected(lib, row):
    """The kernel-name patterns eavqa_gemm_route promises for a row (two for a row-split problem), or None without that entry point."""
    import ctypes as C
    if not hasattr(lib, "eavqa_gemm_route"):
        return None
    out, split = [], C.c_int(0)
    dt, a, b, M, N, K, ln, kn = row
    r = lib.eavqa_gemm_route(dt, a, b, M, N, K, ln, kn, C.byref(split))
    while True:
        if r < 0:
            return out + [f"error {r}"]
        kind, idx = r >> 8, r & 255
        out.append(KERNEL[kind] + ("|" + (LAYOUT[idx] if kind < 2 else SHAPED[idx] if kind == 4 else K64[idx]) if kind in (0, 1, 4, 6) else ""))
        if not split.value:
            return out
        M, kn = split.value, 0
        r = lib.eavqa_gemm_route(dt, a, b, M, N, K, ln, 0, C.byref(split))


def drive(table, calls_path):
    import torch
    from eavqa_amd import ops, _lib
    lib = _lib.load()
    dev = "cuda"
    lines = []
    for i, row in enumerate(load_table(table)):
        dt, a_kc, b_kc, M, N, K, ln, kn = row
        dtype = torch.bfloat16 if dt == 1 else torch.float32
        A = torch.zeros((M, K) if a_kc else (K, M), device=dev, dtype=dtype)
        B = torch.zeros((N, K) if b_kc else (K, N), device=dev, dtype=dtype)
        out = torch.empty((M, N), device=dev, dtype=dtype)
        kw = dict(a_kc=bool(a_kc), b_kc=bool(b_kc), out=out)
        if ln:
            kw.update(copy_out=torch.empty((M, N), device=dev, dtype=dtype), stats_out=torch.empty((M, (N + 63) // 64, 2), device=dev))
        forms = [("ln" if ln else "ex" if kn else "plain", kw)]
        if dt == 1 and not ln and not kn:
            forms.append(("pf", dict(kw, prefetch=B)))
        for form, k in forms:
            ops.KernelSelect.gemm = kn
            try:
                ops.gemm(A, B, **k)
                status = "ok"
            except _lib.EavqaError as e:
                status = "rejected: " + str(e)
            finally:
                ops.KernelSelect.gemm = 0
            exp = expected(lib, row)
            lines.append(f"{i}\t{form}\t{row}\t{status}\t{exp}")
        torch.cuda.synchronize()
        del A, B, out, kw, forms
    if calls_path:
        os.makedirs(os.path.dirname(os.path.abspath(calls_path)), exist_ok=True)
        with open(calls_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} calls issued")


def read_trace(path):
    """(kernel name, grid, workgroup size, LDS bytes) of every GEMM kernel of a rocprofv3 kernel trace, in dispatch order."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    key = {k.lower(): k for k in rows[0]}
    col = lambda r, n: r[key[n]]
    rows.sort(key=lambda r: int(col(r, "dispatch_id")))
    out = []
    for r in rows:
        name = col(r, "kernel_name")
        if "gemm_" not in name or "anonymous namespace" not in name:
            continue
        out.append((name, tuple(int(col(r, f"grid_size_{d}")) for d in "xyz"), tuple(int(col(r, f"workgroup_size_{d}")) for d in "xyz"),
                    int(col(r, "lds_block_size"))))
    return out


def compare(old_csv, new_csv, calls_path):
    old, new = read_trace(old_csv), read_trace(new_csv)
    bad = 0
    if len(old) != len(new):
        print(f"DIFFERENT: {len(old)} launches against {len(new)}")
        bad += 1
    for i, (o, n) in enumerate(zip(old, new)):
        if o != n:
            bad += 1
            print(f"DIFFERENT at launch {i}:\n  old {o}\n  new {n}")
    print(f"{len(new)} GEMM launches compared, {bad} differences")
    if calls_path:
        it = iter(new)
        calls = wrong = 0
        for line in open(calls_path):
            i, form, row, status, exp = line.rstrip("\n").split("\t")
            calls += 1
            if status != "ok":
                continue
            pats = eval(exp)
            for pat in pats:
                name = next(it)[0]
                parts = pat.split("|")
                # the look-ahead form: a tile that carries it, one launch (the second launch of a row-split problem drops the region)
                want = parts[0] + ("pf_kernel" if form == "pf" and len(pats) == 1 and parts[0].endswith("k64s_") and parts[1] in K64_PF else "")
                if want not in name or (len(parts) > 1 and f"<{parts[1]}" not in re.sub(r"\s+", " ", name)):
                    wrong += 1
                    print(f"row {i} ({form}) {row}: route says {pat}, launched {name}")
        rest = len(list(it))
        print(f"{calls} calls checked against eavqa_gemm_route: {wrong} wrong kernels, {rest} launches unaccounted for")
        bad += wrong + rest
    return 1 if bad else 0


# the full-line tiles that carry the look-ahead form (WITH_LN in K64_SHAPES)
K64_PF = {K64[i] for i in (3, 4, 5, 9, 10)}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=os.path.join(ROOT, "tests", "test_gemm_route_cpu.py"))
    ap.add_argument("--calls", default=None)
    ap.add_argument("--compare", nargs=2, metavar=("OLD_CSV", "NEW_CSV"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.calls))
    drive(a.table, a.calls)
