"""Recorder of the entry-point calls the Python passes make (tests/test_lm_pass_trace_cpu.py; the cases: tests/_lm_pass_cases.py).

The passes are pure enqueue, so on CPU tensors whose contents are never read the list of ``eavqa_*`` calls with all their arguments is
what they do.  ``_lib.call`` / ``_lib_llama.call`` / ``ops.call`` are replaced by a printer, ``ops._dev`` and ``ops._stream`` by stubs; the library itself is
the real one, so split plans and workspace sizes are its own host arithmetic.  One line per call: the entry name, then every argument -
ints verbatim, floats as ``float.hex``, a null pointer as ``0``, any other pointer as ``<label>+<byte offset>`` where the label is the
attribute path of a tensor the model owns (``layers[1].w_fc1``, ``head_t``) or ``b<n>`` by order of first appearance in the case;
structs field by field.  An address is resolved to (storage, offset) by range; every storage whose address was ever taken stays alive
until the case ends, so no label depends on the allocator handing a freed address out again.

``python tests/_lm_pass_trace.py`` prints the trace of every case (the body of tests/golden/lm_pass_trace.txt)."""
import bisect
import contextlib
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from eavqa_amd import _lib      # noqa: E402

# entry -> index of the B operand's pointer among its arguments
GEMM_FAMILY = {entry: _lib.PARAMS[entry].index("B") for entry in ("eavqa_gemm", "eavqa_gemm_pf", "eavqa_gemm_splitk")}


def _owned(root):
    """{storage address: attribute path} of every tensor reachable from ``root`` through attributes, lists, tuples and dicts."""
    out, seen = {}, set()

    def walk(o, path, depth):
        if isinstance(o, torch.Tensor):
            out.setdefault(o.untyped_storage().data_ptr(), path)
            return
        if depth > 5 or id(o) in seen or o is None or isinstance(o, (int, float, str, bool, torch.dtype, torch.device)):
            return
        seen.add(id(o))
        if isinstance(o, (list, tuple)):
            for i, v in enumerate(o):
                walk(v, f"{path}[{i}]", depth + 1)
        elif isinstance(o, dict):
            for k, v in o.items():
                walk(v, f"{path}[{k}]", depth + 1)
        elif not type(o).__module__.startswith(("torch", "builtins", "ctypes", "numpy", "collections")):
            names = [n for cls in type(o).__mro__ for n in getattr(cls, "__slots__", ())] + list(getattr(o, "__dict__", {}))
            for n in names:
                if hasattr(o, n):
                    walk(getattr(o, n), f"{path}.{n}" if path else n, depth + 1)

    walk(root, "", 0)
    return out


class Recorder:
    def __init__(self, root):
        self.root, self.lines = root, []
        self.bases, self.storages, self.labels, self.n_anon = [], {}, {}, 0

    # ---- addresses
    def keep(self, t):
        s = t.untyped_storage()
        base = s.data_ptr()
        if base and base not in self.storages:
            self.storages[base] = s
            bisect.insort(self.bases, base)

    def ptr(self, addr):
        if not addr:
            return "0"
        i = bisect.bisect_right(self.bases, addr) - 1
        base = self.bases[i] if i >= 0 else None
        if base is None or addr - base > self.storages[base].nbytes():
            raise AssertionError(f"a pointer argument ({addr:#x}) lies in no tensor whose address was taken")
        if base not in self.labels:
            name = _owned(self.root).get(base)
            if name is None:
                name, self.n_anon = f"b{self.n_anon}", self.n_anon + 1
            self.labels[base] = name
        return f"{self.labels[base]}+{addr - base}"

    # ---- values
    def value(self, ctype, v):
        if ctype is C.c_void_p:
            return self.ptr(v.value if isinstance(v, C.c_void_p) else v)
        if ctype is C.c_float:
            return float(v).hex()
        if isinstance(ctype, type) and issubclass(ctype, C.Array):
            return "[" + ",".join(self.value(ctype._type_, x) for x in v) + "]"
        if isinstance(ctype, type) and issubclass(ctype, C._Pointer):
            obj = getattr(v, "_obj", v)                       # C.byref(struct) or an array of structs
            items = list(obj) if isinstance(obj, C.Array) else [obj]
            return "[" + ",".join("{" + ",".join(f"{n}={self.value(t, getattr(s, n))}" for n, t in s._fields_) + "}" for s in items) + "]"
        return str(int(v))

    def call(self, name, *args):
        from eavqa_amd import _lib, _lib_llama
        types = _lib.SIGNATURES[name] if name in _lib.SIGNATURES else _lib_llama.SIGNATURES[name]
        assert len(types) == len(args), name
        self.lines.append(" ".join([name] + [self.value(t, a) for t, a in zip(types, args)]))


@contextlib.contextmanager
def recording(root):
    """Every ``eavqa_*`` call made inside goes to the yielded recorder's ``lines`` instead of the library."""
    from eavqa_amd import _lib, _lib_llama, ops
    rec = Recorder(root)
    real_ptr = torch._C.TensorBase.data_ptr

    def data_ptr(t):
        rec.keep(t)
        return real_ptr(t)

    saved = (_lib.call, _lib_llama.call, ops.call, ops._dev, ops._stream)
    _lib.call = _lib_llama.call = ops.call = rec.call
    ops._dev, ops._stream = (lambda t: None), (lambda: 0)
    torch.Tensor.data_ptr = data_ptr
    try:
        yield rec
    finally:
        del torch.Tensor.data_ptr
        _lib.call, _lib_llama.call, ops.call, ops._dev, ops._stream = saved


def trace_case(case):
    model = case.make("cpu")
    with recording(case.root(model)) as rec:
        case.run(model, "cpu")
    return rec.lines


def trace_all():
    """``== <case>`` followed by the case's call lines, for every case."""
    from _lm_pass_cases import CASES
    out = []
    for case in CASES:
        out.append(f"== {case.name}")
        out += trace_case(case)
    return "\n".join(out) + "\n"


def parse(text):
    """{case: [call lines]} of a trace (``#`` lines are the file's header)."""
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("#"):
            continue
        if line.startswith("== "):
            cur = out[line[3:]] = []
        else:
            cur.append(line)
    return out


if __name__ == "__main__":
    from eavqa_amd import build
    build.build(verbose=False)
    sys.stdout.write(trace_all())
