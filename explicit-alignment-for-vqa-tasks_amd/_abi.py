"""Reader of the C ABI headers: include/eavqa.h and include/eavqa_test.h are the only description of the ABI, and the ctypes
bindings of ``_lib`` are derived from them here.

``parse`` accepts exactly the subset of C the two headers use - comments, preprocessor lines (of which only
``#define EAVQA_X <integer>`` means something), the ``extern "C" {`` wrapper, anonymous enums with explicit values,
``typedef struct { ... } eavqa_*_t;`` of scalars, pointers and fixed arrays of them, and prototypes with named parameters - and raises
``AbiError`` naming the header and the offending text on anything else, so that a declaration it does not understand can never be bound
wrongly.  ``bind`` maps what was parsed to ctypes.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple


class AbiError(Exception):
    pass


class Decl(NamedTuple):
    """One declarator: ``base`` is the type name without ``const``, ``pointer`` whether a ``*`` follows it, ``count`` the length of a
    fixed array (0: not an array)."""
    base: str
    pointer: bool
    name: str
    count: int = 0


class Header(NamedTuple):
    constants: dict     # name -> int: the #define'd integers and the enum members, in order of appearance
    structs: dict       # typedef name -> [Decl]
    functions: dict     # name -> (return Decl with an empty name, [Decl])


_SPACE = re.compile(r"\s*")
_INT = r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+)"
_DEFINE = re.compile(rf"#\s*define\s+(EAVQA_\w+)\s+({_INT})\s*$")
_ENUM = re.compile(r"enum\s*\{([^{}]*)\}\s*;")
_MEMBER = re.compile(rf"\s*(EAVQA_\w+)\s*=\s*({_INT})\s*$")
_STRUCT = re.compile(r"typedef\s+struct\s*\{([^{}]*)\}\s*(eavqa_\w+_t)\s*;")
_FIELD = re.compile(r"\s*(?:const\s+)?(\w+)\b(.*)$", re.S)
_DECLARATOR = re.compile(r"\s*(\*?)\s*([A-Za-z_]\w*)\s*(?:\[\s*(\d+)\s*\])?\s*$")
_PROTO = re.compile(r"(const\s+char\s*\*|int64_t\b|int\b)\s*(eavqa_\w+)\s*\(([^()]*)\)\s*;")
_PARAM = re.compile(r"\s*(?:const\s+)?(\w+)(\s*\*\s*|\s+)([A-Za-z_]\w*)\s*$")

SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float}
_KEYWORDS = {"const", "struct", "union", "enum", "unsigned", "signed", "long", "short", "volatile", "restrict"}


def parse(text: str, header: str) -> Header:
    def bad(what, where):
        return AbiError(f"{header}: {what}: {' '.join(where.split())[:200]!r}")

    def decl(base, pointer, name, count, where):
        if base in _KEYWORDS or name in _KEYWORDS or (not pointer and base not in SCALARS):
            raise bad(f"unsupported type {base!r}", where)
        return Decl(base, pointer, name, count)

    constants, structs, functions = {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    lines = []
    for line in text.split("\n"):
        if line.lstrip().startswith("#"):
            if line.rstrip().endswith("\\"):
                raise bad("continued preprocessor line", line)
            m = _DEFINE.match(line.strip())
            if m:
                constants[m.group(1)] = int(m.group(2), 0)
            line = ""
        lines.append(line)
    text = "\n".join(lines)

    pos, wrapped = 0, False
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            break
        rest = text[pos:]
        stmt = rest[:rest.find(";") + 1] or rest
        m = re.match(r'extern\s+"C"\s*\{', rest)
        if m and not wrapped:
            wrapped, pos = True, pos + m.end()
            continue
        if rest[0] == "}" and wrapped:
            wrapped, pos = False, pos + 1
            continue
        if rest.startswith("enum"):
            m = _ENUM.match(rest)
            if not m:
                raise bad("unsupported enum", stmt)
            for member in m.group(1).split(","):
                mm = _MEMBER.match(member)
                if not mm:
                    raise bad("enum member that is not EAVQA_NAME = <integer>", member or stmt)
                constants[mm.group(1)] = int(mm.group(2), 0)
        elif rest.startswith("typedef"):
            m = _STRUCT.match(rest)
            if not m:
                raise bad("unsupported typedef", rest[:rest.find("}") + 1] or stmt)
            fields = []
            for field in m.group(1).split(";"):
                if not field.strip():
                    continue
                f = _FIELD.match(field)
                declarators = [_DECLARATOR.match(d) for d in f.group(2).split(",")] if f else [None]
                if not all(declarators):
                    raise bad("unsupported struct field", field)
                fields += [decl(f.group(1), bool(d.group(1)), d.group(2), int(d.group(3) or 0), field) for d in declarators]
            structs[m.group(2)] = fields
        else:
            m = _PROTO.match(rest)
            if not m:
                raise bad("unsupported declaration", stmt)
            ret = Decl("char" if "char" in m.group(1) else m.group(1), "char" in m.group(1), "")
            params = []
            if m.group(3).strip() != "void":
                for p in m.group(3).split(","):
                    pm = _PARAM.match(p)
                    if not pm:
                        raise bad("unsupported parameter", p or stmt)
                    params.append(decl(pm.group(1), "*" in pm.group(2), pm.group(3), 0, p))
            functions[m.group(2)] = (ret, params)
        pos += m.end()
    if wrapped:
        raise bad('unclosed extern "C" {', text[-80:])
    return Header(constants, structs, functions)


def merge(headers) -> Header:
    """One table of several parsed headers; a name declared twice is an error."""
    out = Header({}, {}, {})
    for h in headers:
        for dst, src in zip(out, h):
            dup = set(dst) & set(src)
            if dup:
                raise AbiError(f"declared twice: {sorted(dup)}")
            dst.update(src)
    return out


class Bound(NamedTuple):
    structs: dict       # typedef name -> ctypes.Structure subclass
    argtypes: dict      # function -> [ctype]
    restypes: dict      # function -> ctype
    params: dict        # function -> (parameter name, ...)


def bind(abi: Header, overrides: dict) -> Bound:
    """The ctypes form of ``abi``.  Scalars by ``SCALARS``; a pointer to an ABI struct is ``POINTER(Struct)`` (a host table or argument
    block, passed with ``byref`` or as an array), any other pointer ``c_void_p`` (an address handed over as an int, ``None`` = NULL); a
    ``const char*`` return is ``c_char_p``.  ``overrides`` replaces single results: ``"<type>*"`` for every pointer to that type,
    ``"<function>.<parameter>"`` for one parameter."""
    structs = {}

    def ctype(d: Decl, fn=None):
        if d.pointer:
            if d.base.startswith("eavqa_") and d.base not in structs:
                raise AbiError(f"pointer to {d.base}, which no header defines (or defines only further down)")
            hit = overrides.get(f"{fn}.{d.name}") or overrides.get(d.base + "*")
            t = hit or (C.POINTER(structs[d.base]) if d.base in structs else C.c_void_p)
        else:
            t = SCALARS[d.base]
        return t * d.count if d.count else t

    for name, fields in abi.structs.items():
        structs[name] = type(name, (C.Structure,), {"_fields_": [(d.name, ctype(d)) for d in fields], "__doc__": f"``{name}``."})
    used = set()
    argtypes = {fn: [ctype(d, fn) for d in params] for fn, (_, params) in abi.functions.items()}
    for fn, (_, params) in abi.functions.items():
        used |= {f"{fn}.{d.name}" for d in params} | {d.base + "*" for d in params if d.pointer}
    if set(overrides) - used:
        raise AbiError(f"override of something the headers do not declare: {sorted(set(overrides) - used)}")
    restypes = {fn: C.c_char_p if ret.pointer else SCALARS[ret.base] for fn, (ret, _) in abi.functions.items()}
    params = {fn: tuple(d.name for d in ps) for fn, (_, ps) in abi.functions.items()}
    return Bound(structs, argtypes, restypes, params)
