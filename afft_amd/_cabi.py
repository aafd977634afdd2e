"""Reader of include/afft_hip.h, the single statement of the C ABI: its constants, structs and prototypes as ctypes objects.

The grammar is the one written at the top of the header.  Anything outside it raises HeaderError with the line: the reader
never guesses, because a wrong guess is a wrong kernel argument.  Type mapping, one rule for fields, arguments and results:
int / int32_t / int64_t / uint32_t / float -> the ctypes scalar; pointer to a struct of the header -> POINTER(struct); pointer to
pointer -> POINTER(c_void_p); any other pointer -> c_void_p; a `const char*` result -> c_char_p.
"""
from __future__ import annotations

import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "afft_hip.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float}
_POINTEES = set(SCALARS) | {"void", "uint8_t"}
_FRAME = re.compile(r"#\s*(ifndef\s+\w+|define\s+\w+|include\s*<stdint\.h>|endif)\s*")      # the include guard and its include
_ITEM = re.compile(r"""\s*(?: enum\s*\{(?P<enum>[^{};]*)\}\s*;
                            | typedef\s+struct\s*(?P<tag>\w*)\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;
                            | (?P<ret>[\w\s*]+?)\b(?P<fn>afft_\w+)\s*\((?P<args>[^(){};]*)\)\s*; )""", re.X)


class HeaderError(ValueError):
    pass


def _blank(m):
    return " " + "\n" * m.group(0).count("\n")        # line numbers survive


def parse(text: str):
    """(consts, structs, protos) of a header: {AFFT_NAME: int}, {name_t: Structure class} in declaration order,
    {afft_name: (argtypes, restype)}."""
    consts, structs, protos, tags, pending = {}, {}, {}, {}, {}

    def fail(at, what):
        raise HeaderError(f"afft_hip.h:{text.count(chr(10), 0, at) + 1}: {what}")

    def ctype(base, stars, at, ret=False):
        if base.startswith("struct "):
            tag = base.split()[1]
            if tag not in tags:                      # a struct defined further down: legal behind a pointer only
                tags[tag], pending[tag] = type(tag, (C.Structure,), {}), at
            cls = tags[tag]
        else:
            cls = structs.get(base)
        if stars == 0 and base in SCALARS:
            return SCALARS[base]
        if stars == 0 and cls is not None and hasattr(cls, "_fields_"):
            return cls
        if stars == 1 and cls is not None:
            return C.POINTER(cls)
        if stars == 1 and base == "char" and ret:
            return C.c_char_p
        if stars == 1 and base in _POINTEES:
            return C.c_void_p
        if stars == 2 and (cls is not None or base in _POINTEES):
            return C.POINTER(C.c_void_p)
        fail(at, f"type {base + '*' * stars!r} is outside the header's grammar")

    def decl(s, at, ret=False):
        """`[const] type [*..] a, b, c` -> [(name, ctypes type)]"""
        m = re.fullmatch(r"\s*(struct\s+\w+|\w+)\b(.*)", re.sub(r"\bconst\b", " ", s), re.S)
        out = []
        for d in m.group(2).split(",") if m else [""]:
            dm = re.fullmatch(r"\s*((?:\*\s*)*)(\w+)\s*", d)
            if not dm:
                fail(at, f"cannot read the declaration {' '.join(s.split())!r}")
            out.append((dm.group(2), ctype(" ".join(m.group(1).split()), dm.group(1).count("*"), at, ret)))
        return out

    text = re.sub(r"/\*.*?\*/|//[^\n]*", _blank, text, flags=re.S)
    text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif", _blank, text, flags=re.S)        # extern "C" { and its }
    for m in re.finditer(r"^[ \t]*#[^\n]*", text, re.M):
        c = re.fullmatch(r"\s*#\s*define\s+(AFFT_\w+)\s+(-?\d+)\s*", m.group(0))
        if c:
            consts[c.group(1)] = int(c.group(2))
        elif not _FRAME.fullmatch(m.group(0).strip()):
            fail(m.start(), f"cannot read the directive {m.group(0).strip()!r}")
    text = re.sub(r"^[ \t]*#[^\n]*", _blank, text, flags=re.M)

    pos = 0
    while text[pos:].strip():
        m = _ITEM.match(text, pos)
        if not m:
            at = pos + len(text[pos:]) - len(text[pos:].lstrip())
            fail(at, f"cannot read {text[at:].splitlines()[0]!r}")
        pos = m.end()
        if m["enum"] is not None:
            for e in filter(str.strip, m["enum"].split(",")):
                c = re.fullmatch(r"\s*(AFFT_\w+)\s*=\s*(-?\d+)\s*", e)
                if not c:
                    fail(m.start("enum"), f"cannot read the enumerator {e.strip()!r}")
                consts[c.group(1)] = int(c.group(2))
        elif m["struct"] is not None:
            at, fields = m.start("body"), []
            *decls, tail = m["body"].split(";")
            if tail.strip():
                fail(at + len(m["body"]) - len(tail), f"field without ';': {tail.strip()!r}")
            for d in decls:
                fields += decl(d, at + len(d) - len(d.lstrip()))
                at += len(d) + 1
            cls = type(m["struct"], (C.Structure,), {})
            if m["tag"]:
                cls = tags.setdefault(m["tag"], cls)
                pending.pop(m["tag"], None)
            cls._fields_ = fields
            structs[m["struct"]] = cls
        else:
            args = [] if m["args"].strip() == "void" else [decl(a, m.start("args"))[0][1] for a in m["args"].split(",")]
            protos[m["fn"]] = (args, decl(m["ret"] + " result", m.start("ret"), ret=True)[0][1])
    for tag, at in pending.items():
        fail(at, f"struct {tag} is used but never defined")
    return consts, structs, protos


with open(HEADER, "rb") as _f:
    TEXT = _f.read()                     # the bytes the binding was derived from (_lib.lib() compares them with the library's copy)
consts, structs, protos = parse(TEXT.decode())
