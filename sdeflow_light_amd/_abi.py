"""Strict reader of include/msgm_hip.h: the header is the single source of the ctypes binding.

``parse(text)`` returns an ``Abi`` with every ``msgm_*`` prototype, every ``typedef struct { ... } msgm_*_t;`` (as field
lists and as ``ctypes.Structure`` classes) and every integer constant (enumerators and ``#define MSGM_* <integer>``).
Anything it does not understand raises ``MsgmError`` with the header's line number: a token that is skipped or guessed
would shift the arguments of a launch.  ``load()`` parses the repository's header once per process.

Pointer rule (the header's naming convention): a pointer to a scalar or to void is an address (``c_void_p``); so is a
pointer to an ``msgm_*_t`` whose parameter name ends in ``_dev`` (a device table); any other pointer to an ``msgm_*_t``
is ``POINTER(<its Structure>)``, so callers pass the instance (or ``byref``) and an int is refused.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
from typing import NamedTuple

HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "msgm_hip.h")


class MsgmError(RuntimeError):
    pass


SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32,
           "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "msgm_stream_t": C.c_void_p}


class Abi(NamedTuple):
    functions: dict    # name -> (restype, [(param_name, ctype)])
    structs: dict      # msgm_foo_t -> [(field, ctype)], in declaration order
    classes: dict      # msgm_foo_t -> the ctypes.Structure class FooT with those fields
    constants: dict    # enumerator or #define name -> int


_INT = r"[-+]?(?:0[xX][0-9a-fA-F]+|\d+)"
_WS = re.compile(r"\s*")
_ITEMS = [(kind, re.compile(rx)) for kind, rx in (
    ("extern", r'extern\s+"C"\s*\{'),
    ("close", r"\}"),
    ("stream", r"typedef\s+void\s*\*\s*msgm_stream_t\s*;"),
    ("enum", r"enum\s*\{([^{}]*)\}\s*;"),
    ("struct", r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;"),
    ("proto", r"([\w\s*]+?)\b(msgm_\w+)\s*\(([^(){};]*)\)\s*;"))]
_ARRAY = r"(?:\s*\[\s*(\d+)\s*\])?"
_DECL = re.compile(r"(?:const\s+)?(\w+)(?:\s*(\*)\s*|\s+)(\w+)" + _ARRAY)     # [const] type [*] name [[n]]
_MORE = re.compile(r"(\w+)" + _ARRAY)                                         # a further declarator of the same statement
_RET = re.compile(r"(const\s+)?(\w+)\s*(\*?)")
_ENUMERATOR = re.compile(rf"(\w+)(?:\s*=\s*({_INT}))?")
_DEFINE = re.compile(r"\s*#\s*define\s+(MSGM_\w+)(.*)")


def parse(text: str) -> Abi:
    fns, structs, classes, consts = {}, {}, {}, {}

    def fail(pos, msg):
        raise MsgmError(f"msgm_hip.h:{text.count(chr(10), 0, pos) + 1}: {msg}")

    def add(table, name, value, pos):
        if name in table:
            fail(pos, f"duplicate name {name!r}")
        table[name] = value

    def ctype(base, star, name, pos, field=False):
        if not star:
            if base not in SCALARS:
                fail(pos, f"unknown type {base!r}")
            return SCALARS[base]
        if base in SCALARS or base == "void":
            return C.c_void_p
        if base not in classes:
            fail(pos, f"pointer to {base!r}, which is neither a scalar nor a struct declared above")
        return C.c_void_p if field or name.endswith("_dev") else C.POINTER(classes[base])

    def declarations(body, pos, field):
        """[(name, ctype)] of a parameter list, or of a struct body (``field``: several declarators per statement)."""
        out = {}
        for part in body.split(";" if field else ","):
            at, pos = pos + len(part) - len(part.lstrip()), pos + len(part) + 1
            if field and not part.strip():
                continue                                      # what follows the last ';' of a struct body
            first, *more = [s.strip() for s in part.split(",")] if field else [part.strip()]
            m = _DECL.fullmatch(first)
            if not m or (m.group(4) and not field) or (more and m.group(2)):
                fail(at, f"cannot parse the declaration {part.strip()!r}")
            base, star, name, dim = m.groups()
            t = ctype(base, star, name, at, field)
            add(out, name, t * int(dim) if dim else t, at)
            for d in more:
                m = _MORE.fullmatch(d)
                if not m:
                    fail(at, f"cannot parse the declarator {d!r}")
                add(out, m.group(1), t * int(m.group(2)) if m.group(2) else t, at)
        return list(out.items())

    # comments and preprocessor lines become blanks, their newlines stay: positions still give the header's line numbers
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)
    for m in re.finditer(r"^[ \t]*#[^\n]*", text, flags=re.M):
        if m.group().rstrip().endswith("\\"):
            fail(m.start(), "continued preprocessor line")
        d = _DEFINE.fullmatch(m.group())
        if d and d.group(2).strip():                          # a bare #define MSGM_X is the include guard
            if not re.fullmatch(_INT, d.group(2).strip()):
                fail(m.start(), f"#define {d.group(1)} is not an integer")
            add(consts, d.group(1), int(d.group(2).strip(), 0), m.start())
    text = re.sub(r"^[ \t]*#[^\n]*", lambda m: " " * len(m.group()), text, flags=re.M)

    pos, extern_open = _WS.match(text).end(), False
    while pos < len(text):
        kind, m = next(((k, m) for k, rx in _ITEMS for m in [rx.match(text, pos)] if m), (None, None))
        if kind is None or (kind == "close" and not extern_open):
            fail(pos, f"cannot parse {text[pos:pos + 60].splitlines()[0]!r}")
        if kind in ("extern", "close"):
            extern_open = kind == "extern"
        elif kind == "enum":
            value = 0
            for e in m.group(1).split(","):
                em = _ENUMERATOR.fullmatch(e.strip())
                if not em:
                    fail(pos, f"cannot parse the enumerator {e.strip()!r}")
                value = int(em.group(2), 0) if em.group(2) else value
                add(consts, em.group(1), value, pos)
                value += 1
        elif kind == "struct":
            name = m.group(2)
            if not re.fullmatch(r"msgm_\w+_t", name):
                fail(pos, f"struct name {name!r} is not msgm_*_t")
            add(structs, name, declarations(m.group(1), m.start(1), True), pos)
            # msgm_foo_bar_t -> FooBarT
            classes[name] = type("".join(p.capitalize() for p in name.split("_")[1:]), (C.Structure,),
                                 {"_fields_": structs[name], "__doc__": f"{name} (include/msgm_hip.h)."})
        elif kind == "proto":
            r = _RET.fullmatch(m.group(1).strip())
            if not r or (r.group(3) and not (r.group(1) and r.group(2) == "char")):
                fail(pos, f"unknown return type {m.group(1).strip()!r}")
            res = C.c_char_p if r.group(3) else ctype(r.group(2), "", "", pos)
            params = [] if m.group(3).strip() == "void" else declarations(m.group(3), m.start(3), False)
            add(fns, m.group(2), (res, params), pos)
        pos = _WS.match(text, m.end()).end()
    if extern_open:
        fail(len(text), 'extern "C" { is not closed')
    return Abi(fns, structs, classes, consts)


@functools.lru_cache(maxsize=None)
def load() -> Abi:
    """The repository's header, read and parsed once per process."""
    with open(HEADER_PATH) as f:
        return parse(f.read())
