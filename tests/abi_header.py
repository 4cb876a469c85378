"""A small parser of include/mvsgi.h for the tests: the header is the single source of the C ABI, and mvs_gi_amd/_lib.py::SIGNATURES
and the constants of mvs_gi_amd/hip_ops.py are hand-kept copies of it.

parse(text) -> Header with
  prototypes   {name: Proto(restype, argtypes, launching)} in ctypes terms:
                 any pointer or array parameter and mvsgi_stream_t -> c_void_p; int, unsigned, long long, float, double, size_t -> their
                 ctypes; a `const char*` return -> c_char_p; `(void)` -> no parameters
  launching    a prototype with an mvsgi_stream_t parameter (it enqueues work on a stream)
  defines      {NAME: int} for every `#define MVSGI_<NAME> <integer>`

Comments and preprocessor lines are stripped; every statement that is left must be one of: the `extern "C"` braces, the typedef of
mvsgi_stream_t, or a prototype whose every type is in the mapping.  Anything else raises HeaderError: a declaration is never skipped.
"""
from __future__ import annotations

import os
import re
from collections import namedtuple
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_uint, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mvsgi.h")

Proto = namedtuple("Proto", "restype argtypes launching")
Header = namedtuple("Header", "prototypes defines")

STREAM = "mvsgi_stream_t"
# scalar types by value, longest token sequence first
_SCALARS = ((("long", "long"), c_longlong), (("unsigned", "int"), c_uint), (("unsigned",), c_uint), (("int",), c_int),
            (("float",), c_float), (("double",), c_double), (("size_t",), c_size_t), ((STREAM,), c_void_p))
_IDENT = re.compile(r"[A-Za-z_][A-Za-z0-9_]*\Z")
_PROTO = re.compile(r"(?P<ret>[A-Za-z_][A-Za-z0-9_\s\*]*?)\s*\b(?P<name>[A-Za-z_][A-Za-z0-9_]*)\s*\((?P<params>[^()]*)\)\Z", re.S)
_INT = re.compile(r"(0[xX][0-9a-fA-F]+|\d+)[uUlL]*\Z")


# ctypes names an alias by its target (c_longlong is c_long on LP64): messages use the names the binding writes
_NAMES = {c_int: "c_int", c_uint: "c_uint", c_longlong: "c_longlong", c_float: "c_float", c_double: "c_double", c_size_t: "c_size_t",
          c_void_p: "c_void_p", c_char_p: "c_char_p"}


def type_name(t) -> str:
    return _NAMES.get(t) or getattr(t, "__name__", repr(t))


class HeaderError(ValueError):
    """A declaration the parser cannot classify."""


def strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _scalar(tokens, what: str):
    """tokens of a by-value type, optionally followed by ONE parameter name -> (ctypes type, is the stream)"""
    for seq, ct in _SCALARS:
        n = len(seq)
        if tuple(tokens[:n]) == seq:
            rest = tokens[n:]
            if len(rest) > 1 or (rest and (not _IDENT.match(rest[0]) or rest[0] in ("int", "long", "unsigned", "float", "double", "char", "short", "signed"))):
                break
            return ct, seq == (STREAM,)
    raise HeaderError(f"{what}: cannot classify the type {' '.join(tokens)!r}")


def _param(decl: str, what: str):
    if "*" in decl or "[" in decl:
        if "(" in decl:
            raise HeaderError(f"{what}: function pointers are not part of this ABI ({decl!r})")
        return c_void_p, False
    tokens = [t for t in decl.split() if t != "const"]
    if not tokens:
        raise HeaderError(f"{what}: empty parameter")
    return _scalar(tokens, what)


def _return(decl: str, what: str):
    tokens = decl.replace("*", " * ").split()
    if tokens == ["const", "char", "*"]:
        return c_char_p
    if "*" in tokens:
        raise HeaderError(f"{what}: cannot classify the return type {decl!r}")
    tokens = tuple(t for t in tokens if t != "const")
    for seq, ct in _SCALARS:
        if tokens == seq and seq != (STREAM,):
            return ct
    raise HeaderError(f"{what}: cannot classify the return type {decl!r}")


def parse(text: str) -> Header:
    text = strip_comments(text).replace("\\\n", " ")
    defines, body = {}, []
    for line in text.split("\n"):
        s = line.strip()
        if s.startswith("#"):
            m = re.match(r"#\s*define\s+MVSGI_([A-Za-z0-9_]+)\s*(.*)\Z", s)
            if m:
                name, val = m.group(1), m.group(2).strip()
                if "(" in name or val.startswith("("):
                    raise HeaderError(f"#define MVSGI_{name}: function-like or parenthesised macros are not part of this ABI")
                if val:
                    if not _INT.match(val):
                        raise HeaderError(f"#define MVSGI_{name}: {val!r} is not an integer literal")
                    defines[name] = int(re.sub(r"[uUlL]+\Z", "", val), 0)
                elif name != "H":                                   # the include guard is the one define without a value
                    raise HeaderError(f"#define MVSGI_{name}: no value")
            continue
        body.append(line)
    text = "\n".join(body)
    text, n_open = re.subn(r'extern\s+"C"\s*\{', " ", text)
    if n_open:
        if n_open != 1 or text.count("}") != 1 or text.rstrip()[-1:] != "}":
            raise HeaderError('unbalanced extern "C" block')
        text = text.rstrip()[:-1]
    if "{" in text or "}" in text:
        raise HeaderError("braces outside the extern \"C\" block: definitions are not part of this ABI")
    prototypes = {}
    statements = text.split(";")
    if statements[-1].strip():
        raise HeaderError(f"unterminated declaration: {statements[-1].strip()[:80]!r}")
    for st in statements[:-1]:
        st = " ".join(st.split())
        if not st:
            continue
        if st.startswith("typedef"):
            if st.replace(" ", "") != f"typedefvoid*{STREAM}":
                raise HeaderError(f"unknown typedef: {st!r}")
            continue
        m = _PROTO.match(st)
        if not m:
            raise HeaderError(f"not a prototype: {st[:120]!r}")
        name = m.group("name")
        if name in prototypes:
            raise HeaderError(f"{name}: declared twice")
        restype = _return(m.group("ret"), name)
        params = m.group("params").strip()
        args, launching = [], False
        if params != "void":
            if not params:
                raise HeaderError(f"{name}: an empty parameter list declares nothing in C; write (void)")
            for i, p in enumerate(params.split(",")):
                ct, stream = _param(p.strip(), f"{name} parameter {i}")
                args.append(ct)
                launching |= stream
        prototypes[name] = Proto(restype, args, launching)
    return Header(prototypes, defines)


def load(path: str = HEADER) -> Header:
    with open(path) as f:
        return parse(f.read())


def launching_symbols(path: str = HEADER) -> set:
    return {n for n, p in load(path).prototypes.items() if p.launching}


def first_difference(name: str, proto: Proto, signature) -> str:
    """'' when `signature` = (restype, argtypes) of a ctypes table equals the parsed prototype, else the symbol and the first slot that
    differs."""
    restype, argtypes = signature
    if restype is not proto.restype:
        return f"{name}: return type {type_name(restype)}, the header says {type_name(proto.restype)}"
    for i, (a, b) in enumerate(zip(argtypes, proto.argtypes)):
        if a is not b:
            return f"{name}: argument {i} is {type_name(a)}, the header says {type_name(b)}"
    if len(argtypes) != len(proto.argtypes):
        return f"{name}: {len(argtypes)} arguments, the header says {len(proto.argtypes)} (first unmatched slot {min(len(argtypes), len(proto.argtypes))})"
    return ""
