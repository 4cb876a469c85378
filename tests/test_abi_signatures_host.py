"""CPU: include/mvsgi.h is the single source of the C ABI.  The ctypes table (mvs_gi_amd/_lib.py::SIGNATURES) and the constants
mvs_gi_amd/hip_ops.py restates are compared with the parsed header slot by slot; the compiler's own check of the definitions stays
in place as long as every file that defines an entry point includes the header.  tests/abi_header.py is the parser; its self-test
below shows that each kind of mismatch the functional tests would miss is caught."""
import glob
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_uint, c_void_p

import pytest

import abi_header
from mvs_gi_amd import _lib, hip_ops

ROOT = abi_header.ROOT
HEADER = abi_header.load()


def test_header_parses_completely():
    # every `mvsgi_xxx(` of the comment-free header is a parsed prototype: nothing was skipped
    text = abi_header.strip_comments(open(abi_header.HEADER).read())
    text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))
    named = set(re.findall(r"\b(mvsgi_[a-z0-9_]+)\s*\(", text))
    assert named == set(HEADER.prototypes)
    assert len(named) >= 116
    assert HEADER.prototypes["mvsgi_conv3d_f32"].launching and not HEADER.prototypes["mvsgi_conv3d_up2_poly_plan_fmt"].launching
    assert not HEADER.prototypes["mvsgi_abi_version"].argtypes


def test_signature_table_equals_the_header():
    assert sorted(_lib.SIGNATURES) == sorted(HEADER.prototypes), "ctypes SIGNATURES and the header declare different symbols"
    bad = [d for d in (abi_header.first_difference(n, p, _lib.SIGNATURES[n]) for n, p in sorted(HEADER.prototypes.items())) if d]
    assert not bad, "ctypes SIGNATURES out of step with include/mvsgi.h:\n  " + "\n  ".join(bad)


# the defines without a same-named constant in hip_ops, and where their copy lives instead
ELSEWHERE = {"ABI_VERSION": lambda: _lib.ABI_VERSION,
             "METRICS_RANGE_FRAME": lambda: hip_ops.METRICS_RANGE_SCOPES["frame"],
             "METRICS_RANGE_BATCH": lambda: hip_ops.METRICS_RANGE_SCOPES["batch"]}


def test_constants_equal_the_header():
    d = HEADER.defines
    for fam in ("CONV_AUTO", "CONV_DIRECT", "CONV_MFMA", "CONV_BF16X3", "CONV_BF16X3_C16", "CONV_BF16X3_V32", "CONV_BF16X3_D32", "CONV_F16",
                "SPLIT_F16", "SAT_SWEEP", "SAT_SPLIT", "SAT_WINO", "SA_AUTO", "SA_PIXEL", "SA_BAND", "METRICS_MASK_NONE",
                "METRICS_MASK_TENSOR", "METRICS_MASK_RANGE", "METRICS_RANGE_FRAME", "METRICS_RANGE_BATCH", "LOSSES_P_NONE", "LOSSES_P_GIVEN",
                "LOSSES_P_FUSED", "LOSSES_VOL_NONE", "LOSSES_VOL_PIXEL", "LOSSES_VOL_VOLUME", "LOSSES_PX_NONE", "LOSSES_PX_TENSOR",
                "LOSSES_PX_LABEL_MAX", "ABI_VERSION"):
        assert fam in d, f"MVSGI_{fam} is no longer defined in the header"
    bad, unmatched = [], []
    for name, value in sorted(d.items()):
        if name in ELSEWHERE:
            got = ELSEWHERE[name]()
        elif hasattr(hip_ops, name):
            got = getattr(hip_ops, name)
        else:
            unmatched.append(name)
            continue
        if got != value or isinstance(got, bool):
            bad.append(f"MVSGI_{name} = {value} in the header, {got!r} in Python")
    assert not bad, "\n".join(bad)
    assert not unmatched, f"defines without a Python constant (add it to hip_ops or to ELSEWHERE): {unmatched}"
    assert set(hip_ops.METRICS_RANGE_SCOPES) == {"frame", "batch"}


def test_every_defining_file_includes_the_header():
    """A definition that does not see its prototype is not checked against it by the compiler (extern "C": no mangling, so a
    mismatch links)."""
    csrc = os.path.join(ROOT, "mvs_gi_amd", "csrc")
    defining, defined = [], set()
    for path in sorted(glob.glob(os.path.join(csrc, "*"))):
        if not os.path.isfile(path) or not path.endswith((".hip", ".cpp", ".hpp", ".inc", ".h", ".cc", ".cu")):
            continue
        src = abi_header.strip_comments(open(path).read())
        # a definition: `mvsgi_xxx(parameters) {`, behind `extern "C"` on its own line or inside an `extern "C" { ... }` block
        names = re.findall(r'\b(mvsgi_[a-z0-9_]+)\s*\([^;{}()]*\)\s*\{', src)
        if not names or not re.search(r'extern\s+"C"', src):
            continue
        defining.append(os.path.basename(path))
        defined |= set(names)
        assert re.search(r'#\s*include\s+"common\.hpp"', src) or re.search(r'#\s*include\s+["<][^">]*mvsgi\.h[">]', src), \
            f"{os.path.basename(path)} defines {names[0]} without including common.hpp or mvsgi.h"
    common = abi_header.strip_comments(open(os.path.join(csrc, "common.hpp")).read())
    assert re.search(r'#\s*include\s+"[^"]*include/mvsgi\.h"', common), "common.hpp no longer includes include/mvsgi.h"
    assert len(defining) >= 20
    assert defined == set(HEADER.prototypes), f"declared but not defined with extern \"C\": {sorted(set(HEADER.prototypes) - defined)}; " \
                                              f"defined but not declared: {sorted(defined - set(HEADER.prototypes))}"


# ---- the parser on synthetic declarations: each kind of mismatch is caught ----
SYNTH = """
/* a comment with a fake(prototype int x); inside */
#ifndef MVSGI_H
#define MVSGI_H
#define MVSGI_ALPHA 3   /* three */
#define MVSGI_FLAG  0x100
#define MVSGI_BIT   4u
#ifdef __cplusplus
extern "C" {
#endif
typedef void* mvsgi_stream_t;
int mvsgi_version(void);
const char* mvsgi_text(void);
size_t mvsgi_bytes(long long B, int H,
                   int W);
int mvsgi_big(const float* x, unsigned char* m, long long n, mvsgi_stream_t stream);   // n: 64 bits
int mvsgi_scaled(const float* x, float* y, int H, double scale, float post_div,
                 int variant /* MVSGI_ALPHA */,
                 mvsgi_stream_t stream);
int mvsgi_tables(const float* const* gates_host, const float lo[4], unsigned* flags, unsigned count, int n);
#ifdef __cplusplus
}
#endif
#endif
"""
P = c_void_p
LL, SZ = "c_longlong", "c_size_t"
SYNTH_TABLE = {
    "mvsgi_version": (c_int, []),
    "mvsgi_text": (c_char_p, []),
    "mvsgi_bytes": (c_size_t, [c_longlong, c_int, c_int]),
    "mvsgi_big": (c_int, [P, P, c_longlong, P]),
    "mvsgi_scaled": (c_int, [P, P, c_int, c_double, c_float, c_int, P]),
    "mvsgi_tables": (c_int, [P, P, P, c_uint, c_int]),
}


def _diffs(table):
    h = abi_header.parse(SYNTH)
    assert sorted(h.prototypes) == sorted(table)
    return [d for d in (abi_header.first_difference(n, p, table[n]) for n, p in sorted(h.prototypes.items())) if d]


def test_parser_self_test_agrees_on_a_correct_table():
    h = abi_header.parse(SYNTH)
    assert h.defines == {"ALPHA": 3, "FLAG": 0x100, "BIT": 4}
    assert {n for n, p in h.prototypes.items() if p.launching} == {"mvsgi_big", "mvsgi_scaled"}
    assert _diffs(SYNTH_TABLE) == []


@pytest.mark.parametrize("symbol,signature,slot", [
    ("mvsgi_big", (c_int, [P, P, c_int, P]), f"argument 2 is c_int, the header says {LL}"),            # long long against int
    ("mvsgi_bytes", (c_size_t, [c_int, c_int, c_int]), f"argument 0 is c_int, the header says {LL}"),
    ("mvsgi_scaled", (c_int, [P, P, c_int, c_float, c_float, c_int, P]), "argument 3 is c_float, the header says c_double"),   # double against float
    ("mvsgi_scaled", (c_int, [P, P, c_int, c_double, c_float, c_int]), "6 arguments, the header says 7 (first unmatched slot 6)"),    # a dropped trailing argument
    ("mvsgi_scaled", (c_int, [P, P, c_int, c_double, c_float, P]), "argument 5 is c_void_p, the header says c_int"),   # a dropped middle one
    ("mvsgi_version", (c_int, [c_int]), "1 arguments, the header says 0 (first unmatched slot 0)"),                                    # (void) has no parameters
    ("mvsgi_text", (c_int, []), "return type c_int, the header says c_char_p"),
    ("mvsgi_bytes", (c_int, [c_longlong, c_int, c_int]), f"return type c_int, the header says {SZ}"),
    ("mvsgi_tables", (c_int, [P, P, P, c_int, c_int]), "argument 3 is c_int, the header says c_uint"),
])
def test_parser_self_test_catches(symbol, signature, slot):
    got = _diffs(dict(SYNTH_TABLE, **{symbol: signature}))
    assert got == [f"{symbol}: {slot}"]


@pytest.mark.parametrize("decl", [
    "int mvsgi_f(short n);",                               # a type outside the mapping
    "int mvsgi_f(mvsgi_handle_t h);",                      # an unknown typedef name
    "int mvsgi_f(int a b);",                               # two names
    "void* mvsgi_f(int n);",                               # a pointer return that is not const char*
    "void mvsgi_f(int n);",                                # a void return
    "int mvsgi_f();",                                      # no prototype in C
    "int mvsgi_f(int (*cb)(int));",                        # a function pointer
    "typedef int mvsgi_status_t;",                         # a typedef the parser does not know
    "struct mvsgi_s { int a; };",                          # a definition
    "int mvsgi_f(int n)",                                  # unterminated
    "static inline int mvsgi_f(int n) { return n; }",      # an inline definition
    "#define MVSGI_X (1 << 3)\n",                          # a define that is not an integer literal
    "#define MVSGI_X\n",                                   # a define without a value
    "int mvsgi_f(int n); int mvsgi_f(long long n);",       # declared twice
])
def test_parser_raises_on_what_it_cannot_classify(decl):
    with pytest.raises(abi_header.HeaderError):
        abi_header.parse(decl)
