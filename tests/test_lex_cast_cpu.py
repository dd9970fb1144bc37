"""The lexical casts (RDFGPU_EX_CAST_STRING / RDFGPU_EX_CAST_LEX) without a GPU: the builder's lowering and encodings, the compile
refusals and the parsers themselves as stand-alone host programs (the parsers' header is plain C++ without HIP: the text the device
runs), the generated table of powers of five."""
import os
import re
import subprocess
import sys

import pytest

from rdf_fusion_amd import abi
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, EBV
import lex_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rdf-fusion_amd", "csrc")
FUZZ_ROWS, FUZZ_SEED = 1_200_000, 20261019


def test_abi_values_and_the_header_agree():
    assert abi.EX_CAST == 45 and abi.EX_CAST_STRING == 46 and abi.EX_CAST_LEX == 47
    h = open(os.path.join(ROOT, "include", "rdfgpu.h")).read()
    assert re.search(r"RDFGPU_EX_CAST = 45,", h) and re.search(r"RDFGPU_EX_CAST_STRING = 46,", h) and re.search(r"RDFGPU_EX_CAST_LEX = 47,", h)
    assert h.index("RDFGPU_EX_CAST_LEX = 47") < h.index("RDFGPU_EX__COUNT")


def test_builder_lowering_and_encodings():
    a = ENC_TV(col(2))
    s = P.xsd_string(a)
    assert s.nodes == [(abi.EX_COLUMN, 0, 0, 2, 0, 0), (abi.EX_CAST_STRING, 0, 0, 0, 0, 0)]      # the id form: no ENC_TV
    assert P.CAST_LEX(s, abi.TV_FLOAT).nodes[-1] == (abi.EX_CAST_LEX, 0, 0, abi.TV_FLOAT, 0, 0)
    helpers = [(P.xsd_boolean, abi.TV_BOOLEAN), (P.xsd_int, abi.TV_INT), (P.xsd_integer, abi.TV_INTEGER), (P.xsd_decimal, abi.TV_DECIMAL),
               (P.xsd_float, abi.TV_FLOAT), (P.xsd_double, abi.TV_DOUBLE)]
    for fn, tag in helpers:
        assert fn(a).nodes == P.CAST(a, tag).nodes and fn(a, lexical=False).nodes == P.CAST(a, tag).nodes      # the default is unchanged
        assert fn(s, lexical=True).nodes == s.nodes + [(abi.EX_CAST_LEX, 0, 0, tag, 0, 0)]
    for bad in (col(2), ENC_TV(P.lit_id(5)), P.STR(col(2)), P.xsd_float(a), P.lit_str("1.5")):
        with pytest.raises(ValueError):
            P.xsd_string(bad)


def test_the_plan_prints_as_the_reference_prints_it():
    pb = PlanBuilder()
    t = pb.table(0, 2, names=["product", "price"])
    f = pb.filter(t, EBV(P.LT(P.xsd_float(P.xsd_string(ENC_TV(col(1))), lexical=True), P.float32(2.5))))
    assert P.explain(pb, f)[0].startswith("FilterExec: EBV(LT(xsd:float(xsd:string(ENC_TV(price@1))), ")


def write_cases(path):
    with open(path, "w") as f:
        for t in L.TARGETS:
            for s in L.CASES[t]:
                st, bits, may = L.expected(s, t)
                if st == "ok" and bits is None:
                    st = "any"                                      # a signed NaN: must be declined
                v = (bits or 0) & ((1 << (128 if t == "decimal" else 64)) - 1)
                f.write(f"{t} x{s.encode('utf-8').hex()} {st} {v & ((1 << 64) - 1)} {v >> 64} {int(may)}\n")


def build(target, sanitize=False):
    out = subprocess.run(["make", "-C", CSRC, "-s", target] + (["SANITIZE=1"] if sanitize else []), capture_output=True, text=True)
    sys.stdout.write(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def test_the_compile_checks_build_and_pass_as_a_stand_alone_program():
    """tests/host/lex_compile_checks.cpp: kinds, targets, the rank-only literal, routing to the generic VM in FilterExec and the four
    join types, the aggregate and EXTEND hosts that take the two ops."""
    assert "\n0 failure(s)" in build("host-checks-lex-compile")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_parsers_as_a_stand_alone_host_program(tmp_path, sanitize):
    """tests/host/lex_parse_checks.cpp includes lex_parse.hpp as plain C++: every row of the case tables against the Python reference's
    bits, then generated strings against glibc's strtof / strtod — every row matches bit for bit or is declined, and over the strings
    of at most 19 digits nothing is declined for f32 and less than 0.1 % for f64 (the program's exit status).  Once more under
    AddressSanitizer + UndefinedBehaviorSanitizer (host code, its own main)."""
    build("lex-parse-checks", sanitize)
    exe = os.path.join(ROOT, "rdf-fusion_amd", "build", "lex_parse_checks" + ("_san" if sanitize else ""))
    cases = tmp_path / "cases.txt"
    write_cases(str(cases))
    out = subprocess.run([exe, "cases", str(cases)], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and " 0 failure(s)" in out.stdout
    out = subprocess.run([exe, "fuzz", str(FUZZ_ROWS), str(FUZZ_SEED)], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "mismatches 0, declined: f32 0," in out.stdout


def test_the_generated_table_is_what_the_generator_prints():
    text = subprocess.run([sys.executable, os.path.join(CSRC, "gen_lex_pow5.py")], capture_output=True, text=True, check=True).stdout
    assert text == open(os.path.join(CSRC, "lex_pow5_table.hpp")).read()
    assert text.count("ull},") == 651


def test_the_reference_knows_its_own_edges():
    """The Python restatement against a few values worked out by hand (and against float() for f64, at import)."""
    assert L.parse("1.0000000596046448", "float") == ("ok", 0x3F800001)
    assert L.parse("3.4028235e38", "float") == ("ok", 0x7F7FFFFF) and L.parse("3.4028236e38", "float") == ("ok", 0x7F800000)
    assert L.parse("1e-45", "float") == ("ok", 1) and L.parse("7e-46", "float") == ("ok", 0) and L.parse("7.1e-46", "float") == ("ok", 1)
    assert L.parse("-0", "double") == ("ok", 1 << 63) and L.parse("-0.0e5", "float") == ("ok", 1 << 31)
    assert L.parse("NaN", "float") == ("ok", 0x7FC00000) and L.parse("-INF", "double") == ("ok", 0xFFF0000000000000)
    assert L.parse("1" + "0" * 399, "double") == ("ok", 0x7FF0000000000000) and L.parse("1e-999999999999", "double") == ("ok", 0)
    assert L.parse("-9223372036854775808", "integer") == ("ok", -(1 << 63)) and L.parse("9223372036854775808", "integer")[0] == "error"
    assert L.parse("0." + "1" * 19, "decimal")[0] == "error" and L.parse("1.5" + "0" * 30, "decimal") == ("ok", 15 * 10 ** 17)
    assert L.parse("5.", "decimal") == ("ok", 5 * 10 ** 18) and L.parse(".", "decimal")[0] == "error"
    assert [L.parse(s, "boolean")[0] for s in L.BOOLEAN_CASES[:7]] == ["ok"] * 4 + ["error"] * 3
    assert L.declines(L.DECLINING, "double") and L.declines("-nan", "float") and not L.declines("NaN", "float")
