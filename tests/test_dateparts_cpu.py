"""The date parts (RDFGPU_EX_YEAR .. RDFGPU_EX_SECONDS), the timezone offset of the ABI and GROUP BY over value columns
(RDFGPU_PLAN_VALUE_KEYS) without a GPU: the header's constants, the builder's encodings and plan text, the Python reference against
`datetime` and the time line, the arithmetic's header compiled as plain C++ against that reference, the reference's own known answers, and
the compile checks as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from rdf_fusion_amd import abi, xsd
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, EBV
import datepart_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rdf-fusion_amd", "csrc")
FUZZ_ROWS, FUZZ_SEED = 100_000, 20261021
HEADER = open(os.path.join(ROOT, "include", "rdfgpu.h")).read()


def build(target, sanitize=False):
    out = subprocess.run(["make", "-C", CSRC, "-s", target] + (["SANITIZE=1"] if sanitize else []), capture_output=True, text=True)
    sys.stdout.write(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


# ---------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------
def test_abi_values_and_the_header_agree():
    ops = ["YEAR", "MONTH", "DAY", "HOURS", "MINUTES", "SECONDS"]
    assert [getattr(abi, "EX_" + n) for n in ops] == list(range(48, 54))
    for k, n in enumerate(ops):
        assert re.search(rf"RDFGPU_EX_{n} = {48 + k},", HEADER), n
    assert HEADER.index("RDFGPU_EX_SECONDS = 53") < HEADER.index("RDFGPU_EX__COUNT")
    assert abi.EX_CAST_LEX == 47 and abi.EX_COLUMN == 1                                   # the existing values did not move
    assert abi.PLAN_VALUE_KEYS == 4 and re.search(r"#define RDFGPU_PLAN_VALUE_KEYS 4u", HEADER)
    assert abi.MAX_GROUP_KEYS == 8 and re.search(r"#define RDFGPU_MAX_GROUP_KEYS 8u", HEADER)
    assert abi.MAX_KEYS == 4 and re.search(r"#define RDFGPU_MAX_KEYS 4u", HEADER)          # joins, TopK and Sort keep their bound
    assert re.search(r"#define RDFGPU_ABI_VERSION 4u", HEADER) and abi.ABI_VERSION == 4    # an addendum: no struct changed size


def test_the_offset_field_is_the_former_reserved_half_word():
    assert re.search(r"int16_t tz_minutes;", HEADER) and "uint16_t reserved;\n} rdfgpu_typed_value" not in HEADER
    assert C.sizeof(abi.TypedValue) == 16 and abi.TypedValue.tz_minutes.offset == 14 and abi.TypedValue.tz_minutes.size == 2
    assert TV_DTYPE.itemsize == 16 and TV_DTYPE.fields["tz_minutes"][1] == 14 and TV_DTYPE.fields["tz_minutes"][0] == np.dtype("<i2")
    row = np.zeros(1, TV_DTYPE)
    row["tz_minutes"] = -840
    assert np.frombuffer(row.tobytes(), np.uint32)[3] == (0xFCB8 << 16)                    # bits 16..31 of the row's fourth dword
    v = abi.TypedValue(tz_minutes=-330)
    assert bytes(v)[14:16] == (-330 & 0xFFFF).to_bytes(2, "little")


def test_literals_carry_the_offset_beside_the_presence_bit():
    v, has = xsd.parse_date_time("2024-03-01T02:00:00+05:30")
    (op, tag, flags, u, lo, hi), = P.date_time(v, has, 330).nodes
    assert (op, tag) == (abi.EX_LIT_TV, abi.TV_DATE_TIME) and u == (1 | (330 << 16)) and (hi << 64 | lo & (2 ** 64 - 1)) == v
    assert P.date_time(v, True, -840).nodes[0][3] == (1 | (0xFCB8 << 16))
    assert P.date_time(v, has).nodes == P.date_time(v, has, 0).nodes and P.date_time(v, has).nodes[0][3] == 1      # the default is what it was
    assert P.date_time(v, False).nodes[0][3] == 0
    with pytest.raises(ValueError):
        P.date_time(v, False, 60)                      # an offset without a timezone
    with pytest.raises(ValueError):
        P.date_time(v, True, 841)
    e = abi.ExprNode(*[(o, t, f, 0, u_, l, h) for (o, t, f, u_, l, h) in P.date_time(v, True, -1).nodes][0])
    assert e.u == 0xFFFF0001


def test_builder_ops_and_the_plan_text():
    a = ENC_TV(col(1))
    fns = [(P.YEAR, abi.EX_YEAR, "YEAR"), (P.MONTH, abi.EX_MONTH, "MONTH"), (P.DAY, abi.EX_DAY, "DAY"), (P.HOURS, abi.EX_HOURS, "HOURS"),
           (P.MINUTES, abi.EX_MINUTES, "MINUTES"), (P.SECONDS, abi.EX_SECONDS, "SECONDS")]
    pb = PlanBuilder()
    t = pb.table(0, 2, names=["val", "tv"])
    for fn, op, name in fns:
        assert fn(a).nodes == a.nodes + [(op, 0, 0, 0, 0, 0)]
        f = pb.filter(t, EBV(P.EQ(fn(a), P.integer(7))))
        assert P.explain(pb, f)[0] == f"FilterExec: EBV(EQ({name}(ENC_TV(tv@1)), 9:7))"
    # the Wind Farm projection: `MUL(9:10, FLOOR(DIV(MINUTES(tv), 10.0))) as minute_10, HOURS(tv) as hour, ..`
    m10 = P.MUL(P.integer(10), P.FLOOR(P.DIV(P.MINUTES(a), P.decimal(10 * D.SCALE))))
    x = pb.extend(t, [m10, P.HOURS(a), P.DAY(a), P.MONTH(a), P.YEAR(a)], keep=[0], names=["minute_10", "hour", "day", "month", "year"])
    line = P.explain(pb, x)[0]
    assert line.startswith("ProjectionExec: expr=[val@0 as val, MUL(9:10, FLOOR(DIV(MINUTES(ENC_TV(tv@1)), 7:")
    assert line.endswith("HOURS(ENC_TV(tv@1)) as hour, DAY(ENC_TV(tv@1)) as day, MONTH(ENC_TV(tv@1)) as month, YEAR(ENC_TV(tv@1)) as year]")


# ---------------------------------------------------------------------------------------------------
# the reference, the header, the golden answers
# ---------------------------------------------------------------------------------------------------
def test_the_reference_agrees_with_datetime_and_the_time_line():
    D.check_reference()
    p = D.parts(*xsd.parse_date_time("2024-03-01T02:00:00+05:30"), 330)
    assert (p["year"], p["month"], p["day"], p["hours"], p["minutes"], p["seconds"]) == (2024, 3, 1, 2, 0, 0)
    assert D.parts(-D.SCALE // 2, True, 0)["seconds"] == 59 * D.SCALE + D.SCALE // 2 and D.parts(-(D.SCALE // 2), True, 0)["day"] == 1   # truncation first


def test_the_cases_cover_what_they_name():
    got = [(name, D.parts(v, has, tz)) for name, v, has, tz in D.CASES]
    by = dict(got)
    assert (by["0001-01-01T00:00:00Z"]["year"], by["the second before 0001-01-01"]["year"]) == (1, 0)
    assert by["the second before 0001-01-01"]["month"] == 12 and by["the second before 0001-01-01"]["seconds"] == 59 * D.SCALE
    assert min(p["year"] for _, p in got) < -10 ** 12 and max(p["year"] for _, p in got) > 10 ** 12
    for name, p in got:
        m = re.match(r"(\d+)-(\d\d)-(\d\d)T(\d\d):(\d\d):(\d\d(?:\.\d+)?)", name)
        if m and "T24" not in name:                                                 # a lexical form: the parts are the ones written
            assert (p["year"], p["month"], p["day"], p["hours"], p["minutes"]) == tuple(int(x) for x in m.groups()[:5]), name
    # the offsets cross a day, a month and a year boundary: the UTC instant's date differs from the local one
    for name in ("2024-01-01T05:00:00+14:00", "2023-12-31T20:00:00-14:00", "2024-03-01T02:00:00+05:30", "2024-02-29T22:00:00-05:30"):
        _, v, has, tz = next(c for c in D.CASES if c[0] == name)
        utc, local = D.parts(v, True, 0), D.parts(v, True, tz)
        assert (utc["year"], utc["month"], utc["day"]) != (local["year"], local["month"], local["day"]), name
    assert sorted(D.NOT_DATE_TIME) == [t for t in range(15) if t != abi.TV_DATE_TIME]


def run_program(exe, tmp_path, stamps):
    src = tmp_path / "stamps.txt"
    with open(src, "w") as f:
        for v, has, tz in stamps:
            lo, hi = D.split_i128(v)
            f.write(f"{lo} {hi} {tz if has else 0}\n")
    out = subprocess.run([exe, str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(rows) == len(stamps)
    return rows


def as_row(p):
    lo, hi = D.split_i128(p["seconds"])
    return (p["year"], p["month"], p["day"], p["hours"], p["minutes"], lo, hi)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_header_as_a_stand_alone_host_program(tmp_path, sanitize):
    """tests/host/date_parts_checks.cpp includes date_parts.hpp as plain C++ — the text the device runs: every case row, the golden
    timestamps and a seeded fuzz of 10^5 timestamps against the Python reference; once more under AddressSanitizer + UBSan."""
    build("date-parts-checks", sanitize)
    exe = os.path.join(ROOT, "rdf-fusion_amd", "build", "date_parts_checks" + ("_san" if sanitize else ""))
    stamps = [(v, has, tz) for _, v, has, tz in D.CASES] + [D.golden_timestamp(c) for c in D.golden()] + D.fuzz_timestamps(FUZZ_ROWS, FUZZ_SEED)
    rows = run_program(exe, tmp_path, stamps)
    bad = [(s, r, as_row(D.parts(*s))) for s, r in zip(stamps, rows) if r != as_row(D.parts(*s))]
    assert not bad, bad[:5]


def test_the_known_answers_of_the_reference(tmp_path):
    """tests/golden/datepart_kats.json: what the reference's own unit tests assert of year() .. second() — met by the Python reference and
    by the header (Date and Time go through the same Timestamp functions there)."""
    build("date-parts-checks")
    exe = os.path.join(ROOT, "rdf-fusion_amd", "build", "date_parts_checks")
    cases = D.golden()
    assert len(cases) == 29 and {c["part"] for c in cases} == set(D.PARTS)
    rows = run_program(exe, tmp_path, [D.golden_timestamp(c) for c in cases])
    for c, r in zip(cases, rows):
        want = c["expected"]
        if c["part"] == "seconds":
            from fractions import Fraction
            want = int(Fraction(want) * D.SCALE)
            got_c = (r[6] << 64) | (r[5] & (2 ** 64 - 1))
        else:
            got_c = r[D.PARTS.index(c["part"])]
        assert D.parts(*D.golden_timestamp(c))[c["part"]] == want, c
        assert got_c == want, c


# ---------------------------------------------------------------------------------------------------
# compile checks
# ---------------------------------------------------------------------------------------------------
def test_the_compile_checks_build_and_pass_as_a_stand_alone_program():
    """tests/host/value_keys_compile_checks.cpp: the six ops type-check and are refused over an id; with RDFGPU_PLAN_VALUE_KEYS 5..8 keys and
    value keys compile with the right origins, 9 keys and the flag without RDFGPU_PLAN_AGG_COLUMNS are refused, without the flag the texts
    of today come back verbatim, a value column as join key stays refused."""
    assert "\n0 failure(s)" in build("host-checks-value-keys")


def test_builder_takes_eight_group_columns_and_value_columns():
    pb = PlanBuilder()
    t = pb.table(0, 3, names=["site", "wtur", "tv"])
    a = ENC_TV(col(2))
    x = pb.extend(t, [P.YEAR(a), P.MONTH(a), P.DAY(a), P.HOURS(a), P.MINUTES(a)], keep=[0, 1, 2], names=["year", "month", "day", "hour", "minute"])
    g = pb.aggregate(x, [0, 1, 3, 4, 5, 6, 7], [(abi.AGG_COUNT_STAR, None)])
    n = pb.nodes[g]
    assert n.n_keys == 7 and list(n.left_keys) == [0, 1, 3, 4] and list(n.right_keys)[:3] == [5, 6, 7]       # keys 4.. ride in right_keys[]
    assert pb.values[g] == [False, False, True, True, True, True, True, True]                                # a value key stays a value column
    d = pb.build(g, agg_columns=True, value_keys=True)
    assert d.flags == abi.PLAN_AGG_COLUMNS | abi.PLAN_VALUE_KEYS and d.value_columns == [2, 3, 4, 5, 6, 7]
    assert pb.build(g, agg_columns=True).flags == abi.PLAN_AGG_COLUMNS
    with pytest.raises(ValueError):
        pb.build(g, value_keys=True)                                                                         # only valid with agg_columns
    line = P.explain(pb, g, agg_columns=True)[0]
    assert line == ("AggregateExec: mode=Single, gby=[site@0 as site, wtur@1 as wtur, ENC_PT(year@3) as year, ENC_PT(month@4) as month, "
                    "ENC_PT(day@5) as day, ENC_PT(hour@6) as hour, ENC_PT(minute@7) as minute], aggr=[COUNT(*)], values=[COUNT(*)@7]")
    eight = pb.aggregate(x, list(range(8)), [])
    assert pb.nodes[eight].n_keys == 8 and list(pb.nodes[eight].right_keys) == [4, 5, 6, 7]
    nine = pb.aggregate(pb.table(1, 9), list(range(9)), [])          # more than 8 is the library's to refuse
    assert pb.nodes[nine].n_keys == 9
