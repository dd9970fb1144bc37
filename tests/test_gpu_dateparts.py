"""The date parts (RDFGPU_EX_YEAR .. RDFGPU_EX_SECONDS) on the MI355X: every case row of datepart_cases.py through a FILTER, through a
computed column and as an aggregate's input expression, against the Python reference there; timestamp literals with an offset; a store
that leaves tz_minutes 0; and the comparisons of timestamps, which never look at the offset."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, xsd
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, EBV
from test_gpu_parity import table_on_device
import datepart_cases as D
import numeric_ref as nr

FNS = {"year": P.YEAR, "month": P.MONTH, "day": P.DAY, "hours": P.HOURS, "minutes": P.MINUTES, "seconds": P.SECONDS}
INTEGER, DEC = abi.TV_INTEGER, abi.TV_DECIMAL


class Zoo:
    """One store: id 1 + i = case i of D.CASES (a dateTime, its offset in tz_minutes); behind them one id per kind that is not a dateTime;
    behind those, on demand, xsd:integer / xsd:decimal ids for the values a test compares with."""

    def __init__(self):
        self.rows, self.dec, self.numbers, self.frozen = [(0, 0, 0, 0)], [], {}, False
        self.case_ids = [self.add(abi.TV_DATE_TIME, None, 1 if has else 0, tz if has else 0, v) for _, v, has, tz in D.CASES]
        self.other_ids = {tag: self.add(tag, lo, aux, 0, scaled) for tag, (lo, aux, scaled) in D.NOT_DATE_TIME.items()}
        # the same instants as stored by a host that knows nothing of the field: aux bit 0 set, tz_minutes 0
        self.utc_ids = [self.add(abi.TV_DATE_TIME, None, 1, 0, v) for _, v, has, tz in D.CASES if has]

    def add(self, tag, lo, aux, tz, scaled=None):
        if scaled is not None:
            lo = len(self.dec)
            self.dec.append(D.split_i128(scaled))
        self.rows.append((lo, aux, tag, tz))
        return len(self.rows) - 1

    def number(self, tag, v):
        """the id of xsd:integer v / xsd:decimal v (scaled)"""
        if (tag, v) not in self.numbers:
            assert not self.frozen, "the store is built: every number a test compares with is added by the fixture"
            self.numbers[(tag, v)] = self.add(tag, v, 0, 0, v if tag == DEC else None)
        return self.numbers[(tag, v)]

    def store(self):
        tv = np.zeros(len(self.rows), TV_DTYPE)
        for i, (lo, aux, tag, tz) in enumerate(self.rows):
            tv[i] = (lo, aux, tag, 0, tz)
        self.frozen = True
        gs = rf.GpuQuadStore()
        gs.set_typed_values(tv, np.array(self.dec, np.int64).reshape(-1, 2))
        return gs


def expected_of(z):
    """{id: parts or None (the error value)} for every id that stands for a case or a kind"""
    out = {0: None}
    for i, (_, v, has, tz) in zip(z.case_ids, D.CASES):
        out[i] = D.parts(v, has, tz)
    for i in z.other_ids.values():
        out[i] = None
    for i, (_, v, has, tz) in zip(z.utc_ids, [c for c in D.CASES if c[2]]):
        out[i] = D.parts(v, True, 0)
    return out


def part_value(part, p):
    """the typed value of a part: (tag, payload)"""
    return (abi.TV_NULL, 0) if p is None else ((DEC if part == "seconds" else INTEGER), p[part])


@pytest.fixture(scope="module")
def zoo(torch_cuda):
    z = Zoo()
    want = expected_of(z)
    # candidates a FILTER compares with: the expected value and its two neighbours (SECONDS: one unit of 10^-18)
    for i, p in want.items():
        for part in D.PARTS:
            if p is not None:
                for d in (-1, 0, 1):
                    z.number(DEC if part == "seconds" else INTEGER, p[part] + d)
    z.number(INTEGER, 2024); z.number(DEC, 0)
    return z, z.store(), want


def run(torch, gs, tables, root_of, timing=False, value_keys=False):
    pb = PlanBuilder()
    nodes = [pb.table(slot, len(t)) for slot, t in enumerate(tables)]
    plan = gs.plan(pb.build(root_of(pb, nodes), agg_columns=True, value_keys=value_keys))
    if timing:
        plan.enable_kernel_timing(True)
    plan._keep = []
    for slot, cols in enumerate(tables):
        keep, ptrs = table_on_device(torch, cols)
        plan._keep.append(keep)
        plan.bind_table(slot, ptrs, len(cols[0]))
    return plan.execute()


def cols_of(rows):
    return [np.array(c, np.uint32) for c in zip(*rows)]


@pytest.mark.parametrize("part", D.PARTS)
def test_filter_every_case(torch_cuda, zoo, part):
    """EQ(PART(ENC_TV(t)), ENC_TV(candidate)): every id with the expected value and both neighbours — exactly the rows of the expected
    value pass; an id that is no dateTime passes with no candidate (the error value drops the row)"""
    z, gs, want = zoo
    tag = DEC if part == "seconds" else INTEGER
    rows, passing = [], []
    for i, p in want.items():
        for d in (-1, 0, 1):
            cand = z.number(tag, (p[part] if p else 2024 if tag == INTEGER else 0) + (d if p else 0))
            rows.append((i, cand, len(rows) + 1))
            if p is not None and d == 0:
                passing.append(len(rows))
    plan = run(torch_cuda, gs, [cols_of(rows)], lambda pb, t: pb.filter(t[0], EBV(P.EQ(FNS[part](ENC_TV(col(0))), ENC_TV(col(1))))), timing=True)
    assert sorted(plan.fetch()[2].tolist()) == passing
    assert any(s[0].startswith("void rdfgpu::filter_kernel<0>") or "filter_kernel<5>" in s[0] for s in plan.kernel_stats()), plan.kernel_stats()


def test_filter_against_an_integer_literal(torch_cuda, zoo):
    """the issue's shape, EQ(YEAR(ENC_TV(col)), integer): the ids whose local year is 2024"""
    z, gs, want = zoo
    ids = sorted(want)
    plan = run(torch_cuda, gs, [[np.array(ids, np.uint32)]], lambda pb, t: pb.filter(t[0], EBV(P.EQ(P.YEAR(ENC_TV(col(0))), P.integer(2024)))))
    exp = [i for i in ids if want[i] and want[i]["year"] == 2024]
    assert len(exp) >= 5 and sorted(plan.fetch()[0].tolist()) == exp


def test_extend_every_case(torch_cuda, zoo):
    """six computed columns, the values fetched: tag and payload bit for bit; what is no dateTime is unbound (entry 0, tag 0)"""
    z, gs, want = zoo
    ids = sorted(want) + [len(z.rows) + 5]                         # (.. and an id behind the table: null)
    plan = run(torch_cuda, gs, [[np.array(ids, np.uint32)]], lambda pb, t: pb.extend(t[0], [FNS[p](ENC_TV(col(0))) for p in D.PARTS]), timing=True)
    assert plan.result_info() == (len(ids), 7)
    assert any("extend_lex_kernel" in s[0] or s[0].startswith("rdfgpu::extend_kernel") for s in plan.kernel_stats())
    entries = plan.fetch()
    for q, part in enumerate(D.PARTS, start=1):
        got = [nr.device_bits(int(v["tag"]), int(v["lo"]), int(v["hi"])) for v in plan.fetch_column_values(q)]
        exp = [nr.bits(part_value(part, want.get(i))) for i in ids]
        assert got == exp, (part, [(ids[r], g, e) for r, (g, e) in enumerate(zip(got, exp)) if g != e][:4])
        assert entries[q].tolist() == [0 if e[0] == abi.TV_NULL else r + 1 for r, e in enumerate(exp)]


def test_the_wind_farm_bucket_expression(torch_cuda, zoo):
    """MUL(10, FLOOR(DIV(MINUTES(tv), 10.0))) as the GroupedProduction plans compute their 10-minute bucket: a decimal, bit for bit"""
    z, gs, want = zoo
    ids = sorted(want)
    ten = P.decimal(10 * D.SCALE)
    plan = run(torch_cuda, gs, [[np.array(ids, np.uint32)]], lambda pb, t: pb.extend(t[0], [P.MUL(P.integer(10), P.FLOOR(P.DIV(P.MINUTES(ENC_TV(col(0))), ten)))]))
    ref = lambda p: (abi.TV_NULL, 0) if p is None else nr.binary(abi.EX_MUL, (INTEGER, 10), nr.unary(abi.EX_FLOOR, nr.binary(abi.EX_DIV, (INTEGER, p["minutes"]), (DEC, 10 * D.SCALE))))
    got = [nr.device_bits(int(v["tag"]), int(v["lo"]), int(v["hi"])) for v in plan.fetch_column_values(1)]
    assert got == [nr.bits(ref(want[i])) for i in ids]
    buckets = {((g[2] << 64) | (g[1] & (2 ** 64 - 1))) // D.SCALE for g in got if g[0] == DEC}
    assert {0, 20, 30, 50} <= buckets <= {0, 10, 20, 30, 40, 50}


@pytest.mark.parametrize("form", [None, "NO_AGG_LDS"])
def test_aggregate_input_expressions(torch_cuda, zoo, form):
    """every id twice, grouped by id: AVG(YEAR(..)) is the year as a decimal, SUM(SECONDS(..)) twice the seconds, MIN(MINUTES) / MAX(HOURS)
    the value itself; a group whose timestamp is no dateTime: AVG, MIN and MAX are the error value and SUM skips the rows (integer 0)"""
    z, gs, want = zoo
    ids = [i for i in sorted(want) if i != 0]
    t = np.array(ids + ids[::-1], np.uint32)
    a = ENC_TV(col(0))
    aggs = [(abi.AGG_AVG, P.YEAR(a)), (abi.AGG_SUM, P.SECONDS(a)), (abi.AGG_MIN, P.MINUTES(a)), (abi.AGG_MAX, P.HOURS(a)), (abi.AGG_SUM, P.MONTH(a)), (abi.AGG_AVG, P.DAY(a))]
    pb = PlanBuilder()
    plan = gs.plan(pb.build(pb.aggregate(pb.table(0, 1), [0], aggs), agg_columns=True))
    if form:
        plan.set_option(form, 1)
    keep, ptrs = table_on_device(torch_cuda, [t])
    plan.bind_table(0, ptrs, len(t))
    plan.execute()
    keys = plan.fetch()[0].tolist()
    assert sorted(keys) == ids
    cols = [[nr.device_bits(int(v["tag"]), int(v["lo"]), int(v["hi"])) for v in plan.fetch_column_values(q)] for q in range(1, 7)]
    for g, i in enumerate(keys):
        p = want[i]
        if p is None:
            exp = [(abi.TV_NULL, 0), (INTEGER, 0), (abi.TV_NULL, 0), (abi.TV_NULL, 0), (INTEGER, 0), (abi.TV_NULL, 0)]
        else:
            avg = lambda v: (DEC, nr.dec_div(2 * v * D.SCALE, 2 * D.SCALE))
            exp = [avg(p["year"]), (DEC, 2 * p["seconds"]), (INTEGER, p["minutes"]), (INTEGER, p["hours"]), (INTEGER, 2 * p["month"]), avg(p["day"])]
            assert exp[0][1] == p["year"] * D.SCALE
        assert [c[g] for c in cols] == [nr.bits(e) for e in exp], (i, p)


def test_literals_with_an_offset(torch_cuda, zoo):
    """a timestamp literal carries its offset in bits 16..31 of `u`: its parts are local; without a timezone they are the value's own"""
    z, gs, want = zoo
    rows = [np.arange(1, 4, dtype=np.uint32)]
    for name, v, has, tz in D.CASES:
        p = D.parts(v, has, tz)
        lit = P.date_time(v, has, tz)
        pred = None
        for part in ("year", "month", "day", "hours", "minutes"):
            c = EBV(P.EQ(FNS[part](lit), P.integer(p[part])))
            pred = c if pred is None else P.AND(pred, c)
        pred = P.AND(P.AND(pred, EBV(P.EQ(P.SECONDS(lit), P.decimal(p["seconds"])))), P.BOUND(col(0)))
        plan = run(torch_cuda, gs, [rows], lambda pb, t: pb.filter(t[0], pred))
        assert plan.result_info()[0] == 3, (name, p)
        if tz:                                                        # .. and the offset matters: the UTC instant has other parts
            utc = D.parts(v, True, 0)
            part = next(k for k in ("minutes", "hours", "day") if utc[k] != p[k])
            plan = run(torch_cuda, gs, [rows], lambda pb, t: pb.filter(t[0], EBV(P.EQ(FNS[part](lit), P.integer(utc[part])))))
            assert plan.result_info()[0] == 0, name


def test_a_store_that_leaves_the_offset_zero_gets_utc_parts(torch_cuda, zoo):
    z, gs, want = zoo
    moved = [(u, c) for u, c in zip(z.utc_ids, [i for i, cs in zip(z.case_ids, D.CASES) if cs[2]]) if want[u] != want[c]]
    assert len(moved) >= 8                                            # the cases with an offset: the two stores of one instant differ
    ids = [u for u, _ in moved]
    plan = run(torch_cuda, gs, [[np.array(ids, np.uint32)]], lambda pb, t: pb.extend(t[0], [P.HOURS(ENC_TV(col(0))), P.DAY(ENC_TV(col(0)))]))
    assert plan.column_values(1) == [want[u]["hours"] for u in ids] and plan.column_values(2) == [want[u]["day"] for u in ids]


def test_comparisons_never_look_at_the_offset(torch_cuda, zoo):
    """equality and order of dateTimes are by value and presence of a timezone (date_time.rs:1605-1654): a stored offset and a literal's
    offset change nothing, in the specialised filter (ENC_TV(col) cmp literal) and in the generic VM"""
    z, gs, want = zoo
    with_tz = [(i, c) for i, c in zip(z.case_ids, D.CASES) if c[2]]
    both = [i for i, _ in with_tz] + z.utc_ids                        # every instant twice: with its offset, and with offset 0
    t = [[np.array(both, np.uint32)]]
    _, v, _, _ = next(c for c in D.CASES if c[0] == "2024-03-01T02:00:00+05:30")
    for lit_tz in (0, 330, -840):
        lit = P.date_time(v, True, lit_tz)
        eq = run(torch_cuda, gs, t, lambda pb, tt: pb.filter(tt[0], EBV(P.EQ(ENC_TV(col(0)), lit)))).fetch()[0].tolist()
        k = next(k for k, (_, c) in enumerate(with_tz) if c[1] == v)
        assert sorted(eq) == sorted([with_tz[k][0], z.utc_ids[k]])
        lt = run(torch_cuda, gs, t, lambda pb, tt: pb.filter(tt[0], EBV(P.LT(ENC_TV(col(0)), lit)))).result_info()[0]
        assert lt == 2 * sum(1 for _, c in with_tz if c[1] < v)
        vm = run(torch_cuda, gs, t, lambda pb, tt: pb.filter(tt[0], P.AND(EBV(P.EQ(ENC_TV(col(0)), lit)), EBV(P.EQ(P.YEAR(lit), P.YEAR(lit)))))).result_info()[0]
        assert vm == 2                                                # (the VM instantiation that carries the offset in `aux`)
    no_tz = P.date_time(v, False)
    assert run(torch_cuda, gs, t, lambda pb, tt: pb.filter(tt[0], EBV(P.EQ(ENC_TV(col(0)), no_tz)))).result_info()[0] == 0
