"""MUL, DIV, NEG, PLUS, ABS, ROUND, CEIL, FLOOR and the numeric casts on the MI355X, in FilterExec, join filters and as the input of SUM /
AVG.  The CPU oracle cannot evaluate these ops: the expectation is the restatement in numeric_ref.py (checked against the reference's
own known answers by test_numeric_cpu.py).  Every comparison is exact: integer, decimal, float and double payloads bit for bit (any
NaN equals any NaN)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import RdfGpuError, TV_DTYPE
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, EBV
from test_gpu_parity import both_stores, table_on_device, typed_zoo, check_filter
from test_aggregate_cpu import sum_agg, avg_agg
import numeric_ref as R

EMPTY = (np.zeros(0, np.uint32),) * 4
SUM, AVG = abi.AGG_SUM, abi.AGG_AVG
E18 = R.E18


def unary_ops():
    return [(P.NEG, abi.EX_NEG), (P.PLUS, abi.EX_PLUS), (P.ABS, abi.EX_ABS), (P.ROUND, abi.EX_ROUND), (P.CEIL, abi.EX_CEIL), (P.FLOOR, abi.EX_FLOOR)]


def plain(v):
    """A value of the restatement as test_aggregate_cpu's accumulators take it: Python int / float payloads"""
    return v[0], None if v[1] is None else (int(v[1]) if v[0] in (abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_BOOLEAN) else float(v[1]))


def exact(result):
    """sum_agg / avg_agg's result with a float / double payload made exact: the terms added one after the other from 0 in the result's
    format, as the reference does, then divided by the count.  (Used where every order of the additions gives the same bits.)"""
    tag, p = result
    if not hasattr(p, "terms"):
        return result
    T = np.float32 if tag == abi.TV_FLOAT else np.float64
    with np.errstate(all="ignore"):
        acc = T(0)
        for x in p.terms:
            acc = acc + T(x)
        return tag, acc / T(p.divisor)


def extended_zoo():
    """typed_zoo plus the edge values it lacks; returns (tv, dec, ids): about 60 ids to pair up — every added value, one of each
    non-numeric kind except simple literals (a cast would have to parse those), id 0 and an id beyond the table."""
    tv, dec = typed_zoo()
    f32 = lambda x: int(np.float32(x).view(np.uint32))
    f64 = lambda x: int(np.float64(x).view(np.int64))
    big = np.float64(2.0 ** 127) / np.float64(1e18)
    decs = [E18 // 2, 15 * E18 // 10, 25 * E18 // 10, -E18 // 2, -25 * E18 // 10, R.I128_MIN, R.I128_MIN + 1, R.I128_MAX, 1, E18 // 10, E18 // 100]
    rows = [(abi.TV_INT, v) for v in (R.I32_MIN, R.I32_MAX, 65536, 7, -3)]
    rows += [(abi.TV_INTEGER, v) for v in (R.I64_MIN, R.I64_MAX, 65536, 10, -7)]
    rows += [(abi.TV_DECIMAL, len(dec) + i) for i in range(len(decs))]
    rows += [(abi.TV_FLOAT, f32(x)) for x in (0.5, -0.5, 2.5, -2.5, 2.0 ** 63, 1e20, 1e-45, -1e-40, np.inf, -np.inf, np.nan, 3.0, -0.0)]
    rows += [(abi.TV_DOUBLE, f64(x)) for x in (0.5, -0.5, 2.5, -2.5, 0.49999999999999994, 2.0 ** 63, 1e20, big, np.nextafter(big, 0), np.nextafter(big, np.inf),
                                               5e-324, -2e-310, np.inf, -np.inf, np.nan, 10.0, -0.0, 1e-18)]
    ext = np.zeros(len(rows), TV_DTYPE)
    for i, (tag, lo) in enumerate(rows):
        ext[i] = (lo, 0, tag, 0, 0)
    dext = np.zeros((len(decs), 2), np.int64)
    for i, d in enumerate(decs):
        u = d & ((1 << 128) - 1)
        lo, hi = u & ((1 << 64) - 1), u >> 64
        dext[i] = (lo - (1 << 64) if lo >= 1 << 63 else lo, hi - (1 << 64) if hi >= 1 << 63 else hi)
    n0 = len(tv)
    tv, dec = np.concatenate([tv, ext]), np.concatenate([dec, dext])
    tags = tv["tag"][:n0]
    first = lambda sel: int(np.flatnonzero(sel)[0])
    others = [0, len(tv) + 5, first(tags == abi.TV_NAMED_NODE), first((tags == abi.TV_STRING) & (tv["aux"][:n0] != 0)), first(tags == abi.TV_DATE_TIME),
              first(tags == abi.TV_OTHER), first(tags == abi.TV_DURATION)] + np.flatnonzero(tags == abi.TV_BOOLEAN).tolist()
    return tv, dec, np.array(list(range(n0, len(tv))) + others, np.uint32)


def value_of(tv, dec):
    def val(i):
        if i == 0 or i >= len(tv):
            return (abi.TV_NULL, None), 0
        tag, lo, aux = int(tv[i]["tag"]), int(tv[i]["lo"]), int(tv[i]["aux"])
        if tag == abi.TV_DECIMAL:
            return (tag, (int(dec[lo][1]) << 64) | (int(dec[lo][0]) & ((1 << 64) - 1))), aux
        if tag == abi.TV_FLOAT:
            return (tag, np.uint32(lo & 0xFFFFFFFF).view(np.float32)), aux
        if tag == abi.TV_DOUBLE:
            return (tag, np.int64(lo).view(np.float64)), aux
        if tag in (abi.TV_INT, abi.TV_INTEGER, abi.TV_BOOLEAN):
            return (tag, lo), aux
        return (tag, None), aux
    return val


@pytest.fixture(scope="module")
def zoo():
    tv, dec, ids = extended_zoo()
    gs, os_ = both_stores(EMPTY, typed=tv, decimals=dec)
    a, b = np.repeat(ids, len(ids)), np.tile(ids, len(ids))
    return dict(tv=tv, dec=dec, ids=ids, gs=gs, os=os_, val=value_of(tv, dec), pairs=[a, b, np.arange(len(a), dtype=np.uint32)],
                singles=[ids, ids, np.arange(len(ids), dtype=np.uint32)])


def run(gs, cols, root_of, form=None, timing=False):
    import torch
    pb = PlanBuilder()
    t = pb.table(0, len(cols))
    plan = gs.plan(pb.build(root_of(pb, t)))
    if form:
        plan.set_option(form)
    if timing:
        plan.enable_kernel_timing(True)
    keep, ptrs = table_on_device(torch, cols)
    plan.bind_table(0, ptrs, len(cols[0]))
    plan.execute()
    plan._keep_cols = keep
    return plan


def check_one_row_groups(z, cols, exprs, refs):
    """SUM(e) and AVG(e) per expression over keys (a, b, row): every group is one row; refs[i](row) = the restatement's value of e."""
    for at in range(0, len(exprs), 4):
        part = exprs[at:at + 4]
        aggs = [(fn, e) for e in part for fn in (SUM, AVG)]
        plan = run(z["gs"], cols, lambda pb, t: pb.aggregate(t, [0, 1, 2], aggs))
        n, _ = plan.result_info()
        assert n == len(cols[0])
        rows = plan.fetch()[2].tolist()
        vals = [plan.fetch_aggregate(a) for a in range(len(aggs))]
        for k in range(len(part)):
            s, v = vals[2 * k], vals[2 * k + 1]
            for r, row in enumerate(rows):
                ref = refs[at + k](row)
                got_s = R.device_bits(int(s["tag"][r]), int(s["lo"][r]), int(s["hi"][r]))
                got_a = R.device_bits(int(v["tag"][r]), int(v["lo"][r]), int(v["hi"][r]))
                want_s, want_a = R.bits(exact(sum_agg([plain(ref)]))), R.bits(exact(avg_agg([plain(ref)])))
                assert got_s == want_s and got_a == want_a, (at + k, row, int(cols[0][row]), int(cols[1][row]), ref, got_s, got_a)


# ---------------------------------------------------------------------------------------------------
# 1. every op, every kind pair, value exact
# ---------------------------------------------------------------------------------------------------
def test_mul_div_every_pair(torch_cuda, zoo):
    z, val = zoo, zoo["val"]
    a, b = ENC_TV(col(0)), ENC_TV(col(1))
    A, B = z["pairs"][0].tolist(), z["pairs"][1].tolist()
    refs = [lambda r, op=op: R.binary(op, val(A[r])[0], val(B[r])[0]) for op in (abi.EX_MUL, abi.EX_DIV)]
    check_one_row_groups(z, z["pairs"], [P.MUL(a, b), P.DIV(a, b)], refs)


def cast_ref(val, tag, i):
    v, aux = val(i)
    return R.cast(tag, v, aux)


def test_unary_ops_casts_and_nested(torch_cuda, zoo):
    z, val = zoo, zoo["val"]
    x = ENC_TV(col(0))
    X = z["singles"][0].tolist()
    exprs = [fn(x) for fn, _ in unary_ops()] + [P.CAST(x, t) for t in abi.CAST_TARGETS]
    refs = [lambda r, op=op: R.unary(op, val(X[r])[0]) for _, op in unary_ops()] + [lambda r, t=t: cast_ref(val, t, X[r]) for t in abi.CAST_TARGETS]
    # the Wind Farm shape: MUL(10, FLOOR(DIV(x, 10.0)))
    exprs.append(P.MUL(P.integer(10), P.FLOOR(P.DIV(x, P.double(10.0)))))
    refs.append(lambda r: R.binary(abi.EX_MUL, (abi.TV_INTEGER, 10), R.unary(abi.EX_FLOOR, R.binary(abi.EX_DIV, val(X[r])[0], (abi.TV_DOUBLE, np.float64(10.0))))))
    check_one_row_groups(z, z["singles"], exprs, refs)


@pytest.mark.parametrize("form", [None, "NO_AGG_LDS"])
def test_lds_accumulators_with_expression_inputs(torch_cuda, form):
    """48 groups of 75 rows: the LDS partials form (and, with NO_AGG_LDS, the HBM form) under expression inputs.  Float / double inputs are
    small integers, so their sums are exact in any order and no tolerance is needed."""
    vals = [(abi.TV_INTEGER, v) for v in range(-4, 5)] + [(abi.TV_INT, 3), (abi.TV_DECIMAL, 0), (abi.TV_DECIMAL, 1), (abi.TV_FLOAT, 0), (abi.TV_DOUBLE, 0)]
    tv = np.zeros(len(vals) + 1, TV_DTYPE)
    for i, (tag, lo) in enumerate(vals, start=1):
        tv[i] = (lo, 0, tag, 0, 0)
    tv[-2]["lo"] = int(np.float32(2.0).view(np.uint32))
    tv[-1]["lo"] = int(np.float64(-3.0).view(np.int64))
    dec = np.array([[15 * E18 // 10, 0], [-E18 // 4, -1]], np.int64)
    gs, _ = both_stores(EMPTY, typed=tv, decimals=dec)
    val = value_of(tv, dec)
    rng = np.random.default_rng(5)
    n = 48 * 75
    key = np.repeat(np.arange(48, dtype=np.uint32), 75)
    kind = key % 4      # group kinds: integers only; with decimals; with the float; with the double
    pick = lambda hi: rng.integers(1, hi, n).astype(np.uint32)
    a = np.where(kind == 0, pick(11), np.where(kind == 1, pick(13), np.where(kind == 2, np.where(rng.random(n) < 0.3, 13, pick(11)), np.where(rng.random(n) < 0.3, 14, pick(11))))).astype(np.uint32)
    b = pick(11)
    perm = rng.permutation(n)
    key, a, b = key[perm], a[perm], b[perm]
    exprs = [P.MUL(ENC_TV(col(1)), ENC_TV(col(2))), P.NEG(ENC_TV(col(1))), P.xsd_decimal(ENC_TV(col(2)))]
    refs = [lambda r: R.binary(abi.EX_MUL, val(int(a[r]))[0], val(int(b[r]))[0]), lambda r: R.unary(abi.EX_NEG, val(int(a[r]))[0]),
            lambda r: R.cast(abi.TV_DECIMAL, val(int(b[r]))[0])]
    aggs = [(fn, e) for e in exprs for fn in (SUM, AVG)] + [(SUM, 1)]
    plan = run(gs, [key, a, b], lambda pb, t: pb.aggregate(t, [0], aggs), form, timing=True)
    names = [s[0] for s in plan.kernel_stats()]
    assert any(k.startswith("void rdfgpu::agg_accum_expr_kernel<%s>" % ("false" if form else "true")) for k in names), names
    keys = plan.fetch()[0].tolist()
    out = [plan.fetch_aggregate(i) for i in range(len(aggs))]
    for g, k in enumerate(keys):
        rows = np.flatnonzero(key == k)
        for i, (fn, e) in enumerate(aggs):
            members = [plain(refs[i // 2](r)) if i < 6 else plain(val(int(a[r]))[0]) for r in rows]
            tag, payload = exact((sum_agg if fn == SUM else avg_agg)(members))   # float / double: small integers, exact in any order
            got = R.device_bits(int(out[i]["tag"][g]), int(out[i]["lo"][g]), int(out[i]["hi"][g]))
            assert got == R.bits((tag, payload)), (k, i, tag, payload, got)


# ---------------------------------------------------------------------------------------------------
# 2. FilterExec and join filter
# ---------------------------------------------------------------------------------------------------
def cmp_num(a, b):
    """PartialOrd of two numeric values (typed_value.rs:162-261): -1 / 0 / 1 or None"""
    (ta, va), (tb, vb) = a, b
    if ta not in R.NUMERIC or tb not in R.NUMERIC:
        return None
    k = ta if R.RANK[ta] >= R.RANK[tb] else tb
    if k in (R.FLT, R.DBL):
        x, y = (R.to_f32(ta, va), R.to_f32(tb, vb)) if k == R.FLT else (R.to_f64(ta, va), R.to_f64(tb, vb))
        return None if np.isnan(x) or np.isnan(y) else int(x > y) - int(x < y)
    x, y = (R.to_dec(ta, va), R.to_dec(tb, vb)) if k == R.DEC else (va, vb)
    return int(x > y) - int(x < y)


def kept_rows(plan):
    n, _ = plan.result_info()
    return sorted(zip(*[c[:n].tolist() for c in plan.fetch()]))


def test_filters_over_numeric_ops(torch_cuda, zoo):
    z, val = zoo, zoo["val"]
    cols = z["pairs"]
    A, B, N = cols[0].tolist(), cols[1].tolist(), len(cols[0])
    rows = lambda keep: sorted((A[r], B[r], r) for r in range(N) if keep(r))
    a, b = ENC_TV(col(0)), ENC_TV(col(1))
    plan = run(z["gs"], cols, lambda pb, t: pb.filter(t, EBV(P.GT(P.MUL(a, b), P.integer(6)))))
    assert kept_rows(plan) == rows(lambda r: cmp_num(R.binary(abi.EX_MUL, val(A[r])[0], val(B[r])[0]), (abi.TV_INTEGER, 6)) == 1)
    plan = run(z["gs"], cols, lambda pb, t: pb.filter(t, EBV(P.EQ(P.xsd_integer(a), P.integer(2)))))
    want = rows(lambda r: cast_ref(val, abi.TV_INTEGER, A[r]) == (abi.TV_INTEGER, 2))
    assert kept_rows(plan) == want and len(want) >= len(z["ids"])      # 2.5 as decimal, float and double
    plan = run(z["gs"], cols, lambda pb, t: pb.filter(t, EBV(P.xsd_boolean(b))))
    assert kept_rows(plan) == rows(lambda r: cast_ref(val, abi.TV_BOOLEAN, B[r]) == (abi.TV_BOOLEAN, 1))


def test_join_filter_with_div(torch_cuda):
    import torch
    tv = np.zeros(41, TV_DTYPE)
    tv["tag"][1:] = abi.TV_INTEGER
    tv["lo"][1:] = np.arange(-10, 30)
    gs, _ = both_stores(EMPTY, typed=tv)
    rng = np.random.default_rng(9)
    lk, lv = rng.integers(1, 12, 200).astype(np.uint32), rng.integers(1, 41, 200).astype(np.uint32)
    rk, rv = rng.integers(1, 12, 200).astype(np.uint32), rng.integers(1, 41, 200).astype(np.uint32)
    pb = PlanBuilder()
    l, r = pb.table(0, 2), pb.table(1, 2)
    f = EBV(P.LT(P.DIV(ENC_TV(col(1)), P.integer(3)), ENC_TV(col(3))))
    plan = gs.plan(pb.build(pb.hash_join(l, r, on=[(0, 0)], filter=f)))
    kl, pl = table_on_device(torch, [lk, lv])
    kr, pr = table_on_device(torch, [rk, rv])
    plan.bind_table(0, pl, 200)
    plan.bind_table(1, pr, 200)
    plan.execute()
    value = lambda i: int(tv["lo"][i])
    want = sorted((int(lk[i]), int(lv[i]), int(rk[j]), int(rv[j])) for i in range(200) for j in range(200)
                  if lk[i] == rk[j] and R.dec_div(value(lv[i]) * E18, 3 * E18) < value(rv[j]) * E18)
    assert kept_rows(plan) == want and want
    del kl, kr


# ---------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------
def compile_status(gs, build):
    pb = PlanBuilder()
    t = pb.table(0, 3)
    root = build(pb, t)
    with pytest.raises(RdfGpuError) as e:
        gs.plan(pb.build(root))
    return e.value.status


def test_compile_refusals(torch_cuda, zoo):
    gs = zoo["gs"]
    x = ENC_TV(col(1))
    U, INV = abi.ERR_UNSUPPORTED, abi.ERR_INVALID
    for tag in (abi.TV_STRING, abi.TV_DATE_TIME, abi.TV_NULL, abi.TV_OTHER, 200):
        assert compile_status(gs, lambda pb, t: pb.filter(t, EBV(P.CAST(x, tag)))) == U, tag
    for fn in (abi.AGG_COUNT, abi.AGG_COUNT_DISTINCT):
        assert compile_status(gs, lambda pb, t: pb.aggregate(t, [0], [(fn, P.NEG(x))])) == U, fn
    assert compile_status(gs, lambda pb, t: pb.aggregate(t, [0], [(SUM, EBV(x))])) == INV        # leaves a BOOL
    assert compile_status(gs, lambda pb, t: pb.aggregate(t, [0], [(SUM, P.LANGMATCHES_LANG(x, "en", ["", "en"]))])) == U   # pattern / table ops are prepared for filters and joins only
    assert compile_status(gs, lambda pb, t: pb.aggregate(t, [0], [(AVG, col(1))])) == INV        # leaves an ID

    def bad_offset(pb, t):
        g = pb.aggregate(t, [0], [(SUM, P.NEG(x))])
        pb.pool[pb.nodes[g].table_slot + 1] = abi.AGG_INPUT_EXPR | (len(pb.pool) - 1)         # the pair would end outside the pool
        return g
    assert compile_status(gs, bad_offset) == INV


def test_cast_of_a_simple_literal_fails_the_execute(torch_cuda, zoo):
    z = zoo
    tags, aux = z["tv"]["tag"], z["tv"]["aux"]
    simple = int(np.flatnonzero((tags == abi.TV_STRING) & (aux == 0))[0])
    ids = z["ids"]
    for with_literal in (True, False):
        c = np.append(ids, simple).astype(np.uint32) if with_literal else ids
        build = lambda pb, t: pb.aggregate(t, [0], [(SUM, P.xsd_double(ENC_TV(col(0))))])
        if with_literal:
            with pytest.raises(RdfGpuError) as e:
                run(z["gs"], [c], build)
            assert e.value.status == abi.ERR_UNSUPPORTED
        else:
            assert run(z["gs"], [c], build).result_info()[0] == len(set(c.tolist()))


# ---------------------------------------------------------------------------------------------------
# 4. the column-input aggregate and an ADD-only filter are what they were
# ---------------------------------------------------------------------------------------------------
def test_unchanged_paths(torch_cuda, zoo):
    import torch
    z, val = zoo, zoo["val"]
    cols = z["pairs"]
    check_filter(torch, z["gs"], z["os"], EBV(P.GT(P.ADD(ENC_TV(col(0)), ENC_TV(col(1))), P.integer(3))), cols)
    plan = run(z["gs"], cols, lambda pb, t: pb.aggregate(t, [0, 1, 2], [(SUM, 1), (AVG, 1)]), timing=True)
    assert not any("agg_accum_expr_kernel" in s[0] for s in plan.kernel_stats())
    rows = plan.fetch()[2].tolist()
    s, v = plan.fetch_aggregate(0), plan.fetch_aggregate(1)
    B = cols[1].tolist()
    for r, row in enumerate(rows):
        ref = val(B[row])[0]
        assert R.device_bits(int(s["tag"][r]), int(s["lo"][r]), int(s["hi"][r])) == R.bits(exact(sum_agg([plain(ref)]))), (row, ref)
        assert R.device_bits(int(v["tag"][r]), int(v["lo"][r]), int(v["hi"][r])) == R.bits(exact(avg_agg([plain(ref)]))), (row, ref)
