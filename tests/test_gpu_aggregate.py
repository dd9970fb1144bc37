"""AggregateExec (GROUP BY with COUNT / COUNT DISTINCT / SUM / AVG) on the MI355X.

The CPU oracle has no aggregate operator.  The expected values come from it anyway: it runs the aggregate's INPUT plan, and the
restatement of the reference's accumulators in test_aggregate_cpu.py is applied to those rows, group by group.  COUNT, integer and
decimal results are compared exactly; float and double results against the bound include/rdfgpu.h states, computed with math.fsum.
The large shapes (up to 2^24 rows) take their expectation from numpy over the same bound table."""
from collections import defaultdict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rdf_fusion_amd import abi, bsbm
from rdf_fusion_amd.engine import RdfGpuError, TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, quad_pattern, col, integer, EBV, GT, ENC_TV
from test_gpu_parity import both_stores, table_on_device, typed_zoo
from test_aggregate_cpu import sum_agg, avg_agg, count_agg, count_distinct_agg, same, decimal_checked_div, E18

EMPTY = (np.zeros(0, np.uint32),) * 4
STAR, COUNT, DISTINCT, SUM, AVG = abi.AGG_COUNT_STAR, abi.AGG_COUNT, abi.AGG_COUNT_DISTINCT, abi.AGG_SUM, abi.AGG_AVG
FORMS = [None, "NO_AGG_LDS"]


def value_table(tv, dec):
    """object id -> (tag, payload) as test_aggregate_cpu's restatement takes it; ids beyond the table and id 0 are unbound."""
    out = []
    for i in range(len(tv)):
        tag, lo = int(tv[i]["tag"]), int(tv[i]["lo"])
        if i == 0:
            out.append((abi.TV_NULL, None))
        elif tag == abi.TV_DECIMAL:
            d = (int(np.uint64(np.int64(dec[lo][1]).view(np.uint64))) << 64) | int(np.int64(dec[lo][0]).view(np.uint64))
            out.append((tag, d - (1 << 128) if d >= 1 << 127 else d))
        elif tag == abi.TV_FLOAT:
            out.append((tag, float(np.array([lo & 0xFFFFFFFF], np.uint32).view(np.float32)[0])))
        elif tag == abi.TV_DOUBLE:
            out.append((tag, float(np.array([lo], np.int64).view(np.float64)[0])))
        else:
            out.append((tag, lo))
    return lambda i: out[i] if 0 < i < len(out) else (abi.TV_NULL, None)


def expected_groups(cols, n, keys, aggs, val):
    """{key tuple: [expected (tag, payload | Approx) per aggregate]} by the restatement, over rows [0, n) of host columns `cols`."""
    groups = defaultdict(list)
    kc = [np.asarray(cols[k][:n]).tolist() for k in keys]
    for r in range(n):
        groups[tuple(c[r] for c in kc)].append(r)
    if not keys and not groups:
        groups[()] = []
    out = {}
    for key, rows in groups.items():
        res = []
        for fn, c in aggs:
            ids = [int(cols[c][r]) for r in rows] if c is not None else []
            if fn == STAR:
                res.append((abi.TV_INTEGER, len(rows)))
            elif fn == COUNT:
                res.append(count_agg(ids))
            elif fn == DISTINCT:
                res.append(count_distinct_agg(ids))
            elif fn == SUM:
                res.append(sum_agg([val(i) for i in ids]))
            else:
                res.append(avg_agg([val(i) for i in ids]))
        out[key] = res
    return out


def device_groups(plan, n_aggs):
    n, nk = plan.result_info()
    keys = plan.fetch()
    vals = [plan.fetch_aggregate(a) for a in range(n_aggs)]
    assert plan.agg_count() == n_aggs
    out = {}
    for r in range(n):
        key = tuple(int(keys[q][r]) for q in range(nk))
        assert key not in out, f"group {key} appears twice"
        out[key] = [(int(v["tag"][r]), int(v["lo"][r]), int(v["hi"][r])) for v in vals]
    return out


def check_groups(exp, got):
    assert set(exp) == set(got), (len(exp), len(got))
    for key, e in exp.items():
        for a, (ev, gv) in enumerate(zip(e, got[key])):
            assert same(ev, gv), (key, a, ev if not hasattr(ev[1], "terms") else (ev[0], ev[1].exact()), gv)


def run_table(gs, cols, keys, aggs, form=None, timing=False):
    import torch
    pb = PlanBuilder()
    t = pb.table(0, len(cols))
    desc = pb.build(pb.aggregate(t, keys, aggs))
    keep, ptrs = table_on_device(torch, cols)
    plan = gs.plan(desc)
    if form:
        plan.set_option(form)
    if timing:
        plan.enable_kernel_timing(True)
    plan.bind_table(0, ptrs, len(cols[0]))
    plan.execute()
    plan._keep_cols = keep
    return plan


# ---------------------------------------------------------------------------------------------------
# 1. every function x 0..4 keys x both accumulator forms, over typed_zoo values
# ---------------------------------------------------------------------------------------------------
def zoo_columns(tv, n_rows, n_keys, key_range, rng):
    tags = tv["tag"]
    ids = np.arange(len(tv) + 2, dtype=np.uint32)            # with id 0 and ids beyond the table (unbound)
    pick = lambda sel: rng.choice(ids[sel], n_rows).astype(np.uint32)
    num = np.isin(np.append(tags, [0, 0]), [abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE])
    lo = np.append(tv["lo"], [0, 0])
    small_int = np.isin(np.append(tags, [0, 0]), [abi.TV_INT, abi.TV_INTEGER]) & (np.abs(lo) < 10 ** 6)
    dec_ok = small_int | (np.append(tags, [0, 0]) == abi.TV_DECIMAL)
    flt = small_int | (np.append(tags, [0, 0]) == abi.TV_FLOAT)
    keys = [rng.integers(0, key_range, n_rows).astype(np.uint32) for _ in range(n_keys)]
    vals = [pick(slice(None)), pick(num), pick(small_int), pick(dec_ok), pick(flt)]
    return keys + vals


@pytest.mark.parametrize("n_keys", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("few", [True, False])
@pytest.mark.parametrize("form", FORMS)
def test_every_function_keys_and_forms(torch_cuda, n_keys, few, form):
    tv, dec = typed_zoo()
    gs, _ = both_stores(EMPTY, typed=tv, decimals=dec)
    val = value_table(tv, dec)
    rng = np.random.default_rng(n_keys * 10 + few)
    key_range = {0: 1, 1: 6, 2: 3, 3: 2, 4: 2}[n_keys] if few else {0: 1, 1: 900, 2: 30, 3: 10, 4: 6}[n_keys]
    cols = zoo_columns(tv, 3000, n_keys, key_range, rng)
    k = list(range(n_keys))
    v_all, v_num, v_int, v_dec, v_flt = range(n_keys, n_keys + 5)
    plans = [[(STAR, None), (COUNT, v_all), (DISTINCT, v_all), (SUM, v_all), (AVG, v_all), (SUM, v_int), (AVG, v_dec), (SUM, v_num)],
             [(AVG, v_int), (SUM, v_dec), (SUM, v_flt), (AVG, v_flt), (AVG, v_num), (COUNT, v_int), (DISTINCT, v_num)]]
    for aggs in plans:
        plan = run_table(gs, cols, k, aggs, form, timing=True)
        check_groups(expected_groups(cols, len(cols[0]), k, aggs, val), device_groups(plan, len(aggs)))
        names = [s[0] for s in plan.kernel_stats()]
        if form:
            assert any(n.startswith("void rdfgpu::agg_accum_kernel<false>") for n in names), names
    if few and form is None:   # every group's accumulators fit: the LDS partials form ran
        assert any(n.startswith("void rdfgpu::agg_accum_kernel<true>") for n in names), names


# ---------------------------------------------------------------------------------------------------
# 2. group counts, hot groups, sorted and shuffled (numpy expectation)
# ---------------------------------------------------------------------------------------------------
def integer_store():
    tv = np.zeros(1001, TV_DTYPE)                 # id i = xsd:integer i
    tv["tag"][1:] = abi.TV_INTEGER
    tv["lo"][1:] = np.arange(1, 1001)
    gs, _ = both_stores(EMPTY, typed=tv)
    return gs


def check_numpy(plan, key, val):
    uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    sums = np.bincount(inv, weights=val.astype(np.float64)).astype(np.int64)
    pairs = np.unique(inv.astype(np.int64) << 32 | val.astype(np.int64))
    dcnt = np.bincount((pairs >> 32).astype(np.int64), minlength=len(uk))
    n, _ = plan.result_info()
    assert n == len(uk)
    gk = plan.fetch()[0]
    order = np.argsort(gk)
    assert np.array_equal(gk[order], uk)
    star, s, d = (plan.fetch_aggregate(a)[order] for a in range(3))
    assert (star["tag"] == abi.TV_INTEGER).all() and np.array_equal(star["lo"], cnt)
    assert (s["tag"] == abi.TV_INTEGER).all() and np.array_equal(s["lo"], sums)
    assert np.array_equal(d["lo"], dcnt)


@pytest.mark.parametrize("groups,rows", [(1, 1 << 22), (64, 1 << 22), (4096, 1 << 22), (1 << 20, 1 << 22), (1 << 22, 1 << 24)])
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_group_counts(torch_cuda, groups, rows, order):
    gs = integer_store()
    rng = np.random.default_rng(groups)
    key = (rng.integers(0, groups, rows) * 7 + 3).astype(np.uint32)
    val = rng.integers(1, 1001, rows).astype(np.uint32)
    if order == "sorted":
        o = np.argsort(key, kind="stable")
        key, val = key[o], val[o]
    for form in FORMS:
        plan = run_table(gs, [key, val], [0], [(STAR, None), (SUM, 1), (DISTINCT, 1)], form)
        check_numpy(plan, key, val)


@pytest.mark.parametrize("groups", [1 << 10, 1 << 20])
def test_hot_group(torch_cuda, groups):
    gs = integer_store()
    rng = np.random.default_rng(7)
    rows = 1 << 22
    key = np.where(rng.random(rows) < 0.9, 5, rng.integers(0, groups, rows) + 10).astype(np.uint32)
    val = rng.integers(1, 1001, rows).astype(np.uint32)
    for k, v in ((key, val), (np.sort(key), val)):
        for form in FORMS:
            check_numpy(run_table(gs, [k, v], [0], [(STAR, None), (SUM, 1), (DISTINCT, 1)], form), k, v)


# ---------------------------------------------------------------------------------------------------
# 3. BSBM-shaped plans (Business Intelligence Q8 / Q4 shapes)
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bsbm_stores():
    ds = bsbm.generate(1000)
    gs, os_ = both_stores((ds.g, ds.s, ds.p, ds.o), typed=ds.typed_values, decimals=ds.decimals)
    return ds, gs, os_


def offers_of_type(pb, ds):
    pr = ds.pred
    prod = pb.data_source(quad_pattern("product", pr["rdf:type"], ds.type_base + ds.n_types - 1))
    offers = pb.hash_join(pb.data_source(quad_pattern("offer", pr["bsbm:product"], "product")), prod, on=[(1, 0)], projection=[0, 1])
    return pb.hash_join(offers, pb.data_source(quad_pattern("offer", pr["bsbm:vendor"], "vendor")), on=[(0, 0)], projection=[0, 3])


def offer_pairs(pb, ds, what):
    pr = ds.pred
    return pb.hash_join(pb.data_source(quad_pattern("offer", pr["bsbm:product"], "product")),
                        pb.data_source(quad_pattern("offer", pr[what], "x")), on=[(0, 0)], projection=[0, 1, 3])


@pytest.mark.parametrize("shape", ["q8_count_by_vendor", "avg_price_by_product", "distinct_vendors_by_product"])
@pytest.mark.parametrize("form", FORMS)
def test_bsbm_shapes(torch_cuda, bsbm_stores, shape, form):
    ds, gs, os_ = bsbm_stores
    val = value_table(ds.typed_values, ds.decimals)
    pb = PlanBuilder()
    if shape == "q8_count_by_vendor":            # COUNT(?offer) GROUP BY ?vendor over offers of one product type
        inp, keys, aggs = offers_of_type(pb, ds), [1], [(COUNT, 0), (STAR, None)]
    elif shape == "avg_price_by_product":        # AVG(?price) GROUP BY ?product
        inp, keys, aggs = offer_pairs(pb, ds, "bsbm:price"), [1], [(AVG, 2), (SUM, 2), (COUNT, 2)]
    else:                                        # COUNT(DISTINCT ?vendor) GROUP BY ?product
        inp, keys, aggs = offer_pairs(pb, ds, "bsbm:vendor"), [1], [(DISTINCT, 2), (STAR, None)]
    cols, n, _ = os_.execute(pb.build(inp))
    assert n > 0
    exp = expected_groups(cols, n, keys, aggs, val)
    plan = gs.plan(pb.build(pb.aggregate(inp, keys, aggs)))
    if form:
        plan.set_option(form)
    plan.execute()
    check_groups(exp, device_groups(plan, len(aggs)))


def test_bsbm_distinct_as_join_input(torch_cuda, bsbm_stores):
    """BI Q4 shape: `AggregateExec gby=[x], aggr=[]` over a join, used as the build side of another join.  The oracle runs the same plan
    with the DISTINCT done in numpy and bound as a table."""
    ds, gs, os_ = bsbm_stores
    pr = ds.pred
    pb = PlanBuilder()
    inp = offers_of_type(pb, ds)
    d = pb.aggregate(inp, [1])
    top = pb.hash_join(d, pb.data_source(quad_pattern("vendor", pr["bsbm:country"], "country")), on=[(0, 0)], projection=[0, 2])
    plan = gs.plan(pb.build(top)).execute()
    n, _ = plan.result_info()
    got = sorted(zip(*[c.tolist() for c in plan.fetch()]))
    cols, m, _ = os_.execute(pb.build(inp))
    vendors = np.unique(np.asarray(cols[1][:m]))
    pb2 = PlanBuilder()
    t = pb2.table(0, 1, ["vendor"])
    top2 = pb2.hash_join(t, pb2.data_source(quad_pattern("vendor", pr["bsbm:country"], "country")), on=[(0, 0)], projection=[0, 2])
    ecols, ne, _ = os_.execute(pb2.build(top2), [[vendors]])
    assert n == ne > 0
    assert got == sorted(zip(*[np.asarray(c[:ne]).tolist() for c in ecols]))


# ---------------------------------------------------------------------------------------------------
# 4. edge cases
# ---------------------------------------------------------------------------------------------------
def test_empty_input(torch_cuda):
    """With keys an empty input has no group; without keys there is one: COUNT 0, SUM integer 0, AVG integer 0 (avg.rs)."""
    import torch
    gs = integer_store()
    aggs = [(STAR, None), (COUNT, 1), (SUM, 1), (AVG, 1), (DISTINCT, 1)]
    keep, ptrs = table_on_device(torch, [np.arange(1, 101, dtype=np.uint32), np.arange(1, 101, dtype=np.uint32)])
    for keys, rows in (([], 1), ([0], 0)):
        for filtered in (True, False):   # no row passes the filter (count on the device) / an empty bound table
            pb = PlanBuilder()
            t = pb.table(0, 2)
            src = pb.filter(t, EBV(GT(ENC_TV(col(1)), integer(10 ** 9)))) if filtered else t
            plan = gs.plan(pb.build(pb.aggregate(src, keys, aggs)))
            plan.bind_table(0, ptrs, 100 if filtered else 0)
            plan.execute()
            assert plan.result_info() == (rows, len(keys))
            if rows:
                assert [plan.aggregate_values(a) for a in range(len(aggs))] == [[0]] * 5
                assert [int(plan.fetch_aggregate(a)["tag"][0]) for a in range(len(aggs))] == [abi.TV_INTEGER] * 5
    del keep


def test_integer_overflow_and_decimal_truncation(torch_cuda):
    tv = np.zeros(6, TV_DTYPE)
    tv[1] = (2 ** 63 - 1, 0, abi.TV_INTEGER, 0, 0)
    tv[2] = (1, 0, abi.TV_INTEGER, 0, 0)
    tv[3] = (2, 0, abi.TV_INTEGER, 0, 0)
    tv[4] = (-1, 0, abi.TV_INTEGER, 0, 0)
    tv[5] = (0, 0, abi.TV_DECIMAL, 0, 0)          # decimal 10^-18
    dec = np.array([[1, 0]], np.int64)
    gs, _ = both_stores(EMPTY, typed=tv, decimals=dec)
    key = np.array([1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5] + [6] * 10, np.uint32)
    val = np.array([1, 2, 2, 3, 3, 1, 2, 4, 4, 3, 3, 1] + [5] + [0] * 9, np.uint32)
    from fractions import Fraction
    big = 2 ** 63 - 1
    want = {1: (None, Fraction(decimal_checked_div((big + 1) * E18, 2 * E18), E18)),   # i64 max + 1: SUM overflows, AVG is a decimal
            2: (5, Fraction(1666666666666666666, E18)),                             # AVG(1, 2, 2) truncated
            3: (big, Fraction(decimal_checked_div(big * E18, 3 * E18), E18)),        # the total decides, not the prefix
            4: (3, Fraction(1)),                                                    # (-1 + 2 + 2) / 3
            5: (big, Fraction(big)),
            6: (Fraction(1, E18), None)}                                            # unbound rows: SUM skips them, AVG is an error
    for form in FORMS:
        plan = run_table(gs, [key, val], [0], [(SUM, 1), (AVG, 1)], form)
        got = dict(zip(plan.fetch()[0].tolist(), zip(plan.aggregate_values(0), plan.aggregate_values(1))))
        assert got == want, (form, got)


def test_reexecute_and_store_mutation(torch_cuda):
    tv = np.zeros(64, TV_DTYPE)
    tv["tag"][1:] = abi.TV_INTEGER
    tv["lo"][1:] = np.arange(1, 64)
    rng = np.random.default_rng(3)
    s, o = rng.integers(1, 40, 500).astype(np.uint32), rng.integers(1, 64, 500).astype(np.uint32)
    quads = (np.zeros(500, np.uint32), s, np.full(500, 50, np.uint32), o)
    gs, os_ = both_stores(quads, typed=tv)
    pb = PlanBuilder()
    src = pb.data_source(quad_pattern("s", 50, "o"))
    aggs = [(STAR, None), (SUM, 1), (AVG, 1), (DISTINCT, 1)]
    plan = gs.plan(pb.build(pb.aggregate(src, [0], aggs)))
    val = value_table(tv, np.zeros((0, 2), np.int64))
    for step in range(3):
        if step == 2:
            more = (np.zeros(50, np.uint32), rng.integers(30, 60, 50).astype(np.uint32), np.full(50, 50, np.uint32),
                    rng.integers(1, 64, 50).astype(np.uint32))
            assert gs.extend(*more) == os_.extend(*more)
        plan.execute()
        cols, n, _ = os_.execute(pb.build(src))
        check_groups(expected_groups(cols, n, [0], aggs, val), device_groups(plan, len(aggs)))


def test_arrow_export_of_keys_and_aggregates(torch_cuda):
    import pyarrow as pa
    tv, dec = typed_zoo()
    gs, _ = both_stores(EMPTY, typed=tv, decimals=dec, batch=100)
    rng = np.random.default_rng(11)
    cols = zoo_columns(tv, 2000, 1, 300, rng)
    aggs = [(COUNT, 1), (AVG, 2), (SUM, 3)]
    plan = run_table(gs, cols, [0], aggs)
    n, _ = plan.result_info()
    batches = list(plan.batches())
    assert sum(len(b) for b in batches) == n and all(0 < len(b) <= 100 for b in batches)
    arr = pa.concat_arrays(batches)
    assert arr.type.num_fields == 4
    assert arr.type.field(1).type == pa.struct([("tag", pa.uint8()), ("lo", pa.int64()), ("hi", pa.int64())])
    keys = plan.fetch()[0]
    assert arr.field(0).is_null().to_numpy(zero_copy_only=False).tolist() == (keys == 0).tolist()   # id 0 (a group of its own) is a null
    assert arr.field(0).fill_null(0).to_numpy().tolist() == keys.tolist()
    for a in range(len(aggs)):
        v = plan.fetch_aggregate(a)
        child = arr.field(1 + a)
        assert child.is_null().to_numpy(zero_copy_only=False).tolist() == (v["tag"] == abi.TV_NULL).tolist()
        assert child.field("lo").to_numpy().tolist() == v["lo"].tolist()
        assert child.field("hi").to_numpy().tolist() == v["hi"].tolist()
        assert child.field("tag").to_numpy().tolist() == v["tag"].tolist()


def test_device_pointer(torch_cuda):
    gs = integer_store()
    plan = run_table(gs, [np.array([1, 2, 1], np.uint32), np.array([3, 4, 5], np.uint32)], [0], [(SUM, 1)])
    assert plan.aggregate_device(0) != 0
    assert sorted(plan.aggregate_values(0)) == [4, 8]


# ---------------------------------------------------------------------------------------------------
# 5. refused at compile
# ---------------------------------------------------------------------------------------------------
def test_compile_refusals(torch_cuda):
    gs = integer_store()

    def compile_status(build):
        pb = PlanBuilder()
        t = pb.table(0, 6)
        root = build(pb, t)
        with pytest.raises(RdfGpuError) as e:
            gs.plan(pb.build(root))
        return e.value.status

    U = abi.ERR_UNSUPPORTED
    for fn in (abi.AGG_MIN, abi.AGG_MAX, abi.AGG_SAMPLE, abi.AGG_GROUP_CONCAT, abi.AGG_SUM_DISTINCT, abi.AGG_AVG_DISTINCT,
               abi.AGG_COUNT_DISTINCT_STAR):
        assert compile_status(lambda pb, t: pb.aggregate(t, [0], [(fn, 1)])) == U, fn
    assert compile_status(lambda pb, t: pb.filter(pb.aggregate(t, [0], [(COUNT, 1)]), EBV(GT(ENC_TV(col(0)), integer(1))))) == U
    assert compile_status(lambda pb, t: pb.hash_join(pb.aggregate(t, [0], [(SUM, 1)]), t, on=[(0, 0)])) == U
    assert compile_status(lambda pb, t: pb.aggregate(t, [0, 1, 2, 3, 4], [(COUNT, 5)])) == U
    assert compile_status(lambda pb, t: pb.aggregate(t, [0], [(COUNT, 1)] * 9)) == U
    assert compile_status(lambda pb, t: pb.aggregate(t, [0], [(99, 1)])) == abi.ERR_INVALID
    # the DISTINCT form (no aggregates) is an id operator: fine anywhere
    pb = PlanBuilder()
    t = pb.table(0, 2)
    gs.plan(pb.build(pb.hash_join(pb.aggregate(t, [1]), t, on=[(0, 1)])))


def test_input_of_2_32_rows_fails_at_execute(torch_cuda):
    gs = integer_store()
    import torch
    keep, ptrs = table_on_device(torch, [np.ones(16, np.uint32)])
    pb = PlanBuilder()
    plan = gs.plan(pb.build(pb.aggregate(pb.table(0, 1), [0], [(STAR, None)])))
    plan.set_option("NO_PRIMING")          # (no run over a prefix of the table first: the 16 rows are all there is)
    plan.bind_table(0, ptrs, 1 << 32)      # never read: refused before any launch
    with pytest.raises(RdfGpuError) as e:
        plan.execute()
    assert e.value.status == abi.ERR_UNSUPPORTED
    del keep
