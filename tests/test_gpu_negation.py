"""LeftSemi / LeftAnti joins (FILTER EXISTS, FILTER NOT EXISTS, MINUS) on the MI355X.

The CPU oracle runs every join type other than LEFT as an inner join, so it is never given a semi or anti join.  The expected
rows are derived from it instead: run the left input on its own (Lrows); run the same join as INNER, with the same keys and
filter, projected onto the left columns; the distinct tuples of that are the left rows that have a match (M).  Semi = the rows
of Lrows whose tuple is in M, anti = the others, both as multisets.  Exact, because whether a left row matches depends only on
its values."""
import json
import os
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rdf_fusion_amd import abi, bsbm
from rdf_fusion_amd.plan import (PlanBuilder, quad_pattern, col, integer, ENC_TV, LT, ADD, EBV, ID_NEQ, ID_EQ, AND, OR, NOT,
                                 BOUND, IS_COMPATIBLE)
from test_gpu_parity import both_stores, table_on_device, typed_zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEMI, ANTI = abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT_ANTI
EMPTY = (np.zeros(0, np.uint32),) * 4


def rows_of(cols, n):
    return Counter(zip(*[np.asarray(c[:n]).tolist() for c in cols])) if cols else Counter({(): n} if n else {})


def derive(os_, build, kind, on, flt, anti, proj=None, tables=None):
    """The semi / anti join's expected multiset, from two oracle runs (see the module docstring).  `build(pb) -> (left, right)`."""
    pb = PlanBuilder()
    l, _ = build(pb)
    wl = pb.width[l]
    lcols, nl, _ = os_.execute(pb.build(l), tables)
    pb = PlanBuilder()
    l, r = build(pb)
    keep = list(range(wl))
    if kind != abi.NODE_HASH_JOIN and flt is None:   # no keys, no filter: every left row matches iff the right input has a row
        _, nr, _ = os_.execute(pb.build(r), tables)
        M = set(rows_of(lcols, nl)) if nr else set()
    elif kind == abi.NODE_HASH_JOIN:
        m = pb.hash_join(l, r, on, join_type=abi.JOIN_INNER, filter=flt, projection=keep)
    else:
        m = pb.nested_loop_join(l, r, abi.JOIN_INNER, filter=flt, projection=keep)
    if kind == abi.NODE_HASH_JOIN or flt is not None:
        mcols, nm, _ = os_.execute(pb.build(m), tables)
        M = set(rows_of(mcols, nm))
    out = Counter()
    for t, c in rows_of(lcols, nl).items():
        if (t in M) != anti:
            out[t if proj is None else tuple(t[q] for q in proj)] += c
    return out


def fetch_rows(plan):
    n, _ = plan.result_info()
    return rows_of(plan.fetch(), n)


def kernels(plan):
    return [k[0] for k in plan.kernel_stats()]


# ---------------------------------------------------------------------------------------------------
# 1. the reference's vectors: testsuite/oxigraph-tests/sparql/{values_in_filter_exists, values_in_filter_not_exists,
#    subquery_in_filter_not_exists}.rq -> values_in_filter_exists.srx (manifest.ttl:96-109)
# ---------------------------------------------------------------------------------------------------
def test_reference_filter_exists_vectors(torch_cuda):
    with open(os.path.join(ROOT, "tests", "golden", "negation_kats.json")) as f:
        k = json.load(f)
    term = k["terms"]
    expected = Counter(tuple(term[v] for v in row) for row in k["expected"]["rows"])
    gs, _ = both_stores(EMPTY)
    for case in k["cases"]:
        outer = np.array([term[v] for v in case["outer_values"]["s"]], np.uint32)
        inner = np.array([term[v] for v in case["inner_values"]["s"]], np.uint32)
        pb = PlanBuilder()
        o, i = pb.table(0, 1, ["s"]), pb.table(1, 1, ["s"])     # VALUES ?s { .. } as bound tables
        root = pb.sparql_exists(o, i, negate=case["negate"])
        ko, po = table_on_device(torch_cuda, [outer])
        ki, pi = table_on_device(torch_cuda, [inner])
        plan = gs.plan(pb.build(root))
        plan.bind_table(0, po, len(outer)); plan.bind_table(1, pi, len(inner))
        for _ in range(2):
            plan.execute()
            assert fetch_rows(plan) == expected, case["name"]
        del ko, ki


# ---------------------------------------------------------------------------------------------------
# 2. every table form, semi and anti, with and without a join filter
# ---------------------------------------------------------------------------------------------------
FORMS = {
    # name: (join kind, store options, right rows, kernel that has to have run)
    "lds_set": (abi.NODE_HASH_JOIN, {}, 700, "semi_join_kernel<0, "),
    "lds_set_large": (abi.NODE_HASH_JOIN, {"LDS_MAX_BUILD": 8192}, 8000, "semi_join_kernel<0, "),
    "hbm_set_forced": (abi.NODE_HASH_JOIN, {"NO_SEMI_LDS": 1}, 700, "semi_join_kernel<1, "),
    "hbm_set_large": (abi.NODE_HASH_JOIN, {}, 12_000, "semi_join_kernel<1, "),
    "nested_loop": (abi.NODE_NESTED_LOOP_JOIN, {}, 900, "semi_nested_kernel<"),
}
FILTERS = {
    "none": None,
    "id_pair": ID_NEQ(col(1), col(4)),                                                              # left col 1 vs right col 1
    "vm": AND(EBV(LT(ENC_TV(col(4)), ADD(ENC_TV(col(2)), integer(3)))), BOUND(col(1))),
}


def rand_cols(rng, n, ncols, n_ids, null_frac=0.1):
    cols = [rng.integers(1, n_ids, n).astype(np.uint32) for _ in range(ncols)]
    for c in cols:
        c[rng.random(n) < null_frac] = 0
    return cols


def run_case(torch, gs, os_, kind, jt, L, R, on, flt, proj, expect_kernel=None, options=None):
    def build(pb):
        return pb.table(0, len(L)), pb.table(1, len(R))
    pb = PlanBuilder()
    l, r = build(pb)
    if kind == abi.NODE_HASH_JOIN:
        root = pb.hash_join(l, r, on, join_type=jt, filter=flt, projection=proj)
    else:
        root = pb.nested_loop_join(l, r, jt, filter=flt, projection=proj)
    desc = pb.build(root)
    exp = derive(os_, build, kind, on, flt, jt == ANTI, proj, tables=[L, R])
    kl, pl = table_on_device(torch, L)
    kr, pr = table_on_device(torch, R)
    seen = set()
    for fresh in range(2):
        plan = gs.plan(desc).enable_kernel_timing(True)
        for name, value in (options or {}).items():
            plan.set_option(name, value)
        plan.bind_table(0, pl, len(L[0])); plan.bind_table(1, pr, len(R[0]))
        for _ in range(3 if fresh == 0 else 1):
            plan.execute()
            assert fetch_rows(plan) == exp
            m = plan.metrics()
            assert m.exact_reruns == 0 and m.output_rows == sum(exp.values())
            seen.update(kernels(plan))
    if expect_kernel is not None:
        assert any(expect_kernel in k for k in seen), (expect_kernel, sorted(seen))
    del kl, kr
    return exp


@pytest.fixture(scope="module")
def zoo_stores():
    tv, dec = typed_zoo()
    return both_stores(EMPTY, typed=tv, decimals=dec)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("filt", list(FILTERS))
def test_every_table_form(torch_cuda, zoo_stores, form, filt):
    kind, options, nr, kernel = FORMS[form]
    gs, os_ = zoo_stores
    rng = np.random.default_rng(len(form) * 31 + len(filt))
    n_ids = 200
    L = rand_cols(rng, 8000, 3, n_ids)
    L = [np.concatenate([c, c[:300]]) for c in L]                  # duplicate left rows
    R = rand_cols(rng, nr, 2, n_ids, null_frac=0.05)              # small domain: duplicate right keys
    flt = FILTERS[filt]
    if kind == abi.NODE_NESTED_LOOP_JOIN and flt is None:
        flt = ID_EQ(col(0), col(3))                                # a nested-loop join that has something to decide per row
    keysets = [[(0, 0)], [(0, 0), (1, 1)]] if kind == abi.NODE_HASH_JOIN else [[]]
    for on in keysets:
        for jt in (SEMI, ANTI):
            for proj in (None, [2, 0]):
                run_case(torch_cuda, gs, os_, kind, jt, L, R, on, flt, proj, kernel, options)


@pytest.mark.parametrize("kind", [abi.NODE_HASH_JOIN, abi.NODE_NESTED_LOOP_JOIN])
def test_empty_sides_and_filterless_nested_loop(torch_cuda, zoo_stores, kind):
    gs, os_ = zoo_stores
    rng = np.random.default_rng(5)
    L, R = rand_cols(rng, 3000, 3, 30), rand_cols(rng, 200, 2, 30)
    Z3, Z2 = [c[:0] for c in L], [c[:0] for c in R]
    on = [(0, 0)] if kind == abi.NODE_HASH_JOIN else []
    for jt in (SEMI, ANTI):
        for flt in (None, FILTERS["id_pair"]):
            for l, r in ((L, Z2), (Z3, R), (Z3, Z2), (L, R)):
                exp = run_case(torch_cuda, gs, os_, kind, jt, l, r, on, flt, [1, 2])
                if len(r[0]) == 0:
                    assert sum(exp.values()) == (len(l[0]) if jt == ANTI else 0)


def test_right_input_counted_on_the_device(torch_cuda, zoo_stores):
    """The right input is a FilterExec (its row count stays on the device): the nested-loop form without a filter decides on
    the device whether the right input has a row."""
    gs, os_ = zoo_stores
    rng = np.random.default_rng(9)
    L, R = rand_cols(rng, 4000, 2, 50), rand_cols(rng, 300, 1, 50)
    for pred in (BOUND(col(0)), AND(BOUND(col(0)), NOT(BOUND(col(0))))):      # the filter keeps some rows / none
        for jt in (SEMI, ANTI):
            for kind in (abi.NODE_NESTED_LOOP_JOIN, abi.NODE_HASH_JOIN):
                def build(pb):
                    return pb.table(0, 2), pb.filter(pb.table(1, 1), pred)
                pb = PlanBuilder()
                l, r = build(pb)
                on = [(1, 0)] if kind == abi.NODE_HASH_JOIN else []
                root = pb.hash_join(l, r, on, join_type=jt) if on else pb.nested_loop_join(l, r, jt)
                exp = derive(os_, build, kind, on, None, jt == ANTI, tables=[L, R])
                kl, pl = table_on_device(torch_cuda, L)
                kr, pr = table_on_device(torch_cuda, R)
                plan = gs.plan(pb.build(root))
                plan.bind_table(0, pl, len(L[0])); plan.bind_table(1, pr, len(R[0]))
                plan.execute()
                assert fetch_rows(plan) == exp, (jt, kind)
                del kl, kr


# ---------------------------------------------------------------------------------------------------
# 3. BSBM: NOT EXISTS in the Q3 shape equals OPTIONAL + FILTER(!BOUND); 4. inside larger plans
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bsbm_neg():
    ds = bsbm.generate(2000)
    gs, os_ = both_stores((ds.g, ds.s, ds.p, ds.o), typed=ds.typed_values, decimals=ds.decimals)
    return ds, gs, os_


def _features(ds):
    pf = ds.pred["bsbm:productFeature"]
    f, c = np.unique(ds.o[ds.p == pf], return_counts=True)
    top = f[np.argsort(-c)]
    return int(top[0]), int(top[1]), pf


def test_bsbm_not_exists_equals_optional_not_bound(bsbm_neg):
    ds, gs, os_ = bsbm_neg
    f1, f2, pf = _features(ds)

    def build(pb):
        l = pb.sparql_join(pb.data_source(quad_pattern("product", pf, f1)), pb.data_source(quad_pattern("product", ds.pred["rdfs:label"], "label")))
        return l, pb.data_source(quad_pattern("product", pf, f2))
    pb = PlanBuilder()
    l, r = build(pb)
    w = pb.width[l]
    anti = pb.sparql_exists(l, r, negate=True)
    pb2 = PlanBuilder()
    l2, r2 = build(pb2)
    opt = pb2.filter(pb2.hash_join(l2, r2, on=[(0, 0)], join_type=abi.JOIN_LEFT), NOT(BOUND(col(w))), projection=list(range(w)))
    exp = derive(os_, build, abi.NODE_HASH_JOIN, [(0, 0)], None, True)
    plan = gs.plan(pb.build(anti))
    for _ in range(3):
        plan.execute()
        assert fetch_rows(plan) == exp
    o_cols, o_n, _ = os_.execute(pb2.build(opt))
    assert rows_of(o_cols, o_n) == exp
    oplan = gs.plan(pb2.build(opt)).execute()
    assert fetch_rows(oplan) == exp
    assert 0 < sum(exp.values())
    # EXISTS: the complement within the left rows
    pb3 = PlanBuilder()
    l3, r3 = build(pb3)
    semi = gs.plan(pb3.build(pb3.sparql_exists(l3, r3))).execute()
    assert fetch_rows(semi) == derive(os_, build, abi.NODE_HASH_JOIN, [(0, 0)], None, False)


def test_semi_and_anti_inside_larger_plans(bsbm_neg, torch_cuda):
    ds, gs, os_ = bsbm_neg
    f1, f2, pf = _features(ds)
    label = ds.pred["rdfs:label"]

    def base(pb):   # (product, label) JOIN (product, feature): a join the engine may fuse into a look-up chain
        return pb.sparql_join(pb.sparql_join(pb.data_source(quad_pattern("product", pf, f1)),
                                             pb.data_source(quad_pattern("product", label, "label"))),
                              pb.data_source(quad_pattern("product", pf, "feat")))

    def build(pb):
        return base(pb), pb.data_source(quad_pattern("product", pf, f2))
    pb = PlanBuilder()
    l, r = build(pb)
    for jt in (SEMI, ANTI):
        exp = derive(os_, build, abi.NODE_HASH_JOIN, [(0, 0)], None, jt == ANTI)
        # the join itself over a fusable left input
        pb = PlanBuilder(); l, r = build(pb)
        s = pb.hash_join(l, r, [(0, 0)], join_type=jt)
        plan = gs.plan(pb.build(s))
        for _ in range(3):
            plan.execute()
            assert fetch_rows(plan) == exp
        # the probe side of an inner join above it
        pb = PlanBuilder(); l, r = build(pb)
        s = pb.hash_join(l, r, [(0, 0)], join_type=jt)
        top = pb.hash_join(s, pb.data_source(quad_pattern("product", ds.pred["rdf:type"], "type")), [(0, 0)], projection=[0, 2, 4])
        plan = gs.plan(pb.build(top))
        tcols, tn, _ = os_.execute(type_rows_plan(ds))
        types = {}
        for p_, t_ in zip(*[c[:tn].tolist() for c in tcols]):
            types.setdefault(p_, []).append(t_)
        want = Counter()
        for row, c in exp.items():
            for t_ in types.get(row[0], []):
                want[(row[0], row[2], t_)] += c
        for _ in range(3):
            plan.execute()
            assert fetch_rows(plan) == want
        # under UnionExec: semi UNION anti = the left rows
        pb = PlanBuilder(); l, r = build(pb)
        u = pb.union(pb.hash_join(l, r, [(0, 0)], join_type=SEMI), pb.hash_join(l, r, [(0, 0)], join_type=ANTI))
        lcols, ln_, _ = os_.execute(pb.build(l))
        uplan = gs.plan(pb.build(u))
        for _ in range(2):
            uplan.execute()
            assert fetch_rows(uplan) == rows_of(lcols, ln_)
        # under TopK: DISTINCT (product, feat) ORDER BY product, feat LIMIT 7
        pb = PlanBuilder(); l, r = build(pb)
        s = pb.hash_join(l, r, [(0, 0)], join_type=jt, projection=[0, 2])
        tk = pb.topk(s, [(0, abi.SORT_BY_ID)], 7)
        want = sorted({(row[0], row[2]) for row in exp})[:7]
        kplan = gs.plan(pb.build(tk))
        for _ in range(2):
            kplan.execute()
            n, _ = kplan.result_info()
            got = list(zip(*[c[:n].tolist() for c in kplan.fetch()]))      # as a sequence: TopK's rows come out in ORDER BY order
            assert got == want


def type_rows_plan(ds):
    pb = PlanBuilder()
    return pb.build(pb.data_source(quad_pattern("product", ds.pred["rdf:type"], "type")))


# ---------------------------------------------------------------------------------------------------
# 5. seeded random differential
# ---------------------------------------------------------------------------------------------------
RANDOM_OPTIONS = [{}, {"NO_SEMI_LDS": 1}, {"LDS_MAX_BUILD": 8192}, {"FORCE_GENERIC_VM": 1}, {"NO_SPECULATION": 1}]


def test_random_differential(torch_cuda, zoo_stores):
    gs, os_ = zoo_stores
    rng = np.random.default_rng(20261016)
    for case in range(200):
        n_ids = int(rng.integers(5, 60))
        nl, nr = int(rng.integers(0, 2000)), int(rng.choice([0, 1, 5, 300, 2000]))
        L, R = rand_cols(rng, nl, 4, n_ids, rng.random() * 0.3), rand_cols(rng, nr, 4, n_ids, rng.random() * 0.3)
        kind = abi.NODE_HASH_JOIN if rng.random() < 0.75 else abi.NODE_NESTED_LOOP_JOIN
        nk = int(rng.integers(1, 5)) if kind == abi.NODE_HASH_JOIN else 0
        on = [(int(a), int(b)) for a, b in zip(rng.permutation(4)[:nk], rng.permutation(4)[:nk])]
        flt = [None, ID_NEQ(col(int(rng.integers(0, 4))), col(4 + int(rng.integers(0, 4)))),
               AND(IS_COMPATIBLE(col(0), col(4)), OR(BOUND(col(1)), BOUND(col(5)))),
               EBV(LT(ENC_TV(col(4 + int(rng.integers(0, 4)))), ADD(ENC_TV(col(int(rng.integers(0, 4)))), integer(2))))][int(rng.integers(0, 4))]
        jt = SEMI if rng.random() < 0.5 else ANTI
        proj = None if rng.random() < 0.5 else [int(c) for c in rng.permutation(4)[:int(rng.integers(1, 5))]]
        opts = RANDOM_OPTIONS[int(rng.integers(0, len(RANDOM_OPTIONS)))]
        try:
            run_case(torch_cuda, gs, os_, kind, jt, L, R, on, flt, proj, options=opts)
        except AssertionError as e:
            raise AssertionError(f"case {case}: kind={kind} jt={jt} nl={nl} nr={nr} on={on} opts={opts}") from e
