"""Parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same inputs,
and against the reference's own known-answer vectors.  Bit-exact: all of this is u32 / i64 / IEEE
single-operation arithmetic (stated tolerance for float comparisons and ADD/SUB: 0 ulp)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import (PlanBuilder, MemIndexScanInstruction as I, MemIndexScanPredicate as P,
                                 quad_pattern, col, lit_id, lit_tv, lit_bool, integer, int32, double, float32,
                                 decimal, boolean, ENC_TV, GT, LT, GEQ, LEQ, EQ, NEQ, ADD, SUB, EBV, ID_EQ,
                                 ID_NEQ, AND, OR, NOT, IS_COMPATIBLE, BOUND, BOOLEAN_AS_TERM, REGEX, REGEX_VAR, CONTAINS, STRSTARTS, STRENDS)
from oracle import oracle as orc
import kat_util as ku


import os
ENGINE_TOGGLED = any(k.startswith(("RDFGPU_NO_", "RDFGPU_FORCE_")) for k in os.environ)   # a debugging toggle is set for the whole run


def both_stores(quads, batch=8192, typed=None, decimals=None):
    g, s, p, o = ku.quad_columns(quads) if not isinstance(quads, tuple) else quads
    gs, os_ = rf.GpuQuadStore(batch_size=batch), orc.OracleStore(batch_size=batch)
    if len(g):
        a, b = gs.extend(g, s, p, o), os_.extend(g, s, p, o)
        assert a == b
    if typed is not None:
        gs.set_typed_values(typed, decimals)
        os_.set_typed_values(typed, decimals)
    return gs, os_


def run_both(gs, os_, desc, gpu_tables=None, cpu_tables=None, ordered=False):
    """ordered: the plan's root is a TopK, whose rows come out in a stated order: the sequences are compared as well"""
    plan = gs.plan(desc)
    if gpu_tables:
        for slot, (ptrs, n) in enumerate(gpu_tables):
            plan.bind_table(slot, ptrs, n)
    plan.execute()
    got = plan.fetch()
    n_got, _ = plan.result_info()
    exp, n_exp, _ = os_.execute(desc, cpu_tables)
    assert n_got == n_exp, (n_got, n_exp)
    assert len(got) == len(exp)
    np.testing.assert_array_equal(ku.multiset(got, n_got), ku.multiset(exp, n_exp))
    if ordered:
        ku.assert_same_sequence(got, exp, n_exp)
    return plan, got


# ---------------------------------------------------------------------------------------------------
# the reference's own KATs, through the GPU
# ---------------------------------------------------------------------------------------------------
def test_reference_scan_kats(kats):
    for case in kats["scan"]:
        gs = rf.GpuQuadStore(batch_size=case["batch"])
        if case["quads"]:
            gs.extend(*ku.quad_columns(case["quads"]))
        pb = PlanBuilder()
        # the reference tests scan ONE GSPO index directly; patterns are chosen so GSPO is also what
        # choose_index picks, except where the expected rows do not depend on the index
        desc = pb.build(pb.data_source(ku.instrs(case["instr"])))
        plan = gs.plan(desc).execute()
        n, ncols = plan.result_info()
        names = [v for v, _ in sorted(pb.vars.items(), key=lambda kv: kv[1])]
        name = case["name"]
        if "n_rows" in case:
            assert n == case["n_rows"], name
        if "n_cols" in case:
            assert ncols == case["n_cols"], name
        if "columns" in case:
            got = plan.fetch()
            order = []
            for ins in case["instr"]:
                if ins[0] == "S" and ins[1] not in order:
                    order.append(ins[1])
            for k, v in case["columns"].items():
                assert got[order.index(k)].tolist() == v, name      # sorted, like the reference's output
        if "batches" in case:
            assert [len(b) for b in plan.batches()] == case["batches"], name
        if "first_batch_rows" in case:
            # zero-column batch: only the row count travels
            assert n == case["first_batch_rows"], name
        del names


def test_reference_store_kats(kats):
    for case in kats["store"]:
        gs = rf.GpuQuadStore(batch_size=10)
        gs.extend(*ku.quad_columns(case["quads_gspo"]))
        pb = PlanBuilder()
        node = pb.data_source(ku.instrs(case["instr"]))
        plan = gs.plan(pb.build(node)).execute()
        if "chosen" in case:
            assert abi.INDEX_NAMES[plan.selected_index(node)] == case["chosen"], case["name"]
        got = plan.fetch()
        for k, name in enumerate(case["order"]):
            assert got[k].tolist() == case["columns"][name], case["name"]
        if case["name"] == "insert_quad_then_read":   # g = 0 surfaces as an Arrow null (mem_quad_storage.rs:60-104)
            b = next(iter(plan.batches()))
            assert b.field(0).null_count == 1 and b.field(1).null_count == 0
            assert b.field(1).to_pylist() == [1]


def test_reference_remove_and_dedupe_kats(kats):
    for case in kats["remove"]:
        gs = rf.GpuQuadStore(batch_size=10)
        if case["insert"]:
            gs.extend(*ku.quad_columns(case["insert"]))
        assert gs.remove(*ku.quad_columns(case["remove"])) == case["removed"], case["name"]
        assert len(gs) == case["remaining"], case["name"]
    for case in kats["dedupe"]:
        gs = rf.GpuQuadStore(batch_size=case["size"])
        gs.extend(*ku.quad_columns([[v] * 4 for v in case["first"]]))
        assert gs.extend(*ku.quad_columns([[v] * 4 for v in case["second"]])) == 1
        assert len(gs) == case["length"]


def test_reference_prune_kats_as_located_ranges(kats):
    """K1 must locate exactly the rows the reference's row-group pruning keeps."""
    for case in kats["prune"]:
        gs, os_ = both_stores(case["quads"], batch=case["size"])
        sl, _ = os_.prune(abi.GSPO, ku.instrs(case["instr"]))
        kept = sum(e - s for s, e in sl)
        pb = PlanBuilder()
        # all-traverse patterns: the result is a bare row count; residual predicates may shrink it, so
        # compare with the oracle's scan as well
        node = pb.data_source(ku.instrs(case["instr"]))
        plan = gs.plan(pb.build(node)).execute()
        n, _ = plan.result_info()
        exp = os_.scan(ku.instrs(case["instr"]))
        assert n == exp["n_rows"], case["src"]
        if not case.get("kept"):
            assert plan.metrics().input_rows == kept or plan.selected_index(node) != abi.GSPO, case["src"]


def test_reference_numeric_kats(kats, torch_cuda):
    """checked add/sub at the type bounds and Decimal -> Double (the reference's xsd in-file tests), on the device"""
    gs = rf.GpuQuadStore()
    one = [np.array([7], dtype=np.uint32)]
    keep, ptrs = table_on_device(torch_cuda, one)
    for name, desc, n_expected in ku.numeric_kat_plans(kats):
        plan = gs.plan(desc)
        plan.bind_table(0, ptrs, 1)
        assert plan.execute().result_info()[0] == n_expected, name


def test_reference_join_lowering_kats(kats, torch_cuda):
    """lib/logical/src/join/rewrite.rs:381-481 on the device: no shared variable => every pair (inner) / every left row, unbound
    on the right when the right input is empty (left); shared variables => equi-join on all of them."""
    for case in kats["join_lowering"]:
        pb = PlanBuilder()
        node = pb.sparql_join(pb.table(0, 1, case["left"]), pb.table(1, 1, case["right"]), abi.JOIN_INNER if case["join_type"] == "Inner" else abi.JOIN_LEFT)
        desc = pb.build(node)
        a, b = np.array([5, 6, 7], np.uint32), np.array([8, 9], np.uint32)
        for right in (b, b[:0]):
            ka, pa = table_on_device(torch_cuda, [a]); kb, pb_ = table_on_device(torch_cuda, [right])
            gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4)
            run_both(gs, os_, desc, gpu_tables=[(pa, 3), (pb_, len(right))], cpu_tables=[[a], [right]])


JOIN_TABLE_MODES = {
    # name: (store options, copies of the fixture's data, substring of a kernel that has to have run; the engine reports the fused join
    #        kernel by its class `lds_join_kernel<FS, PFS, ITEMS, MODE, CHAIN` — the key-count argument that follows is not part of it)
    "lds_hash": ({}, 1, "lds_join_kernel<0, 0, "),                                  # every workgroup builds the table in LDS
    "lds_hash_scaled": ({"NO_INDEX_JOIN": 1, "NO_TABLE_CACHE": 1, "LDS_MAX_BUILD": 1 << 20}, 300, ", 0, false"),
    "classic_hbm_chains": ({"NO_LDS_JOIN": 1}, 1, "join_probe_kernel"),             # heads / next chains in HBM, count + scan + write
    "hbm_hash_built_per_run": ({"LDS_MAX_BUILD": 1, "NO_TABLE_CACHE": 1, "NO_PARTITIONED_JOIN": 1, "NO_STREAM_JOIN": 1}, 3000, ", 1, false"),
    "hbm_hash_cached_slice": ({"LDS_MAX_BUILD": 1, "NO_DIRECT_TABLE": 1, "NO_STREAM_JOIN": 1}, 3000, ", 1, false"),
    "hbm_hash_streamed": ({"LDS_MAX_BUILD": 1, "NO_TABLE_CACHE": 1, "NO_PARTITIONED_JOIN": 1}, 3000, "stream_join_kernel"),   # the same table, rows kept in registers (stream_join.hip)
    "direct_address": ({"LDS_MAX_BUILD": 1}, 3000, "stream_join_kernel"),   # unique dense keys: row = direct[key - min]; rows stay in registers (stream_join.hip)
    "direct_address_generic_kernel": ({"LDS_MAX_BUILD": 1, "NO_STREAM_JOIN": 1}, 3000, ", 2, false"),   # the same table under the queueing kernel
    "csr": ({"LDS_MAX_BUILD": 1}, 3000, ", 3, false"),                             # (the data gets duplicate keys, see below)
    "radix_partitioned": ({"LDS_MAX_BUILD": 1, "NO_TABLE_CACHE": 1, "PARTITION_MIN_BUILD": 1}, 3000, "part_join_kernel"),
}


@pytest.mark.parametrize("mode", list(JOIN_TABLE_MODES))
def test_reference_join_row_fixture_in_every_table_mode(kats, mode):
    """Join ROW results against a vector the reference holds: testsuite/oxigraph-tests/sparql/nested_anonymous.{rq,ttl,srx}
    (a three-pattern BGP = two equi-joins; expected: the one solution ?a = "t1").  The literal fixture runs in the modes a
    6-quad store reaches; disjoint renamed copies of its data (expected = the .srx row once per copy) push the same join
    shape through the HBM hash, direct-address, CSR and radix-partitioned tables.  Every association order of the three
    patterns; first execution, speculative re-execution and a fresh compile."""
    import itertools
    options, copies, kernel = JOIN_TABLE_MODES[mode]
    for case in kats["join_fixtures"]:
        quads, rows = (case["quads_gspo"], case["rows"]) if copies == 1 else ku.scaled_join_fixture(case, copies)
        if mode == "csr":      # duplicate join keys: every subject of the first pattern gets a second object (a second ?a per ?x)
            p1, big = case["patterns"][0][1], (copies + 5) * (max(case["terms"].values()) + 1)
            answers = {r[0] for r in rows}
            extra = [[0, q[1], q[2], q[3] + big] for q in quads if q[2] == p1]
            rows = rows + [[e[3]] for e in extra if e[3] - big in answers]
            quads = quads + extra
        gs, os_ = both_stores(quads)
        for name, value in options.items():
            gs.set_option(name, value)
        seen = set()
        for order in itertools.permutations(range(len(case["patterns"]))):
            pb, root = ku.bgp_plan(case["patterns"], case["select"], order)
            desc = pb.build(root)
            plan = gs.plan(desc).enable_kernel_timing(True)
            for _ in range(3):
                got = plan.execute().fetch()
                assert sorted(zip(*[c.tolist() for c in got])) == sorted(map(tuple, rows)), (case["name"], mode, order)
                seen.update(k[0] for k in plan.kernel_stats())
            run_both(gs, os_, desc)                      # ... and the oracle agrees on the same plan
        assert any(kernel in k for k in seen), (mode, sorted(seen))


def test_reference_pushdown_and_dynamic_filter_kats(kats):
    """Filter push-down INTO the DataSourceExec leaf: try_pushdown_filters with its display strings
    (pattern_data_source.rs:192-234), test_dynamic_filters as the reference wrote it (static Between(2,3) on the scan, dynamic
    Between(subject,1,2) arriving at execute time, scan.rs:617-672) and the index switch a dynamic filter causes (:674-729)."""
    # --- pattern_data_source.rs: `?subject <http://example.com/test> ?object`, filters on object
    for case in kats["pushdown_display"]:
        gs = rf.GpuQuadStore(batch_size=10)
        gs.extend(*ku.quad_columns([[0, 5, 7, v] for v in (1, 2, 5, 9, 10, 4000000000)]))
        pb = PlanBuilder()
        node = pb.data_source(quad_pattern("subject", 7, "object"))
        plan = gs.plan(pb.build(node))
        flt = case["filters"]
        obj = pb.vars["object"]
        if len(flt) == 1:
            f = [("binary", obj, {"Eq": abi.OP_EQ, "Gt": abi.OP_GT, "GtEq": abi.OP_GTEQ, "Lt": abi.OP_LT, "LtEq": abi.OP_LTEQ}[flt[0][0]], flt[0][1])]
        else:      # `object > a AND object < b` arrives as ONE Between (predicate_pushdown.rs:189-249; KAT A.4: > 123 AND <= 456 => Between(124, 456))
            lo = max(v + 1 if op == "Gt" else v for op, v in flt if op in ("Gt", "GtEq"))
            hi = min(v - 1 if op == "Lt" else v for op, v in flt if op in ("Lt", "LtEq"))
            f = [("between", obj, lo, hi)]
        assert plan.pushdown_filters(node, f + [("unsupported",)]) == [True, False]
        assert abi.INDEX_NAMES[plan.selected_index(node)] == "GPOS"
        assert repr(plan.source_predicate(node, 3)) == case["display"], case    # "object == 1" / "object in (2..9)" (pattern_data_source.rs:232)
        got = plan.execute().fetch()
        allv = np.array([1, 2, 5, 9, 10, 4000000000], dtype=np.int64)
        keep = np.ones(len(allv), bool)
        for op, v in flt:
            keep &= {"Eq": allv == v, "Gt": allv > v, "GtEq": allv >= v, "Lt": allv < v, "LtEq": allv <= v}[op]
        assert sorted(got[1].tolist()) == allv[keep].tolist(), case
    # --- scan.rs test_dynamic_filters
    gs = rf.GpuQuadStore(batch_size=100)
    gs.extend(*ku.quad_columns([[0, 1, 10, 100], [0, 2, 10, 100], [0, 2, 10, 200], [0, 3, 10, 100]]))
    pb = PlanBuilder()
    node = pb.data_source([I.traverse(0), I.scan_with_predicate("subject", P.between(2, 3)), I.traverse(), I.traverse(200)])
    plan = gs.plan(pb.build(node))
    assert plan.execute().result_info()[0] == 1                     # only (0,2,10,200) has object 200 and subject in 2..3
    plan.set_dynamic_filters(node, [("between", pb.vars["subject"], 1, 2)])
    assert plan.execute().result_info()[0] == 1 and plan.fetch()[0].tolist() == [2]
    assert repr(plan.source_predicate(node, 1)) == "== 2" or repr(plan.source_predicate(node, 1)) == "in (2..2)"
    plan.set_dynamic_filters(node, [("between", pb.vars["subject"], 3, 9)])   # the filter moves: subject 3 has no object 200
    assert plan.execute().result_info()[0] == 0
    plan.set_dynamic_filters(node, [])
    assert plan.execute().result_info()[0] == 1
    # --- scan.rs test_collect_relevant_batches_dynamic_filters_choose_better_index
    gs = rf.GpuQuadStore(batch_size=100)
    gs.extend(*ku.quad_columns([[0, 1, 10, 100]]))
    pb = PlanBuilder()
    node = pb.data_source([I.traverse(0), I.scan("subject"), I.scan("predicate"), I.scan("object")])
    plan = gs.plan(pb.build(node))
    plan.execute()
    assert abi.INDEX_NAMES[plan.selected_index(node)] == "GSPO"
    plan.set_dynamic_filters(node, [("between", pb.vars["object"], 1, 200)])
    got = plan.execute().fetch()
    assert abi.INDEX_NAMES[plan.selected_index(node)] == "GOSP"     # "Switches to GOSP because the dynamic filter filters the object component"
    assert [c.tolist() for c in got] == [[1], [10], [100]]         # columns stay in G,S,P,O order of the variables
    # --- errors like the reference's: a filter on a variable the pattern does not bind
    with pytest.raises(rf.RdfGpuError):
        plan.pushdown_filters(node, [("binary", 77, abi.OP_EQ, 1)])


def test_pushdown_equals_filter_above_the_scan(torch_cuda):
    """try_pushdown_filters answers PushedDown::Yes: DataFusion then drops the FilterExec — the pushed-down scan must return
    exactly what the scan followed by the filter returns (here: numpy on the unfiltered scan), whichever index it switches to."""
    rng = np.random.default_rng(21)
    g, s_, p, o = random_quads(rng, 60_000, 900, graphs=2)
    gs, os_ = both_stores((g, s_, p, o))
    for trial in range(40):
        pb = PlanBuilder()
        const_p = int(rng.choice(p))
        shape = trial % 4
        pat = [quad_pattern("s", const_p, "o"), quad_pattern("s", "p", "o", graph="all", graph_variable="g"),
               quad_pattern(int(rng.choice(s_)), "p", "o"), quad_pattern("s", "p", int(rng.choice(o)), graph="all")][shape]
        node = pb.data_source(pat)
        desc = pb.build(node)
        base_cols, n, _ = os_.execute(desc)
        names = [v for v, _ in sorted(pb.vars.items(), key=lambda kv: kv[1]) if v in pb.names[node]]
        names = pb.names[node]
        var = names[int(rng.integers(0, len(names)))]
        col_i = names.index(var)
        lo, hi = sorted(int(x) for x in rng.integers(0, 900, 2))
        kind = trial % 3
        if kind == 0:
            f, keep = [("between", pb.vars[var], lo, hi)], (base_cols[col_i][:n] >= lo) & (base_cols[col_i][:n] <= hi)
        elif kind == 1:
            f, keep = [("binary", pb.vars[var], abi.OP_GT, lo)], base_cols[col_i][:n] > lo
        else:
            f, keep = [("binary", pb.vars[var], abi.OP_EQ, hi), ("true",)], base_cols[col_i][:n] == hi
        plan = gs.plan(desc)
        assert all(plan.pushdown_filters(node, f))
        got = plan.execute().fetch()
        exp = [c[:n][keep] for c in base_cols]
        np.testing.assert_array_equal(ku.multiset(got, plan.result_info()[0]), ku.multiset(exp, int(keep.sum())), err_msg=f"trial {trial}")
        plan.close()


# ---------------------------------------------------------------------------------------------------
# index build, random scans
# ---------------------------------------------------------------------------------------------------
def random_quads(rng, n, n_ids, graphs=2):
    return (rng.integers(0, graphs, n).astype(np.uint32), rng.integers(1, n_ids, n).astype(np.uint32),
            rng.integers(1, max(2, n_ids // 4), n).astype(np.uint32), rng.integers(1, n_ids, n).astype(np.uint32))


@pytest.mark.parametrize("n,n_ids", [(1, 5), (1000, 12), (50_000, 300), (400_000, 5000)])
def test_index_build_matches_oracle(n, n_ids):
    rng = np.random.default_rng(n)
    g, s, p, o = random_quads(rng, n, n_ids)
    gs, os_ = both_stores((g, s, p, o))
    assert len(gs) == len(os_)
    for comp in (abi.GSPO, abi.GPOS, abi.GOSP):
        for a, b in zip(gs.read_index(comp), os_.read_index(comp)):
            np.testing.assert_array_equal(a, b)
    # idempotence: inserting the same quads again changes nothing
    assert gs.extend(g, s, p, o) == 0
    # incremental extend + remove agree with the oracle
    g2, s2, p2, o2 = random_quads(rng, max(1, n // 3), n_ids)
    assert gs.extend(g2, s2, p2, o2) == os_.extend(g2, s2, p2, o2)
    assert gs.remove(g[: n // 2], s[: n // 2], p[: n // 2], o[: n // 2]) == os_.remove(g[: n // 2], s[: n // 2], p[: n // 2], o[: n // 2])
    for comp in (abi.GSPO, abi.GPOS, abi.GOSP):
        for a, b in zip(gs.read_index(comp), os_.read_index(comp)):
            np.testing.assert_array_equal(a, b)


def random_instruction(rng, lvl, n_ids):
    r = rng.integers(0, 8)
    if r == 0:
        return I.traverse()
    if r == 1:
        return I.traverse(int(rng.integers(0, n_ids)))
    if r in (2, 3):
        return I.scan(f"v{lvl if rng.random() < 0.8 else 1}")
    a = int(rng.integers(0, n_ids))
    b = a + int(rng.integers(0, max(1, n_ids // 3)))
    if r == 4:
        return I.scan_with_predicate(f"v{lvl}", P.between(a, b))
    if r == 5:
        return I.traverse_with_predicate(P.in_(rng.integers(0, n_ids, size=int(rng.integers(1, 5))).tolist()))
    if r == 6:
        return I.scan_with_predicate(f"v{lvl}", P.in_(rng.integers(0, n_ids, size=int(rng.integers(1, 4))).tolist()))
    return I.traverse_with_predicate(P.false()) if rng.random() < 0.2 else I.traverse_with_predicate(P.between(a, b))


def test_random_scans_match_oracle():
    rng = np.random.default_rng(11)
    for n, n_ids, batch in ((3000, 9, 64), (60_000, 40, 8192)):
        quads = random_quads(rng, n, n_ids)
        gs, os_ = both_stores(quads, batch=batch)
        for _ in range(150):
            ins = [random_instruction(rng, lvl, n_ids) for lvl in range(4)]
            pb = PlanBuilder()
            node = pb.data_source(ins)
            desc = pb.build(node)
            plan = gs.plan(desc).execute()
            exp = os_.scan(ins)
            n_got, ncols = plan.result_info()
            assert n_got == exp["n_rows"], [vars(i) for i in ins]
            assert plan.selected_index(node) == exp["index"]
            got = plan.fetch()
            # ORDERED equality: the scan output keeps index order, like the reference's
            for k, name in enumerate(exp["order"]):
                np.testing.assert_array_equal(got[k], exp["columns"][name])
            # batch stream: sizes sum up, no empty batch, every batch <= batch_size
            sizes = [len(b) for b in plan.batches()] if ncols else []
            if ncols:
                assert sum(sizes) == n_got and all(0 < x <= batch for x in sizes)


# ---------------------------------------------------------------------------------------------------
# FILTER semantics: every typed-value kind against every other, all operators
# ---------------------------------------------------------------------------------------------------
def typed_zoo():
    """object id -> typed value covering every tag and the numeric edge cases"""
    f32 = lambda x: int(np.array([x], dtype=np.float32).view(np.uint32)[0])
    f64 = lambda x: int(np.array([x], dtype=np.float64).view(np.int64)[0])
    E18 = 10 ** 18
    decs = [0, 5 * E18, -5 * E18, 15 * E18 // 10, 1, (1 << 127) - 1, -(1 << 127), 1000 * E18, 2 ** 63 * E18 // 7,
            123456789012345678901234567890 * 1000, 170141183460469231731687303715884105727 // 3]
    rows = [(abi.TV_NULL, 0, 0, 0)]
    rows += [(abi.TV_NAMED_NODE, r, 0, 0) for r in (1, 2, 7)]
    rows += [(abi.TV_BLANK_NODE, r, 0, 0) for r in (1, 3)]
    rows += [(abi.TV_STRING, r, lang, fl) for r, lang, fl in ((0, 0, abi.TVF_EMPTY_STRING), (5, 0, 0), (9, 0, 0), (5, 1, 0), (6, 1, 0), (5, 2, 0), (0, 1, abi.TVF_EMPTY_STRING))]
    rows += [(abi.TV_BOOLEAN, b, 0, 0) for b in (0, 1)]
    rows += [(abi.TV_FLOAT, f32(x), 0, 0) for x in (0.0, -0.0, 1.5, -2.25, 16777217.0, float("nan"), float("inf"), 3.0e38, 1e-40, 1000.0)]
    rows += [(abi.TV_DOUBLE, f64(x), 0, 0) for x in (0.0, -0.0, 1.5, 5.0, 9007199254740993.0, float("nan"), float("-inf"), 1e300, 5e-324, 1000.0, 0.1)]
    rows += [(abi.TV_DECIMAL, i, 0, 0) for i in range(len(decs))]
    rows += [(abi.TV_INT, v, 0, 0) for v in (0, 1, -1, 5, 1000, 2 ** 31 - 1, -2 ** 31)]
    rows += [(abi.TV_INTEGER, v, 0, 0) for v in (0, 1, -1, 5, 1000, 2 ** 63 - 1, -2 ** 63, 9007199254740993, 16777217, 120)]
    rows += [(abi.TV_DATE_TIME, 1, 0, 0), (abi.TV_DATE, 2, 0, 0), (abi.TV_DURATION, 3, 0, 0)]
    rows += [(abi.TV_OTHER, lex, dt, 0) for lex, dt in ((1, 1), (1, 2), (2, 1))]
    tv = np.zeros(len(rows) + 1, dtype=TV_DTYPE)      # id 0 = null
    for i, (tag, lo, aux, fl) in enumerate(rows, start=1):
        tv[i] = (lo, aux, tag, fl, 0)
    dec = np.zeros((len(decs), 2), dtype=np.int64)
    for i, d in enumerate(decs):
        u = d & ((1 << 128) - 1)
        lo, hi = u & ((1 << 64) - 1), u >> 64
        dec[i] = (lo - (1 << 64) if lo >= 1 << 63 else lo, hi - (1 << 64) if hi >= 1 << 63 else hi)
    return tv, dec


def table_on_device(torch, cols):
    ts = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint32).view(np.int32)).cuda() for c in cols]
    return ts, [t.data_ptr() for t in ts]


def check_filter(torch, gs, os_, expr, cols, projection=None):
    pb = PlanBuilder()
    desc = pb.build(pb.filter(pb.table(0, len(cols)), expr, projection=projection))
    keep, ptrs = table_on_device(torch, cols)
    plan, got = run_both(gs, os_, desc, gpu_tables=[(ptrs, len(cols[0]))], cpu_tables=[cols])
    # independent check against the row-wise evaluator too
    mask = os_.eval_bool(expr, cols)
    assert plan.result_info()[0] == int((mask == 1).sum())
    del keep
    return got


def test_filter_semantics_all_kinds(torch_cuda):
    tv, dec = typed_zoo()
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv, decimals=dec)
    n = len(tv) + 2                       # includes id 0 (null) and an id beyond the table (unknown => null)
    a, b = np.meshgrid(np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32), indexing="ij")
    a, b = a.ravel(), b.ravel()
    rowid = np.arange(1, len(a) + 1, dtype=np.uint32)
    cols = [a, b, rowid]
    A, B = ENC_TV(col(0)), ENC_TV(col(1))
    for cmp_ in (GT, LT, GEQ, LEQ, EQ, NEQ):
        check_filter(torch_cuda, gs, os_, EBV(cmp_(A, B)), cols)
        check_filter(torch_cuda, gs, os_, NOT(EBV(cmp_(A, B))), cols)          # NOT(error) stays an error => dropped
    for arith in (ADD, SUB):
        check_filter(torch_cuda, gs, os_, EBV(arith(A, B)), cols)              # EBV of the numeric result / error
        check_filter(torch_cuda, gs, os_, EBV(GT(arith(A, B), integer(3))), cols)
        check_filter(torch_cuda, gs, os_, EBV(LT(arith(A, double(0.5)), B)), cols)
        check_filter(torch_cuda, gs, os_, EBV(EQ(arith(A, B), arith(B, A))), cols)
        check_filter(torch_cuda, gs, os_, EBV(GEQ(arith(A, float32(1.5)), arith(B, decimal(25 * 10 ** 17)))), cols)
        check_filter(torch_cuda, gs, os_, EBV(LEQ(arith(A, int32(7)), arith(B, integer(-9)))), cols)
    check_filter(torch_cuda, gs, os_, EBV(A), cols)
    check_filter(torch_cuda, gs, os_, AND(EBV(A), EBV(B)), cols)
    check_filter(torch_cuda, gs, os_, OR(EBV(A), EBV(B)), cols)
    check_filter(torch_cuda, gs, os_, OR(NOT(EBV(A)), AND(EBV(B), lit_bool(None))), cols)
    check_filter(torch_cuda, gs, os_, EBV(BOOLEAN_AS_TERM(OR(EBV(A), lit_bool(False)))), cols)
    check_filter(torch_cuda, gs, os_, ID_EQ(col(0), col(1)), cols)
    check_filter(torch_cuda, gs, os_, ID_NEQ(col(0), lit_id(7)), cols)
    check_filter(torch_cuda, gs, os_, ID_EQ(col(0), lit_id(0)), cols)
    check_filter(torch_cuda, gs, os_, IS_COMPATIBLE(col(0), col(1)), cols)
    check_filter(torch_cuda, gs, os_, AND(BOUND(col(0)), NOT(BOUND(col(1)))), cols)
    check_filter(torch_cuda, gs, os_, EBV(GT(A, integer(4))), cols, projection=[2])     # specialised shape 2
    check_filter(torch_cuda, gs, os_, EBV(LEQ(A, double(1.5))), cols, projection=[2, 0])
    check_filter(torch_cuda, gs, os_, EBV(NEQ(A, lit_tv(abi.TV_STRING, 5, aux=1))), cols)
    check_filter(torch_cuda, gs, os_, lit_bool(True), cols)
    check_filter(torch_cuda, gs, os_, lit_bool(None), cols)


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 1, 1_300_003, 4_200_001])
def test_streaming_filter_matches_oracle(torch_cuda, n):
    """FILTER over >= 2^20 rows takes the two-pass streaming form (verdict bits + tile counts, scan, ordered write): every
    specialised shape over bound tables (also with a 4/8/12-byte misaligned start) and over a store slice, where a typed
    comparison on the slice's sorted column is answered once per distinct id (runs copied, or one verdict bit per row:
    filter_bits_kernel<4>); rows keep the input order."""
    tv, dec = typed_zoo()
    rng = np.random.default_rng(n)
    n_ids = len(tv)
    # a store: a few quads of other predicates in front (so the slice starts misaligned), then one big predicate partition
    pred_small, pred_big = n_ids + 1, n_ids + 2
    head = int(rng.integers(1, 4))
    subj = (n_ids + 10 + rng.permutation(n + head)).astype(np.uint32)     # distinct subjects: no quad is deduplicated away
    obj = rng.integers(1, n_ids + 2, n + head).astype(np.uint32)          # includes one id beyond the typed table
    prd = np.full(n + head, pred_big, np.uint32); prd[:head] = pred_small
    subj[:head] = np.arange(1, head + 1)
    gs, os_ = both_stores((np.zeros(n + head, np.uint32), subj, prd, obj), typed=tv, decimals=dec)
    exprs = [EBV(GT(ENC_TV(col(1)), integer(4))), EBV(LEQ(ENC_TV(col(1)), double(1.5))), EBV(NEQ(ENC_TV(col(1)), lit_tv(abi.TV_STRING, 5, aux=1))),
             EBV(EQ(ENC_TV(col(1)), decimal(5 * 10 ** 18))), ID_NEQ(col(1), lit_id(7)), ID_EQ(col(1), lit_id(3))]
    pb = PlanBuilder()
    scan_cols = gs.plan(pb.build(pb.data_source(quad_pattern("s", pred_big, "o")))).execute().fetch()
    assert np.all(np.diff(scan_cols[1].astype(np.int64)) >= 0)       # GPOS: the slice is sorted by object
    for k, e in enumerate(exprs):
        for projection in ([0], [0, 1], [1]) if k < 2 else ([0],):
            pb = PlanBuilder()
            desc = pb.build(pb.filter(pb.data_source(quad_pattern("s", pred_big, "o")), e, projection=projection))
            plan = gs.plan(desc).enable_kernel_timing(True)
            got = plan.execute().fetch()
            exp_rows, n_exp, _ = os_.execute(desc, None)
            assert plan.result_info()[0] == n_exp
            np.testing.assert_array_equal(ku.multiset(got, n_exp), ku.multiset(exp_rows, n_exp))
            mask = os_.eval_bool(e, scan_cols) == 1                    # the row-wise evaluator over the scan's rows, in index order
            exp = [scan_cols[c][mask] for c in projection]
            names = [st[0] for st in plan.kernel_stats()]
            ordered = any("filter_write_kernel" in x or "run_copy" in x for x in names)
            assert ordered or ENGINE_TOGGLED
            if ordered:
                for c in range(len(projection)):
                    np.testing.assert_array_equal(got[c], exp[c])      # the streaming / run-copy forms keep the rows in index order
            if k < 4 and not ENGINE_TOGGLED:
                # few ids under many rows: the qualifying runs are copied; then the two fallbacks, each forced
                assert any("run_copy" in x for x in names)
                # where the runs start is searched once per slice and store version (value_runs_kernel) and kept with the slice's tables:
                # the next execution plans its copy in one launch (the comparison per id inside run_scan_kernel) — same rows, same order
                again = plan.execute().fetch()
                names2 = [st[0] for st in plan.kernel_stats()]
                assert any("run_copy" in x for x in names2) and not any("value_runs_kernel" in x for x in names2), names2
                for c in range(len(projection)):
                    np.testing.assert_array_equal(again[c], exp[c])
                p3 = gs.plan(desc).set_option("NO_TABLE_CACHE").enable_kernel_timing(True)     # ... and searched inside the execution when nothing may be kept
                got3 = p3.execute().fetch()
                assert any("value_runs_kernel" in st[0] for st in p3.kernel_stats())
                for c in range(len(projection)):
                    np.testing.assert_array_equal(got3[c], exp[c])
                for option, kernel in (("NO_RUN_COPY", "filter_bits_kernel<4>"), ("NO_VALUE_VERDICTS", "filter_bits_kernel<2>")):
                    p2 = gs.plan(desc).set_option(option).enable_kernel_timing(True)
                    got2 = p2.execute().fetch()
                    assert any(kernel in st[0] for st in p2.kernel_stats())
                    assert p2.result_info()[0] == n_exp
                    for c in range(len(projection)):
                        np.testing.assert_array_equal(got2[c], exp[c])
    # bound tables: unsorted ids, start misaligned by 0 / 1 / 3 words (all columns share the phase)
    ids = rng.integers(0, n_ids + 2, n + 3).astype(np.uint32)
    payload = np.arange(1, n + 4, dtype=np.uint32)
    for skip in (0, 1, 3):
        keep, ptrs = table_on_device(torch_cuda, [ids, payload])
        m = n + 3 - skip
        ptrs = [p_ + 4 * skip for p_ in ptrs]
        for e in (EBV(GT(ENC_TV(col(0)), integer(4))), ID_NEQ(col(0), lit_id(7))):
            pb = PlanBuilder()
            desc = pb.build(pb.filter(pb.table(0, 2), e, projection=[1]))
            plan = gs.plan(desc); plan.bind_table(0, ptrs, m)
            got = plan.execute().fetch()
            exp, n_exp, _ = os_.execute(desc, [[ids[skip:], payload[skip:]]])
            assert plan.result_info()[0] == n_exp
            np.testing.assert_array_equal(got[0], np.sort(exp[0]))      # payload = row number: ascending = input order


def test_filter_edge_sizes(torch_cuda):
    tv, dec = typed_zoo()
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv, decimals=dec)
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 255, 256, 1023, 1024, 1025, 4097, 100_003):
        cols = [rng.integers(0, len(tv) + 1, n).astype(np.uint32), np.arange(1, n + 1, dtype=np.uint32)]
        check_filter(torch_cuda, gs, os_, EBV(GT(ENC_TV(col(0)), integer(1))), cols)
        check_filter(torch_cuda, gs, os_, ID_NEQ(col(0), lit_id(3)), cols, projection=[1])


# ---------------------------------------------------------------------------------------------------
# joins
# ---------------------------------------------------------------------------------------------------
def rand_table(rng, n, ncols, n_ids, null_frac=0.1):
    cols = [rng.integers(1, n_ids, n).astype(np.uint32) for _ in range(ncols)]
    for c in cols:
        c[rng.random(n) < null_frac] = 0
    return cols


@pytest.mark.parametrize("nl,nr,n_ids", [(0, 10, 5), (10, 0, 5), (1, 1, 2), (300, 500, 20), (5000, 20_000, 400),
                                         (70_000, 3_000, 1500), (200_000, 200_000, 50_000)])
def test_hash_join_matches_oracle(torch_cuda, nl, nr, n_ids):
    rng = np.random.default_rng(nl * 7 + nr)
    tv, dec = typed_zoo()
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv, decimals=dec)
    L, R = rand_table(rng, nl, 3, n_ids), rand_table(rng, nr, 2, n_ids)
    big = nl * nr > 10 ** 9
    for join_type in (abi.JOIN_INNER, abi.JOIN_LEFT):
        for on, flt, proj in (([(0, 0)], None, None),
                              ([(0, 0), (1, 1)], None, [0, 1, 2]),
                              ([(1, 0)], ID_NEQ(col(0), col(4)), [0, 4, 2]),
                              ([(0, 0)], AND(EBV(LT(ENC_TV(col(4)), ADD(ENC_TV(col(2)), integer(3)))), BOUND(col(1))), [1, 0])):
            pb = PlanBuilder()
            desc = pb.build(pb.hash_join(pb.table(0, 3), pb.table(1, 2), on=on, join_type=join_type, filter=flt, projection=proj))
            kl, pl = table_on_device(torch_cuda, L)
            kr, prr = table_on_device(torch_cuda, R)
            run_both(gs, os_, desc, gpu_tables=[(pl, nl), (prr, nr)], cpu_tables=[L, R])
    del big


@pytest.mark.parametrize("nb,npr,n_ids,min_build", [(3_000, 9_000, 700, 1000), (6_000, 2_000, 3, 1000), (70_000, 250_000, 30_000, None),
                                                     (400_000, 1_500_000, 900_000, None), (2_500_000, 3_000_000, 4_000_000, None),
                                                     (10_000_000, 12_000_000, 9_000_000, None)])
def test_partitioned_join_matches_oracle(torch_cuda, nb, npr, n_ids, min_build):
    """The radix-partitioned LDS hash join (part_join.hip): HashJoinExec(CollectLeft) over bound tables — builds that are no
    cached store slice — from a few thousand to 10 M rows: sparse single keys and two-column keys, duplicate-heavy keys
    (n_ids = 3: partitions far larger than one LDS table, joined chunk by chunk), null keys, inner / left, no filter /
    id filter / typed filter, projections; against the oracle, and against the same plan with the path switched off."""
    rng = np.random.default_rng(nb + npr)
    tv, dec = typed_zoo()
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv, decimals=dec)
    gs.set_option("PARTITION_MIN_BUILD", min_build or 65536)      # (the default, 2^21 rows, leaves smaller builds to the L2-resident hash table)
    n_tv = len(tv)
    B = [rng.integers(1, n_ids + 1, nb).astype(np.uint32), rng.integers(1, max(2, n_ids // 50) + 1, nb).astype(np.uint32), rng.integers(1, n_tv, nb).astype(np.uint32)]
    Pr = [rng.integers(1, n_ids + 1, npr).astype(np.uint32), rng.integers(1, max(2, n_ids // 50) + 1, npr).astype(np.uint32), rng.integers(1, n_tv, npr).astype(np.uint32)]
    if n_ids > 3:
        for t in (B, Pr):                     # unbound keys never join (NullEqualsNothing)
            t[0][rng.random(len(t[0])) < 0.01] = 0
            t[1][rng.random(len(t[1])) < 0.01] = 0
    kb, pbp = table_on_device(torch_cuda, B)
    kp, ppp = table_on_device(torch_cuda, Pr)
    big = nb >= 2_000_000
    shapes = [([(0, 0)], None, None, abi.JOIN_INNER),
              ([(0, 0), (1, 1)], None, [0, 1, 2, 5], abi.JOIN_INNER),
              ([(0, 0), (1, 1)], ID_NEQ(col(2), col(5)), [0, 2, 5], abi.JOIN_LEFT)]
    if not big:
        shapes += [([(1, 1)], AND(EBV(LT(ENC_TV(col(2)), ADD(ENC_TV(col(5)), integer(3)))), BOUND(col(0))), [0, 3, 2], abi.JOIN_INNER),
                   ([(0, 0)], None, [1, 4], abi.JOIN_LEFT)]
    if n_ids <= 3:                            # every key a heavy hitter: only the selective shapes keep the result small
        shapes = [([(0, 0), (1, 1)], ID_EQ(col(2), col(5)), [0, 2], abi.JOIN_INNER), ([(0, 0), (1, 1)], ID_EQ(col(2), col(5)), [0, 2, 5], abi.JOIN_LEFT)]
    seen = set()
    for on, flt, proj, jt in shapes:
        pb = PlanBuilder()
        # DataFusion builds on the left input (CollectLeft): the larger-or-equal table goes right unless it is a left join
        desc = pb.build(pb.hash_join(pb.table(0, 3), pb.table(1, 3), on=on, join_type=jt, filter=flt, projection=proj))
        exp, n_exp, _ = os_.execute(desc, [B, Pr])
        want = ku.multiset(exp, n_exp)
        plan = gs.plan(desc)
        plan.bind_table(0, pbp, nb); plan.bind_table(1, ppp, npr)
        for rep in range(3):                  # exact sizing, speculative sizing from the first run, then the two-pass form
            if rep == 2:                          # (count a partition's matches, reserve its output range once, write)
                plan.set_option("PARTITION_TWO_PASS_ROWS", 1)
            plan.enable_kernel_timing(True)
            got = plan.execute().fetch()
            assert plan.result_info()[0] == n_exp, (on, jt, rep)
            np.testing.assert_array_equal(ku.multiset(got, n_exp), want, err_msg=f"{on} {jt} rep {rep}")
            seen |= {k[0] for k in plan.kernel_stats()}
        if nb <= 2_500_000:                   # the partition passes the other way: ids materialised + rocPRIM's radix sort instead of part_pass.hip
            plan.set_option("NO_OWN_PARTITION_PASS", 1)
            got = plan.execute().fetch()
            assert any("rocprim radix sort" in k[0] for k in plan.kernel_stats()) or ENGINE_TOGGLED
            np.testing.assert_array_equal(ku.multiset(got, n_exp), want)
            plan.set_option("NO_OWN_PARTITION_PASS", 0)
        if not big:
            plan.set_option("NO_PARTITIONED_JOIN", 1)
            got = plan.execute().fetch()
            assert not any("part_join" in k[0] for k in plan.kernel_stats())
            np.testing.assert_array_equal(ku.multiset(got, n_exp), want)
        plan.close()
    assert any("part_join_kernel" in k for k in seen) or ENGINE_TOGGLED, seen
    assert any("part_pass" in k for k in seen) or ENGINE_TOGGLED, seen
    del kb, kp


@pytest.mark.parametrize("shape", ["unique keys (direct table)", "duplicate keys (CSR)", "two key columns (hash table)"])
def test_left_join_preserved_on_the_probe_side(torch_cuda, shape):
    """OPTIONAL with a small left input and a large store slice on the right: the engine builds on the slice's cached table and probes with
    the left rows, emitting a left row without a match once with a null right side (LdsJoinArgs::probe_outer) — the multiset HashJoinExec(Left)
    gives (join/rewrite.rs:126-168, NullEqualsNothing :89: a left row with a null key is kept, unmatched).  Left rows with null keys, keys
    the slice does not hold, keys it holds once / many times; against the oracle and against the classic form (build left, visited flags,
    tail pass), which RDFGPU_OPT_NO_PROBE_OUTER_JOIN brings back."""
    rng = np.random.default_rng(len(shape))
    n_quads, n_left = 400_000, 30_000
    if shape.startswith("unique"):
        s_ = np.arange(1000, 1000 + n_quads, dtype=np.uint32)                       # every subject once
    else:
        s_ = (1000 + rng.integers(0, n_quads // 7, n_quads)).astype(np.uint32)      # ~7 triples per subject, some subjects absent
    o_ = (900_000 + rng.integers(0, 5000, n_quads)).astype(np.uint32)
    quads = (np.zeros(n_quads, np.uint32), s_, np.full(n_quads, 7, np.uint32), o_)
    gs, os_ = both_stores(quads)
    two = shape.startswith("two")
    Lk = (1000 + rng.integers(0, n_quads + 50_000, n_left)).astype(np.uint32)       # a good part of the keys are not in the slice
    Lk[rng.random(n_left) < 0.05] = 0                                               # null keys: kept, never matched
    L2 = (900_000 + rng.integers(0, 5000, n_left)).astype(np.uint32)
    if two:                                                                           # half of the (s, o) pairs are triples of the slice
        pick = rng.integers(0, n_quads, n_left); hit = rng.random(n_left) < 0.5
        Lk[hit] = s_[pick[hit]]; L2[hit] = o_[pick[hit]]
    Lt = [Lk, L2, np.arange(1, n_left + 1, dtype=np.uint32)]
    keep, ptrs = table_on_device(torch_cuda, Lt)
    pb = PlanBuilder()
    on = [(0, 0), (1, 1)] if two else [(0, 0)]
    desc = pb.build(pb.hash_join(pb.table(0, 3), pb.data_source(quad_pattern("s", 7, "o")), on=on, join_type=abi.JOIN_LEFT, projection=[0, 2, 4]))
    exp, n_exp, _ = os_.execute(desc, [Lt])
    want = ku.multiset(exp, n_exp)
    assert (exp[2][:n_exp] == 0).sum() > n_left // 20 and (exp[2][:n_exp] != 0).sum() > n_left // 20      # both kinds of rows are there
    for option, classic in ((None, False), ("NO_PROBE_OUTER_JOIN", True)):
        plan = gs.plan(desc)
        if option: plan.set_option(option, 1)
        plan.bind_table(0, ptrs, n_left)
        for rep in range(3):                         # exact first run, then speculative sizes
            plan.enable_kernel_timing(True)
            got = plan.execute().fetch()
            assert plan.result_info()[0] == n_exp, (shape, option, rep)
            np.testing.assert_array_equal(ku.multiset(got, n_exp), want, err_msg=f"{shape} {option} rep {rep}")
        names = {k[0] for k in plan.kernel_stats()}
        if not ENGINE_TOGGLED:
            assert any("join_left_unmatched_kernel" in k for k in names) == classic, (shape, option, sorted(names))
        plan.close()
    del keep


@pytest.mark.parametrize("nb,case", [(4096, "exact tile"), (4097, "tile + 1"), (8192, "two tiles"), (300_000, "all null"), (300_000, "one hot key"),
                                     (262_144, "one pass / two pass boundary"), (262_400, "one pass / two pass boundary"), (1_048_576, "clustered")])
def test_partition_passes_edge_cases(torch_cuda, nb, case):
    """The hand-written partition passes (part_pass.hip) at their seams: row counts on / next to a tile boundary (4096 rows), a build
    side on which NO row joins (every key null: all records ride in the last partition), one key on every row (one partition holds
    everything, joined chunk by chunk; every wave's bins are a crowd), the build size where 256 partitions become 512 (one pass ->
    two passes), and rows clustered by key (the wave-aggregated counting).  Two-column keys, inner join; the oracle's multiset and the
    rocPRIM form of the passes."""
    rng = np.random.default_rng(nb)
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4)
    gs.set_option("PARTITION_MIN_BUILD", 1000)
    npr = 50_000
    n_ids = max(16, nb // 3)
    B = [rng.integers(1, n_ids + 1, nb).astype(np.uint32), rng.integers(1, 5, nb).astype(np.uint32), np.arange(1, nb + 1, dtype=np.uint32)]
    Pr = [rng.integers(1, n_ids + 1, npr).astype(np.uint32), rng.integers(1, 5, npr).astype(np.uint32), np.arange(1, npr + 1, dtype=np.uint32)]
    if case == "all null":
        B[0][:] = 0
    elif case == "one hot key":
        B[0][:] = 7; B[1][:] = 2; Pr[0][:40] = 7; Pr[1][:40] = 2          # 40 probe rows x nb build rows
    elif case == "clustered":
        B[0].sort()                                                         # neighbouring rows share their key (and so their partition)
    kb, pbp = table_on_device(torch_cuda, B)
    kp, ppp = table_on_device(torch_cuda, Pr)
    pb = PlanBuilder()
    desc = pb.build(pb.hash_join(pb.table(0, 3), pb.table(1, 3), on=[(0, 0), (1, 1)], join_type=abi.JOIN_INNER, projection=[2, 5]))
    exp, n_exp, _ = os_.execute(desc, [B, Pr])
    want = ku.multiset(exp, n_exp)
    plan = gs.plan(desc)
    plan.bind_table(0, pbp, nb); plan.bind_table(1, ppp, npr)
    for own in (1, 0, 1):
        plan.set_option("NO_OWN_PARTITION_PASS", 0 if own else 1)
        plan.enable_kernel_timing(True)
        got = plan.execute().fetch()
        names = {k[0] for k in plan.kernel_stats()}
        assert plan.result_info()[0] == n_exp, (case, own)
        np.testing.assert_array_equal(ku.multiset(got, n_exp), want, err_msg=f"{case} own={own}")
        if not ENGINE_TOGGLED:
            assert any("part_join_kernel" in k for k in names), names
            assert any("part_pass" in k for k in names) == bool(own), (own, names)
    plan.close()
    del kb, kp


@pytest.mark.parametrize("build_values", ["integers", "one_double"])
def test_stream_join_with_key_value_table_matches_oracle(torch_cuda, build_values):
    """stream_join.hip on a probe side of 4.3 M rows (from where a lane keeps eight rows and the window's build-side operand is decoded once per
    KEY, a.key_vals): TABLE JOIN (?s <p> ?v) ON key = ?s with FILTER(?v < ?y + 30 && ?v > ?y - 30) — unique dense subjects (direct table),
    keys without a row, null keys, non-integer ?y operands (the slow half of the filter), a projection without / with a build column; and a
    slice holding ONE double value (no value table can be built: the kernel gathers typed values as before).  The oracle's multiset, the
    queueing kernel (NO_STREAM_JOIN) and the re-execution agree."""
    rng = np.random.default_rng(len(build_values))
    n_sub, npr = 120_000, 4_300_000
    n_val = 400
    # ids: 1 .. n_val integer literals (value = id * 3), n_val + 1 a double, subjects from 10_000
    tv = np.zeros(10_000 + n_sub + 10, dtype=TV_DTYPE)
    tv["tag"][1:n_val + 1] = abi.TV_INTEGER; tv["lo"][1:n_val + 1] = np.arange(1, n_val + 1) * 3
    tv["tag"][n_val + 1] = abi.TV_DOUBLE; tv["lo"][n_val + 1] = int(np.array([600.5]).view(np.int64)[0])
    tv["tag"][10_000:] = abi.TV_NAMED_NODE; tv["lo"][10_000:] = np.arange(len(tv) - 10_000)
    sub = (10_000 + np.arange(n_sub)).astype(np.uint32)
    val = rng.integers(1, n_val + 1, n_sub).astype(np.uint32)
    if build_values == "one_double":
        val[777] = n_val + 1
    quads = (np.zeros(n_sub, np.uint32), sub, np.full(n_sub, 5, np.uint32), val)
    gs, os_ = both_stores(quads, typed=tv)
    keys = (10_000 + rng.integers(0, n_sub + 8, npr)).astype(np.uint32)          # a few keys behind the slice's range
    keys[rng.random(npr) < 0.01] = 0
    ys = rng.integers(1, n_val + 1, npr).astype(np.uint32)
    ys[rng.random(npr) < 0.001] = n_val + 1                                         # a double y operand: decided by the slow half
    tab = [np.arange(1, npr + 1, dtype=np.uint32), keys, ys]
    keep, ptrs = table_on_device(torch_cuda, tab)
    window = AND(EBV(LT(ENC_TV(col(4)), ADD(ENC_TV(col(2)), integer(30)))), EBV(GT(ENC_TV(col(4)), SUB(ENC_TV(col(2)), integer(30)))))
    for projection in ([0, 1, 2], [0, 4, 3]):
        pb = PlanBuilder()
        desc = pb.build(pb.hash_join(pb.table(0, 3), pb.data_source(quad_pattern("s", 5, "v")), on=[(1, 0)], filter=window, projection=projection))
        exp, n_exp, _ = os_.execute(desc, [tab])
        want = ku.multiset(exp, n_exp)
        assert 100_000 < n_exp < npr // 2
        for option in (None, "NO_STREAM_JOIN", "NO_VALUE_TABLES", "NO_TABLE_CACHE"):
            plan = gs.plan(desc)
            if option:
                plan.set_option(option, 1)
            plan.bind_table(0, ptrs, npr)
            for run in range(2):
                plan.enable_kernel_timing(True)
                got = plan.execute().fetch()
                assert plan.result_info()[0] == n_exp, (build_values, projection, option, run)
                np.testing.assert_array_equal(ku.multiset(got, n_exp), want, err_msg=f"{build_values} {projection} {option} run {run}")
            names = {k[0] for k in plan.kernel_stats()}
            if not ENGINE_TOGGLED:
                assert any("stream_join_kernel" in k for k in names) == (option != "NO_STREAM_JOIN"), (option, names)
            plan.close()
    del keep


@pytest.mark.parametrize("join_type", ["inner", "left"])
def test_partitioned_join_large_output_form_and_table_geometry(torch_cuda, join_type):
    """The partitioned join's large-output form (part_join.hip, BIG: a counting pass, one reservation per partition, then a writing pass that
    filters and writes in one round trip) on a many-to-many join — ~40 partners per probe row — without a filter, with `col != col`, with a
    window over typed values and with a VM filter; six output columns (the second column group of the write-out); under every table
    geometry PARTITION_ROWS / PARTITION_SLOTS allow (partitions joined chunk by chunk included).  The form needs the previous
    execution's cardinality: the first execution runs single-pass, the later ones two-pass; all equal the oracle's multiset."""
    rng = np.random.default_rng(77)
    nb, npr, n_keys = 60_000, 30_000, 1_500
    tv, dec = typed_zoo()
    n_tv = len(tv)
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    gs.set_option("PARTITION_MIN_BUILD", 1000)
    gs.set_option("PARTITION_TWO_PASS_ROWS", 1)
    B = [rng.integers(1, n_keys + 1, nb).astype(np.uint32), rng.integers(1, 40, nb).astype(np.uint32), rng.integers(1, n_tv, nb).astype(np.uint32)]
    Pr = [rng.integers(1, n_keys + 20, npr).astype(np.uint32), rng.integers(1, 40, npr).astype(np.uint32), rng.integers(1, n_tv, npr).astype(np.uint32),
          np.arange(1, npr + 1, dtype=np.uint32)]
    B[0][rng.random(nb) < 0.01] = 0; Pr[0][rng.random(npr) < 0.01] = 0             # null keys join nothing
    B[1][rng.random(nb) < 0.02] = 0; Pr[1][rng.random(npr) < 0.02] = 0             # null operands of the `col != col` / `col = col` filters: never `true`
    kb, pbp = table_on_device(torch_cuda, B)
    kp, ppp = table_on_device(torch_cuda, Pr)
    window = AND(EBV(LT(ENC_TV(col(2)), ADD(ENC_TV(col(5)), integer(40)))), EBV(GT(ENC_TV(col(2)), SUB(ENC_TV(col(5)), integer(40)))))
    # (inner join, `col <=|!=> col` with one operand per side: decided during the chain walk from the LDS table, part_join.hip INL)
    filters = [None, ID_NEQ(col(1), col(4)), ID_EQ(col(4), col(1)), ID_NEQ(col(0), col(1)), window, EBV(GT(ADD(ENC_TV(col(2)), ENC_TV(col(5))), integer(3)))]
    jt = abi.JOIN_INNER if join_type == "inner" else abi.JOIN_LEFT
    for flt in filters:
        pb = PlanBuilder()
        desc = pb.build(pb.hash_join(pb.table(0, 3), pb.table(1, 4), on=[(0, 0)], filter=flt, join_type=jt, projection=[0, 1, 2, 4, 5, 6]))
        exp, n_exp, _ = os_.execute(desc, [B, Pr])
        want = ku.multiset(exp, n_exp)
        for geometry in ({}, {"PARTITION_SLOTS": 1024, "PARTITION_ROWS": 512}, {"PARTITION_SLOTS": 8192, "PARTITION_ROWS": 4096}, {"PARTITION_ROWS": 16}, {"PARTITION_SLOTS": 4096, "PARTITION_ROWS": 100_000}):
            plan = gs.plan(desc)
            for name, value in geometry.items():
                plan.set_option(name, value)
            plan.bind_table(0, pbp, nb); plan.bind_table(1, ppp, npr)
            for run in range(3):
                plan.enable_kernel_timing(True)
                got = plan.execute().fetch()
                assert plan.result_info()[0] == n_exp, (join_type, geometry, run)
                np.testing.assert_array_equal(ku.multiset(got, n_exp), want, err_msg=f"{join_type} {geometry} run {run}")
                if not ENGINE_TOGGLED:
                    assert any("part_join_kernel" in k[0] for k in plan.kernel_stats()), plan.kernel_stats()
            plan.close()
    plan = gs.plan(desc).set_option("PARTITION_SLOTS", 3000)                         # not a power of two: refused when the join is prepared
    plan.bind_table(0, pbp, nb); plan.bind_table(1, ppp, npr)
    with pytest.raises(RuntimeError):
        plan.execute()
    plan.close()
    del kb, kp


@pytest.mark.parametrize("n_quads,nb", [(300_000, 200_000), (2_500_000, 1_200_000)])
def test_partitioned_join_over_sorted_slice(torch_cuda, n_quads, nb):
    """Partitioned join whose probe side is a store slice sorted by one of the join keys: the slice is read in place, its
    partitions are key ranges found by binary search, only the build side (a bound table) is partition-sorted.  One and
    two key columns (the slice's sort key first or second), keys below / above the slice's id range, null keys, inner and
    left joins with a filter; the oracle's multiset, the hash-partitioned form (RDFGPU_OPT_NO_RANGE_PARTITION) and the
    un-partitioned join give the same rows."""
    rng = np.random.default_rng(n_quads)
    n_subj, n_obj = n_quads // 3, n_quads // 40
    s = (1000 + rng.integers(0, n_subj, n_quads)).astype(np.uint32)
    o = (1000 + n_subj + rng.integers(0, n_obj, n_quads)).astype(np.uint32)
    s[rng.random(n_quads) < 0.3] += np.uint32(n_subj + n_obj + 5000)          # a second island of subject ids: empty key ranges in between
    quads = (np.zeros(n_quads, np.uint32), s, np.full(n_quads, 7, np.uint32), o)
    tv, dec = typed_zoo()
    tvx = np.zeros(int(s.max()) + 2, dtype=TV_DTYPE); tvx["tag"][1:] = abi.TV_NAMED_NODE; tvx["lo"][1:] = np.arange(1, len(tvx))
    gs, os_ = both_stores(quads, typed=tvx)
    gs.set_option("PARTITION_MIN_BUILD", 65536)
    gs.set_option("NO_TABLE_CACHE", 1)                    # the slice's own cached table would answer this join without any partitioning
    pick = rng.integers(0, n_quads, nb)
    B = [s[pick].copy(), o[pick].copy(), rng.integers(1, 1000, nb).astype(np.uint32)]
    miss = rng.random(nb) < 0.3
    B[1][miss] = (1000 + n_subj + rng.integers(0, n_obj, int(miss.sum()))).astype(np.uint32)   # pairs that are (mostly) no triple
    B[0][rng.random(nb) < 0.01] = 0                                                            # null keys
    B[0][rng.random(nb) < 0.01] = 5                                                            # below the slice's id range
    B[0][rng.random(nb) < 0.01] = np.uint32(int(s.max()) + 1)                                  # above it
    kb, pbp = table_on_device(torch_cuda, B)
    for on, flt, proj, jt in [([(0, 0), (1, 1)], None, None, abi.JOIN_INNER),
                              ([(1, 1)], ID_EQ(col(0), col(3)), [0, 2, 4], abi.JOIN_INNER),
                              ([(0, 0)], ID_NEQ(col(1), col(4)), [0, 1, 4], abi.JOIN_LEFT)]:
        pb = PlanBuilder()
        desc = pb.build(pb.hash_join(pb.table(0, 3), pb.data_source(quad_pattern("s", 7, "o")), on=on, join_type=jt, filter=flt, projection=proj))
        exp, n_exp, _ = os_.execute(desc, [B])
        want = ku.multiset(exp, n_exp)
        assert n_exp > 1000
        plan = gs.plan(desc)
        plan.bind_table(0, pbp, nb)
        sorts = {}
        for mode in ("range", "range again", "hash", "off"):
            plan.set_option("NO_RANGE_PARTITION", 1 if mode == "hash" else 0)
            plan.set_option("NO_PARTITIONED_JOIN", 1 if mode == "off" else 0)
            plan.enable_kernel_timing(True)
            got = plan.execute().fetch()
            assert plan.result_info()[0] == n_exp, (on, jt, mode)
            np.testing.assert_array_equal(ku.multiset(got, n_exp), want, err_msg=f"{on} {jt} {mode}")
            stats = {k[0]: k[1] for k in plan.kernel_stats()}
            sorts[mode] = (sum(v for k, v in stats.items() if "part_pass" in k), any("part_join_kernel" in k for k in stats))   # (sides that went through the partition passes)
        if not ENGINE_TOGGLED:
            in_place = 1 if any(r == 1 for _, r in on) else 2     # the slice of (?s <7> ?o) is sorted by ?o: a join on ?s alone partitions both sides
            assert sorts["range"] == (in_place, True) and sorts["range again"] == (in_place, True) and sorts["hash"] == (2, True) and not sorts["off"][1], (on, sorts)
        plan.close()
    del kb


def test_cross_and_nested_loop_join(torch_cuda):
    rng = np.random.default_rng(3)
    tv, dec = typed_zoo()
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv, decimals=dec)
    for nl, nr in ((0, 4), (4, 0), (1, 1), (37, 19), (1500, 7), (3, 2500)):
        L, R = rand_table(rng, nl, 2, 30), rand_table(rng, nr, 2, 30)
        kl, pl = table_on_device(torch_cuda, L)
        kr, prr = table_on_device(torch_cuda, R)
        tabs = dict(gpu_tables=[(pl, nl), (prr, nr)], cpu_tables=[L, R])
        pb = PlanBuilder()
        run_both(gs, os_, pb.build(pb.cross_join(pb.table(0, 2), pb.table(1, 2))), **tabs)
        for jt in (abi.JOIN_INNER, abi.JOIN_LEFT):
            pb = PlanBuilder()
            run_both(gs, os_, pb.build(pb.nested_loop_join(pb.table(0, 2), pb.table(1, 2), join_type=jt)), **tabs)
            pb = PlanBuilder()   # IS_COMPATIBLE join of nullable keys (join/rewrite.rs:131-167)
            run_both(gs, os_, pb.build(pb.nested_loop_join(pb.table(0, 2), pb.table(1, 2), join_type=jt,
                                                           filter=IS_COMPATIBLE(col(0), col(2)), projection=[0, 1, 3])), **tabs)


# ---------------------------------------------------------------------------------------------------
# BSBM-shaped end to end: the reference's Q1 / Q5 physical plans
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bsbm_stores():
    ds = bsbm.generate(2000)
    gs, os_ = both_stores((ds.g, ds.s, ds.p, ds.o), typed=ds.typed_values, decimals=ds.decimals)
    return ds, gs, os_


def test_bsbm_q5_matches_oracle(bsbm_stores):
    ds, gs, os_ = bsbm_stores
    rng = np.random.default_rng(0)
    total = 0
    for i in rng.integers(0, ds.n_products, 12):
        plan, got = run_both(gs, os_, bsbm.q5_plan(ds, ds.product(i)))
        total += plan.result_info()[0]
    assert total > 0
    # unknown product constant: statically empty, not an error (snapshot.rs:101-110)
    plan, _ = run_both(gs, os_, bsbm.q5_plan(ds, ds.n_ids + 5))
    assert plan.result_info()[0] == 0


def test_bsbm_q1_matches_oracle(bsbm_stores):
    ds, gs, os_ = bsbm_stores
    rng = np.random.default_rng(1)
    total = 0
    for _ in range(12):
        plan, _ = run_both(gs, os_, bsbm.q1_plan(ds, *bsbm.q1_instance(ds, rng)))
        total += plan.result_info()[0]
    assert total > 0
    for thr in (0, 1, 500, 1000, 1999, 2000, 5000):
        run_both(gs, os_, bsbm.q1_scan_filter_plan(ds, thr))


@pytest.mark.parametrize("batch", [1, 24, 400])
def test_bsbm_q5_batched_equals_per_instance(bsbm_stores, torch_cuda, batch):
    """A batch of Q5 instances as ONE operator tree (shared scans, the constant as a column) must give,
    per instance, exactly the bindings of the per-instance reference plan."""
    ds, gs, os_ = bsbm_stores
    rng = np.random.default_rng(batch)
    prods = [ds.product(i) for i in rng.choice(ds.n_products, batch, replace=False)]
    params = [np.arange(1, batch + 1, dtype=np.uint32), np.array(prods, dtype=np.uint32)]   # inst tags are 1-based: 0 is null
    keep, ptrs = table_on_device(torch_cuda, params)
    plan, got = run_both(gs, os_, bsbm.q5_batch_plan(ds), gpu_tables=[(ptrs, batch)], cpu_tables=[params])
    expected = []
    for i, x in enumerate(prods[:40]):      # per-instance reference plans (oracle) for a sample of the batch
        c, m, _ = os_.execute(bsbm.q5_plan(ds, x))
        expected.append(np.stack([np.full(m, i + 1, np.uint32), c[0], c[1]], axis=1))
    expected = np.concatenate(expected)
    sel = got[0] <= min(batch, 40)
    np.testing.assert_array_equal(ku.multiset([g[sel] for g in got]), ku.multiset(list(expected.T)))
    # graph-sharded form: phase A (constant patterns of the whole batch) then phase B over bound tables
    pa, tab = run_both(gs, os_, bsbm.q5_batch_const_plan(ds), gpu_tables=[(ptrs, batch)], cpu_tables=[params])
    keep_c, ptrs_c = table_on_device(torch_cuda, tab)
    plan_b, got_b = run_both(gs, os_, bsbm.q5_batch_plan(ds, tables=True), gpu_tables=[(ptrs_c, len(tab[0]))], cpu_tables=[tab])
    np.testing.assert_array_equal(ku.multiset(got_b), ku.multiset(got))
    # the multi-GPU exchange binds a fixed-size, zero-padded buffer: a padding row has inst = 0 = null and must never join
    padded = [np.concatenate([c, np.zeros(37, np.uint32)]) for c in tab]
    keep_p, ptrs_p = table_on_device(torch_cuda, padded)
    plan_b.bind_table(0, ptrs_p, len(padded[0]))
    got_p = plan_b.execute().fetch()
    np.testing.assert_array_equal(ku.multiset(got_p), ku.multiset(got))


def test_first_execution_over_a_big_batch_is_primed(torch_cuda):
    """The very first execution of a plan over a big bound table is preceded by a priming run over the table's first
    rows (join tables built, cardinalities extrapolated): the full batch then runs fused, with a small fraction of the
    intermediates an exact un-fused first run materialises — and with the same bindings."""
    ds = bsbm.generate(2000)
    rng = np.random.default_rng(11)
    batch = 60_000
    prods = np.array([ds.product(i) for i in rng.integers(0, ds.n_products, batch)], dtype=np.uint32)
    params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
    keep, ptrs = table_on_device(torch_cuda, params)

    def first_run(option):
        gs = rf.GpuQuadStore()
        gs.extend(ds.g, ds.s, ds.p, ds.o); gs.set_typed_values(ds.typed_values, ds.decimals)
        plan = gs.plan(bsbm.q5_batch_plan(ds))
        if option:
            plan.set_option(option)
        plan.bind_table(0, ptrs, batch)
        plan.execute()
        first = ku.multiset(plan.fetch())
        scratch = plan.metrics().device_bytes
        second = ku.multiset(plan.execute().fetch())
        np.testing.assert_array_equal(first, second)
        return first, scratch

    primed, scratch_primed = first_run(None)
    exact, scratch_exact = first_run("NO_PRIMING")
    np.testing.assert_array_equal(primed, exact)
    assert len(primed) > batch
    if not ENGINE_TOGGLED:
        assert scratch_primed * 4 < scratch_exact, (scratch_primed, scratch_exact)


@pytest.mark.parametrize("shape", ["unique_dense", "dup_sorted", "dup_scattered", "sparse"])
@pytest.mark.parametrize("n_tab", [1, 700, 40_000])
def test_index_join_against_store_slice(torch_cuda, shape, n_tab):
    """TABLE JOIN (?s <p> ?o) with the engine building on the store slice (cached direct-address / CSR / hash
    table) and probing with the table — every table mode, keyed by either end of the pattern, with a residual
    filter, null keys in the table, keys outside the slice, and re-execution from the cache."""
    rng = np.random.default_rng(len(shape) * 100_003 + n_tab)
    n_sub = 6000
    pred, other_pred = 5, 6
    sub = 1000 + (np.arange(n_sub) if shape != "sparse" else np.sort(rng.choice(10_000_000, n_sub, replace=False)))
    if shape == "unique_dense":      # one object per subject: keyed by ?s the keys are unique and dense -> direct
        s_col, o_col = sub, 50_000 + rng.integers(0, 300, n_sub)
    else:                            # ~8 objects per subject: duplicates -> CSR (dense) or hash (sparse)
        s_col = np.repeat(sub, 8)
        o_col = 50_000 + rng.integers(0, 300, len(s_col))
    quads = (np.zeros(len(s_col) + 50, np.uint32),
             np.concatenate([s_col, 1000 + rng.integers(0, n_sub, 50)]).astype(np.uint32),
             np.concatenate([np.full(len(s_col), pred), np.full(50, other_pred)]).astype(np.uint32),
             np.concatenate([o_col, 50_000 + rng.integers(0, 300, 50)]).astype(np.uint32))
    gs, os_ = both_stores(quads)
    # "dup_sorted": key = ?o of the GPOS slice (sorted by the key); the others: key = ?s (scattered inside the slice)
    key_is_object = shape == "dup_sorted"
    key_pool = np.unique(o_col if key_is_object else s_col)
    keys = rng.choice(np.concatenate([key_pool, key_pool[:3] + 9_999_999]), n_tab).astype(np.uint32)
    keys[rng.random(n_tab) < 0.05] = 0                                    # null keys never join
    tab = [rng.integers(1, 9, n_tab).astype(np.uint32), keys, rng.integers(50_000, 50_300, n_tab).astype(np.uint32)]
    keep, ptrs = table_on_device(torch_cuda, tab)
    k_scan = 1 if key_is_object else 0
    for mk in (None, ID_NEQ, ID_EQ):
        pb = PlanBuilder()
        t = pb.table(0, 3)
        scan = pb.data_source(quad_pattern("s", pred, "o"))               # (s, o) at columns 3, 4
        flt = None if mk is None else mk(col(2), col(4))
        desc = pb.build(pb.hash_join(t, scan, on=[(1, k_scan)], filter=flt, projection=[0, 1, 3, 4, 2]))
        plan, got = run_both(gs, os_, desc, gpu_tables=[(ptrs, n_tab)], cpu_tables=[tab])
        plan.enable_kernel_timing(True)
        again = plan.execute().fetch()                                    # second run: cached table, speculative sizes
        np.testing.assert_array_equal(ku.multiset(again), ku.multiset(got))
        if n_tab == 700 and not ENGINE_TOGGLED:   # the table mode is the fourth template argument of the kernel name: 2 direct, 3 CSR, 1 hash
            mode = {"unique_dense": "2", "dup_sorted": "3", "dup_scattered": "3", "sparse": "1"}[shape]
            # (a direct-address or hash table without a VM filter is probed by stream_join.hip's register-resident form)
            joins = [k[0] for k in plan.kernel_stats() if "lds_join_kernel" in k[0] or "stream_join_kernel" in k[0]]
            assert joins and all(("stream_join_kernel" in k and mode in "12") or k.rstrip(">").split(", ")[3] == mode for k in joins), (shape, joins)
        # and with the inputs swapped (the slice as the plan's left child: (s, o) at 0, 1; the table at 2, 3, 4)
        pb = PlanBuilder()
        scan = pb.data_source(quad_pattern("s", pred, "o"))
        t = pb.table(0, 3)
        flt = None if mk is None else mk(col(4), col(1))
        run_both(gs, os_, pb.build(pb.hash_join(scan, t, on=[(k_scan, 1)], filter=flt, projection=[2, 3, 0, 1])),
                 gpu_tables=[(ptrs, n_tab)], cpu_tables=[tab])


# ---------------------------------------------------------------------------------------------------
# REGEX: device position automaton vs the oracle's Pike VM, through plans
# ---------------------------------------------------------------------------------------------------
string_dictionary = ku.string_dictionary


def test_regex_filter_matches_oracle(torch_cuda, monkeypatch):
    import re
    rng = np.random.default_rng(99)
    strings = [ku.random_subject(rng) for _ in range(1500)] + ["", "a", "b", "ab\n", "K", "ſ", "😀"]
    tv, offsets, heap = string_dictionary(strings)
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    gs.set_strings(offsets, heap)
    os_.set_strings(offsets, heap)
    ids = rng.integers(0, len(tv), 20_000).astype(np.uint32)              # includes 0 (null) and the non-string ids
    payload = np.arange(len(ids), dtype=np.uint32) + 1
    keep, ptrs = table_on_device(torch_cuda, [ids, payload])
    fixed = [("^a$", ""), ("a.c", "s"), ("(ab|cd)+e", ""), ("k", "i"), ("^$", ""), ("b$", "m"), ("a", "z"), ("x{2,}", ""), (".", "q"), ("[^a]", ""),
             # inline flags, nested / POSIX classes, class set operations (regex-syntax)
             ("(?i)ab", ""), ("a(?i)b", ""), ("(?i:k)x", ""), ("(?s)a.b", ""), ("(?m)^b$", ""), ("(?i)a(?-i)b", ""), ("[a-z&&[^aeiou]]+", ""), ("[a-k--c-e]x", ""),
             ("[a-c~~b-d]", ""), ("[[:alpha:]]+[[:digit:]]", ""), ("[^a[bc]]", ""), ("[[:^alpha:]]", ""), ("[A-Z&&[a-c]]", "i")]
    n_random, matched_some = 0, 0
    while n_random < 220:
        pat, flags, py, py_flags = ku.random_regex(rng, extended=n_random >= 150)
        try:
            rf.engine.regex_check(pat, flags)
        except rf.engine.RdfGpuError:
            continue                                                      # outside the device subset: refused at compile (tested on CPU)
        fixed.append((pat, flags))
        n_random += 1
    for pat, flags in fixed:
        for negate in (False, True):
            e = EBV(REGEX(ENC_TV(col(0)), pat, flags))
            pb = PlanBuilder()
            desc = pb.build(pb.filter(pb.table(0, 2), NOT(e) if negate else e))
            plan, got = run_both(gs, os_, desc, gpu_tables=[(ptrs, len(ids))], cpu_tables=[[ids, payload]])
            matched_some += plan.result_info()[0] > 0
    assert matched_some > 130
    # per-distinct-term verdict table (filter_kernel<3>) vs per-row VM evaluation: same rows
    for pat, flags in fixed[:12]:
        pb = PlanBuilder()
        desc = pb.build(pb.filter(pb.table(0, 2), EBV(REGEX(ENC_TV(col(0)), pat, flags)), projection=[1]))
        p1 = gs.plan(desc); p1.bind_table(0, ptrs, len(ids)); p1.enable_kernel_timing(True)
        a_rows = np.sort(p1.execute().fetch()[0])
        assert any("filter_kernel<3>" in k[0] or "filter_bits_kernel<3>" in k[0] for k in p1.kernel_stats()) or ENGINE_TOGGLED
        p2 = gs.plan(desc).set_option("NO_STRING_VERDICTS"); p2.bind_table(0, ptrs, len(ids)); p2.enable_kernel_timing(True)
        b_rows = np.sort(p2.execute().fetch()[0])
        assert not any("filter_kernel<3>" in k[0] or "filter_bits_kernel<3>" in k[0] for k in p2.kernel_stats())
        np.testing.assert_array_equal(a_rows, b_rows)
    # an independent spot check of the device against Python's `re` (not via the oracle)
    for pat, py in (("(ab|cd)+e", "(ab|cd)+e"), ("^k.*x$", "^k.*x\\Z"), ("[^a]b", "[^a]b")):
        pb = PlanBuilder()
        plan = gs.plan(pb.build(pb.filter(pb.table(0, 2), EBV(REGEX(ENC_TV(col(0)), pat, "")), projection=[1])))
        plan.bind_table(0, ptrs, len(ids))
        got = np.sort(plan.execute().fetch()[0])
        rx = re.compile(py)
        is_str = (ids >= 1) & (ids <= len(strings))
        exp = np.array([bool(is_str[r]) and rx.search(strings[ids[r] - 1]) is not None for r in range(len(ids))])
        np.testing.assert_array_equal(got, payload[exp])


def test_string_functions_match_oracle(torch_cuda):
    """CONTAINS / STRSTARTS / STRENDS with a constant second argument (contains.rs, str_starts.rs, str_ends.rs), incl.
    the argument-compatibility rule for language-tagged constants."""
    rng = np.random.default_rng(3)
    strings = [ku.random_subject(rng) for _ in range(1200)] + ["", "abc", "ab", "bc", "€uro", "x€"]
    tv, offsets, heap = string_dictionary(strings)
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    gs.set_strings(offsets, heap)
    os_.set_strings(offsets, heap)
    ids = rng.integers(0, len(tv), 15_000).astype(np.uint32)
    payload = np.arange(len(ids), dtype=np.uint32) + 1
    keep, ptrs = table_on_device(torch_cuda, [ids, payload])
    needles = ["", "a", "ab", "b", "€", "k ", "\n", ".", "abc", "x" * 64]
    for fn, py in ((CONTAINS, lambda s_, n: n in s_), (STRSTARTS, str.startswith), (STRENDS, str.endswith)):
        for needle in needles:
            for lang in (0, 7, 9):
                e = EBV(fn(ENC_TV(col(0)), needle, lang))
                for negate in (False, True):
                    pb = PlanBuilder()
                    run_both(gs, os_, pb.build(pb.filter(pb.table(0, 2), NOT(e) if negate else e, projection=[1])),
                             gpu_tables=[(ptrs, len(ids))], cpu_tables=[[ids, payload]])
            # independent of the oracle: Python's own substring tests, simple-literal constant
            pb = PlanBuilder()
            plan = gs.plan(pb.build(pb.filter(pb.table(0, 2), EBV(fn(ENC_TV(col(0)), needle)), projection=[1])))
            plan.bind_table(0, ptrs, len(ids))
            got = np.sort(plan.execute().fetch()[0])
            is_str = (ids >= 1) & (ids <= len(strings))
            exp = np.array([bool(is_str[r]) and py(strings[ids[r] - 1], needle) for r in range(len(ids))])
            np.testing.assert_array_equal(got, payload[exp])
    pb = PlanBuilder()
    with pytest.raises(rf.RdfGpuError):          # needles beyond 64 bytes are outside the device subset
        gs.plan(pb.build(pb.filter(pb.table(0, 2), EBV(CONTAINS(ENC_TV(col(0)), "y" * 65)))))


def test_string_valued_expressions_match_oracle(torch_cuda, kats):
    """STR / STRLEN / SUBSTR / UCASE / LCASE inside plan expressions: string VIEWS over the heap on the device against
    the oracle's materialised strings; the reference's STR vectors (unary__STR(PLAIN_TERM).snap, small_iri_str.rq) through the GPU;
    what the device does not restate fails the execute loudly."""
    from rdf_fusion_amd.plan import STR, STRLEN, SUBSTR, UCASE, LCASE, STRBEFORE, STRAFTER, lit_str
    # the reference's vectors: STR(term) = its lexical form as written, for every kind of term
    cases = kats["str_plain_term"]
    tv, off, heap, _ = ku.term_dictionary([c["term"] for c in cases])
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    gs.set_strings(off, heap); os_.set_strings(off, heap)
    for k, c in enumerate(cases):
        one = [np.array([k + 1], np.uint32)]
        got = check_filter(torch_cuda, gs, os_, EBV(EQ(STR(col(0)), lit_str(c["str"]))), one)
        assert got[0].tolist() == [k + 1], c
        check_filter(torch_cuda, gs, os_, EBV(EQ(STRLEN(STR(col(0))), integer(len(c["str"])))), one)
    for c in kats["str_queries"]:
        tv1, off1, heap1, _ = ku.term_dictionary([c["term"]])
        g1, o1 = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv1)
        g1.set_strings(off1, heap1); o1.set_strings(off1, heap1)
        got = check_filter(torch_cuda, g1, o1, EBV(EQ(STR(col(0)), lit_str(c["equals"]))), [np.array([1], np.uint32)])
        assert (len(got[0]) == 1) == c["answer"]
    # random dictionary: ASCII words, non-ASCII words, language tags, IRIs, integers
    rng = np.random.default_rng(17)
    alphabet = list("abcdeABC019 _-.")
    ascii_words = ["".join(rng.choice(alphabet, rng.integers(0, 14))) for _ in range(400)]
    words = ascii_words + ["äpfel", "日本語テキスト", "🤖 robot", "naïve café", "Ünïcode"]
    terms = [["literal", w, None if k % 4 else "@en"] for k, w in enumerate(words)] + [["iri", "http://example.org/" + w.strip()] for w in ascii_words[:40]] + \
            [["literal", str(k), "xsd:integer"] for k in range(10)]
    tv, off, heap, langs = ku.term_dictionary(terms)
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    gs.set_strings(off, heap); os_.set_strings(off, heap)
    n_ascii = len(ascii_words)
    ids = rng.integers(0, len(tv) + 2, 6000).astype(np.uint32)
    ascii_ids = np.concatenate([rng.integers(1, n_ascii + 1, 3000), rng.integers(len(words) + 1, len(tv), 500)]).astype(np.uint32)   # (case mapping: ASCII strings, IRIs, integers)
    en = langs.index("en")
    exprs_any = [
        EBV(EQ(STR(col(0)), lit_str(ascii_words[3]))), EBV(LT(STR(col(0)), lit_str("b"))), EBV(GEQ(STR(col(0)), lit_str("http://example.org/c"))),
        EBV(CONTAINS(STR(col(0)), "example.org/a")), EBV(STRSTARTS(STR(col(0)), "http://")), EBV(REGEX(STR(col(0)), "^[0-9]+$")),
        EBV(GT(STRLEN(ENC_TV(col(0))), integer(5))), EBV(EQ(STRLEN(STR(col(0))), integer(7))),
        EBV(EQ(SUBSTR(ENC_TV(col(0)), integer(2), integer(3)), lit_str("bc"))), EBV(EQ(SUBSTR(ENC_TV(col(0)), integer(2), integer(3)), lit_str("bc", en))),
        EBV(STRENDS(SUBSTR(STR(col(0)), integer(3)), "a")), EBV(SUBSTR(ENC_TV(col(0)), integer(4))), EBV(SUBSTR(ENC_TV(col(0)), integer(0))),
        EBV(LT(SUBSTR(ENC_TV(col(0)), integer(1), integer(2)), SUBSTR(ENC_TV(col(0)), integer(2), integer(2)))),
        EBV(EQ(SUBSTR(STR(col(0)), integer(8), integer(40)), STR(col(0)))),
        NOT(EBV(EQ(STRLEN(SUBSTR(ENC_TV(col(0)), integer(2), integer(300))), integer(0)))),
        # STRBEFORE / STRAFTER (str_before.rs / str_after.rs): views cut at the first occurrence; "" when absent; language rules
        EBV(EQ(STRBEFORE(ENC_TV(col(0)), lit_str("b")), lit_str("a"))), EBV(EQ(STRBEFORE(ENC_TV(col(0)), lit_str("b")), lit_str("a", en))),
        EBV(EQ(STRAFTER(STR(col(0)), lit_str("example.org/")), lit_str(ascii_words[2].strip()))), EBV(STRAFTER(ENC_TV(col(0)), lit_str("c"))),
        EBV(EQ(STRLEN(STRBEFORE(ENC_TV(col(0)), lit_str(""))), integer(0))), EBV(EQ(STRAFTER(ENC_TV(col(0)), lit_str("")), ENC_TV(col(0)))),
        EBV(STRBEFORE(ENC_TV(col(0)), lit_str("_", en))), EBV(GT(STRLEN(STRAFTER(ENC_TV(col(0)), lit_str("a", en))), integer(2))),
        EBV(CONTAINS(STRAFTER(STRBEFORE(STR(col(0)), lit_str(".")), lit_str("a")), "b")), EBV(REGEX(STRAFTER(STR(col(0)), lit_str("://")), "^example")),
        EBV(LT(STRBEFORE(ENC_TV(col(0)), lit_str(" ")), STRAFTER(ENC_TV(col(0)), lit_str(" ")))),
        EBV(EQ(STRBEFORE(ENC_TV(col(0)), SUBSTR(ENC_TV(col(0)), integer(3), integer(1))), SUBSTR(ENC_TV(col(0)), integer(1), integer(2)))),
        EBV(STRAFTER(ENC_TV(col(0)), lit_str("ä"))), EBV(EQ(STRBEFORE(ENC_TV(col(0)), lit_str("語")), lit_str("日本"))),
    ]
    for e in exprs_any:
        check_filter(torch_cuda, gs, os_, e, [ids])
    exprs_ascii = [
        EBV(EQ(UCASE(ENC_TV(col(0))), lit_str(ascii_words[5].upper()))), EBV(CONTAINS(LCASE(ENC_TV(col(0))), "ab")),
        EBV(REGEX(UCASE(STR(col(0))), "^HTTP://EXAMPLE")), EBV(LT(LCASE(STR(col(0))), lit_str("c"))),
        EBV(EQ(UCASE(SUBSTR(LCASE(ENC_TV(col(0))), integer(2), integer(2))), lit_str("BC"))),
        EBV(EQ(LCASE(ENC_TV(col(0))), UCASE(ENC_TV(col(0))))),
        EBV(EQ(STRBEFORE(UCASE(ENC_TV(col(0))), lit_str("B")), lit_str("A"))), EBV(STRAFTER(LCASE(STR(col(0))), lit_str("example.org/a"))),
        EBV(CONTAINS(UCASE(STRAFTER(ENC_TV(col(0)), lit_str("a"))), "C")),
    ]
    for e in exprs_ascii:
        check_filter(torch_cuda, gs, os_, e, [ascii_ids])
    # not restated on the device: never answered differently, the execute fails (and the oracle refuses the same)
    for e, rows in ((EBV(EQ(UCASE(ENC_TV(col(0))), lit_str("X"))), np.array([n_ascii + 1], np.uint32)),
                    (EBV(SUBSTR(ENC_TV(col(0)), double(2.0))), np.array([1, 2], np.uint32))):
        pb = PlanBuilder()
        desc = pb.build(pb.filter(pb.table(0, 1), e))
        keep, ptrs = table_on_device(torch_cuda, [rows])
        plan = gs.plan(desc); plan.bind_table(0, ptrs, len(rows))
        with pytest.raises(rf.RdfGpuError) as err:
            plan.execute()
        assert err.value.status == abi.ERR_UNSUPPORTED
        with pytest.raises(RuntimeError):
            os_.execute(desc, [[rows]])
    pb = PlanBuilder()                       # a string literal given by rank only next to computed strings: refused at compile time
    with pytest.raises(rf.RdfGpuError):
        gs.plan(pb.build(pb.filter(pb.table(0, 1), EBV(EQ(STR(col(0)), lit_tv(abi.TV_STRING, 3))))))


def test_regex_perl_classes_and_word_boundaries(torch_cuda):
    """`\\d \\w \\s \\D \\W \\S` (alone and inside classes) and `\\b \\B`: device automaton vs the oracle's Pike VM and vs
    Python's `re` (re.ASCII) over an all-ASCII dictionary — both the per-term verdict table and the per-row VM."""
    import re
    rng = np.random.default_rng(123)
    strings = [ku.random_subject(rng, ascii_only=True) for _ in range(1500)] + ["", "a", "foo", "a foo b", "afoo", "ab12", "GraduateStudent42 x"]
    tv, offsets, heap = string_dictionary(strings)
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    gs.set_strings(offsets, heap)
    os_.set_strings(offsets, heap)
    ids = rng.integers(0, len(tv), 20_000).astype(np.uint32)
    payload = np.arange(len(ids), dtype=np.uint32) + 1
    keep, ptrs = table_on_device(torch_cuda, [ids, payload])
    is_str = (ids >= 1) & (ids <= len(strings))
    cases = [("\\d+", "", "\\d+", re.A), ("^\\w+$", "", "^\\w+\\Z", re.A), ("\\bfoo\\b", "", "\\bfoo\\b", re.A), ("\\Bfoo", "", "\\Bfoo", re.A),
             ("[\\d\\s]x", "", "[\\d\\s]x", re.A), ("grad\\w*\\d{2}\\b", "i", "grad\\w*\\d{2}\\b", re.A | re.I), ("\\S\\s\\S", "", "\\S\\s\\S", re.A),
             # Unicode general categories: their ASCII members (all-ASCII subjects), folded before negation under `i`
             ("\\p{L}+\\p{Nd}", "", "[A-Za-z]+[0-9]", re.A), ("^\\p{Lu}", "", "^[A-Z]", re.A), ("\\P{L}", "", "[^A-Za-z]", re.A), ("[\\p{Nd}x]\\pL", "", "[0-9x][A-Za-z]", re.A),
             ("(?i)\\P{Lu}", "", "[^A-Za-z]", re.A), ("\\p{Pd}\\p{Zs}?", "", "-[ ]?", re.A), ("[\\w--\\d]+7", "", "[A-Za-z_]+7", re.A)]
    while len(cases) < 190:
        pat, flags, py, py_flags = ku.random_regex(rng, perl=True, extended=len(cases) >= 140)
        if "x" in flags and len(cases) >= 140 and any(t in pat for t in ("[:", "&&", "--", "~~")):
            continue                          # (Python's verbose mode reads the spelled-out classes its own way)
        try:
            rf.engine.regex_check(pat, flags)
            rx = re.compile(py, py_flags)
        except (rf.engine.RdfGpuError, re.error):
            continue
        cases.append((pat, flags, py, py_flags))
    matched_some = 0
    for k, (pat, flags, py, py_flags) in enumerate(cases):
        pb = PlanBuilder()
        desc = pb.build(pb.filter(pb.table(0, 2), EBV(REGEX(ENC_TV(col(0)), pat, flags)), projection=[1]))
        plan, got = run_both(gs, os_, desc, gpu_tables=[(ptrs, len(ids))], cpu_tables=[[ids, payload]])
        matched_some += plan.result_info()[0] > 0
        rx = re.compile(py, py_flags)
        if "\\B" not in pat:              # Python (< 3.14) never matches \B against the empty string
            exp = np.array([bool(is_str[r]) and rx.search(strings[ids[r] - 1]) is not None for r in range(len(ids))])
            np.testing.assert_array_equal(np.sort(got[0]), payload[exp], err_msg=repr((pat, flags)))
        if k % 4 == 0:                    # the per-row VM path gives the same rows as the verdict table
            p2 = gs.plan(desc).set_option("NO_STRING_VERDICTS"); p2.bind_table(0, ptrs, len(ids))
            np.testing.assert_array_equal(np.sort(p2.execute().fetch()[0]), np.sort(got[0]))
    assert matched_some > 90


def test_regex_perl_class_over_non_ascii_subject_is_a_loud_error(torch_cuda):
    """`\\d \\w \\s \\b` are compiled with their ASCII members (the crate's Unicode tables are not restated): a row whose
    subject holds a non-ASCII character is refused at run time — never answered from the ASCII approximation; rows
    that do not touch such a string are answered, and patterns without those classes stay exact on any subject."""
    strings = ["abc 12", "caf\u00e9 12", "x"]
    tv, offsets, heap = string_dictionary(strings, lang_every=100)
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    gs.set_strings(offsets, heap)
    os_.set_strings(offsets, heap)
    for option in (None, "NO_STRING_VERDICTS"):
        for pat in ("\\d+", "\\bcaf", "[\\s]1"):
            pb = PlanBuilder()
            desc = pb.build(pb.filter(pb.table(0, 1), EBV(REGEX(ENC_TV(col(0)), pat, ""))))
            ascii_rows = np.array([1, 3, 1, 0, 4], np.uint32)
            keep, ptrs = table_on_device(torch_cuda, [ascii_rows])
            plan = gs.plan(desc)
            if option:
                plan.set_option(option)
            plan.bind_table(0, ptrs, len(ascii_rows))
            got = plan.execute().fetch()
            exp, n_exp, _ = os_.execute(desc, [[ascii_rows]])
            np.testing.assert_array_equal(ku.multiset(got, plan.result_info()[0]), ku.multiset(exp, n_exp))
            rows = np.array([1, 2, 3], np.uint32)
            keep2, ptrs2 = table_on_device(torch_cuda, [rows])
            plan.bind_table(0, ptrs2, len(rows))
            with pytest.raises(rf.RdfGpuError, match="Unicode"):
                plan.execute()
            with pytest.raises(Exception, match="Unicode"):
                os_.execute(desc, [[rows]])
            plan.bind_table(0, ptrs, len(ascii_rows))          # the plan stays usable after the refusal
            np.testing.assert_array_equal(ku.multiset(plan.execute().fetch(), n_exp), ku.multiset(exp, n_exp))
        pb = PlanBuilder()
        desc = pb.build(pb.filter(pb.table(0, 1), EBV(REGEX(ENC_TV(col(0)), "caf.", ""))))
        rows = np.array([1, 2, 3], np.uint32)
        keep2, ptrs2 = table_on_device(torch_cuda, [rows])
        plan, got = run_both(gs, os_, desc, gpu_tables=[(ptrs2, 3)], cpu_tables=[[rows]])
        assert got[0].tolist() == [2]


def test_regex_variable_pattern_rq(torch_cuda):
    """testsuite/oxigraph-tests/sparql/regex_variable.rq as written: `VALUES (?l ?r) { ("a" "^a$") ("b" "^a$") }
    FILTER(REGEX(?l, ?r))` -> one solution, ?l = "a" (regex_variable.srx).  The pattern is a per-row value
    (regex.rs:59-76): the host announces the distinct pattern literals, the row picks its program by object id."""
    strings = ["a", "b", "^a$"]
    tv, offsets, heap = string_dictionary(strings, lang_every=100)
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    gs.set_strings(offsets, heap)
    os_.set_strings(offsets, heap)
    l = np.array([1, 2], np.uint32); r = np.array([3, 3], np.uint32)
    keep, ptrs = table_on_device(torch_cuda, [l, r])
    pb = PlanBuilder()
    desc = pb.build(pb.filter(pb.table(0, 2), EBV(REGEX_VAR(ENC_TV(col(0)), ENC_TV(col(1)), {3: "^a$"})), projection=[0]))
    plan, got = run_both(gs, os_, desc, gpu_tables=[(ptrs, 2)], cpu_tables=[[l, r]])
    assert got[0].tolist() == [1]                    # ?l = "a"


def test_regex_variable_patterns_match_oracle(torch_cuda):
    """Many distinct per-row patterns (incl. an invalid-flag program, a language-tagged "pattern" = error value, nulls and
    non-strings); a pattern id the host did not announce is a loud run-time error, not a non-match."""
    rng = np.random.default_rng(5)
    patterns = ["^a", "b$", "a.c", "(ab|cd)+", "\\d", "^\\w+$", "x{2,}", "k", "[^a]b", "\\bfoo\\b"]
    subjects = [ku.random_subject(rng, ascii_only=True) for _ in range(600)] + ["", "foo", "abc", "xx7"]
    strings = subjects + patterns
    tv, offsets, heap = string_dictionary(strings, lang_every=97)       # some subjects and one pattern carry a language tag
    first_pat = 1 + len(subjects)
    table = {first_pat + k: p for k, p in enumerate(patterns)}
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    gs.set_strings(offsets, heap)
    os_.set_strings(offsets, heap)
    n = 30_000
    val = rng.integers(0, len(tv), n).astype(np.uint32)
    pat = rng.integers(first_pat, first_pat + len(patterns), n).astype(np.uint32)
    pat[rng.random(n) < 0.02] = 0                                       # unbound pattern
    pat[rng.random(n) < 0.02] = len(tv) - 1                             # a non-string "pattern": the error value
    payload = np.arange(n, dtype=np.uint32) + 1
    keep, ptrs = table_on_device(torch_cuda, [val, pat, payload])
    for flags in ("", "i", "s"):
        for negate in (False, True):
            e = EBV(REGEX_VAR(ENC_TV(col(0)), ENC_TV(col(1)), table, flags))
            pb = PlanBuilder()
            desc = pb.build(pb.filter(pb.table(0, 3), NOT(e) if negate else e, projection=[2]))
            plan, got = run_both(gs, os_, desc, gpu_tables=[(ptrs, n)], cpu_tables=[[val, pat, payload]])
            assert 0 < plan.result_info()[0] < n
    partial = dict(list(table.items())[:-1])
    pb = PlanBuilder()
    desc = pb.build(pb.filter(pb.table(0, 3), EBV(REGEX_VAR(ENC_TV(col(0)), ENC_TV(col(1)), partial)), projection=[2]))
    plan = gs.plan(desc); plan.bind_table(0, ptrs, n)
    with pytest.raises(rf.RdfGpuError, match="announce"):
        plan.execute()


def test_enc_pt_decode_on_device(torch_cuda):
    """ENC_PT (object_id_mapping.rs:331-374) of result columns, decoded on the device: term type, lexical form, tag and aux
    of every row against the CPU restatement; null / unknown ids are null structs; windows of rows; multi-byte UTF-8, empty
    and long forms; an empty result; a store without lexical forms refuses."""
    rng = np.random.default_rng(21)
    forms = ["http://example.org/" + "x" * int(rng.integers(0, 40)) + str(i) for i in range(300)]
    forms += ["_:b%d" % i for i in range(50)] + ["", "caf\u00e9", "\u20acuro \U0001F600", "y" * 5000] + [ku.random_subject(rng) for _ in range(600)]
    tv, offsets, heap = string_dictionary(forms, n_other=6)
    tv["tag"][1:301] = abi.TV_NAMED_NODE; tv["tag"][301:351] = abi.TV_BLANK_NODE
    # the non-string ids get lexical forms too (ENC_PT needs every term's): rebuild offsets / heap for ALL ids
    n_ids = len(tv)
    all_forms = [""] + forms + [str(int(tv["lo"][i])) for i in range(1 + len(forms), n_ids)]
    blob = [f.encode("utf-8") for f in all_forms]
    offsets = np.zeros(n_ids + 1, dtype=np.uint64); offsets[1:] = np.cumsum([len(b) for b in blob])
    heap = b"".join(blob)
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    ids = rng.integers(0, n_ids + 3, 50_000).astype(np.uint32)           # 0 = null, >= n_ids = unknown
    other = np.arange(1, len(ids) + 1, dtype=np.uint32)
    keep, ptrs = table_on_device(torch_cuda, [ids, other])
    pb = PlanBuilder()
    plan = gs.plan(pb.build(pb.filter(pb.table(0, 2), lit_bool(True))))
    plan.bind_table(0, ptrs, len(ids)); plan.execute()
    with pytest.raises(rf.RdfGpuError):                                  # no lexical forms installed yet
        plan.decode_terms(0)
    gs.set_strings(offsets, heap)
    got_ids = plan.fetch()[0]
    exp = orc.decode_terms(got_ids, tv, offsets, heap)
    for first, n in ((0, None), (0, 0), (17, 1), (4999, 20_001), (len(ids), 0)):
        arr = plan.decode_terms(0, first, n)
        rows = arr.to_pylist()
        want = exp[first:] if n is None else exp[first:first + n]
        assert len(rows) == len(want)
        for r, w in zip(rows, want):
            assert (r is None) == (w is None)
            if w is not None:
                assert (r["term_type"], r["value"], r["tag"], r["aux"]) == w
    assert arr.type.field(1).type == __import__("pyarrow").utf8()
    pb = PlanBuilder()
    empty = gs.plan(pb.build(pb.filter(pb.table(0, 2), lit_bool(False))))
    empty.bind_table(0, ptrs, len(ids)); empty.execute()
    assert len(empty.decode_terms(1)) == 0
    with pytest.raises(rf.RdfGpuError):
        plan.decode_terms(5)


def _nt_text(rng, n, n_subj=500, messy=True):
    """random N-Triples: IRIs, blank nodes, plain / language-tagged / typed literals with escapes, `>` `.` `#` and multi-byte
    UTF-8 inside strings; blank lines, comment lines, tabs, CRLF and trailing comments when `messy`"""
    subj = ["<http://example.org/s%d>" % i for i in range(n_subj)] + ["_:b%d" % i for i in range(n_subj // 10)]
    pred = ["<http://example.org/p%d>" % i for i in range(20)]
    lits = ['"plain %d"' % i for i in range(300)] + ['"caf\u00e9 \u20ac"@fr', '"quote \\" inside > . # x"', '"tab\\tnew\\nline"@en-GB', '""',
            '"12"^^<http://www.w3.org/2001/XMLSchema#integer>', '"1.5E3"^^<http://www.w3.org/2001/XMLSchema#double>', '"\U0001F600"']
    lines = []
    for i in range(n):
        s_ = subj[int(rng.integers(0, len(subj)))]
        p_ = pred[int(rng.integers(0, len(pred)))]
        o_ = (subj if rng.random() < 0.5 else lits)[int(rng.integers(0, len(subj) if rng.random() < 0 else min(len(subj), len(lits))))]
        sep = "\t" if messy and i % 7 == 0 else " "
        end = " ." if not (messy and i % 11 == 0) else "."
        if o_.startswith("_:") and end == ".":
            end = " ."                                   # `_:b1.` would make the dot part of nothing: keep it unambiguous half the time
        line = s_ + sep + p_ + sep + o_ + end
        if messy and i % 13 == 0:
            line += "  # trailing comment"
        if messy and i % 17 == 0:
            line += "\r"
        lines.append(line)
        if messy and i % 29 == 0:
            lines.append("")
        if messy and i % 31 == 0:
            lines.append("# a comment line <x> <y> <z> .")
    return "\n".join(lines) + ("\n" if n % 2 else "")


@pytest.mark.parametrize("n", [0, 1, 1000, 200_000])
def test_ntriples_to_ids_on_device(torch_cuda, n):
    """N-Triples text -> object ids on the device (rdfgpu_ntriples_parse): the same triples as the CPU restatement of the
    reference's interning loop, through a different id assignment (a bijection onto the distinct terms); the id columns feed
    rdfgpu_store_extend_device directly; malformed lines fail with their number."""
    rng = np.random.default_rng(n + 3)
    text = _nt_text(rng, n)
    terms_ref, s_ref, p_ref, o_ref = orc.ntriples_encode(text)
    nt = rf.NTriples(text, first_id=5)
    assert nt.n_triples == len(s_ref) and nt.n_terms == len(terms_ref)
    terms = nt.terms()
    assert sorted(terms) == sorted(terms_ref) and len(set(terms)) == len(terms)
    if n:
        sp, pp, op = nt.columns()
        gs = rf.GpuQuadStore()
        zeros = torch_cuda.zeros(nt.n_triples, dtype=torch_cuda.int32, device="cuda")
        gs.extend_device(zeros.data_ptr(), sp, pp, op, nt.n_triples)
        g, s_, p_, o_ = gs.read_index(abi.GSPO)
        got = sorted({(terms[a - 5], terms[b - 5], terms[c - 5]) for a, b, c in zip(s_.tolist(), p_.tolist(), o_.tolist())})
        exp = sorted({(terms_ref[a - 1], terms_ref[b - 1], terms_ref[c - 1]) for a, b, c in zip(s_ref, p_ref, o_ref)})
        assert got == exp and len(got) > 0
    nt.close()
    for bad, line in (("<a> <b> <c> .\n<a> <b> .\n", 2), ('<a> <b> "open\n', 1), ("<a> <b> <c> <d> .\n", 1), ('"lit" <b> <c> .\n', 1), ("<a> <b> <c>\n", 1)):
        with pytest.raises(rf.RdfGpuError, match="triple line %d" % line):
            rf.NTriples(bad)
        with pytest.raises(ValueError):
            orc.ntriples_encode(bad)


def test_ntriples_escapes_and_typed_literals_on_device(torch_cuda):
    """rdfgpu_ntriples_decoded: terms are interned by the canonical form the reference's parser produces (ECHAR / UCHAR
    decoded, language tags lower-cased, `^^xsd:string` = simple literal), the decoded lexical forms and the typed-value rows of
    xsd:integer / int / boolean / decimal / (exactly convertible) double / float literals come from the device — against an
    independent Python restatement (oracle.ntriples_decode_term / ntriples_typed_value: re, int, Fraction)."""
    X = "http://www.w3.org/2001/XMLSchema#"
    lits = [
        # one term, several spellings -> one id
        '"aA\\n"', '"a\\u0041\\n"', '"\\u0061\\U00000041\\u000A"', '"x"', '"x"^^<%sstring>' % X, '"v"@en-GB', '"v"@EN-gb', '"v"@en-gb',
        # escapes of every kind, quotes and delimiters inside strings
        '"q\\"uote \\\\ back \\t tab \\b \\r \\f \\\' end"', '"\\U0001F600 and \\u20AC"', '"> . # <"', '""',
        # typed literals
        '"12"^^<%sinteger>' % X, '"012"^^<%sinteger>' % X, '"+7"^^<%sint>' % X, '"-9223372036854775808"^^<%slong>' % X, '"9223372036854775808"^^<%sinteger>' % X,
        '"2147483648"^^<%sint>' % X, '"1 2"^^<%sinteger>' % X, '""^^<%sinteger>' % X, '"255"^^<%sunsignedByte>' % X, '"-"^^<%sinteger>' % X,
        '"true"^^<%sboolean>' % X, '"0"^^<%sboolean>' % X, '"TRUE"^^<%sboolean>' % X,
        '"1.50"^^<%sdecimal>' % X, '".5"^^<%sdecimal>' % X, '"-12."^^<%sdecimal>' % X, '"."^^<%sdecimal>' % X, '"1.0000000000000000001"^^<%sdecimal>' % X,
        '"170141183460469231731.687303715884105727"^^<%sdecimal>' % X, '"170141183460469231732"^^<%sdecimal>' % X, '"1e3"^^<%sdecimal>' % X,
        '"1.5E3"^^<%sdouble>' % X, '"0.1"^^<%sdouble>' % X, '"-0"^^<%sdouble>' % X, '"INF"^^<%sdouble>' % X, '"-inf"^^<%sdouble>' % X, '"NaN"^^<%sdouble>' % X,
        '"1e22"^^<%sdouble>' % X, '"1e23"^^<%sdouble>' % X, '"9007199254740993"^^<%sdouble>' % X, '"123456789012345678901234"^^<%sdouble>' % X, '"1."^^<%sdouble>' % X,
        '"abc"^^<%sdouble>' % X, '"0.000001"^^<%sdouble>' % X, '"1234.5e-7"^^<%sdouble>' % X,
        '"0.1"^^<%sfloat>' % X, '"16777217"^^<%sfloat>' % X, '"3.5e10"^^<%sfloat>' % X, '"1e11"^^<%sfloat>' % X, '"2.5"^^<%sfloat>' % X,
        '"2004-03-01T06:00:00Z"^^<%sdateTime>' % X, '"P1Y"^^<%sduration>' % X, '"x"^^<http://example.org/dt>', '"x"^^<http://example.org/d\\u0074>',
    ]
    iris = ["<http://example.org/s%d>" % i for i in range(40)] + ["<http://example.org/caf\\u00E9>", "<http://example.org/caf\u00e9>", "_:b1", "_:b2"]
    rng = np.random.default_rng(8)
    lines = []
    for k, o_ in enumerate(lits * 3 + iris):
        s_ = iris[int(rng.integers(0, len(iris)))]
        lines.append("%s <http://example.org/p%d> %s ." % (s_ if not s_.startswith('"') else iris[0], k % 5, o_))
    text = "\n".join(lines) + "\n"
    terms_ref, s_ref, p_ref, o_ref = orc.ntriples_encode(text)
    canon_ref = [orc.ntriples_decode_term(t) for t in terms_ref]
    assert len(set(canon_ref)) == len(canon_ref)
    nt = rf.NTriples(text, first_id=3)
    assert nt.n_triples == len(s_ref) and nt.n_terms == len(terms_ref)
    decoded, typed, dec_hi = nt.decoded()
    assert sorted(decoded) == sorted(canon_ref)                       # the same distinct terms, decoded alike
    assert len(set(decoded)) == nt.n_terms
    # the spellings that must have merged
    one = lambda lex, kind=3, sfx=b"": sum(1 for d in decoded if d == (kind, lex, sfx))
    assert one(b"aA\n") == 1 and one(b"x") == 1 and one(b"v", 4, b"en-gb") == 1 and one("http://example.org/caf\u00e9".encode(), 1) == 1
    assert one(b"x", 5, b"http://example.org/dt") == 1
    # the triples, through the ids, are the restatement's triples
    sp, pp, op = nt.columns()
    gs = rf.GpuQuadStore()
    zeros = torch_cuda.zeros(nt.n_triples, dtype=torch_cuda.int32, device="cuda")
    gs.extend_device(zeros.data_ptr(), sp, pp, op, nt.n_triples)
    g, s_, p_, o_ = gs.read_index(abi.GSPO)
    got = sorted({(decoded[a - 3], decoded[b - 3], decoded[c - 3]) for a, b, c in zip(s_.tolist(), p_.tolist(), o_.tolist())})
    exp = sorted({(canon_ref[a - 1], canon_ref[b - 1], canon_ref[c - 1]) for a, b, c in zip(s_ref, p_ref, o_ref)})
    assert got == exp
    # typed values
    n_parsed = n_host = 0
    for t, (kind, lex, sfx) in enumerate(decoded):
        tag, lo, flags, hi, host = orc.ntriples_typed_value(kind, lex, sfx)
        row = typed[t]
        assert row["tag"] == tag, (lex, sfx, int(row["tag"]), tag)
        if host:                                                   # the device may leave it to the host — or not: if it parsed it, the value must be right
            assert row["flags"] & abi.TVF_NEEDS_HOST, (lex, sfx)
            n_host += 1
            continue
        assert not (row["flags"] & abi.TVF_NEEDS_HOST), (lex, sfx)
        if host is None:                                           # NaN: any payload
            assert np.isnan(np.array([row["lo"]], np.int64).view(np.float64)[0])
            continue
        assert (int(row["lo"]), int(row["flags"]), int(dec_hi[t])) == (lo, flags, hi), (lex, sfx, int(row["lo"]), lo, int(dec_hi[t]), hi)
        n_parsed += tag in (abi.TV_INTEGER, abi.TV_INT, abi.TV_BOOLEAN, abi.TV_DECIMAL, abi.TV_DOUBLE, abi.TV_FLOAT)
    assert n_parsed >= 20 and n_host >= 6
    nt.close()
    for bad in ('<a> <b> "bad \\q escape" .\n', '<a> <b> "\\u12" .\n', '<a> <b> "\\uD800" .\n', '<a\\n> <b> <c> .\n', '<a> <b> "\\U00110000" .\n'):
        with pytest.raises(rf.RdfGpuError, match="triple line 1"):
            rf.NTriples(bad)
        with pytest.raises(ValueError):
            orc.ntriples_encode(bad)


def test_regex_unsupported_is_refused_loudly(torch_cuda):
    tv, offsets, heap = string_dictionary(["abc"])
    gs, _ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    pb = PlanBuilder()
    desc = pb.build(pb.filter(pb.table(0, 1), EBV(REGEX(ENC_TV(col(0)), "a", ""))))
    with pytest.raises(rf.RdfGpuError):          # no strings installed
        gs.plan(desc)
    gs.set_strings(offsets, heap)
    gs.plan(desc)
    for bad in ("\\p{Greek}", "(?u)a", "a|^b", "[é]"):      # (\\p{L}, (?i)a, [a&&b] are inside the subset since ABI 3: tests/test_regex_cpu.py)
        pb = PlanBuilder()
        with pytest.raises(rf.RdfGpuError):
            gs.plan(pb.build(pb.filter(pb.table(0, 1), EBV(REGEX(ENC_TV(col(0)), bad, "")))))
    pb = PlanBuilder()
    with pytest.raises(rf.RdfGpuError, match="no lexical form on the device"):   # REGEX over a literal given by rank only: refused at compile
        gs.plan(pb.build(pb.filter(pb.table(0, 1), EBV(REGEX(lit_tv(abi.TV_STRING, 0), "a", "")))))
    from rdf_fusion_amd.plan import STRLEN, UCASE, lit_str
    for e in (EBV(EQ(STRLEN(lit_tv(abi.TV_STRING, 0)), integer(1))), EBV(CONTAINS(UCASE(lit_tv(abi.TV_STRING, 0)), "A"))):
        pb = PlanBuilder()
        with pytest.raises(rf.RdfGpuError, match="no lexical form on the device"):
            gs.plan(pb.build(pb.filter(pb.table(0, 1), e)))
    pb = PlanBuilder()                            # ... while the same literal WITH its bytes is an ordinary operand
    gs.plan(pb.build(pb.filter(pb.table(0, 1), EBV(REGEX(lit_str("abc"), "a", "")))))


def test_lubm_shaped_optional_plus_regex(torch_cuda):
    """BASELINE config 5 shape: a star join, an OPTIONAL (left-outer join) and a REGEX FILTER over a string-valued
    variable — `?s type Student . ?s name ?n . OPTIONAL { ?s email ?e } FILTER regex(?n, "^Grad.*[0-9]7$")`."""
    rng = np.random.default_rng(5)
    n_students = 4000
    TYPE, NAME, EMAIL, STUDENT = 1, 2, 3, 4
    base = 10
    names = [("GraduateStudent" if rng.random() < 0.5 else "UndergraduateStudent") + str(int(rng.integers(0, 500))) for _ in range(n_students)]
    emails = [f"s{k}@dept{int(rng.integers(0, 20))}.univ.edu" for k in range(n_students)]
    strings = names + emails
    tv, offsets, heap = string_dictionary(strings, n_other=0)
    # string ids start at 1: shift every id by the entity ids that come first
    n_entities = base + n_students
    shift = n_entities
    tv2 = np.zeros(shift + len(tv), dtype=TV_DTYPE)
    tv2[shift:] = tv
    tv2["tag"][1:shift] = abi.TV_NAMED_NODE
    tv2["lo"][1:shift] = np.arange(1, shift)
    off2 = np.concatenate([np.zeros(shift, np.uint64), offsets])
    stu = base + np.arange(n_students, dtype=np.uint32)
    name_id = (shift + 1 + np.arange(n_students)).astype(np.uint32)
    email_id = (shift + 1 + n_students + np.arange(n_students)).astype(np.uint32)
    has_email = rng.random(n_students) < 0.6
    s_col = np.concatenate([stu, stu, stu[has_email]])
    p_col = np.concatenate([np.full(n_students, TYPE), np.full(n_students, NAME), np.full(has_email.sum(), EMAIL)]).astype(np.uint32)
    o_col = np.concatenate([np.full(n_students, STUDENT, np.uint32), name_id, email_id[has_email]])
    gs, os_ = both_stores((np.zeros(len(s_col), np.uint32), s_col.astype(np.uint32), p_col, o_col.astype(np.uint32)), typed=tv2)
    gs.set_strings(off2, heap)
    os_.set_strings(off2, heap)
    total = 0
    for pat, flags in (("^Grad.*[0-9]7$", ""), ("student1[0-9]$", "i"), ("^Under", ""), ("7", "q")):
        pb = PlanBuilder()
        typ = pb.data_source(quad_pattern("s", TYPE, STUDENT))            # (s)
        nam = pb.data_source(quad_pattern("s", NAME, "n"))                # (s, n)
        eml = pb.data_source(quad_pattern("s", EMAIL, "e"))               # (s, e)
        j = pb.hash_join(typ, nam, on=[(0, 0)], projection=[0, 2])        # (s, n)
        opt = pb.hash_join(j, eml, on=[(0, 0)], join_type=abi.JOIN_LEFT, projection=[0, 1, 3])   # (s, n, e?)
        flt = pb.filter(opt, EBV(REGEX(ENC_TV(col(1)), pat, flags)))
        plan, got = run_both(gs, os_, pb.build(flt))
        total += plan.result_info()[0]
        if pat == "^Under":
            assert (got[2] == 0).any() and (got[2] != 0).any()             # OPTIONAL: bound and unbound ?e both survive
    assert total > 0


def test_lubm_q9_optional_regex_matches_oracle():
    """BASELINE config 5 at test scale: LUBM-shaped data (rdf_fusion_amd/lubm.py), Q9's student - advisor - course
    triangle (a two-key join closes it), a REGEX FILTER on the student's name and the OPTIONAL e-mail address."""
    from rdf_fusion_amd import lubm
    ds = lubm.generate(6)
    gs, os_ = both_stores((ds.g, ds.s, ds.p, ds.o), typed=ds.typed_values)
    gs.set_strings(ds.str_offsets, ds.str_heap)
    os_.set_strings(ds.str_offsets, ds.str_heap)
    total = 0
    for pattern, flags in (("^GraduateStudent1", ""), (".", ""), ("student[0-9]*7$", "i"), ("^Undergraduate", ""), ("^Nobody", "")):
        plan, got = run_both(gs, os_, lubm.q9_optional_regex_plan(ds, pattern, flags))
        total += plan.result_info()[0]
        if pattern == ".":
            assert (got[4] == 0).any() and (got[4] != 0).any()             # OPTIONAL: students with and without an address
            x, y, z = got[0], got[1], got[2]                                # the triangle, checked on the raw triples
            key = lambda a, b: (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)
            for pname, a, b in (("ub:advisor", x, y), ("ub:teacherOf", y, z), ("ub:takesCourse", x, z)):
                m = ds.p == ds.pred[pname]
                assert np.isin(key(a, b), key(ds.s[m], ds.o[m])).all()
    assert total > 100


def test_fused_lookup_chain_equals_unfused(bsbm_stores, torch_cuda, monkeypatch):
    """Re-executions of the batched Q5 run the window / label joins inside the candidate join's resolve phase (one
    kernel, nothing materialised in between); every execution must still equal the oracle, also when the parameters
    change between executions, and equal the unfused engine."""
    ds, gs, os_ = bsbm_stores
    desc = bsbm.q5_batch_plan(ds)
    plan = gs.plan(desc)
    rng = np.random.default_rng(77)
    fused_seen = band_seen = False
    for it in range(4):
        batch = 150 + 40 * it
        prods = np.array([ds.product(i) for i in rng.choice(ds.n_products, batch, replace=False)], dtype=np.uint32)
        params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
        keep, ptrs = table_on_device(torch_cuda, params)
        plan.bind_table(0, ptrs, batch)
        plan.enable_kernel_timing(True)
        got = plan.execute().fetch()
        exp, n_exp, _ = os_.execute(desc, [params])
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        names = [k[0] for k in plan.kernel_stats()]
        fused_seen = fused_seen or any("lds_join_kernel" in n and n.rstrip(">").endswith("true") for n in names)
        band_seen = band_seen or any("band_mask_kernel" in n for n in names)
        if it == 3:
            plan.set_option("NO_CHAIN_FUSION", 1)
            plain = plan.execute().fetch()
            assert not any("lds_join_kernel" in k[0] and k[0].rstrip(">").endswith("true") for k in plan.kernel_stats())
            np.testing.assert_array_equal(ku.multiset(plain), ku.multiset(got))
            plan.set_option("NO_CHAIN_FUSION", 0)
    assert fused_seen or ENGINE_TOGGLED, "the lookup chain was never fused"
    assert band_seen or ENGINE_TOGGLED, "the candidate join's chain never ran as a band join"
    # the store changes under the compiled plan: every cached table / value table / range index must be rebuilt
    extra_p = rng.choice(ds.n_products, 300, replace=False)
    g2 = np.zeros(600, np.uint32)
    s2 = np.concatenate([[ds.product(int(i)) for i in extra_p]] * 2).astype(np.uint32)
    p2 = np.concatenate([np.full(300, ds.pred["bsbm:productFeature"]), np.full(300, ds.pred["bsbm:productPropertyNumeric1"])]).astype(np.uint32)
    o2 = np.concatenate([ds.feature_base + rng.integers(0, ds.n_features, 300), ds.int_base + rng.integers(0, 2000, 300)]).astype(np.uint32)
    try:
        assert gs.extend(g2, s2, p2, o2) == os_.extend(g2, s2, p2, o2)
        for it in range(3):
            got = plan.execute().fetch()
            exp, n_exp, _ = os_.execute(desc, [params])
            np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
    finally:   # the module-scoped stores go back to their original content
        assert gs.remove(g2, s2, p2, o2) == os_.remove(g2, s2, p2, o2)
    got = plan.execute().fetch()
    exp, n_exp, _ = os_.execute(desc, [params])
    np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))


TOGGLES = ["RDFGPU_NO_CHAIN_FUSION", "RDFGPU_NO_INDEX_JOIN", "RDFGPU_NO_TABLE_CACHE", "RDFGPU_NO_SPECULATION",
           "RDFGPU_NO_FIRST_RUN_SPECULATION", "RDFGPU_NO_DIRECT_TABLE", "RDFGPU_FORCE_GENERIC_VM", "RDFGPU_NO_LDS_JOIN",
           "RDFGPU_NO_GLOBAL_TABLE_JOIN", "RDFGPU_NO_FILTER_FUSION", "RDFGPU_NO_VALUE_TABLES", "RDFGPU_NO_RANGE_INDEX",
           "RDFGPU_NO_BAND_JOIN", "RDFGPU_NO_PARTITIONED_JOIN", "RDFGPU_NO_JOIN_REORDER", "RDFGPU_NO_STRING_VERDICTS",
           "RDFGPU_NO_VALUE_VERDICTS", "RDFGPU_NO_RUN_COPY", "RDFGPU_NO_PRIMING", "RDFGPU_NO_ORDERED_JOIN", "RDFGPU_NO_BAND_PACK16", "RDFGPU_NO_RANGE_PARTITION",
           "RDFGPU_NO_OWN_PARTITION_PASS", "RDFGPU_NO_BAND_COMPACT", "RDFGPU_NO_PROBE_OUTER_JOIN", "RDFGPU_NO_STREAM_JOIN"]


@pytest.mark.parametrize("toggle", TOGGLES)
def test_engine_toggles_do_not_change_results(bsbm_stores, torch_cuda, request, toggle):
    """Every physical rewrite / table form / speculation mode can be switched off; the bindings must not notice."""
    ds, gs, os_ = bsbm_stores
    before = gs.get_option(toggle)
    gs.set_option(toggle, 1)            # plans compiled from here on copy it (the environment is only read once per process)
    request.addfinalizer(lambda: gs.set_option(toggle, before))
    rng = np.random.default_rng(len(toggle))
    for x in rng.choice(ds.n_products, 3, replace=False):
        run_both(gs, os_, bsbm.q5_plan(ds, ds.product(int(x))))
    run_both(gs, os_, bsbm.q1_plan(ds, *bsbm.q1_instance(ds, rng)))
    run_both(gs, os_, bsbm.q10_plan(ds, ds.product(3), ds.country_base + 3, max_days=9, after="2004-03-01T06:00:00"))
    feats = np.bincount(ds.o[ds.p == ds.pred["bsbm:productFeature"]] - ds.feature_base).argsort()[::-1][:3] + ds.feature_base
    run_both(gs, os_, bsbm.q4_plan(ds, ds.type_base + ds.n_types - 1, int(feats[0]), int(feats[1]), int(feats[2]), 300, 400))
    desc = bsbm.q5_batch_plan(ds)
    plan = gs.plan(desc)
    for batch in (60, 90, 75, 80, 70, 85):                       # re-executions: speculative sizes, cached tables, fusion, the record-writing ordered join
        prods = np.array([ds.product(i) for i in rng.choice(ds.n_products, batch, replace=False)], dtype=np.uint32)
        params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
        keep, ptrs = table_on_device(torch_cuda, params)
        plan.bind_table(0, ptrs, batch)
        got = plan.execute().fetch()
        exp, n_exp, _ = os_.execute(desc, [params])
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))


@pytest.mark.parametrize("n_tab,dup", [(3_000, False), (40_000, True), (200_000, True)])
def test_ordered_slice_join_matches_oracle(torch_cuda, n_tab, dup):
    """A small table joined with a store slice on a column the slice is NOT sorted by, followed by look-up joins keyed by
    table columns: on re-execution the matches are emitted in the slice's order (ordered_join.hip) — the same rows as the
    probe-ordered index join and as the oracle, sorted by the slice's sort column; table rows with a null / unknown key or
    without a look-up row join nothing; duplicate table keys multiply."""
    rng = np.random.default_rng(n_tab)
    n_subj, n_obj = 30_000, 900
    P_LINK, P_A, P_B = 50_001, 50_002, 50_003
    subj = rng.integers(1000, 1000 + n_subj, 150_000).astype(np.uint32)
    obj = rng.integers(40_000, 40_000 + n_obj, 150_000).astype(np.uint32)
    sa = rng.choice(np.arange(1000, 1000 + n_subj, dtype=np.uint32), int(n_subj * 0.9), replace=False)   # 10 % of the subjects have no <a>
    sb = rng.choice(np.arange(1000, 1000 + n_subj, dtype=np.uint32), int(n_subj * 0.95), replace=False)
    s_all = np.concatenate([subj, sa, sb])
    p_all = np.concatenate([np.full(len(subj), P_LINK), np.full(len(sa), P_A), np.full(len(sb), P_B)]).astype(np.uint32)
    o_all = np.concatenate([obj, rng.integers(1, 500, len(sa)).astype(np.uint32), rng.integers(1, 500, len(sb)).astype(np.uint32)])
    gs, os_ = both_stores((np.zeros(len(s_all), np.uint32), s_all, p_all, o_all))
    pb = PlanBuilder()
    scan = lambda p_: pb.data_source(quad_pattern("s", p_, "v"))
    c = pb.hash_join(pb.table(0, 2), scan(P_LINK), on=[(1, 0)], projection=[0, 1, 3])            # (tag, X, o)
    c = pb.hash_join(c, scan(P_A), on=[(1, 0)], projection=[0, 1, 2, 4])                          # + a
    c = pb.hash_join(c, scan(P_B), on=[(1, 0)], projection=[0, 1, 2, 3, 5])                       # + b
    desc = pb.build(c)
    plan = gs.plan(desc).enable_kernel_timing(True)
    plan_off = gs.plan(desc).set_option("NO_ORDERED_JOIN")
    used = 0
    for it in range(4):
        keys = rng.integers(1000, 1000 + n_subj, n_tab).astype(np.uint32) if dup else rng.choice(np.arange(1000, 1000 + n_subj, dtype=np.uint32), n_tab, replace=False)
        keys[rng.random(n_tab) < 0.02] = 0                                   # unbound
        keys[rng.random(n_tab) < 0.02] = 999_999                             # not a subject of the slice
        tab = [np.arange(1, n_tab + 1, dtype=np.uint32), keys]
        keep, ptrs = table_on_device(torch_cuda, tab)
        exp, n_exp, _ = os_.execute(desc, [tab])
        for pl in (plan, plan_off):
            pl.bind_table(0, ptrs, n_tab)
            got = pl.execute().fetch()
            assert pl.result_info()[0] == n_exp
            np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        if any("oj_write_kernel" in k[0] for k in plan.kernel_stats()):
            used += 1
            got = plan.fetch()
            assert np.all(np.diff(got[2].astype(np.int64)) >= 0)             # sorted by the slice's sort column (?o of the GPOS slice)
    assert used >= 2 or ENGINE_TOGGLED or n_tab * 5 * 8 < 150_000


def test_plan_outlives_its_store_handle(torch_cuda):
    """Shared ownership like the reference's Arc'ed snapshot: destroying the store handle while a plan is alive is fine."""
    rng = np.random.default_rng(1)
    g, s_, p, o = random_quads(rng, 5000, 200, graphs=1)
    gs, os_ = both_stores((g, s_, p, o))
    pb = PlanBuilder()
    desc = pb.build(pb.data_source(quad_pattern("s", int(p[0]), "o")))
    plan = gs.plan(desc)
    exp, n_exp, _ = os_.execute(desc)
    gs.close()                                                   # rdfgpu_store_destroy
    got = plan.execute().fetch()
    np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
    plan.close()


@pytest.mark.parametrize("option", ["NO_INDEX_JOIN", "NO_BAND_JOIN"])
def test_held_back_ordered_join_output_after_an_option_change(bsbm_stores, torch_cuda, option):
    """The ordered slice join of the batched Q5 holds its write pass back once the band join above it has taken its records
    (NodeInfo::band.takes_records, kept across executions).  An option set on the plan afterwards routes that join elsewhere:
    NO_INDEX_JOIN makes the held-back table the BUILD side of a hash table built in the step, NO_BAND_JOIN the probe side of an
    ordinary index join.  Either way the write pass has to run before the table is read: the bindings stay the oracle's."""
    ds, gs, os_ = bsbm_stores
    rng = np.random.default_rng(11)
    # more parameter rows than the productFeature slice has (the constants' first join builds on the slice, ordered), few of them
    # products: the constants table (~7.5 k rows) stays smaller than the slice, so under NO_INDEX_JOIN the candidate join builds on it
    n_rows, n_prod = 40_000, 400
    xs = ds.feature_base + rng.integers(0, ds.n_features, n_rows)                       # ids that are no product's
    xs[rng.choice(n_rows, n_prod, replace=False)] = [ds.product(int(i)) for i in rng.choice(ds.n_products, n_prod, replace=False)]
    params = [np.arange(1, n_rows + 1, dtype=np.uint32), xs.astype(np.uint32)]
    keep, ptrs = table_on_device(torch_cuda, params)
    desc = bsbm.q5_batch_plan(ds)
    exp, n_exp, _ = os_.execute(desc, [params])
    plan = gs.plan(desc).enable_kernel_timing(True)
    plan.bind_table(0, ptrs, n_rows)
    fused = False
    for _ in range(6):
        got = plan.execute().fetch()
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        fused = fused or any("oj_write_band_kernel" in k[0] for k in plan.kernel_stats())
    assert fused or ENGINE_TOGGLED
    plan.set_option(option, 1)
    got = plan.execute().fetch()
    np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
    names = {k[0] for k in plan.kernel_stats()}
    if not ENGINE_TOGGLED:
        assert plan.metrics().exact_reruns == 0 and any("oj_write_kernel" in k for k in names), sorted(names)   # the held-back pass ran on its own
        if option == "NO_INDEX_JOIN":
            assert any("gjoin_build_kernel" in k for k in names), sorted(names)


def test_tables_rebuilt_inside_a_fused_execution(torch_cuda):
    """rdfgpu_store_drop_tables (what any extend / remove does to the cached join tables): a plan with history keeps its fused
    form — the tables it needs are built inside the next execution, which still runs the ordered slice join + band join and
    still answers like the oracle; an extend / remove pair does the same through a real mutation."""
    ds = bsbm.generate(2000)
    gs, os_ = both_stores((ds.g, ds.s, ds.p, ds.o), typed=ds.typed_values, decimals=ds.decimals)
    rng = np.random.default_rng(77)
    desc = bsbm.q5_batch_plan(ds)
    plan = gs.plan(desc).enable_kernel_timing(True)
    def run(batch):
        prods = np.array([ds.product(i) for i in rng.choice(ds.n_products, batch, replace=False)], dtype=np.uint32)
        params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
        keep, ptrs = table_on_device(torch_cuda, params)
        plan.bind_table(0, ptrs, batch)
        got = plan.execute().fetch()
        exp, n_exp, _ = os_.execute(desc, [params])
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        return plan.metrics(), {k[0] for k in plan.kernel_stats()}
    run(1500); run(1400); run(1420); run(1460)
    m, ran = run(1450)
    if not ENGINE_TOGGLED:
        assert any("oj_write_band_kernel" in k for k in ran), sorted(ran)
    if not ENGINE_TOGGLED:
        assert m.tables_built == 0 and m.host_syncs == 1 and any("band_mask_kernel" in k for k in ran), (m.tables_built, m.host_syncs, sorted(ran))
    gs.drop_tables()
    m, ran = run(1480)
    if not ENGINE_TOGGLED:
        assert m.tables_built >= 4 and m.exact_reruns == 0, (m.tables_built, m.exact_reruns)
        assert any("band_mask_kernel" in k for k in ran) and any("band_entries_kernel" in k for k in ran), sorted(ran)
    m, ran = run(1500)
    if not ENGINE_TOGGLED:
        assert m.tables_built == 0 and m.host_syncs == 1
    # a real mutation: one foreign quad in and out again
    q = [np.array([0], np.uint32), np.array([ds.product(0)], np.uint32), np.array([ds.pred["rdfs:label"]], np.uint32), np.array([ds.product(1)], np.uint32)]
    assert gs.extend(*q) == os_.extend(*q) == 1
    run(1300)
    assert gs.remove(*q) == os_.remove(*q) == 1
    run(1350)


def test_topk_distinct_matches_oracle(torch_cuda):
    """DISTINCT + ORDER BY ... LIMIT k per group (the operators above the path) against the oracle,
    incl. empty input, a single group, many tiny groups, unbound sort values, duplicates."""
    rng = np.random.default_rng(12)
    strings = [f"label {i:04d}" for i in rng.permutation(500)]
    tv, _, _ = string_dictionary(strings, n_other=3)
    tv["tag"][-3:] = abi.TV_NAMED_NODE
    gs, os_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv)
    for n, n_groups, limit in ((0, 3, 5), (1, 1, 5), (7000, 50, 5), (60_000, 1, 6), (4000, 900, 2), (200_000, 3000, 5)):
        g = rng.integers(1, n_groups + 1, n).astype(np.uint32)
        lab = rng.integers(0, len(tv), n).astype(np.uint32)
        prod = rng.integers(1000, 1060, n).astype(np.uint32)
        tab = [g, lab, prod]
        keep, ptrs = table_on_device(torch_cuda, tab)
        for group, proj in ((0, None), (None, [1, 2]), (0, [2, 0, 1])):
            pb = PlanBuilder()
            desc = pb.build(pb.topk(pb.table(0, 3), keys=[(1, abi.SORT_BY_TERM), (2, abi.SORT_BY_ID)], limit=limit, group=group, projection=proj))
            run_both(gs, os_, desc, gpu_tables=[(ptrs, n)], cpu_tables=[tab], ordered=True)
        pb = PlanBuilder()                                                 # three keys (Q4's ORDER BY label, product, propertyTextual)
        four = [g, lab, prod % 7 + 1, prod]
        keep4, ptrs4 = table_on_device(torch_cuda, four)
        for group, proj in ((None, [1, 2, 3]), (0, None)):
            pb = PlanBuilder()
            run_both(gs, os_, pb.build(pb.topk(pb.table(0, 4), keys=[(1, abi.SORT_BY_TERM), (2, abi.SORT_BY_ID), (3, abi.SORT_BY_ID)], limit=limit + 10,
                                               group=group, projection=proj)), gpu_tables=[(ptrs4, n)], cpu_tables=[four], ordered=True)
        pb = PlanBuilder()                                                 # one key, by id
        run_both(gs, os_, pb.build(pb.topk(pb.table(0, 3), keys=[(2, abi.SORT_BY_ID)], limit=limit, group=0, projection=[0, 2])),
                 gpu_tables=[(ptrs, n)], cpu_tables=[tab], ordered=True)
    # ORDER BY a numeric value (ENC_SORT of a numeric = Double::from(Numeric), total order; Q10's xsd:double(str(?price)))
    import test_oracle_pyarrow as tp
    tvn, decn, _ = tp.numeric_table(np.random.default_rng(6), 400)
    gn, on_ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tvn, decimals=decn)
    for n, limit, n_groups in ((0, 5, 1), (5000, 40, 1), (60_000, 7, 500)):
        tab = [rng.integers(1, n_groups + 1, n).astype(np.uint32), rng.integers(1, 50, n).astype(np.uint32), rng.integers(0, 402, n).astype(np.uint32)]
        keep, ptrs = table_on_device(torch_cuda, tab)
        for group in (None, 0):
            pb = PlanBuilder()
            run_both(gn, on_, pb.build(pb.topk(pb.table(0, 3), keys=[(2, abi.SORT_BY_DOUBLE), (1, abi.SORT_BY_ID), (2, abi.SORT_BY_ID)], limit=limit, group=group,
                                               projection=[1, 2] if group is None else None)), gpu_tables=[(ptrs, n)], cpu_tables=[tab], ordered=True)
    # a numeric column cannot be ordered as a term here: refused loudly
    tv2 = tv.copy(); tv2["tag"][5] = abi.TV_INTEGER
    gs2, _ = both_stores((np.zeros(0, np.uint32),) * 4, typed=tv2)
    tab = [np.ones(10, np.uint32), np.full(10, 5, np.uint32), np.arange(10, dtype=np.uint32) + 1]
    keep, ptrs = table_on_device(torch_cuda, tab)
    pb = PlanBuilder()
    plan = gs2.plan(pb.build(pb.topk(pb.table(0, 3), keys=[(1, abi.SORT_BY_TERM), (2, abi.SORT_BY_ID)], limit=3, group=0)))
    plan.bind_table(0, ptrs, 10)
    with pytest.raises(rf.RdfGpuError):
        plan.execute()
    pb = PlanBuilder()
    with pytest.raises(rf.RdfGpuError):          # an output column outside (group, keys) would make DISTINCT ambiguous
        gs.plan(pb.build(pb.topk(pb.table(0, 3), keys=[(1, abi.SORT_BY_TERM)], limit=3, group=0, tie_break=False)))


def test_bsbm_q5_whole_query_on_device(bsbm_stores, torch_cuda):
    """Q5 including DISTINCT + ORDER BY ?productLabel LIMIT 5: per query and as a batch grouped by instance."""
    ds, gs, os_ = bsbm_stores
    rng = np.random.default_rng(21)
    for x in rng.choice(ds.n_products, 4, replace=False):
        plan, got = run_both(gs, os_, bsbm.q5_plan(ds, ds.product(int(x)), topk=True), ordered=True)
        assert plan.result_info()[0] <= 5
    desc = bsbm.q5_batch_plan(ds, topk=True)
    plan = gs.plan(desc)
    for batch in (1, 90, 300):
        prods = np.array([ds.product(i) for i in rng.choice(ds.n_products, batch, replace=False)], dtype=np.uint32)
        params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
        keep, ptrs = table_on_device(torch_cuda, params)
        plan.bind_table(0, ptrs, batch)
        got = plan.execute().fetch()
        exp, n_exp, _ = os_.execute(desc, [params])
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        ku.assert_same_sequence(got, exp, n_exp, f"batch of {batch}")      # instances ascending, each one's rows in ORDER BY order
        assert len(got[0]) <= 5 * batch
        # per instance the batch's rows are exactly the single-query plan's rows
        for i in (0, batch - 1):
            c, m, _ = os_.execute(bsbm.q5_plan(ds, int(prods[i]), topk=True))
            sel = got[0] == i + 1
            np.testing.assert_array_equal(ku.multiset([got[1][sel], got[2][sel]]), ku.multiset(c, m))


def test_bsbm_10m_scale_configs(torch_cuda):
    """BASELINE config 2 (BSBM scale-10M, Q1 single-pattern scan + FILTER) and the Q5 / batched-Q5 plans at that scale:
    the scan + FILTER against numpy (a size-independent property: the survivors are exactly the products whose value
    exceeds the threshold), the plans against the oracle (which adopts the device-built permutations)."""
    ds = bsbm.generate(28_500)                                   # ~10 M triples
    gs = rf.GpuQuadStore()
    gs.extend(ds.g, ds.s, ds.p, ds.o)
    gs.set_typed_values(ds.typed_values, ds.decimals)
    assert len(gs) > 9_000_000
    os_ = orc.OracleStore()
    for comp in (abi.GSPO, abi.GPOS, abi.GOSP):
        os_.adopt_sorted(comp, gs.read_index(comp))
    os_.set_typed_values(ds.typed_values, ds.decimals)
    num1 = ds.p == ds.pred["bsbm:productPropertyNumeric1"]
    values = ds.o[num1].astype(np.int64) - ds.int_base + 1
    for thr in (1, 400, 1000, 1999):
        plan = gs.plan(bsbm.q1_scan_filter_plan(ds, thr)).execute()
        got = np.sort(plan.fetch()[0])
        np.testing.assert_array_equal(got, np.sort(ds.s[num1][values > thr]))
    rng = np.random.default_rng(10)
    for x in rng.choice(ds.n_products, 3, replace=False):
        run_both(gs, os_, bsbm.q5_plan(ds, ds.product(int(x))))
    run_both(gs, os_, bsbm.q1_plan(ds, *bsbm.q1_instance(ds, rng)))
    batch = 64
    prods = np.array([ds.product(i) for i in rng.choice(ds.n_products, batch, replace=False)], dtype=np.uint32)
    params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
    keep, ptrs = table_on_device(torch_cuda, params)
    desc = bsbm.q5_batch_plan(ds, topk=True)
    plan = gs.plan(desc)
    plan.bind_table(0, ptrs, batch)
    for _ in range(2):                                           # second run: speculative, fused
        got = plan.execute().fetch()
        exp, n_exp, _ = os_.execute(desc, [params])
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        ku.assert_same_sequence(got, exp, n_exp)


def test_bsbm_100m_timed_path_answers_to_the_oracle(torch_cuda):
    """BASELINE config 3 at its size (285 000 products, ~98 M triples): a 40 000-instance Q5 batch through ONE compiled plan,
    three executions — exact first run (primed), then the speculative fused path bench.py times (ordered slice join + band
    join, one host sync).  After every execution the bindings of 12 instance tags spread over the batch are multiset-equal to
    the oracle's per-query plans, the count is stable, and the last execution did run the band join."""
    ds = bsbm.generate(285_000)
    gs = rf.GpuQuadStore()
    gs.extend(ds.g, ds.s, ds.p, ds.o)
    gs.set_typed_values(ds.typed_values, ds.decimals)
    assert len(gs) > 95_000_000
    os_ = orc.OracleStore()
    for comp in (abi.GSPO, abi.GPOS, abi.GOSP):
        os_.adopt_sorted(comp, gs.read_index(comp))
    os_.set_typed_values(ds.typed_values, ds.decimals)
    rng = np.random.default_rng(100)
    batch = 40_000
    prods = np.array([ds.product(i) for i in rng.choice(ds.n_products, batch, replace=False)], dtype=np.uint32)
    params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
    keep, ptrs = table_on_device(torch_cuda, params)
    tags = sorted({1, 2, 3, batch // 3, batch // 2, batch - 2, batch - 1, batch} | set(int(t) for t in rng.integers(1, batch + 1, 4)))
    expected = []
    for t in tags:
        cols, n, _ = os_.execute(bsbm.q5_plan(ds, int(prods[t - 1])))
        expected.append(np.stack([np.full(n, t, np.uint32), cols[0][:n], cols[1][:n]], axis=1))
    expected = ku.multiset(list(np.concatenate(expected).T))
    plan = gs.plan(bsbm.q5_batch_plan(ds)).enable_kernel_timing(True)
    plan.bind_table(0, ptrs, batch)
    counts, forms = [], []
    for run in range(6):      # 1: exact (primed); 2, 3: speculative, fused (ordered slice join -> table C -> band join); from 4 on the ordered
        got = plan.execute().fetch()      # join writes the band join's row records itself (no table C, no decode pass)
        counts.append(len(got[0]))
        sel = np.isin(got[0], tags)
        np.testing.assert_array_equal(ku.multiset([c[sel] for c in got]), expected)
        ran = {k[0] for k in plan.kernel_stats()}
        forms.append("records" if any("oj_write_band_kernel" in k for k in ran) else "table" if any("band_decode_kernel" in k for k in ran) else "unfused")
    assert len(set(counts)) == 1 and counts[0] > 100 * batch // 2
    if not ENGINE_TOGGLED:
        assert any("band_mask_kernel" in k for k in ran), sorted(ran)
        assert "table" in forms and forms[-1] == "records", forms
        assert plan.metrics().host_syncs == 1
    # the 16-byte row records of the last runs (packed windows, one row output column, no full-semantics pass) against the 32-byte form
    plan.set_option("NO_BAND_COMPACT", 1)
    got32 = plan.execute().fetch()
    sel = np.isin(got32[0], tags)
    assert len(got32[0]) == counts[0]
    np.testing.assert_array_equal(ku.multiset([c[sel] for c in got32]), expected)
    np.testing.assert_array_equal(ku.multiset(got32), ku.multiset(got))      # the whole result, not only the sampled tags


def test_fused_chain_with_mixed_numeric_kinds(torch_cuda):
    """The fused window stages decide all-xsd:integer candidates on a fast path (decoded value tables, checked i64
    arithmetic); anything else must fall back to the full promotion rules: some numeric literals become doubles and
    decimals here, on the slice side and on the instance side."""
    import struct
    ds = bsbm.generate(1500)
    tv = ds.typed_values.copy()
    dec = []
    for v in range(1, 2001, 7):            # every 7th integer literal "v" becomes the double v + 0.5
        tv["tag"][ds.int_base + v - 1] = abi.TV_DOUBLE
        tv["lo"][ds.int_base + v - 1] = struct.unpack("<q", struct.pack("<d", v + 0.5))[0]
    for k, v in enumerate(range(3, 2001, 11)):   # every 11th: the decimal v.25
        tv["tag"][ds.int_base + v - 1] = abi.TV_DECIMAL
        tv["lo"][ds.int_base + v - 1] = k
        raw = v * 10 ** 18 + 25 * 10 ** 16
        dec += [raw & ((1 << 64) - 1), raw >> 64]
    dec = np.array(dec, dtype=np.uint64).astype(np.int64)
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    assert gs.extend(ds.g, ds.s, ds.p, ds.o) == os_.extend(ds.g, ds.s, ds.p, ds.o)
    gs.set_typed_values(tv, dec)
    os_.set_typed_values(tv, dec)
    rng = np.random.default_rng(31)
    desc = bsbm.q5_batch_plan(ds)
    plan = gs.plan(desc)
    for it in range(3):
        batch = 200
        prods = np.array([ds.product(i) for i in rng.choice(ds.n_products, batch, replace=False)], dtype=np.uint32)
        params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
        keep, ptrs = table_on_device(torch_cuda, params)
        plan.bind_table(0, ptrs, batch)
        plan.enable_kernel_timing(True)
        got = plan.execute().fetch()
        exp, n_exp, _ = os_.execute(desc, [params])
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
    assert any("lds_join_kernel" in k[0] and k[0].rstrip(">").endswith("true") for k in plan.kernel_stats()) or ENGINE_TOGGLED
    for x in prods[:3]:
        run_both(gs, os_, bsbm.q5_plan(ds, int(x)))


def _band_store(rng, n_prod, n_feat, fan, missing=0.1):
    """(product, pF, feature) with `fan` features per product, (product, pV1 / pV2, integer literal), (product, pL, label);
    ids: predicates 1..4, features, products, integer literals -500 .. 2499 (3000), a zoo of other kinds, labels."""
    pF, pV1, pV2, pL = 1, 2, 3, 4
    feat0 = 10
    prod0 = feat0 + n_feat
    int0 = prod0 + n_prod
    n_int = 3000
    zoo0 = int0 + n_int
    zoo = [(abi.TV_DOUBLE, np.float64(700.5).view(np.int64)), (abi.TV_DOUBLE, np.float64("nan").view(np.int64)), (abi.TV_INTEGER, 2 ** 63 - 1),
           (abi.TV_INTEGER, -2 ** 63), (abi.TV_INTEGER, 2 ** 63 - 100), (abi.TV_NAMED_NODE, 5), (abi.TV_INT, 900), (abi.TV_FLOAT, int(np.array([1200.0], np.float32).view(np.uint32)[0])),
           (abi.TV_STRING, 3), (abi.TV_BOOLEAN, 1)]
    lab0 = zoo0 + len(zoo)
    n_ids = lab0 + n_prod
    tv = np.zeros(n_ids, dtype=TV_DTYPE)
    tv["tag"][1:] = abi.TV_NAMED_NODE
    tv["lo"][1:] = np.arange(1, n_ids)
    tv["tag"][int0:int0 + n_int] = abi.TV_INTEGER
    tv["lo"][int0:int0 + n_int] = np.arange(n_int) - 500
    for i, (tag, lo) in enumerate(zoo):
        tv["tag"][zoo0 + i] = tag; tv["lo"][zoo0 + i] = lo
    tv["tag"][lab0:] = abi.TV_STRING
    tv["lo"][lab0:] = np.arange(n_prod)
    prod = np.arange(prod0, prod0 + n_prod, dtype=np.uint32)
    S, Pc, O = [], [], []
    def emit(s, p, o):
        S.append(np.asarray(s, np.uint32)); Pc.append(np.full(len(s), p, np.uint32)); O.append(np.asarray(o, np.uint32))
    f = rng.integers(fan[0], fan[1] + 1, n_prod)
    # skewed features: a few hot ones (groups of a few hundred rows = several 64-entry chunks) and a long tail, some never used
    feat = feat0 + np.minimum((rng.random(int(f.sum())) ** 1.3 * n_feat).astype(np.int64), n_feat - 1)
    emit(np.repeat(prod, f), pF, feat)
    for pv in (pV1, pV2):
        keep = rng.random(n_prod) >= missing                       # products without the value: no stage row
        emit(prod[keep], pv, int0 + rng.integers(0, n_int, int(keep.sum())))
    keep = rng.random(n_prod) >= missing / 2
    emit(prod[keep], pL, lab0 + np.arange(n_prod)[keep])
    s, p, o = np.concatenate(S), np.concatenate(Pc), np.concatenate(O)
    ids = dict(pF=pF, pV1=pV1, pV2=pV2, pL=pL, feat0=feat0, n_feat=n_feat, prod0=prod0, n_prod=n_prod, int0=int0, n_int=n_int, zoo0=zoo0, n_zoo=len(zoo))
    return (np.zeros(len(s), np.uint32), s, p, o), tv, ids


@pytest.mark.parametrize("shape", ["two_windows_neq", "one_window", "lookups_only", "leq_geq_eq"])
def test_band_join_matches_oracle(torch_cuda, shape):
    """The key-partitioned band join (band_join.hip) = the fused look-up chain, group by group: bound table T(inst, X, f,
    y1, y2) JOIN (product pF f) ON f [product != X] JOIN (product pV1 v1) ON product [window(v1; y1)] JOIN pV2 [window(v2; y2)]
    JOIN (product pL label), against the oracle's operator-at-a-time answer.  Groups of 1 .. ~350 entries (up to six
    64-entry chunks), keys without probe rows, probe rows without a group, null keys and null operands, products
    without a stage row, windows that are empty / overflow i64 / have operands of other kinds (the full-semantics
    path), and the same plan with the band join switched off."""
    rng = np.random.default_rng(5)
    quads, tv, ids = _band_store(rng, n_prod=6000, n_feat=220, fan=(1, 6))
    gs, os_ = both_stores(quads, typed=tv)
    n = 9000
    inst = np.arange(1, n + 1, dtype=np.uint32)
    X = (ids["prod0"] + rng.integers(0, ids["n_prod"], n)).astype(np.uint32)
    X[rng.random(n) < 0.02] = 0                                     # unbound: `product != X` is not true
    f = (ids["feat0"] + rng.integers(-3, ids["n_feat"] + 3, n)).astype(np.uint32)   # some ids that are no feature at all
    f[rng.random(n) < 0.02] = 0                                     # null key: never joins
    def operand():
        y = (ids["int0"] + rng.integers(0, ids["n_int"], n)).astype(np.uint32)
        odd = rng.random(n) < 0.06                                  # other kinds, i64 edges, NaN: the full semantics decide
        y[odd] = (ids["zoo0"] + rng.integers(0, ids["n_zoo"], int(odd.sum()))).astype(np.uint32)
        y[rng.random(n) < 0.01] = 0
        return y
    T = [inst, X, f, operand(), operand()]
    keep, ptrs = table_on_device(torch_cuda, T)
    pb = PlanBuilder()
    t = pb.table(0, 5)
    scan = lambda p, v: pb.data_source(quad_pattern("product", ids[p], v))
    win = lambda x, y, w, lo_op=GT, hi_op=LT: AND(EBV(hi_op(ENC_TV(col(x)), ADD(ENC_TV(col(y)), integer(w)))), EBV(lo_op(ENC_TV(col(x)), SUB(ENC_TV(col(y)), integer(w)))))
    if shape == "lookups_only":
        node = pb.hash_join(t, scan("pF", "f"), on=[(2, 1)], projection=[0, 5, 3, 4])                       # (inst, product, y1, y2)
        node = pb.hash_join(node, scan("pV1", "v1"), on=[(1, 0)], projection=[0, 1, 5])                    # + v1
        node = pb.hash_join(node, scan("pL", "label"), on=[(1, 0)], projection=[0, 1, 2, 4])
    else:
        node = pb.hash_join(t, scan("pF", "f"), on=[(2, 1)], filter=ID_NEQ(col(5), col(1)) if shape == "two_windows_neq" else None, projection=[0, 5, 3, 4])
        if shape == "leq_geq_eq":
            node = pb.hash_join(node, scan("pV1", "v1"), on=[(1, 0)], filter=win(5, 2, 300, GEQ, LEQ), projection=[0, 1, 2, 3])
            # an `=` half is no interval: this stage keeps the chain off the band path (and must still be right)
            node = pb.hash_join(node, scan("pV2", "v2"), on=[(1, 0)], filter=AND(EBV(EQ(ENC_TV(col(5)), ADD(ENC_TV(col(3)), integer(0)))), EBV(GT(ENC_TV(col(5)), SUB(ENC_TV(col(3)), integer(9))))), projection=[0, 1, 5])
        else:
            node = pb.hash_join(node, scan("pV1", "v1"), on=[(1, 0)], filter=win(5, 2, 400), projection=[0, 1, 2, 3])
            if shape == "two_windows_neq":
                node = pb.hash_join(node, scan("pV2", "v2"), on=[(1, 0)], filter=win(5, 3, 900), projection=[0, 1, 2, 3])
            node = pb.hash_join(node, scan("pL", "label"), on=[(1, 0)], projection=[0, 1, 5])
    desc = pb.build(node)
    exp, n_exp, _ = os_.execute(desc, [T])
    assert n_exp > (10 if shape == "leq_geq_eq" else 1000)
    want = ku.multiset(exp, n_exp)
    plan = gs.plan(desc)
    plan.bind_table(0, ptrs, n)
    seen = set()
    for rep in range(4):                                            # fusion needs the cardinalities of a first execution
        plan.enable_kernel_timing(True)
        got = plan.execute().fetch()
        assert plan.result_info()[0] == n_exp
        np.testing.assert_array_equal(ku.multiset(got, n_exp), want, err_msg=f"{shape} rep {rep}")
        seen |= {k[0] for k in plan.kernel_stats()}
    if shape != "leq_geq_eq" and not ENGINE_TOGGLED:
        assert any("band_mask_kernel" in k for k in seen) and any("band_emit_kernel" in k for k in seen), seen
    # timing mode 2: only the launches of the kernel that took longest in the last fully timed execution are bracketed
    full = {k[0]: k[2] for k in plan.kernel_stats()}
    plan.enable_kernel_timing(2)
    got = plan.execute().fetch()
    np.testing.assert_array_equal(ku.multiset(got, n_exp), want)
    focus = [k[0] for k in plan.kernel_stats()]
    assert focus == [max(full, key=full.get)], (focus, full)
    plan.enable_kernel_timing(True)
    plan.set_option("NO_BAND_PACK16", 1)                            # both windows with 32-bit arithmetic instead of packed 16-bit
    got = plan.execute().fetch()
    np.testing.assert_array_equal(ku.multiset(got, n_exp), want)
    plan.set_option("NO_BAND_PACK16", 0)
    plan.set_option("NO_BAND_JOIN", 1)
    got = plan.execute().fetch()
    assert not any("band_" in k[0] for k in plan.kernel_stats())
    np.testing.assert_array_equal(ku.multiset(got, n_exp), want)
    plan.set_option("NO_BAND_JOIN", 0)
    # the parameters change (fewer rows, other keys), the plan stays: sizes are speculative, results exact
    m = 2500
    T2 = [c[:m].copy() for c in T]
    T2[2] = (ids["feat0"] + rng.integers(0, 12, m)).astype(np.uint32)   # every row on a hot feature: many rows per key
    keep2, ptrs2 = table_on_device(torch_cuda, T2)
    plan.bind_table(0, ptrs2, m)
    exp2, n2, _ = os_.execute(desc, [T2])
    for rep in range(2):
        got = plan.execute().fetch()
        assert plan.result_info()[0] == n2
        np.testing.assert_array_equal(ku.multiset(got, n2), ku.multiset(exp2, n2))
    # operands that are all xsd:integer: the full-semantics pass is not launched any more — then rows that need it come
    # back: the execution notices (its decode pass counts them) and answers them exactly all the same
    T3 = [c.copy() for c in T]
    for k in (3, 4):
        T3[k] = (ids["int0"] + rng.integers(0, ids["n_int"], n)).astype(np.uint32)
    keep3, ptrs3 = table_on_device(torch_cuda, T3)
    exp3, n3, _ = os_.execute(desc, [T3])
    plan.bind_table(0, ptrs3, n)
    for rep in range(3):
        got = plan.execute().fetch()
        np.testing.assert_array_equal(ku.multiset(got, n3), ku.multiset(exp3, n3))
    plan.bind_table(0, ptrs, n)
    for rep in range(2):
        got = plan.execute().fetch()
        assert plan.result_info()[0] == n_exp
        np.testing.assert_array_equal(ku.multiset(got, n_exp), want)
    del keep, keep2, keep3


def test_band_join_piecewise_sorted_probe(torch_cuda):
    """A probe side of more than 2^21 rows that arrives as a few runs sorted by the join key (what a hash repartition of
    sorted shards delivers): after one execution has seen the runs, the partition pass is the counting sort with one
    atomic per run of equal neighbouring keys instead of the radix sort.  Same multiset either way and as the oracle's;
    then the same plan over the rows in random order (no runs: back to the radix sort)."""
    rng = np.random.default_rng(77)
    quads, tv, ids = _band_store(rng, n_prod=6000, n_feat=3000, fan=(1, 4))
    gs, os_ = both_stores(quads, typed=tv)
    n = (1 << 21) + 300_001
    runs = []
    for r in range(4):                                                # four sorted runs of unequal length, null keys and strangers inside
        m = n // 4 + (r - 1) * 1000 if r < 3 else n - sum(len(x) for x in runs)
        f = (ids["feat0"] + rng.integers(-2, ids["n_feat"] + 2, m)).astype(np.uint32)
        f[rng.random(m) < 0.01] = 0
        runs.append(np.sort(f))
    f = np.concatenate(runs)
    inst = np.arange(1, n + 1, dtype=np.uint32)
    X = (ids["prod0"] + rng.integers(0, ids["n_prod"], n)).astype(np.uint32)
    y = lambda: (ids["int0"] + rng.integers(0, ids["n_int"], n)).astype(np.uint32)
    T = [inst, X, f, y(), y()]
    pb = PlanBuilder()
    t = pb.table(0, 5)
    scan = lambda p, v: pb.data_source(quad_pattern("product", ids[p], v))
    win = lambda x, yy, w: AND(EBV(LT(ENC_TV(col(x)), ADD(ENC_TV(col(yy)), integer(w)))), EBV(GT(ENC_TV(col(x)), SUB(ENC_TV(col(yy)), integer(w)))))
    node = pb.hash_join(t, scan("pF", "f"), on=[(2, 1)], filter=ID_NEQ(col(5), col(1)), projection=[0, 5, 3, 4])
    node = pb.hash_join(node, scan("pV1", "v1"), on=[(1, 0)], filter=win(5, 2, 400), projection=[0, 1, 2, 3])
    node = pb.hash_join(node, scan("pV2", "v2"), on=[(1, 0)], filter=win(5, 3, 900), projection=[0, 1, 2, 3])
    node = pb.hash_join(node, scan("pL", "label"), on=[(1, 0)], projection=[0, 1, 5])
    desc = pb.build(node)
    plan = gs.plan(desc)
    for order in ("runs", "random"):
        if order == "random":
            perm = rng.permutation(n)
            T = [c[perm] for c in T]
        keep, ptrs = table_on_device(torch_cuda, T)
        exp, n_exp, _ = os_.execute(desc, [T])
        assert n_exp > 10_000
        want = ku.multiset(exp, n_exp)
        plan.bind_table(0, ptrs, n)
        for rep in range(3):
            plan.enable_kernel_timing(True)
            got = plan.execute().fetch()
            assert plan.result_info()[0] == n_exp
            np.testing.assert_array_equal(ku.multiset(got, n_exp), want, err_msg=f"{order} rep {rep}")
        names = {k[0] for k in plan.kernel_stats()}
        if not ENGINE_TOGGLED:
            assert any("band_mask_kernel" in k for k in names), names
            assert ("rocprim radix sort" in names) == (order == "random"), (order, names)
        del keep


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("n,n_nodes,n_graphs", [(0, 5, 1), (1, 1, 1), (3, 3, 1), (300, 40, 2), (2000, 900, 4), (60_000, 120_000, 3), (5000, 5000, 700)])
def test_closure_matches_oracle(torch_cuda, cross, n, n_nodes, n_graphs):
    """KleenePlusClosureExec (physical.rs:246-384) as sorted-key semi-naive iteration on the device vs the oracle's set
    restatement: random multi-graph inputs incl. the default graph, duplicates and self loops; within and across graphs;
    behind a FilterExec (device-side row count) and under a join."""
    import test_closure_cpu as tc
    rng = np.random.default_rng(n * 31 + n_graphs + cross)
    g, s, e = tc.random_paths(rng, n, n_nodes, n_graphs)
    keep, ptrs = table_on_device(torch_cuda, [g, s, e])
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    plan, got = run_both(gs, os_, tc.closure_plan(cross), gpu_tables=[(ptrs, n)], cpu_tables=[[g, s, e]])
    rows = list(zip(*(c.tolist() for c in got)))
    assert len(rows) == len(set(rows))
    if n <= 300:
        assert set(rows) == tc.numpy_closure(g, s, e, cross)
    pb = PlanBuilder()
    inner = pb.filter(pb.table(0, 3), ID_NEQ(col(1), lit_id(9)))            # the row count of the inner paths lives on the device
    reach = pb.closure(inner, allow_cross_graph_paths=cross)
    run_both(gs, os_, pb.build(pb.hash_join(reach, pb.table(0, 3), on=[(2, 1)], projection=[0, 1, 5]) if n <= 5000 else reach),
             gpu_tables=[(ptrs, n)], cpu_tables=[[g, s, e]])


def test_closure_chain_cycle_fixture_and_null(torch_cuda):
    import test_closure_cpu as tc
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    chain = np.arange(1, 401, dtype=np.uint32)
    t = [np.zeros(399, np.uint32), chain[:-1], chain[1:]]                    # 399 iterations
    keep, ptrs = table_on_device(torch_cuda, t)
    plan, got = run_both(gs, os_, tc.closure_plan(), gpu_tables=[(ptrs, 399)], cpu_tables=[t])
    assert plan.result_info()[0] == 399 * 400 // 2
    ring = np.arange(1, 301, dtype=np.uint32)
    t = [np.full(300, 5, np.uint32), ring, np.roll(ring, -1)]
    keep, ptrs = table_on_device(torch_cuda, t)
    plan, got = run_both(gs, os_, tc.closure_plan(), gpu_tables=[(ptrs, 300)], cpu_tables=[t])
    assert plan.result_info()[0] == 300 * 300
    # the reference's fixture one_or_more_shared.{ttl,rq,srx}: ?s ex:p+ ?s  =>  ex:s, ex:m
    t = [np.zeros(3, np.uint32), np.array([11, 12, 12], np.uint32), np.array([12, 11, 13], np.uint32)]
    keep, ptrs = table_on_device(torch_cuda, t)
    plan, got = run_both(gs, os_, tc.closure_plan(same_ends=True), gpu_tables=[(ptrs, 3)], cpu_tables=[t])
    assert sorted(got[0].tolist()) == [11, 12]
    t = [np.zeros(2, np.uint32), np.array([1, 0], np.uint32), np.array([2, 3], np.uint32)]
    keep, ptrs = table_on_device(torch_cuda, t)
    p = gs.plan(tc.closure_plan())
    p.bind_table(0, ptrs, 2)
    with pytest.raises(rf.RdfGpuError, match="start / end"):
        p.execute()


@pytest.mark.parametrize("nl,nr", [(0, 0), (0, 900), (1300, 0), (1, 1), (70_000, 130_001)])
def test_union_matches_oracle(torch_cuda, nl, nr):
    """UnionExec (Q4 / Q11 (Execution Plan).snap): bag union; inputs with host-known and with device-side row counts
    (a FilterExec below), empty sides, a projection, a join above the union."""
    rng = np.random.default_rng(nl + 3 * nr)
    L = [rng.integers(0, 60, nl).astype(np.uint32) for _ in range(3)]
    R = [rng.integers(0, 60, nr).astype(np.uint32) for _ in range(3)]
    kl, pl = table_on_device(torch_cuda, L)
    kr, pr = table_on_device(torch_cuda, R)
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    tabs = dict(gpu_tables=[(pl, nl), (pr, nr)], cpu_tables=[L, R])
    pb = PlanBuilder()
    plan, got = run_both(gs, os_, pb.build(pb.union(pb.table(0, 3), pb.table(1, 3))), **tabs)
    np.testing.assert_array_equal(got[1], np.concatenate([L[1], R[1]]))            # left rows first, order kept
    pb = PlanBuilder()
    f = lambda t: pb.filter(t, ID_NEQ(col(0), lit_id(7)))
    run_both(gs, os_, pb.build(pb.union(f(pb.table(0, 3)), pb.table(1, 3), projection=[2, 0])), **tabs)
    pb = PlanBuilder()
    run_both(gs, os_, pb.build(pb.union(pb.table(0, 3), f(pb.table(1, 3)))), **tabs)
    pb = PlanBuilder()
    u = pb.union(f(pb.table(0, 3)), f(pb.table(1, 3)), projection=[0, 1])
    run_both(gs, os_, pb.build(pb.hash_join(u, pb.union(pb.table(1, 3), pb.table(0, 3), projection=[1, 2]), on=[(1, 0)], projection=[0, 3])
                               if nl + nr < 10_000 else u), **tabs)


def test_bsbm_q4_matches_oracle(bsbm_stores):
    """BSBM Explore Q4 (Q4 (Execution Plan).snap:11-38): UnionExec of two five-join pipelines with integer FilterExecs."""
    ds, gs, os_ = bsbm_stores
    rng = np.random.default_rng(4)
    feats = ds.o[ds.p == ds.pred["bsbm:productFeature"]]
    common = np.bincount(feats - ds.feature_base).argsort()[::-1][:6] + ds.feature_base
    total = 0
    for it in range(10):
        f1, f2, f3 = (int(x) for x in rng.choice(common, 3, replace=False))
        plan, got = run_both(gs, os_, bsbm.q4_plan(ds, ds.type_base + ds.n_types - 1, f1, f2, f3, int(rng.integers(100, 900)), int(rng.integers(100, 900))))
        total += plan.result_info()[0]
    assert total > 5
    # the whole query: + DISTINCT + ORDER BY label, product, propertyTextual + TopK(fetch = 15) (Q4 (Execution Plan).snap:7-8;
    # the OFFSET 5 above it, GlobalLimitExec, drops rows of a 15-row table on the host)
    plan, got = run_both(gs, os_, bsbm.q4_plan(ds, ds.type_base + ds.n_types - 1, f1, f2, f3, 200, 300, topk=True), ordered=True)
    assert 0 < plan.result_info()[0] <= 15


def test_lang_matches_filter_matches_oracle(torch_cuda):
    """BSBM explore Q8's FILTER `EBV(LANGMATCHES(LANG(ENC_TV(text)), "EN"))` (Q8 (Execution Plan).snap:18): language-tagged
    and plain literals, IRIs / blank nodes / unbound (errors), a language id outside the host's table; as a FilterExec,
    negated, and as a join filter."""
    import test_lang_cpu as tl
    from rdf_fusion_amd.plan import LANGMATCHES_LANG, NOT
    tv = tl.lang_table()
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    gs.set_typed_values(tv)
    os_.set_typed_values(tv)
    rng = np.random.default_rng(3)
    n = 30_000
    ids = rng.integers(0, 15, n).astype(np.uint32)
    row = np.arange(n, dtype=np.uint32)
    keep, ptrs = table_on_device(torch_cuda, [ids, row])
    for lang_range in ("EN", "*", "de", "zh-hant", ""):
        e = EBV(LANGMATCHES_LANG(ENC_TV(col(0)), lang_range, tl.LANGUAGES))
        for expr in (e, NOT(e)):
            pb = PlanBuilder()
            plan, got = run_both(gs, os_, pb.build(pb.filter(pb.table(0, 2), expr, projection=[1])), gpu_tables=[(ptrs, n)], cpu_tables=[[ids, row]])
            assert sorted(got[0].tolist()) == tl.expected_rows(ids.tolist(), lang_range, expr is not e)
    k = rng.integers(1, 200, 3000).astype(np.uint32)
    R = [k, ids[:3000]]
    L = [rng.integers(1, 200, 2000).astype(np.uint32), row[:2000]]
    kl, pl = table_on_device(torch_cuda, L)
    kr, pr = table_on_device(torch_cuda, R)
    pb = PlanBuilder()
    desc = pb.build(pb.hash_join(pb.table(0, 2), pb.table(1, 2), on=[(0, 0)], filter=EBV(LANGMATCHES_LANG(ENC_TV(col(3)), "en", tl.LANGUAGES))))
    plan, got = run_both(gs, os_, desc, gpu_tables=[(pl, 2000), (pr, 3000)], cpu_tables=[L, R])
    assert plan.result_info()[0] > 1000


def test_bsbm_q10_matches_oracle(bsbm_stores):
    """BSBM Explore Q10 (Q10 (Execution Plan).snap:12-27): a two-key hash join, an integer FilterExec and a dateTime
    FilterExec (some validTo values carry a timezone, the literal does not: the +-14 h rule decides)."""
    ds, gs, os_ = bsbm_stores
    total = 0
    for i in range(30):
        plan, got = run_both(gs, os_, bsbm.q10_plan(ds, ds.product(i * 7), ds.country_base + i % ds.n_countries, max_days=9, after="2004-03-01T06:00:00"))
        total += plan.result_info()[0]
    plan, got = run_both(gs, os_, bsbm.q10_plan(ds, ds.product(1), ds.country_base))      # the query's own constants
    # the whole query: + DISTINCT + ORDER BY xsd:double(str(?price)), ?offer, ?price LIMIT 10 (Q10 (Execution Plan).snap:6-8)
    for i in range(6):
        plan, got = run_both(gs, os_, bsbm.q10_plan(ds, ds.product(i * 7), ds.country_base + i % ds.n_countries, max_days=21, after="2001-03-01T06:00:00", topk=True), ordered=True)
        assert plan.result_info()[0] <= 10
    assert total > 10


def test_timestamp_comparisons_match_oracle(torch_cuda):
    """xsd:dateTime / date / time FILTERs (BSBM explore Q7 / Q8 / Q10 compare dates): the Timestamp order of
    date_time.rs:1617-1654 incl. the +-14 h rule for a missing timezone, i128 edges, other kinds and nulls — per-row VM,
    the `col cmp literal` kernel and a join filter, all against the oracle (itself pinned by the reference's own
    equals / cmp known answers in tests/test_timestamp_cpu.py)."""
    import test_timestamp_cpu as tc
    from rdf_fusion_amd import xsd
    from rdf_fusion_amd.plan import date_time, date, time as time_lit, GEQ, LEQ, EQ, NEQ
    rng = np.random.default_rng(77)
    values = tc.random_timestamps(rng, 600)
    tv, dec = tc.timestamp_table(values)
    tv = np.concatenate([tv, np.zeros(2, dtype=TV_DTYPE)])
    tv["tag"][-2], tv["lo"][-2] = abi.TV_INTEGER, 5
    tv["tag"][-1], tv["lo"][-1] = abi.TV_DECIMAL, 3            # a decimal shares the i128 side table
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    gs.set_typed_values(tv, dec)
    os_.set_typed_values(tv, dec)
    n = 50_000
    a = rng.integers(0, len(tv) + 2, n).astype(np.uint32)      # incl. null (0) and ids beyond the table
    b = rng.integers(0, len(tv), n).astype(np.uint32)
    tag = np.arange(n, dtype=np.uint32)
    keep, ptrs = table_on_device(torch_cuda, [a, b, tag])
    total = 0
    for op in (GT, LT, GEQ, LEQ, EQ, NEQ):
        pb = PlanBuilder()
        desc = pb.build(pb.filter(pb.table(0, 3), EBV(op(ENC_TV(col(0)), ENC_TV(col(1)))), projection=[2]))
        plan, got = run_both(gs, os_, desc, gpu_tables=[(ptrs, n)], cpu_tables=[[a, b, tag]])
        total += plan.result_info()[0]
        for lit in (date_time(*xsd.parse_date_time("2008-06-20T00:00:00Z")), date_time(*xsd.parse_date_time("2008-06-20T03:00:00")),
                    date(*xsd.parse_date("2004-12-25")), time_lit(*xsd.parse_time("12:00:00+01:00")), date_time((1 << 127) - 1, False)):
            pb = PlanBuilder()
            desc = pb.build(pb.filter(pb.table(0, 3), EBV(op(ENC_TV(col(0)), lit)), projection=[2, 0]))
            plan, got = run_both(gs, os_, desc, gpu_tables=[(ptrs, n)], cpu_tables=[[a, b, tag]])
            total += plan.result_info()[0]
    assert total > 2 * n
    # join filter: L(k, a) JOIN R(k, b) ON k WHERE a < b
    k1, k2 = rng.integers(1, 300, 4000).astype(np.uint32), rng.integers(1, 300, 3000).astype(np.uint32)
    L, R = [k1, a[:4000]], [k2, b[:3000]]
    kl, pl = table_on_device(torch_cuda, L)
    kr, pr = table_on_device(torch_cuda, R)
    pb = PlanBuilder()
    desc = pb.build(pb.hash_join(pb.table(0, 2), pb.table(1, 2), on=[(0, 0)], filter=EBV(LT(ENC_TV(col(1)), ENC_TV(col(3))))))
    plan, got = run_both(gs, os_, desc, gpu_tables=[(pl, 4000), (pr, 3000)], cpu_tables=[L, R])
    assert plan.result_info()[0] > 1000


@pytest.mark.parametrize("world", [2, 8])
def test_subject_hash_shard_keeps_the_index_join_path(torch_cuda, world):
    """A hash(subject) shard of a predicate slice keeps the slice's id range with 1/G of its rows: the engine must
    still build its direct-address / CSR tables on it (phase B of the graph-sharded run is the same fused chain as on
    one GPU), and the union of the shards' bindings is the unsharded answer."""
    from rdf_fusion_amd import sharding
    ds = bsbm.generate(12_000)        # 1500 products per shard at G = 8: slices above the LDS-table size
    full_o = orc.OracleStore()
    full_o.extend(ds.g, ds.s, ds.p, ds.o)
    full_o.set_typed_values(ds.typed_values, ds.decimals)
    rng = np.random.default_rng(world)
    batch = 300
    prods = np.array([ds.product(i) for i in rng.choice(ds.n_products, batch, replace=False)], dtype=np.uint32)
    params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
    c_tab, n_c, _ = full_o.execute(bsbm.q5_batch_const_plan(ds), [params])          # what the all-gather delivers
    c_tab = [np.ascontiguousarray(c[:n_c]) for c in c_tab]
    exp_all, n_all, _ = full_o.execute(bsbm.q5_batch_plan(ds), [params])
    keep, ptrs = table_on_device(torch_cuda, c_tab)
    desc = bsbm.q5_batch_plan(ds, tables=True)
    union = []
    for r in sorted({0, world - 1}) if world > 2 else range(world):
        g, s, p, o = sharding.shard_dataset(ds, r, world)
        gs, os_ = both_stores((g, s, p, o), typed=ds.typed_values, decimals=ds.decimals)
        plan = gs.plan(desc)
        for it in range(3):
            plan.bind_table(0, ptrs, n_c)
            plan.enable_kernel_timing(True)
            got = plan.execute().fetch()
        exp, n_exp, _ = os_.execute(desc, [c_tab])
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        # the fused chain: as a band join over the shard's CSR groups, or inside the candidate join's resolve phase
        assert any(("lds_join_kernel" in k[0] and k[0].rstrip(">").endswith("true")) or "band_mask_kernel" in k[0] for k in plan.kernel_stats()) or ENGINE_TOGGLED
        union.append(ku.multiset(got))
    if world == 2:
        np.testing.assert_array_equal(ku.multiset(list(np.concatenate(union).T)), ku.multiset(exp_all, n_all))


def test_generic_vm_equals_specialised_kernels(bsbm_stores):
    ds, gs, os_ = bsbm_stores
    desc = bsbm.q5_plan(ds, ds.product(17))
    a = gs.plan(desc).execute().fetch()
    gs.set_option("FORCE_GENERIC_VM", 1)
    try:
        b = gs.plan(desc).execute().fetch()
    finally:
        gs.set_option("FORCE_GENERIC_VM", 0)
    np.testing.assert_array_equal(ku.multiset(a), ku.multiset(b))


def test_result_keeps_its_snapshot_across_store_mutations(torch_cuda):
    """a pure-scan result is zero-copy slices of the permutations; extend / remove / clear replace every column.
    An executed plan keeps the generation it ran against: fetch, batches and the device pointers after the mutation still
    show the pre-mutation rows (the reference's plan keeps its Arc'ed snapshot, snapshot.rs:35-37); the next execute sees
    the new contents."""
    rng = np.random.default_rng(3)
    g, s_, p, o = random_quads(rng, 30_000, 500, graphs=1)
    gs, os_ = both_stores((g, s_, p, o), batch=4096)
    pb = PlanBuilder()
    desc = pb.build(pb.data_source(quad_pattern("s", int(p[0]), "o")))
    plan = gs.plan(desc).execute()
    n_before, _ = plan.result_info()
    before = ku.multiset(plan.fetch())
    assert n_before > 100
    add = random_quads(rng, 20_000, 500, graphs=1)
    gs.extend(*add)                                              # frees and replaces every column of every permutation
    np.testing.assert_array_equal(ku.multiset(plan.fetch()), before)
    gs.remove(g[:5000], s_[:5000], p[:5000], o[:5000])
    assert sum(len(b) for b in plan.batches()) == n_before
    gs.clear()
    np.testing.assert_array_equal(ku.multiset(plan.fetch()), before)
    assert len(gs) == 0
    assert plan.execute().result_info()[0] == 0                 # the next execute reads the current generation
    plan.close()


def test_remove_graph_matches_numpy(torch_cuda):
    """QuadStorage::clear_graph / drop_named_graph (quad_storage.rs:59-68) through rdfgpu_store_remove_graph."""
    rng = np.random.default_rng(9)
    g, s_, p, o = random_quads(rng, 40_000, 300, graphs=4)
    gs = rf.GpuQuadStore()
    n0 = gs.extend(g, s_, p, o)
    uniq = np.unique(np.stack([g, s_, p, o], axis=1), axis=0)
    assert n0 == len(uniq)
    for graph in (2, 0, 7):
        expect = int((uniq[:, 0] == graph).sum())
        assert gs.remove_graph(graph) == expect
        uniq = uniq[uniq[:, 0] != graph]
        assert len(gs) == len(uniq)
        for comp in (abi.GSPO, abi.GPOS, abi.GOSP):
            cols = gs.read_index(comp)
            assert len(cols[0]) == len(uniq) and not (cols[0] == graph).any()
    got = np.stack(gs.read_index(abi.GSPO), axis=1)
    np.testing.assert_array_equal(got, uniq)


def test_plan_is_reexecutable_and_sees_updates(bsbm_stores):
    ds, gs, os_ = bsbm_stores
    desc = bsbm.q1_scan_filter_plan(ds, 900)
    plan = gs.plan(desc)
    a = ku.multiset(plan.execute().fetch())
    b = ku.multiset(plan.execute().fetch())
    np.testing.assert_array_equal(a, b)
    m = plan.metrics()
    assert m.output_rows == len(a) and m.kernels_launched >= 1 and m.elapsed_compute_ms > 0


def test_reexecution_is_speculative_but_exact(torch_cuda):
    """A re-executed plan reuses its located ranges and sizes join outputs from the previous run without
    waiting; when the guess is wrong (the batch grows 20x) or the store changes, results must still be exact."""
    ds = bsbm.generate(800)
    gs, os_ = both_stores((ds.g, ds.s, ds.p, ds.o), typed=ds.typed_values, decimals=ds.decimals)
    desc = bsbm.q5_batch_plan(ds)
    plan = gs.plan(desc)
    rng = np.random.default_rng(9)
    syncs = []
    for batch in (8, 8, 8, 160, 160, 3):
        prods = np.array([ds.product(i) for i in rng.choice(ds.n_products, batch, replace=False)], dtype=np.uint32)
        params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
        keep, ptrs = table_on_device(torch_cuda, params)
        plan.bind_table(0, ptrs, batch)
        got = plan.execute().fetch()
        exp, n_exp, _ = os_.execute(desc, [params])
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        syncs.append(plan.metrics().host_syncs)
    assert syncs[1] < syncs[0] and syncs[2] == syncs[1]          # steady state: no per-join waits
    # the store changes under the compiled plan: ranges are re-located, results follow the data
    x = ds.product(5)
    extra = (np.zeros(3, np.uint32), np.full(3, x, np.uint32), np.full(3, ds.pred["bsbm:productFeature"], np.uint32),
             (ds.feature_base + np.array([1, 2, 3])).astype(np.uint32))
    assert gs.extend(*extra) == os_.extend(*extra)
    params = [np.array([1], np.uint32), np.array([x], np.uint32)]
    keep, ptrs = table_on_device(torch_cuda, params)
    plan.bind_table(0, ptrs, 1)
    got = plan.execute().fetch()
    exp, n_exp, _ = os_.execute(desc, [params])
    np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))


def test_invalid_plans_are_rejected():
    gs = rf.GpuQuadStore()
    pb = PlanBuilder()
    t = pb.table(0, 2)
    with pytest.raises(rf.RdfGpuError):     # column out of range
        gs.plan(pb.build(pb.filter(t, ID_EQ(col(5), lit_id(1)))))
    pb = PlanBuilder()
    with pytest.raises(rf.RdfGpuError):     # predicate is not boolean
        gs.plan(pb.build(pb.filter(pb.table(0, 2), ENC_TV(col(0)))))
    pb = PlanBuilder()
    with pytest.raises(rf.RdfGpuError):     # ill-typed: EBV of an id
        gs.plan(pb.build(pb.filter(pb.table(0, 2), EBV(col(0)))))
    pb = PlanBuilder()
    plan = gs.plan(pb.build(pb.table(0, 1)))
    with pytest.raises(rf.RdfGpuError):     # unbound table
        plan.execute()
