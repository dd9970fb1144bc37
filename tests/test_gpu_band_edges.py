"""The integer-window joins at the edges of their biased intervals (band_cases.py): slice values whose spread sits on either side of
every limit of the packed 16-bit form, the 32-bit form and the range index, at bases from -2^63 + 1 to 2^63 - 1 - spread, probe operands
around them and at the i64 extremes, windows with every operator pairing and literals from 0 to 2^63 - 1.  Every device form of the
chain - the band join packed and 32-bit, compact and not, the range index, the value table, the full semantics, the un-fused joins -
must give the rows of window_reference (Python ints straight from the SPARQL rule; test_band_window_cpu.py holds the oracle to the same)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
from oracle import oracle as orc
import band_cases as bc
import kat_util as ku

ENGINE_TOGGLED = any(k.startswith(("RDFGPU_NO_", "RDFGPU_FORCE_")) for k in os.environ)   # a debugging toggle is set for the whole run
FORMS = [("NO_BAND_PACK16",), ("NO_BAND_COMPACT",), ("NO_BAND_JOIN",), ("NO_BAND_JOIN", "NO_RANGE_INDEX"), ("NO_VALUE_TABLES",), ("NO_CHAIN_FUSION",)]
N_SETS = len(bc.VALUE_SETS)
SET_IDS = [vs.name for vs in bc.VALUE_SETS]


def device_store(st):
    gs = rf.GpuQuadStore()
    gs.extend(*st.quads)
    gs.set_typed_values(st.tv, st.decimals)
    return gs


def on_device(torch, cols):
    ts = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint32).view(np.int32)).cuda() for c in cols]
    return ts, [t.data_ptr() for t in ts]


def band_admitted(vs, big_group=False):
    """chain_band_args takes the chain: a decoded value column (no slice value is the table's own sentinel, -2^63), biased values below 2^32 - 32, groups of at most 512"""
    return not vs.has_min and vs.spread < bc.BAND_SPREAD_LIMIT and not big_group


def has_band(names):
    return any("band_mask_kernel" in k for k in names) and any("band_emit_kernel" in k for k in names)


def no_band(names):
    return not any("band_" in k for k in names)


def fused_chain(names):
    """the chain ran inside the base join's kernel (lds_join_kernel<.., CHAIN = true>)"""
    return any("lds_join_kernel" in k and k.rstrip(">").endswith("true") for k in names)


def run(plan, want, what):
    """one execution: row count and multiset are the reference's; -> the names of the kernels that ran"""
    plan.enable_kernel_timing(True)
    got = plan.execute().fetch()
    assert plan.result_info()[0] == len(want), (what, plan.result_info()[0], len(want))
    np.testing.assert_array_equal(ku.multiset(got, len(want)), want, err_msg=what)
    return {k[0] for k in plan.kernel_stats()}


def check_case(gs, st, ptrs, c, vs, big_group=False):
    what = f"{vs.name} {bc.case_id(c)}"
    want, unfiltered = bc.window_reference(st.quads, st.terms, st.T, c.windows, c.neq)
    plan = gs.plan(bc.band_plan(c.windows, c.neq))
    plan.bind_table(0, ptrs, len(st.T[0]))
    seen = set()
    for rep in range(4):                                            # fusion needs the cardinalities of a first execution
        seen |= run(plan, want, f"{what} rep {rep}")
    print(f"{what}: {len(want)} of {unfiltered} rows; band {has_band(seen)}, fused {fused_chain(seen)}")
    admitted = band_admitted(vs, big_group)
    check_forms = not ENGINE_TOGGLED and len(want) > 0              # (a join that came out empty leaves no cardinalities to fuse on)
    if not ENGINE_TOGGLED and not admitted:
        assert no_band(seen), (what, sorted(seen))
    if check_forms:
        assert has_band(seen) == admitted and (admitted or fused_chain(seen)), (what, sorted(seen))
        if admitted:
            assert any("band_slow_kernel" in k for k in seen), (what, sorted(seen))   # (the table has operands of other kinds and operands that overflow)
    for form in FORMS:
        for o in form:
            plan.set_option(o, 1)
        names = run(plan, want, f"{what} {form}")
        for o in form:
            plan.set_option(o, 0)
        band_off = form[0] in ("NO_BAND_JOIN", "NO_VALUE_TABLES", "NO_CHAIN_FUSION")
        if not ENGINE_TOGGLED and (band_off or not admitted):
            assert no_band(names), (what, form, sorted(names))
        if not ENGINE_TOGGLED and form[0] == "NO_CHAIN_FUSION":
            assert not fused_chain(names), (what, form, sorted(names))
        if check_forms:
            assert has_band(names) == (admitted and not band_off), (what, form, sorted(names))
            assert fused_chain(names) == (not has_band(names) and form[0] != "NO_CHAIN_FUSION"), (what, form, sorted(names))
    names = run(plan, want, f"{what} back to the default")
    gs.drop_tables()
    run(plan, want, f"{what} after drop_tables")
    names = run(plan, want, f"{what} after drop_tables, second")
    if check_forms:
        assert has_band(names) == admitted, (what, sorted(names))
    return len(want), unfiltered


@pytest.mark.parametrize("k", range(N_SETS), ids=SET_IDS)
def test_every_form_equals_reference(torch_cuda, k):
    """Six (window[, second window], ID_NEQ) cases per value set: a fresh plan executed four times, the same plan under each option
    that switches a form off, after drop_tables.  The band kernels ran exactly for the spreads chain_band_args admits."""
    vs = bc.VALUE_SETS[k]
    st = bc.store_of(vs)
    gs = device_store(st)
    keep, ptrs = on_device(torch_cuda, st.T)
    for c in bc.cases_of(k):
        check_case(gs, st, ptrs, c, vs)
    del keep


def test_group_of_513_keeps_off_the_band_path(torch_cuda):
    vs = bc.VALUE_SETS[1]
    st = bc.store_of(vs, big_group=True)
    gs = device_store(st)
    keep, ptrs = on_device(torch_cuda, st.T)
    for c in bc.cases_of(1)[:2]:
        n, unfiltered = check_case(gs, st, ptrs, c, vs, big_group=True)
        assert 0 < n < unfiltered
    del keep


def mask_bytes_per_row(plan, n_build):
    """Bytes per probe row the pair test read, from kernel_stats (the names there are one per kernel class, without template arguments, so
    band_mask_kernel's PACK does not show in them): 16 = the compact record, which exists in the packed 16-bit form only; 28 = sorted
    position + 32-bit record.  None: the pair test did not run."""
    for name, launches, ms, nbytes, rows in plan.kernel_stats():
        if "band_mask_kernel" in name:
            assert launches == 1 and rows > 0 and (nbytes - 16 * n_build) % rows == 0, (launches, nbytes, rows, n_build)
            return (nbytes - 16 * n_build) // rows
    return None


@pytest.mark.parametrize("k", range(N_SETS), ids=SET_IDS)
def test_which_form_decides(torch_cuda, k):
    """x = y (literal 0: nothing overflows) over a table whose operands are all xsd:integer, so that the biased interval alone decides every
    pair.  Packed 16-bit records for spreads up to 65530 and only those; 32-bit records up to 2^32 - 33; beyond, and with -2^63 among the
    slice values, no band join.  With the band join off: the range index is built for spreads below 2^32 - 16 and only those; without
    it the decoded value table; without that the full semantics.  Then operands of other kinds come back into the same plan."""
    vs = bc.VALUE_SETS[k]
    st = bc.store_of(vs)
    windows, neq = (bc.ZERO_WINDOW,), True
    want, unfiltered = bc.window_reference(st.quads, st.terms, st.T_int, windows, neq)
    assert 0 < len(want) < unfiltered
    desc = bc.band_plan(windows, neq)
    keep, ptrs = on_device(torch_cuda, st.T_int)
    n = len(st.T_int[0])
    gs = device_store(st)
    plan = gs.plan(desc)
    plan.bind_table(0, ptrs, n)
    per_row = []
    for rep in range(4):
        names = run(plan, want, f"{vs.name} rep {rep}")
        per_row.append(mask_bytes_per_row(plan, st.n_build))
    print(f"{vs.name}: spread {vs.spread:#x}, {len(want)} rows, pair-test bytes per row {per_row}")
    if not ENGINE_TOGGLED:
        assert has_band(names) == band_admitted(vs), sorted(names)
        if has_band(names):
            assert set(per_row) <= {None, 16, 28}, per_row
            assert (per_row[-1] == 16) == (vs.spread <= bc.PACK_SPREAD_MAX), (vs.spread, per_row)
            assert not any("band_slow_kernel" in k for k in names), sorted(names)       # every row was decided by its interval
            plan.set_option("NO_BAND_PACK16", 1)
            run(plan, want, f"{vs.name} NO_BAND_PACK16")
            assert mask_bytes_per_row(plan, st.n_build) == 28
            plan.set_option("NO_BAND_PACK16", 0)
    # the forms below the band join, each on a store of its own: what a form builds tells that it ran
    built = {}
    for form in (("NO_BAND_JOIN",), ("NO_BAND_JOIN", "NO_RANGE_INDEX"), ("NO_BAND_JOIN", "NO_RANGE_INDEX", "NO_VALUE_TABLES")):
        g2 = device_store(st)
        p2 = g2.plan(desc)
        for o in form:
            p2.set_option(o, 1)
        p2.bind_table(0, ptrs, n)
        built[form] = 0
        for rep in range(3):
            names = run(p2, want, f"{vs.name} {form} rep {rep}")
            built[form] += p2.metrics().tables_built
        if not ENGINE_TOGGLED:
            assert no_band(names) and fused_chain(names), (form, sorted(names))
    b = list(built.values())
    print(f"{vs.name}: tables built with the range index {b[0]}, with the value table {b[1]}, with neither {b[2]}")
    if not ENGINE_TOGGLED:
        assert b[0] - b[1] == (1 if vs.spread < bc.INDEX_SPREAD_LIMIT and not vs.has_min else 0), b
        assert b[1] - b[2] == 1, b                                                       # the decoded value column (tried, and given up, when a value is -2^63)
    # rows that need the full semantics come back (the plan had stopped launching their pass): noticed, and answered exactly
    want_mixed, _ = bc.window_reference(st.quads, st.terms, st.T, windows, neq)
    keep2, ptrs2 = on_device(torch_cuda, st.T)
    plan.bind_table(0, ptrs2, len(st.T[0]))
    for rep in range(2):
        run(plan, want_mixed, f"{vs.name} mixed operands rep {rep}")
    del keep, keep2


def test_ordered_join_route_with_a_wide_spread(torch_cuda):
    """The batched BSBM Q5, whose band join takes its row records from the ordered slice join below it (oj_band_records_kernel), with the
    integer literals moved monotonically onto -2^62 + 70000 v and the windows scaled alike: a spread far past 65530 under a huge negative
    bias, so 32-bit records - which also keeps the in-place route (it needs the 16-byte records) out.  Against the oracle, per batch."""
    ds = bsbm.generate(1500)
    tv = ds.typed_values.copy()
    ints = slice(ds.int_base, ds.int_base + 2000)
    assert (tv["tag"][ints] == abi.TV_INTEGER).all()
    tv["lo"][ints] = -2 ** 62 + 70000 * tv["lo"][ints]
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    assert gs.extend(ds.g, ds.s, ds.p, ds.o) == os_.extend(ds.g, ds.s, ds.p, ds.o)
    gs.set_typed_values(tv, ds.decimals)
    os_.set_typed_values(tv, ds.decimals)
    desc = bsbm.q5_batch_plan(ds, w1=120 * 70000, w2=170 * 70000)
    plan = gs.plan(desc)
    rng = np.random.default_rng(41)
    seen, rows = set(), 0
    for it, batch in enumerate((200, 200, 1200, 1200, 1200, 1200, 1200, 1200, 200)):
        prods = np.array([ds.product(int(i)) for i in rng.choice(ds.n_products, batch, replace=False)], dtype=np.uint32)
        params = [np.arange(1, batch + 1, dtype=np.uint32), prods]
        keep, ptrs = on_device(torch_cuda, params)
        plan.bind_table(0, ptrs, batch)
        exp, n_exp, _ = os_.execute(desc, [params])
        names = run(plan, ku.multiset(exp, n_exp), f"batch {it}")
        seen |= names
        rows += n_exp
        del keep
    print(f"{rows} rows; kernels {sorted(seen)}")
    assert rows > 1000
    if not ENGINE_TOGGLED:
        assert has_band(seen) and any("oj_band_records_kernel" in k for k in seen), sorted(seen)
        assert not any("OjInPlace" in k for k in seen), sorted(seen)
