"""The fused hash join at its queue, tile and table edges (join_cases.py): lds_join_kernel (join_device.hpp) over its LDS, HBM-hash, direct and
CSR tables and stream_join_kernel (stream_join.hip) over its direct and hash forms, with the wave queue, the lanes per CSR row and the LDS
limit set through JOIN_WAVE_Q, CSR_ROW_LANES_LOG2 and LDS_MAX_BUILD.  Every case executes its plan three times - a first-guess (or exact)
execution, a speculative one, one sized from history - and each time the device's rows must be reference()'s multiset and result_info()
its length; where a case is built for a kernel form, the class `lds_join_kernel<FS, PFS, ITEMS, MODE, CHAIN` (MODE 0 LDS, 1 hash, 2 direct,
3 CSR) or stream_join_kernel in kernel_stats() is checked against it (test_join_cases_cpu.py holds the oracle to the same reference)."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
import join_cases as jc

ENGINE_TOGGLED = any(k.startswith(("RDFGPU_NO_", "RDFGPU_FORCE_")) for k in os.environ)   # a debugging toggle is set for the whole run
LDS_CLASS = re.compile(r"lds_join_kernel<(\d), (\d), (\d), (\d), (true|false)")
LEFT_TAIL = "join_left_unmatched_kernel"

# table form -> (store, plan options, what must have run: (kernel, MODE))
FORMS = {
    "lds": ("dense", {"LDS_MAX_BUILD": 8192}, ("lds", 0)),                                          # every workgroup builds the table in LDS
    "hash": ("hash", {"LDS_MAX_BUILD": 1, "NO_STREAM_JOIN": 1}, ("lds", 1)),                        # the slice's cached hash table
    # one lane per probe row; without NO_ORDERED_JOIN a re-execution of a join without a filter would leave lds_join_kernel for the ordered
    # slice join (run_ordered_join; test_gpu_ordered_join_edges.py)
    "csr": ("dense", {"LDS_MAX_BUILD": 1, "CSR_ROW_LANES_LOG2": 1, "NO_ORDERED_JOIN": 1}, ("lds", 3)),
    "direct": ("dense", {"LDS_MAX_BUILD": 1, "NO_STREAM_JOIN": 1}, ("lds", 2)),
    "stream_direct": ("dense", {"LDS_MAX_BUILD": 1}, ("stream", 2)),
    "stream_hash": ("hash", {"LDS_MAX_BUILD": 1}, ("stream", 1)),
    "scratch_hash": ("dense", {"LDS_MAX_BUILD": 1, "NO_PARTITIONED_JOIN": 1, "NO_STREAM_JOIN": 1}, ("lds", 1)),   # a bound table above the LDS limit
    "scratch_hash_streamed": ("dense", {"LDS_MAX_BUILD": 1, "NO_PARTITIONED_JOIN": 1}, ("stream", 1)),
}
_STORES, _REFS, _TABLES, SEEN = {}, {}, {}, {}


def device_store(kind):
    """dense: the slices get their direct-address / CSR tables; hash: the same quads under NO_DIRECT_TABLE, so that they get hash tables
    (a slice's table is kept with the store: one store per family)"""
    if kind not in _STORES:
        _STORES[kind] = jc.fill_store(rf.GpuQuadStore())
        if kind == "hash":
            _STORES[kind].set_option("NO_DIRECT_TABLE", 1)
    return _STORES[kind]


def on_device(torch, name, cols):
    """the columns of a named table, uploaded once (an empty table still gets columns to point at)"""
    if name not in _TABLES:
        ts = [torch.from_numpy(np.ascontiguousarray(c if len(c) else np.zeros(1), dtype=np.uint32).view(np.int32)).cuda() for c in cols]
        _TABLES[name] = (ts, [t.data_ptr() for t in ts], len(cols[0]))
    return _TABLES[name]


def forms_of(names):
    out = {("lds",) + tuple(int(x) for x in m.groups()[:4]) + (m.group(5) == "true",) for m in map(LDS_CLASS.search, names) if m}
    return out | ({("stream",)} if any("stream_join_kernel" in k for k in names) else set())


class Runner:
    """One plan under one table form, executed over one set of bound tables after another."""
    def __init__(self, torch, group, form, join, options=None):
        store, opts, self.must = FORMS[form]
        self.torch, self.group, self.form, self.join = torch, group, form, join
        self.opts = dict(opts, **(options or {}))
        self.plan = device_store(store).plan(jc.plan_of(join)).enable_kernel_timing(True)
        for o, v in self.opts.items():
            self.plan.set_option(o, v)
        self.what = f"{group} {form} {self.opts}"
        self.names, self.last = set(), None

    def execute(self, tables, name):
        """tables: {table name: columns} in slot order.  -> metrics; the rows are the reference's"""
        for slot, (tname, cols) in enumerate(tables.items()):
            _, ptrs, n = on_device(self.torch, tname, cols)
            self.plan.bind_table(slot, ptrs, n)
        key = (self.join, tuple(tables))
        if key not in _REFS:
            _REFS[key] = jc.expected(self.join, list(tables.values()))
        want = _REFS[key]
        got = self.plan.execute().fetch()
        what = f"{self.what}: {name}"
        assert self.plan.result_info()[0] == len(want), (what, self.plan.result_info()[0], len(want))
        jc.assert_rows(got, want, len(self.join.proj), what)
        self.last = {k[0] for k in self.plan.kernel_stats()}
        self.names |= self.last
        return self.plan.metrics()

    def run(self, tables, name, times=3):
        return [self.execute(tables, f"{name} #{k}") for k in range(times)]

    def close(self, items=None, fs=None, pfs=None, check=True):
        """the form the case is built for is among the kernels that ran"""
        seen = forms_of(self.names)
        SEEN.setdefault(self.group, set()).update(seen)
        self.plan.close()
        if ENGINE_TOGGLED or not check:
            return seen
        if self.must[0] == "stream":
            assert ("stream",) in seen and not any(f[0] == "lds" for f in seen), (self.what, sorted(self.names))
        else:
            hit = [f for f in seen if f[0] == "lds" and f[4] == self.must[1] and (items is None or f[3] == items) and (fs is None or f[1] == fs) and (pfs is None or f[2] == pfs)]
            assert hit and ("stream",) not in seen, (self.what, items, fs, pfs, sorted(self.names))
        return seen


def report(group):
    print(f"\n[join forms] {group}: {sorted(SEEN.get(group, ()))}")


# ---------------------------------------------------------------------------------------------------
# 1. queue capacity and pend[]
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [64, 128, None])
@pytest.mark.parametrize("form", ["lds", "hash", "csr"])
def test_group1_queue_capacity(torch_cuda, form, q):
    """`if (qn + n_found > qcap) { pend[k] = hit; full = true; }` (lds_join_body): waves 0 and 7 of a 512-row tile and the live lanes of the
    partial tile of 513 and 575 rows carry 64 rows with 1 partner (q = 64: exactly full, nothing pended), with 2, 3 and 6 (every later
    round pended and resumed), with lane % 5 (rounds of 51, 38, 25, 12: pended with the queue partly full) and one row with 300 beside 63
    with none; no filter, one that rejects every candidate (a flush with qn == 0 reserves nothing) and one that rejects every other.
    q unset: size_wave_queue's 256 .. 1024 from the history of the table before."""
    options = {"JOIN_WAVE_Q": q} if q else {}
    for fname, pred in jc.FILTERS.items():
        r = Runner(torch_cuda, "1 queue", form, jc.slice_join(jc.P_CS, pred), options)
        for pattern in jc.PATTERNS:
            for n in jc.WAVE_ROWS:
                r.run({f"wave-{pattern}-{n}": jc.wave_table(n, pattern)}, f"{fname} {pattern} {n}")
        r.close(items=1, fs={"none": 0, "all": 2, "alt": 3}[fname])
    report("1 queue")


# ---------------------------------------------------------------------------------------------------
# 2. output capacity
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lds", "stream_hash", "hash"])
def test_group2_output_capacity(torch_cuda, form):
    """first_guess (exec_lds_join) = probe rows + 1024 for an LDS or hash table: 512 probe rows with exactly 1536 rows fit, 1537 run again
    exactly; then `prev + prev / 4 + 256` (run_speculative): 2176 after 1536 and 2976 after 2977 fit, 2977 after 2176 and 2178 after 1537 do not (`b + qn > a.out_cap`, and
    `base + total > a.out_cap` in stream_join_kernel)."""
    t = lambda total: {f"total-{total}": jc.total_table(512, total)}
    r = Runner(torch_cuda, "2 capacity", form, jc.slice_join(jc.P_CS))
    for total, reruns in ((1536, 0), (2176, 0), (2977, 1), (2976, 0)):
        m = r.execute(t(total), f"{total} rows")
        assert m.exact_reruns == reruns or ENGINE_TOGGLED, (form, total, m.exact_reruns)
    r.close()
    r = Runner(torch_cuda, "2 capacity", form, jc.slice_join(jc.P_CS))
    for total, reruns in ((1537, 1), (2178, 1), (2978, 0)):
        m = r.execute(t(total), f"{total} rows")
        assert m.exact_reruns == reruns or ENGINE_TOGGLED, (form, total, m.exact_reruns)
    r.close()
    report("2 capacity")


# ---------------------------------------------------------------------------------------------------
# 3. the LDS table
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", jc.LDS_BUILDS)
def test_group3_lds_table_sizes(torch_cuda, n):
    """LDS_MAX_BUILD = 8192 (choose_join_table: `j.global_table = B.cap > lds_limit`): builds of 1 row, around 1024 (4096 -> 8192 slots), around
    4096 (16384 slots), 8192 rows at load 0.5 - table mode 0 - and 8193, which must not carry that mode."""
    form = "lds" if n <= 8192 else "scratch_hash"
    r = Runner(torch_cuda, "3 lds table", form, jc.TABLE_JOIN, {"LDS_MAX_BUILD": 8192})
    r.run({f"lds-build-{n}": jc.lds_build(n), f"lds-probe-{n}": jc.lds_probe(n)}, f"build {n}")
    seen = r.close(items=1)
    assert ENGINE_TOGGLED or (any(f[0] == "lds" and f[4] == 0 for f in seen) == (n <= 8192)), sorted(seen)
    report("3 lds table")


def test_group3_null_build_and_one_key_chain(torch_cuda):
    """a build side whose keys are all 0 (load_keys: nothing enters the table), inner and left; 8192 build rows on one key probed by three
    rows and a null: a chain of 8192 hops per row, 24576 rows against a first guess of 9216"""
    tables = {"null-build": jc.lds_build(600, np.zeros(600)), "lds-probe-600": jc.lds_probe(600)}
    for how in ("inner", "left"):
        r = Runner(torch_cuda, "3 lds table", "lds", jc.TABLE_JOIN._replace(how=how))
        r.run(tables, f"null build {how}")
        r.close()
    one = jc.one_key_tables()
    r = Runner(torch_cuda, "3 lds table", "lds", jc.TABLE_JOIN)
    ms = r.run({"one-key-build": one[0], "one-key-probe": one[1]}, "one key")
    assert ENGINE_TOGGLED or [m.exact_reruns for m in ms] == [1, 0, 0]
    r.close()
    report("3 lds table")


def test_group3_queue_that_does_not_fit(torch_cuda):
    """launch_lds_join: `a.wave_q < 64 || lds > 152 * 1024` fails the execute (RDFGPU_ERR_INVALID, "bytes of LDS"): JOIN_WAVE_Q = 1024 against
    the 16384 slots of an 8192-row build (128 + 64 KiB), JOIN_WAVE_Q = 63 against any build"""
    for n, q in ((8192, 1024), (1024, 63)):
        r = Runner(torch_cuda, "3 lds table", "lds", jc.TABLE_JOIN, {"JOIN_WAVE_Q": q})
        with pytest.raises(rf.RdfGpuError, match="bytes of LDS"):
            r.execute({f"lds-build-{n}": jc.lds_build(n), f"lds-probe-{n}": jc.lds_probe(n)}, f"q {q}")
        r.plan.close()


# ---------------------------------------------------------------------------------------------------
# 4. wrap-around
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lds", "scratch_hash", "scratch_hash_streamed", "hash", "stream_hash"])
def test_group4_wrap_around(torch_cuda, form):
    """`h[k] = (h[k] + 1) & a.tbl_mask` (lds_join_body; `(h[k] + 1) & a.tbl_mask` in stream_join_kernel's walk and extra pass): six keys
    whose home slot is the last or the last but one, one of them twice, form a cluster through slot 0; the probe has all eight such keys
    (two walk the whole cluster to the first empty slot behind the wrap), a null and a stranger.  Tables built in LDS and in scratch from
    a bound table, and the cached table of the slice P_W; in the streaming form the key that is there twice takes the extra pass."""
    if form in ("hash", "stream_hash"):
        r = Runner(torch_cuda, "4 wrap", form, jc.slice_join(jc.P_W))
        r.run({"wrap-table": jc.wrap_table()}, "wrap slice")
    else:
        b, p = jc.wrap_tables()
        r = Runner(torch_cuda, "4 wrap", form, jc.TABLE_JOIN)
        r.run({"wrap-build": b, "wrap-probe": p}, "wrap tables")
    r.close()
    report("4 wrap")


# ---------------------------------------------------------------------------------------------------
# 5. several tiles per workgroup
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 2])
@pytest.mark.parametrize("n", jc.TILE_PROBES)
def test_group5_tiles_per_workgroup(torch_cuda, n, n_keys):
    """launch_lds_join: `max_wg = ... tbl_lds > 64 * 1024 ? 256` - an 8192-row build has 128 KiB of table, so 256 workgroups stride over 256,
    257 and 514 tiles (`tile += gridDim.x`); one key column runs the NK = 1 form with its `have_next` / `nk0[]` prefetch, two run NK = 0.
    Partners only on the first and last row of the first tile, the one row of workgroup 0's second tile, the last row overall and wave 3
    of workgroup 0's third tile (two partners per row)."""
    r = Runner(torch_cuda, "5 tiles", "lds", jc.TILE_JOIN[n_keys])
    r.run({"tile-build": jc.tile_build(), f"tile-probe-{n}": jc.tile_probe(n)}, f"{n} rows {n_keys} keys")
    r.close(items=1)
    report("5 tiles")


# ---------------------------------------------------------------------------------------------------
# 6. ITEMS = 4
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", jc.BIG_ROWS[:2])
def test_group6_items_lds(torch_cuda, n):
    """lds_join_items (kernels.hip): `n_probe_cap >= (global ? min_global : min_lds) ? 4 : 1` with min_lds = 2^20: 2^20 - 1 probe rows run
    ITEMS = 1, 2^20 run ITEMS = 4 (a 2048-row tile), where wave 3's four items bring two full rounds each and the 256-entry queue is full
    after item 1; a partner in the last row."""
    r = Runner(torch_cuda, "6 items", "lds", jc.ITEMS_JOIN)
    r.run({"items-build": jc.items_build(), f"big-{n}": jc.big_table(n)}, f"{n} rows")
    r.close(items=4 if n >= 1 << 20 else 1)
    report("6 items")


@pytest.mark.parametrize("n", [65535, 65536])
def test_group6_items_csr(torch_cuda, n):
    """the same switch for an HBM table is at 2^22 rows x lanes (`lds_join_items(a.n_probe_cap << rl, global)`): CSR_ROW_LANES_LOG2 = 7 (rl = 6)
    with 65535 and 65536 probe rows, a tile of 2048 >> 6 = 32 rows"""
    r = Runner(torch_cuda, "6 items", "csr", jc.slice_join(jc.P_CS), {"CSR_ROW_LANES_LOG2": 7})
    r.run({f"lanes-big-{n}": jc.lanes_big_table(n)}, f"{n} rows")
    r.close(items=4 if n == 65536 else 1)
    report("6 items")


@pytest.mark.parametrize("form", ["stream_direct", "stream_hash"])
@pytest.mark.parametrize("n", jc.BIG_ROWS)
def test_group6_items_streaming(torch_cuda, n, form):
    """direct_stream_join_items / stream_join_items (stream_join.hip): 1 row per lane below 2^20 probe rows, 8 (direct table) or 4 (hash
    table) from there: 2^20 - 1, 2^20 and 2^20 + 1 rows (the last tile of one row)"""
    join = jc.slice_join(jc.P_D, proj=(0, 1, 5), left=("t", 0, 4)) if form == "stream_direct" else jc.slice_join(jc.P_CS, proj=(0, 2, 5), left=("t", 0, 4))._replace(on=((2, 0),))
    r = Runner(torch_cuda, "6 items", form, join)
    r.run({f"big-{n}": jc.big_table(n)}, f"{n} rows")
    r.close()
    report("6 items")


# ---------------------------------------------------------------------------------------------------
# 7. lanes per CSR row
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [jc.P_CS, jc.P_CU], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("rl", jc.ROW_LANES)
def test_group7_lanes_per_csr_row(torch_cuda, rl, P):
    """`s[k].x += tid & ((1u << rl) - 1u)` / `s[k].x += 1u << rl` and `kTileRows = (kLdsBlock * ITEMS) >> rl` (lds_join_body): fan-outs 0, 1,
    2^rl - 1, 2^rl, 2^rl + 1 and 300 on probe sides of a tile less one row, a tile, a tile and a row, three tiles and a row; with and
    without the filter that rejects every other partner; a slice sorted by the key (csr_rows == nullptr) and one that is not."""
    for fname in ("none", "alt"):
        r = Runner(torch_cuda, "7 row lanes", "csr", jc.slice_join(P, jc.FILTERS[fname]), {"CSR_ROW_LANES_LOG2": rl + 1})
        for n in jc.lane_rows(rl):
            r.run({f"lanes-{rl}-{n}": jc.lanes_table(rl, n)}, f"rl {rl} {n} rows {fname}")
        r.close(items=1)
    report("7 row lanes")


# ---------------------------------------------------------------------------------------------------
# 8. dense-table bounds
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["direct", "stream_direct", "csr"])
def test_group8_dense_table_bounds(torch_cuda, form):
    """`h[k] < a.direct_n` with h = key - direct_min (lds_join_body), `d < a.direct_n` (stream_join_kernel): the keys kmin, kmax, kmin - 1,
    kmax + 1, 0, 1, 0xFFFFFFFF and an id inside the range without a row (a kNil entry; an empty CSR group).  The CSR table has no streaming
    form (direct_stream_join_ok): it runs under lds_join_kernel with and without NO_STREAM_JOIN."""
    direct = form != "csr"
    for extra in ({}, {"NO_STREAM_JOIN": 1}) if form == "csr" else ({},):
        r = Runner(torch_cuda, "8 bounds", form, jc.slice_join(jc.P_D if direct else jc.P_CS), extra)
        r.run({f"bounds-{direct}": jc.bounds_table(direct)}, "bounds")
        r.close()
    report("8 bounds")


# ---------------------------------------------------------------------------------------------------
# 9. key columns
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lds", "scratch_hash"])
@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("n_keys", [2, 3, 4])
def test_group9_key_columns(torch_cuda, n_keys, how, form):
    """NK = 0: `for (q = 1; q < RDFGPU_MAX_KEYS; q++) if (q < n_keys) eq = eq && a.build_key[q][c.y] == key[k].k[q]` - every row agrees on
    key 0 (the one the slot holds), the pairs differ in the last key; a 0 in the last key only, on either side (load_keys)"""
    b, p = jc.key_tables()
    r = Runner(torch_cuda, "9 keys", form, jc.key_join(n_keys, how))
    r.run({"keys-build": b, "keys-probe": p}, f"{n_keys} keys {how}")
    seen = r.close(items=1)
    assert ENGINE_TOGGLED or (LEFT_TAIL in " ".join(r.names)) == (how == "left")
    report("9 keys")


# ---------------------------------------------------------------------------------------------------
# 10. output columns
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["direct", "stream_direct", "lds"])
@pytest.mark.parametrize("n_cols", list(jc.PROJECTIONS))
def test_group10_output_columns(torch_cuda, n_cols, form):
    """write_out (lds_join_body): `for (oc0 = 0; oc0 < a.n_out_cols; oc0 += 4)`; stream_join_kernel: the first four columns before the
    reservation, `for (oc0 = 4; ...; oc0 += 4)` after it: 1, 4, 5, 8 and 9 columns from both sides"""
    r = Runner(torch_cuda, "10 columns", form, jc.slice_join(jc.P_D, proj=jc.PROJECTIONS[n_cols]))
    r.run({"bounds-True": jc.bounds_table(True)}, f"{n_cols} columns")
    r.run({"zoo-False": jc.zoo_table(False)}, f"{n_cols} columns, five tiles")
    r.close()
    report("10 columns")


# ---------------------------------------------------------------------------------------------------
# 11. left joins
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lds", "scratch_hash"])
def test_group11_classic_left_join(torch_cuda, form):
    """build on the left input, `a.visited[wq[e].x] = 1` (write_out), join_left_unmatched_kernel behind the matched rows"""
    b, p = jc.classic_left_tables()
    r = Runner(torch_cuda, "11 left", form, jc.TABLE_JOIN._replace(how="left"))
    r.run({"left-build": b, "left-probe": p}, "classic")
    r.close(items=1)
    assert ENGINE_TOGGLED or LEFT_TAIL in " ".join(r.names)
    report("11 left")


@pytest.mark.parametrize("outer", [True, False], ids=["probe_outer", "classic"])
@pytest.mark.parametrize("form", ["direct", "csr", "csr_unsorted", "hash"])
def test_group11_left_join_over_a_slice(torch_cuda, form, outer):
    """choose_build_left: a left join whose right input is a slice of more than 1024 rows, with at most a quarter as many left rows, preserves
    its PROBE side (`hit = kOuterNull`, lds_join_body) - NO_PROBE_OUTER_JOIN gives the classic form over the same tables.  JOIN_WAVE_Q = 64; 513
    left rows: a first wave of 64 rows without a partner (0 keys, keys outside the dense range, a hole: 64 null rows fill the queue
    exactly), 63 rows with 2 partners beside one with none (its null row is queued when the second round is pended), a mix; the one row of
    the second tile has no partner, its 511 dead lanes must emit nothing."""
    direct = form == "direct"
    P = jc.P_D if direct else jc.P_CU if form == "csr_unsorted" else jc.P_CS
    options = {"JOIN_WAVE_Q": 64} if outer else {"JOIN_WAVE_Q": 64, "NO_PROBE_OUTER_JOIN": 1, "LDS_MAX_BUILD": 8192}
    r = Runner(torch_cuda, "11 left", form.replace("_unsorted", "") if outer else "lds", jc.slice_join(P, how="left", proj=(0, 1, 5, 6)), options)
    for name in ("unmatched64", "pend_null", "mixed"):
        r.run({f"left-{name}-{direct}": jc.left_table(name, direct)}, name)
    r.close(items=1)
    assert ENGINE_TOGGLED or (LEFT_TAIL in " ".join(r.names)) == (not outer), sorted(r.names)
    report("11 left")


# ---------------------------------------------------------------------------------------------------
# 12. fused filters of the inputs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["csr", "lds", "hash", "stream_hash"])
def test_group12_fused_input_filters(torch_cuda, form):
    """lprobe_filter<1> (`row_live[k] = j < np && lprobe_filter<PFS>(a, j)`): a FilterExec `flag = KEEP` / `flag != DROP` under the probe
    input, flags of 0 among the rows, over the lane % 5 waves with JOIN_WAVE_Q = 64; and `a.has_post` (base_pass): `?o = literal` /
    `?o != literal` under the slice the join builds on."""
    t = {"flagged-wave": jc.flagged_wave_table()}
    for is_eq, lit in ((True, jc.KEEP), (False, jc.DROP)):
        j = jc.Join(("f", ("t", 0, 6), 5, lit, is_eq), ("s", jc.P_CS), ((1, 0),), "inner", None, (0, 1, 7))
        r = Runner(torch_cuda, "12 input filters", form, j, {"JOIN_WAVE_Q": 64})
        r.run(t, f"probe filter {is_eq}")
        r.close(items=1, pfs=1)
    for is_eq in (True, False):
        j = jc.Join(("t", 0, 6), ("f", ("s", jc.P_CS), 1, jc.POST_LITERAL, is_eq), ((1, 0),), "inner", None, (0, 1, 7))
        r = Runner(torch_cuda, "12 input filters", form, j, {"JOIN_WAVE_Q": 64})
        r.run(t, f"build filter {is_eq}")
        r.close(items=1)
    report("12 input filters")


# ---------------------------------------------------------------------------------------------------
# 13. counts known on the device only
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upper", ["probe", "build"])
def test_group13_counts_on_the_device_only(torch_cuda, upper):
    """`live_rows(a.n_probe_dev, a.n_probe_cap)` / `live_rows(a.n_build_dev, a.n_build_cap)`: the lower join's output is the upper join's
    probe side (against the CSR slice) or the build side of its LDS table; from the second execution on its capacity exceeds its rows;
    then lower-side tables that leave a tenth of the rows, and none"""
    join = jc.UPPER_PROBE if upper == "probe" else jc.UPPER_BUILD
    r = Runner(torch_cuda, "13 device counts", "csr" if upper == "probe" else "lds", join, {"NO_STREAM_JOIN": 1})   # (the lower join: lds_join_kernel too)
    for every in (1, 10, 0, 1):
        tables = {f"sized-1500-{every}": jc.sized_table(1500, True, every)}
        if upper == "build":
            tables["upper"] = jc.upper_table()
        r.run(tables, f"every {every}")
    r.close()
    report("13 device counts")


# ---------------------------------------------------------------------------------------------------
# 14. one plan, many tables
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lds", "hash", "csr", "direct", "stream_direct", "stream_hash"])
def test_group14_one_plan_many_tables(torch_cuda, form):
    """500 rows, 3, 0, 500, a table in which nothing joins, 500 and 500 again through one plan per table form: the output is sized from the
    execution before, the queues and counters start clean"""
    direct = "direct" in form
    r = Runner(torch_cuda, "14 many tables", form, jc.slice_join(jc.P_D if direct else jc.P_CS))
    for name in jc.SEQUENCE:
        r.run({f"seq-{name}-{direct}": jc.sequence_table(name, direct)}, name, times=1 if name == "empty" else 3)
    r.close()
    report("14 many tables")


# ---------------------------------------------------------------------------------------------------
# the predicate shapes
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["direct", "stream_direct", "lds"])
@pytest.mark.parametrize("name", list(jc.PREDICATES))
def test_predicate_shapes(torch_cuda, name, form):
    """FS 0 none, FS 2 ID_EQ / ID_NEQ (a 0 operand: not true), FS 3 the two-window shape over xsd:integers with i64::MIN, i64::MAX and
    operands whose + 3 overflows, an xsd:double and a string (window_fast leaves those to window_slow), FS 1 the expression VM over the
    integers.  The VM shape has no streaming form (direct_stream_join_ok): it stays with lds_join_kernel."""
    fs = {"none": 0, "id_eq": 2, "id_neq": 2, "window": 3, "window_two": 3, "vm": 1}[name]
    if name == "vm" and form == "stream_direct":
        form = "direct"
    r = Runner(torch_cuda, "predicates", form, jc.slice_join(jc.P_D, jc.PREDICATES[name], proj=(0, 3, 4, 6)), {"NO_STREAM_JOIN": 1} if form == "direct" else None)
    r.run({f"zoo-{name == 'vm'}": jc.zoo_table(name == "vm")}, name)
    r.close(fs=fs)
    report("predicates")
