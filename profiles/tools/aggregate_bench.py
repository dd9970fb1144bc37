"""AggregateExec (aggregate.hip): GROUP BY one id column on bound tables and on BSBM-shaped join outputs.

Synthetic: N (default 2^26) bound rows {key, integer value id, double value id} with 1, 64, 4096, 2^20 and 2^24 groups (keys drawn
uniformly, unsorted); per shape COUNT(*), COUNT(DISTINCT value), SUM over integers and AVG over doubles.  Times are device-event kernel
times (rdfgpu_plan_enable_kernel_timing), the median over STEPS steady-state executions; the first execution of a fresh plan is reported
on its own (elapsed_compute_ms).  Roofline fraction: DESIGN §6's formula — per input row 4 B per key column, 4 + 16 per SUM / AVG input,
4 per COUNT / COUNT DISTINCT input; per group 4 B per key + 24 per aggregate — over 8 TB/s.  Every timed result is checked against
numpy (counts, distinct counts and integer sums exactly, double averages to 1e-9 relative).

BSBM (BSBM=n products, 0 = skip; BSBM-100M is 285000): BI Q8's COUNT(?offer) GROUP BY ?vendor over the offers of one product type and
AVG(?price) GROUP BY ?product over all offers.  Reported: the aggregate kernels' time, the time of the join kernels feeding them, and
the time to copy the join output to the host (what handing the rows to a host-side aggregation costs).  Checked against numpy over
that copied join output."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, quad_pattern

N = int(os.environ.get("N", str(1 << 26)))
STEPS = int(os.environ.get("STEPS", "7"))
BSBM = int(os.environ.get("BSBM", "285000"))
OUT = os.environ.get("OUT", "")
ROOF = 8e12
records = []
STAR, DISTINCT, SUM, AVG, COUNT = abi.AGG_COUNT_STAR, abi.AGG_COUNT_DISTINCT, abi.AGG_SUM, abi.AGG_AVG, abi.AGG_COUNT
ROW_BYTES = {STAR: 0, COUNT: 4, DISTINCT: 4, SUM: 20, AVG: 20}


def dev(cols):
    t = [torch.from_numpy(np.ascontiguousarray(c).view(np.int32)).cuda() for c in cols]
    return t, [x.data_ptr() for x in t]


def timed_plan(st, desc, tables):
    """(first execution ms, median kernel ms, kernel stats of the median run, plan)"""
    plan = st.plan(desc)
    for slot, (ptrs, n) in enumerate(tables):
        plan.bind_table(slot, ptrs, n)
    plan.execute()
    first = plan.metrics().elapsed_compute_ms
    plan.enable_kernel_timing(True)
    runs = []
    for _ in range(STEPS):
        plan.execute()
        ks = plan.kernel_stats()
        runs.append((sum(k[2] for k in ks), ks))
    runs.sort(key=lambda r: r[0])
    med = runs[len(runs) // 2]
    return first, med[0], med[1], plan


def synthetic():
    st = rf.GpuQuadStore()
    tv = np.zeros(2001, TV_DTYPE)               # ids 1..1000: xsd:integer 1..1000; ids 1001..2000: xsd:double
    tv["tag"][1:1001] = abi.TV_INTEGER
    tv["lo"][1:1001] = np.arange(1, 1001)
    dbl = np.random.default_rng(5).random(1000) * 1000.0
    tv["tag"][1001:] = abi.TV_DOUBLE
    tv["lo"][1001:] = dbl.view(np.int64)
    st.set_typed_values(tv)
    rng = np.random.default_rng(1)
    iv = rng.integers(1, 1001, N).astype(np.uint32)
    dv = rng.integers(1001, 2001, N).astype(np.uint32)
    for groups in [int(x) for x in os.environ.get("GROUPS", "1,64,4096,1048576,16777216").split(",")]:
        key = (rng.integers(0, groups, N) + 1).astype(np.uint32)
        keep, ptrs = dev([key, iv, dv])
        uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        want = {STAR: cnt, SUM: np.bincount(inv, weights=iv.astype(np.float64), minlength=len(uk)).astype(np.int64),
                AVG: np.bincount(inv, weights=dbl[dv - 1001], minlength=len(uk)) / cnt}
        pairs = np.unique(inv.astype(np.int64) << 32 | iv)
        want[DISTINCT] = np.bincount((pairs >> 32).astype(np.int64), minlength=len(uk))
        for fn, c in ((STAR, None), (DISTINCT, 1), (SUM, 1), (AVG, 2)):
            pb = PlanBuilder()
            desc = pb.build(pb.aggregate(pb.table(0, 3), [0], [(fn, c)]))
            first, ms, ks, plan = timed_plan(st, desc, [(ptrs, N)])
            n, _ = plan.result_info()
            gk = plan.fetch()[0]
            order = np.argsort(gk)
            assert n == len(uk) and np.array_equal(gk[order], uk)
            v = plan.fetch_aggregate(0)[order]
            if fn == AVG:
                got = v["lo"].view(np.float64)
                assert (v["tag"] == abi.TV_DOUBLE).all() and np.allclose(got, want[AVG], rtol=1e-9, atol=0)
            else:
                assert (v["tag"] == abi.TV_INTEGER).all() and np.array_equal(v["lo"], want[fn])
            byt = N * (4 + ROW_BYTES[fn]) + n * (4 + 24)
            agg_ms = sum(k[2] for k in ks if "agg_" in k[0])
            top = max(ks, key=lambda k: k[2])
            rec = dict(shape="bound", aggregate=abi.AGG_NAMES[fn], rows=N, groups=int(n), median_ms=round(ms, 4), agg_kernels_ms=round(agg_ms, 4),
                       first_ms=round(first, 4), roofline=round(byt / (ms * 1e-3) / ROOF, 3), top_kernel=top[0], top_ms=round(top[2], 4),
                       kernels={k[0]: dict(ms=round(k[2], 4), bytes=int(k[3])) for k in ks})
            records.append(rec)
            print("groups %9d %-16s %8.3f ms (first %8.3f)  %.3f of 8 TB/s  top %s %.3f ms" % (
                n, abi.AGG_NAMES[fn], ms, first, rec["roofline"], top[0][-40:], top[2]), flush=True)
            plan.close()
        del keep
    st.close()


def bsbm_cases(n):
    ds = bsbm.generate(n)
    st = rf.GpuQuadStore()
    st.extend(ds.g, ds.s, ds.p, ds.o)
    st.set_typed_values(ds.typed_values, ds.decimals)
    pr = ds.pred

    def q8_input(pb):   # offers of one (leaf) product type with their vendors
        t = ds.type_base
        prod = pb.data_source(quad_pattern("product", pr["rdf:type"], t))
        offers = pb.hash_join(pb.data_source(quad_pattern("offer", pr["bsbm:product"], "product")), prod, on=[(1, 0)], projection=[0, 1])
        return pb.hash_join(offers, pb.data_source(quad_pattern("offer", pr["bsbm:vendor"], "vendor")), on=[(0, 0)], projection=[0, 3])

    def price_input(pb):
        return pb.hash_join(pb.data_source(quad_pattern("offer", pr["bsbm:product"], "product")),
                            pb.data_source(quad_pattern("offer", pr["bsbm:price"], "price")), on=[(0, 0)], projection=[0, 1, 3])

    price_of = ds.typed_values["lo"].view(np.float64)
    for label, build, keys, aggs in (("BI Q8: COUNT(?offer) GROUP BY ?vendor", q8_input, [1], [(COUNT, 0)]),
                                     ("AVG(?price) GROUP BY ?product", price_input, [1], [(AVG, 2)])):
        pb = PlanBuilder()
        inp = build(pb)
        in_first, in_ms, in_ks, in_plan = timed_plan(st, pb.build(inp), [])
        rows, _ = in_plan.result_info()
        t0 = time.perf_counter()
        cols = in_plan.fetch()
        copy_ms = (time.perf_counter() - t0) * 1e3
        first, ms, ks, plan = timed_plan(st, pb.build(pb.aggregate(inp, keys, aggs)), [])
        agg_ms = sum(k[2] for k in ks if "agg_" in k[0])
        join_ms = ms - agg_ms
        uk, inv, cnt = np.unique(cols[keys[0]], return_inverse=True, return_counts=True)
        n_g, _ = plan.result_info()
        gk = plan.fetch()[0]
        order = np.argsort(gk)
        assert n_g == len(uk) and np.array_equal(gk[order], uk)
        v = plan.fetch_aggregate(0)[order]
        if aggs[0][0] == COUNT:
            assert np.array_equal(v["lo"], np.bincount(inv, weights=(cols[0] != 0)).astype(np.int64))
        else:
            want = np.bincount(inv, weights=price_of[cols[2]]) / cnt
            assert (v["tag"] == abi.TV_DOUBLE).all() and np.allclose(v["lo"].view(np.float64), want, rtol=1e-9, atol=0)
        byt = rows * (4 + sum(ROW_BYTES[f] for f, _ in aggs)) + n_g * (4 + 24 * len(aggs))
        rec = dict(shape="bsbm", products=n, query=label, join_rows=int(rows), groups=int(n_g), median_ms=round(ms, 4),
                   agg_kernels_ms=round(agg_ms, 4), join_kernels_ms=round(join_ms, 4), input_plan_median_ms=round(in_ms, 4),
                   copy_join_output_to_host_ms=round(copy_ms, 3), first_ms=round(first, 4),
                   agg_roofline=round(byt / (agg_ms * 1e-3) / ROOF, 3),
                   kernels={k[0]: dict(ms=round(k[2], 4), bytes=int(k[3])) for k in ks})
        records.append(rec)
        print("%-40s join rows %9d groups %7d: aggregate %.3f ms, join %.3f ms, copy of the join output %.3f ms (first %.3f)" % (
            label, rows, n_g, agg_ms, join_ms, copy_ms, first), flush=True)
        plan.close(); in_plan.close()
    st.close()


if __name__ == "__main__":
    synthetic()
    if BSBM:
        bsbm_cases(BSBM)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(dict(rows=N, steps=STEPS, records=records), f, indent=1)
