"""MIN / MAX of AggregateExec (aggregate.hip; plans with abi.PLAN_AGG_COLUMNS): bound tables, and the BI Q5 / Q6 shapes on BSBM.

Synthetic: N (default 2^26) bound rows {key, integer value id, decimal value id} with 1, 64, 4096, 2^20 and 2^24 groups (keys drawn
uniformly, unsorted — the sizes of aggregate_bench.py); per shape MAX over the integers, MAX over the decimals (every decimal shares one
of two high words, so the refinement launch does its work) and SUM over the same integers.  Times are device-event kernel times, the
median over STEPS steady-state executions with the smallest and largest beside it; per record the accumulate pass, the refinement launch
and the finishing launches on their own.  Every timed result is checked against numpy.  A build without MIN / MAX refuses them at
compile: the tool records that and still times the SUM, which is how the parent's SUM pass is measured over the same rows.

BSBM (BSBM=n products, 0 = skip; BSBM-100M is 285000):
  Q5 shape  COUNT(offer) per (vendor country, product); MAX of it per country; the join back with count = max; ORDER BY
  Q6 shape  the global AVG(xsd:float(rating1)); cross join; AVG(xsd:float(rating1)) and MIN(global average) per reviewer; HAVING avg > min * 1.5
Q5's rows are checked against numpy over the fetched join output; Q6's kept rows are checked to satisfy the predicate on the device's own values."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
from rdf_fusion_amd.engine import TV_DTYPE, RdfGpuError
from rdf_fusion_amd.plan import PlanBuilder, quad_pattern, col, decimal, xsd_float, EBV, EQ, GT, MUL, ENC_TV

N = int(os.environ.get("N", str(1 << 26)))
STEPS = int(os.environ.get("STEPS", "7"))
BSBM = int(os.environ.get("BSBM", "285000"))
OUT = os.environ.get("OUT", "")
ROOF = 8e12
E18 = 10 ** 18
records = []
MIN, MAX, SUM, AVG, COUNT = abi.AGG_MIN, abi.AGG_MAX, abi.AGG_SUM, abi.AGG_AVG, abi.AGG_COUNT


def dev(cols):
    t = [torch.from_numpy(np.ascontiguousarray(c).view(np.int32)).cuda() for c in cols]
    return t, [x.data_ptr() for x in t]


def timed_plan(st, desc, tables):
    """(first execution ms, [(total kernel ms, kernel stats)] of STEPS steady executions sorted by time, plan)"""
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
    return first, runs, plan


def part(ks, word):
    return sum(k[2] for k in ks if word in k[0])


def spread(runs, word):
    v = sorted(part(ks, word) for _, ks in runs)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def synthetic():
    st = rf.GpuQuadStore()
    tv = np.zeros(2001, TV_DTYPE)               # ids 1..1000: xsd:integer 1..1000; ids 1001..2000: xsd:decimal, high word 0 or 1
    tv["tag"][1:1001] = abi.TV_INTEGER
    tv["lo"][1:1001] = np.arange(1, 1001)
    rng = np.random.default_rng(5)
    dec = np.stack([rng.integers(0, 1 << 62, 1000), rng.integers(0, 2, 1000)], axis=1).astype(np.int64)
    tv["tag"][1001:] = abi.TV_DECIMAL
    tv["lo"][1001:] = np.arange(1000)
    st.set_typed_values(tv, dec)
    rank = (dec[:, 1] << 62) | dec[:, 0]        # the decimals' order as one int64
    rng = np.random.default_rng(1)
    iv = rng.integers(1, 1001, N).astype(np.uint32)
    dv = rng.integers(1001, 2001, N).astype(np.uint32)
    for groups in [int(x) for x in os.environ.get("GROUPS", "1,64,4096,1048576,16777216").split(",")]:
        key = (rng.integers(0, groups, N) + 1).astype(np.uint32)
        keep, ptrs = dev([key, iv, dv])
        uk, inv = np.unique(key, return_inverse=True)
        inv_t = torch.from_numpy(inv.astype(np.int64)).cuda()          # (the per-group maxima on the device: numpy's ufunc.at is slow at 2^26)
        amax = lambda vals: torch.zeros(len(uk), dtype=torch.int64, device="cuda").scatter_reduce_(
            0, inv_t, torch.from_numpy(vals.astype(np.int64)).cuda(), "amax", include_self=False).cpu().numpy()
        want_max, want_dec = amax(iv), amax(rank[dv - 1001])
        del inv_t
        want_sum = np.bincount(inv, weights=iv.astype(np.float64), minlength=len(uk)).astype(np.int64)
        for label, fn, c in (("MAX(integer)", MAX, 1), ("MAX(decimal)", MAX, 2), ("SUM(integer)", SUM, 1)):
            pb = PlanBuilder()
            desc = pb.build(pb.aggregate(pb.table(0, 3), [0], [(fn, c)]), agg_columns=True)
            try:
                first, runs, plan = timed_plan(st, desc, [(ptrs, N)])
            except RdfGpuError as e:
                records.append(dict(shape="bound", aggregate=label, rows=N, groups=int(len(uk)), refused=str(e)[:120]))
                print("groups %9d %-14s refused: %s" % (len(uk), label, str(e)[:80]), flush=True)
                continue
            n, _ = plan.result_info()
            cols = plan.fetch()
            order = np.argsort(cols[0])
            assert n == len(uk) and np.array_equal(cols[0][order], uk)
            v = plan.fetch_column_values(1)[order]
            if label == "MAX(decimal)":
                assert (v["tag"] == abi.TV_DECIMAL).all() and np.array_equal((v["hi"] << 62) | v["lo"], want_dec)
            else:
                assert (v["tag"] == abi.TV_INTEGER).all() and np.array_equal(v["lo"], want_max if fn == MAX else want_sum)
            ms, ks = runs[len(runs) // 2]
            byt = N * (4 + 20) + n * (4 + 24)
            rec = dict(shape="bound", aggregate=label, rows=N, groups=int(n), first_ms=round(first, 4), total_ms=spread(runs, ""),
                       accumulate_ms=spread(runs, "agg_accum"), refine_ms=spread(runs, "refine"), groups_pass_ms=spread(runs, "agg_groups"),
                       roofline=round(byt / (ms * 1e-3) / ROOF, 3), kernels={k[0]: dict(ms=round(k[2], 4), bytes=int(k[3])) for k in ks})
            records.append(rec)
            print("groups %9d %-14s total %8.3f ms  accumulate %8.3f [%.3f .. %.3f]  refine %7.3f  (first %8.3f)" % (
                n, label, ms, rec["accumulate_ms"]["median"], rec["accumulate_ms"]["min"], rec["accumulate_ms"]["max"], rec["refine_ms"]["median"], first), flush=True)
            plan.close()
        del keep
    st.close()


def bsbm_cases(n):
    ds = bsbm.generate(n)
    st = rf.GpuQuadStore()
    st.extend(ds.g, ds.s, ds.p, ds.o)
    st.set_typed_values(ds.typed_values, ds.decimals)
    pr = ds.pred

    def q5_input(pb):   # (country, product, offer)
        ov = pb.hash_join(pb.data_source(quad_pattern("offer", pr["bsbm:product"], "product")),
                          pb.data_source(quad_pattern("offer", pr["bsbm:vendor"], "vendor")), on=[(0, 0)], projection=[0, 1, 3])
        return pb.hash_join(ov, pb.data_source(quad_pattern("vendor", pr["bsbm:country"], "country")), on=[(2, 0)], projection=[4, 1, 0])

    def q5(pb, t):
        counts = pb.aggregate(t, [0, 1], [(COUNT, 2)])
        best = pb.aggregate(counts, [0], [(MAX, 2)])
        joined = pb.hash_join(counts, best, [(0, 0)], filter=EBV(EQ(ENC_TV(col(2)), ENC_TV(col(4)))), projection=[0, 1, 2])
        return pb.sparql_order_by(joined, [(2, True), (0, False), (1, False)])

    def q6_input(pb):   # (reviewer, score)
        return pb.hash_join(pb.data_source(quad_pattern("review", pr["rev:reviewer"], "reviewer")),
                            pb.data_source(quad_pattern("review", pr["bsbm:rating1"], "score")), on=[(0, 0)], projection=[1, 3])

    def q6(pb, t):
        score = lambda: xsd_float(ENC_TV(col(1)))
        overall = pb.aggregate(t, [], [(AVG, score())])
        per = pb.aggregate(pb.cross_join(t, overall), [0], [(AVG, score()), (MIN, 2)])
        return pb.sparql_having(per, EBV(GT(ENC_TV(col(1)), MUL(ENC_TV(col(2)), decimal(15 * E18 // 10)))))

    for label, build_in, build in (("Q5 shape", q5_input, q5), ("Q6 shape", q6_input, q6)):
        pb = PlanBuilder()
        inp = build_in(pb)
        _, in_runs, in_plan = timed_plan(st, pb.build(inp), [])
        rows, _ = in_plan.result_info()
        cols = in_plan.fetch()
        in_plan.close()
        try:
            first, runs, plan = timed_plan(st, pb.build(build(pb, inp), agg_columns=True), [])
        except RdfGpuError as e:
            records.append(dict(shape="bsbm", products=n, query=label, join_rows=int(rows), refused=str(e)[:120]))
            print("%-10s refused: %s" % (label, str(e)[:80]), flush=True)
            continue
        out_rows, _ = plan.result_info()
        got = plan.fetch()
        if label == "Q5 shape":
            pair, cnt = np.unique(cols[0].astype(np.int64) << 32 | cols[1], return_counts=True)
            country = pair >> 32
            best = np.zeros(int(country.max()) + 1, np.int64)
            np.maximum.at(best, country, cnt)
            keep = cnt == best[country]
            want = sorted(zip((-cnt[keep]).tolist(), country[keep].tolist(), (pair[keep] & 0xFFFFFFFF).tolist()))
            v = plan.fetch_column_values(2)
            assert [(-int(c), int(a), int(b)) for a, b, c in zip(got[0], got[1], v["lo"])] == want
        else:
            avg, low = plan.fetch_column_values(1), plan.fetch_column_values(2)
            assert (avg["tag"] == abi.TV_FLOAT).all() and (low["tag"] == abi.TV_FLOAT).all() and len(set(low["lo"].tolist())) <= 1
            a, m = avg["lo"].astype(np.uint32).view(np.float32), low["lo"].astype(np.uint32).view(np.float32)
            assert (a > m * np.float32(1.5)).all() and 0 < out_rows < len(np.unique(cols[0]))
        ms, ks = runs[len(runs) // 2]
        rec = dict(shape="bsbm", products=n, query=label, join_rows=int(rows), result_rows=int(out_rows), first_ms=round(first, 4),
                   total_ms=spread(runs, ""), input_plan_ms=spread(in_runs, ""), aggregate_kernels_ms=spread(runs, "agg_"),
                   minmax_accumulate_ms=spread(runs, "agg_accum_minmax"), refine_ms=spread(runs, "refine"),
                   kernels={k[0]: dict(launches=int(k[1]), ms=round(k[2], 4), bytes=int(k[3])) for k in ks})
        records.append(rec)
        print("%-10s join rows %9d -> %7d rows: total %.3f ms (input plan %.3f), aggregate kernels %.3f, MIN / MAX accumulate %.3f, refine %.3f (first %.3f)" % (
            label, rows, out_rows, ms, rec["input_plan_ms"]["median"], rec["aggregate_kernels_ms"]["median"], rec["minmax_accumulate_ms"]["median"],
            rec["refine_ms"]["median"], first), flush=True)
        plan.close()
    st.close()


if __name__ == "__main__":
    synthetic()
    if BSBM:
        bsbm_cases(BSBM)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(dict(rows=N, steps=STEPS, records=records), f, indent=1)
