"""Plans that continue above their aggregates (abi.PLAN_AGG_COLUMNS) on BSBM (BSBM=n products; BSBM-100M is 285000), modelled on
aggregate_bench.py.

Q3-shaped (..Business Intelligence - Q3 (Execution Plan).snap): COUNT(?review) GROUP BY ?product, `FilterExec: EBV(GT(count, K))` (a
HAVING), hash-joined on ?product with COUNT(?offer) GROUP BY ?product.
Q6-shaped (..Q6 (Execution Plan).snap): AVG(?rating1) GROUP BY ?reviewer cross-joined with the zero-key AVG(?rating1), then
`FilterExec: EBV(GT(avg, MUL(xsd:double(avg_all), 1.5)))` (the global average has 18 fraction digits: a decimal product with 1.5 would be
Decimal::checked_mul's error value, so it is cast first).

Times are device-event kernel times (rdfgpu_plan_enable_kernel_timing), the median over STEPS steady-state executions; the first
execution of a fresh plan is reported on its own.  Per plan: the time of the aggregate kernels, of the generic VM filter over the value
columns, and of everything else (scans and joins).  Every result is checked against numpy over the store's own triples."""
import json
import os
import sys
from fractions import Fraction

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
from rdf_fusion_amd.plan import PlanBuilder, quad_pattern, col, integer, double, EBV, GT, MUL, ENC_TV, xsd_double

STEPS = int(os.environ.get("STEPS", "7"))
BSBM = int(os.environ.get("BSBM", "285000"))
K = int(os.environ.get("K", "9"))
OUT = os.environ.get("OUT", "")
STAR, SUM, AVG, COUNT = abi.AGG_COUNT_STAR, abi.AGG_SUM, abi.AGG_AVG, abi.AGG_COUNT
records = []


def timed_plan(st, desc):
    """(first execution ms, median kernel ms, kernel stats of the median run, plan)"""
    plan = st.plan(desc)
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


def report(label, first, ms, ks, plan, extra):
    agg_ms = sum(k[2] for k in ks if "agg_" in k[0])
    vm_ms = sum(k[2] for k in ks if "filter_kernel<0>" in k[0])
    rows, _ = plan.result_info()
    rec = dict(query=label, products=BSBM, result_rows=int(rows), median_ms=round(ms, 4), agg_kernels_ms=round(agg_ms, 4),
               vm_filter_ms=round(vm_ms, 4), other_kernels_ms=round(ms - agg_ms - vm_ms, 4), first_ms=round(first, 4),
               kernels={k[0]: dict(launches=int(k[1]), ms=round(k[2], 4), bytes=int(k[3])) for k in ks}, **extra)
    records.append(rec)
    print("%-10s %9d rows: %.3f ms (aggregates %.3f, VM filter %.3f, scans and joins %.3f; first %.3f)  %s" % (
        label, rows, ms, agg_ms, vm_ms, ms - agg_ms - vm_ms, first, extra), flush=True)


def main():
    ds = bsbm.generate(BSBM)
    st = rf.GpuQuadStore()
    st.extend(ds.g, ds.s, ds.p, ds.o)
    st.set_typed_values(ds.typed_values, ds.decimals)
    pr = ds.pred
    pairs = lambda p: (ds.s[ds.p == pr[p]], ds.o[ds.p == pr[p]])

    # ---- Q3-shaped -------------------------------------------------------------------------------
    pb = PlanBuilder()
    reviews = pb.aggregate(pb.data_source(quad_pattern("review", pr["bsbm:reviewFor"], "product")), [1], [(COUNT, 0)])
    many = pb.sparql_having(reviews, EBV(GT(ENC_TV(col(1)), integer(K))))
    offers = pb.aggregate(pb.data_source(quad_pattern("offer", pr["bsbm:product"], "product")), [1], [(COUNT, 0)])
    root = pb.hash_join(many, offers, [(0, 0)], projection=[0, 1, 3])
    first, ms, ks, plan = timed_plan(st, pb.build(root, agg_columns=True))
    _, rp = pairs("bsbm:reviewFor")
    _, op = pairs("bsbm:product")
    up, n_rev = np.unique(rp, return_counts=True)
    uo, n_off = np.unique(op, return_counts=True)
    keep = up[n_rev > K]
    keep = keep[np.isin(keep, uo)]
    got = plan.fetch()
    order = np.argsort(got[0])
    assert plan.value_columns() == [1, 2] and np.array_equal(got[0][order], keep)
    assert np.array_equal(plan.fetch_column_values(1)["lo"][order], n_rev[np.isin(up, keep)])
    assert np.array_equal(plan.fetch_column_values(2)["lo"][order], n_off[np.isin(uo, keep)])
    report("Q3-shaped", first, ms, ks, plan, dict(review_rows=len(rp), offer_rows=len(op), groups=[len(up), len(uo)], having_k=K))
    plan.close()

    # ---- Q6-shaped -------------------------------------------------------------------------------
    pb = PlanBuilder()
    rated = pb.hash_join(pb.data_source(quad_pattern("review", pr["rev:reviewer"], "reviewer")),
                         pb.data_source(quad_pattern("review", pr["bsbm:rating1"], "rating")), [(0, 0)], projection=[1, 3])
    per = pb.aggregate(rated, [0], [(AVG, 1)])
    all_ = pb.aggregate(pb.data_source(quad_pattern("review", pr["bsbm:rating1"], "rating")), [], [(AVG, 1)])
    root = pb.sparql_having(pb.cross_join(per, all_), EBV(GT(ENC_TV(col(1)), MUL(xsd_double(ENC_TV(col(2))), double(1.5)))))
    first, ms, ks, plan = timed_plan(st, pb.build(root, agg_columns=True))
    rs, who = pairs("rev:reviewer")
    rs2, rating = pairs("bsbm:rating1")
    value = ds.typed_values["lo"][rating].astype(np.int64)
    reviewer_of = dict(zip(rs.tolist(), who.tolist()))
    w = np.asarray([reviewer_of[r] for r in rs2.tolist()], np.uint32)
    uw, inv, cnt = np.unique(w, return_inverse=True, return_counts=True)
    sums = np.bincount(inv, weights=value.astype(np.float64)).astype(np.int64)
    limit = float(Fraction(int(value.sum()), len(value))) * 1.5
    want = uw[sums / cnt > limit]
    got = plan.fetch()
    assert plan.value_columns() == [1, 2] and np.array_equal(np.sort(got[0]), want)
    report("Q6-shaped", first, ms, ks, plan, dict(rating_rows=len(rs2), reviewers=len(uw), global_avg_times_1_5=round(limit, 6)))
    plan.close()
    st.close()


if __name__ == "__main__":
    main()
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(dict(steps=STEPS, records=records), f, indent=1)
