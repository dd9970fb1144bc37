"""Computed columns (abi.NODE_EXTEND, PlanBuilder.extend / sparql_bind), modelled on agg_columns_bench.py.  Two workloads:

Q3-shaped (..Business Intelligence - Q3 (Execution Plan).snap) on BSBM (BSBM=n products; BSBM-100M is 285000): COUNT(?review) GROUP BY
?product hash-joined on ?product with COUNT(?offer) GROUP BY ?product, then `DIV(xsd:float(monthCount@1), monthBeforeCount@2) as ratio`.
BIND: sparql_bind of MUL(ENC_TV(a), ENC_TV(b)) over a bound table of ROWS rows (2^24) of small xsd:integer ids.

Times are device-event kernel times (rdfgpu_plan_enable_kernel_timing), the median over STEPS steady-state executions.  Per workload:
the step (all kernels), extend_kernel alone, and its share of the 8 TB/s roofline by its algorithmic bytes
(4 c_read + 16 n_enc_tv + 28 k) N — columns read, typed gathers / value loads, computed columns, rows.  Every result is checked
against numpy."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, quad_pattern, col, ENC_TV, MUL, DIV, xsd_float

STEPS = int(os.environ.get("STEPS", "7"))
BSBM = int(os.environ.get("BSBM", "285000"))
ROWS = int(os.environ.get("ROWS", str(1 << 24)))
OUT = os.environ.get("OUT", "")
PEAK_GBS = 8000.0
COUNT = abi.AGG_COUNT
records = []


def timed_plan(plan):
    """(first execution ms, median kernel ms, kernel stats of the median run)"""
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
    return first, med[0], med[1]


def report(label, first, ms, ks, plan, extra):
    ext = [k for k in ks if "extend_kernel" in k[0]]
    assert len(ext) == 1 and ext[0][1] == 1, ks
    _, _, ext_ms, ext_bytes, ext_rows = ext[0]
    gbs = ext_bytes / ext_ms / 1e6 if ext_ms else 0.0
    rows, _ = plan.result_info()
    rec = dict(workload=label, result_rows=int(rows), step_ms=round(ms, 4), extend_kernel_ms=round(ext_ms, 4), extend_rows=int(ext_rows),
               extend_bytes=int(ext_bytes), extend_gb_per_s=round(gbs, 1), share_of_8_tb_per_s=round(gbs / PEAK_GBS, 4), first_ms=round(first, 4),
               kernels={k[0]: dict(launches=int(k[1]), ms=round(k[2], 4), bytes=int(k[3])) for k in ks}, **extra)
    records.append(rec)
    print("%-10s %9d rows: step %.3f ms, extend_kernel %.4f ms over %d bytes = %.1f GB/s (%.1f %% of 8 TB/s; first %.3f)  %s" % (
        label, rows, ms, ext_ms, ext_bytes, gbs, 100 * gbs / PEAK_GBS, first, extra), flush=True)


def q3_shaped():
    ds = bsbm.generate(BSBM)
    st = rf.GpuQuadStore()
    st.extend(ds.g, ds.s, ds.p, ds.o)
    st.set_typed_values(ds.typed_values, ds.decimals)
    pr = ds.pred
    pb = PlanBuilder()
    reviews = pb.aggregate(pb.data_source(quad_pattern("review", pr["bsbm:reviewFor"], "product")), [1], [(COUNT, 0)])
    offers = pb.aggregate(pb.data_source(quad_pattern("offer", pr["bsbm:product"], "product")), [1], [(COUNT, 0)])
    joined = pb.projection(pb.hash_join(reviews, offers, [(0, 0)], projection=[0, 1, 3]), [0, 1, 2], names=["product", "monthCount", "monthBeforeCount"])
    root = pb.extend(joined, [DIV(xsd_float(ENC_TV(col(1))), ENC_TV(col(2)))], names=["ratio"])
    plan = st.plan(pb.build(root, agg_columns=True))
    first, ms, ks = timed_plan(plan)
    up, n_rev = np.unique(ds.o[ds.p == pr["bsbm:reviewFor"]], return_counts=True)
    uo, n_off = np.unique(ds.o[ds.p == pr["bsbm:product"]], return_counts=True)
    both = np.intersect1d(up, uo)
    want = n_rev[np.isin(up, both)].astype(np.float32) / n_off[np.isin(uo, both)].astype(np.float32)
    got = plan.fetch()
    order = np.argsort(got[0])
    assert plan.value_columns() == [1, 2, 3] and np.array_equal(got[0][order], both)
    ratio = plan.fetch_column_values(3)
    assert (ratio["tag"] == abi.TV_FLOAT).all() and np.array_equal((ratio["lo"][order] & 0xFFFFFFFF).astype(np.uint32), want.view(np.uint32))
    report("Q3-shaped", first, ms, ks, plan, dict(products=BSBM, groups=[len(up), len(uo)]))
    plan.close()
    st.close()


def bind_over_a_table():
    import torch
    tv = np.zeros(1001, TV_DTYPE)
    tv["tag"][1:] = abi.TV_INTEGER
    tv["lo"][1:] = np.arange(1, 1001)
    st = rf.GpuQuadStore()
    st.set_typed_values(tv, np.zeros((0, 2), np.int64))
    rng = np.random.default_rng(1)
    a, b = rng.integers(1, 1001, ROWS).astype(np.uint32), rng.integers(1, 1001, ROWS).astype(np.uint32)
    dev = [torch.from_numpy(c.view(np.int32)).cuda() for c in (a, b)]
    pb = PlanBuilder()
    root = pb.sparql_bind(pb.table(0, 2, ["a", "b"]), MUL(ENC_TV(col(0)), ENC_TV(col(1))), "product")
    plan = st.plan(pb.build(root, agg_columns=True))
    plan.bind_table(0, [t.data_ptr() for t in dev], ROWS)
    first, ms, ks = timed_plan(plan)
    prod = plan.fetch_column_values(2)
    assert (prod["tag"] == abi.TV_INTEGER).all() and np.array_equal(prod["lo"], a.astype(np.int64) * b.astype(np.int64))
    assert np.array_equal(plan.fetch()[2], np.arange(1, ROWS + 1, dtype=np.uint32))
    report("BIND", first, ms, ks, plan, dict(table_rows=ROWS))
    plan.close()
    st.close()
    del dev


if __name__ == "__main__":
    q3_shaped()
    bind_over_a_table()
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(dict(steps=STEPS, records=records), f, indent=1)
