"""The lexical cast (RDFGPU_EX_CAST_STRING under RDFGPU_EX_CAST_LEX), modelled on extend_bench.py.  Three workloads over bound tables of
ROWS rows (2^24) whose ids draw from PRICES distinct BSBM-shaped prices ("1234.56"):

lex_filter    FilterExec EBV(LT(xsd:float(xsd:string(ENC_TV(c))), 5000)) over `"1234.56"^^bsbm:USD` other literals: parsed per row
typed_filter  the same filter with xsd:float(ENC_TV(c)) over xsd:float literals of the same values (the generic VM too: forced)
q8_join       the BI Q8 shape: (product, price) hash-joined on product with AVG(value) GROUP BY product,
              filter=EBV(LT(xsd:float(xsd:string(ENC_TV(price))), avg))

Times are device-event kernel times (rdfgpu_plan_enable_kernel_timing), the median over STEPS steady-state executions: the step (all
kernels) and the kernel that hosts the cast, with its share of the 8 TB/s roofline by its algorithmic bytes — per row the 4-byte id, and
for the lexical form the 4-byte tag word, the 16-byte offset pair and the literal's bytes; for the typed form the 16-byte typed value;
4 bytes per row kept.  Every result is checked against numpy."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, EBV

STEPS = int(os.environ.get("STEPS", "7"))
ROWS = int(os.environ.get("ROWS", str(1 << 24)))
PRICES = int(os.environ.get("PRICES", "100000"))
PRODUCTS = int(os.environ.get("PRODUCTS", "65536"))
OUT = os.environ.get("OUT", "")
PEAK_GBS = 8000.0
records = []


def timed_plan(plan):
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


def report(label, first, ms, ks, host, algo_bytes, rows):
    hk = [k for k in ks if host in k[0]]
    assert hk, ks
    host_ms = sum(k[2] for k in hk)
    gbs = algo_bytes / host_ms / 1e6 if host_ms else 0.0
    rec = dict(workload=label, rows=ROWS, result_rows=int(rows), step_ms=round(ms, 4), host_kernel=hk[0][0], host_kernel_ms=round(host_ms, 4),
               algorithmic_bytes=int(algo_bytes), gb_per_s=round(gbs, 1), share_of_8_tb_per_s=round(gbs / PEAK_GBS, 4), first_ms=round(first, 4),
               ns_per_row=round(host_ms * 1e6 / ROWS, 3), kernels={k[0]: dict(launches=int(k[1]), ms=round(k[2], 4)) for k in ks})
    records.append(rec)
    print("%-13s step %.3f ms, %s %.3f ms (%.3f ns / row), %d algorithmic bytes = %.1f GB/s (%.2f %% of 8 TB/s), %d rows kept" % (
        label, ms, hk[0][0][:40], host_ms, host_ms * 1e6 / ROWS, algo_bytes, gbs, 100 * gbs / PEAK_GBS, rows), flush=True)


def main():
    import torch
    rng = np.random.default_rng(14)
    cents = rng.integers(500, 1_000_000, PRICES)                              # 5.00 .. 9999.99
    texts = ["%d.%02d" % (c // 100, c % 100) for c in cents]
    values = np.array([np.float32(t) for t in texts], np.float32)
    # ids 1 .. PRICES: the other literals; PRICES + 1 .. 2 PRICES: the xsd:float literals of the same values
    n_ids = 2 * PRICES + 1
    tv = np.zeros(n_ids, TV_DTYPE)
    tv["tag"][1:PRICES + 1] = abi.TV_OTHER
    tv["aux"][1:PRICES + 1] = 9
    tv["lo"][1:PRICES + 1] = np.arange(1, PRICES + 1)
    tv["tag"][PRICES + 1:] = abi.TV_FLOAT
    tv["lo"][PRICES + 1:] = values.view(np.uint32)
    lens = np.array([len(t) for t in texts], np.uint64)
    off = np.zeros(n_ids + 1, np.uint64)
    off[2:PRICES + 2] = np.cumsum(lens)
    off[PRICES + 2:] = off[PRICES + 1]
    st = rf.GpuQuadStore()
    st.set_typed_values(tv)
    st.set_strings(off, "".join(texts).encode())
    pick = rng.integers(0, PRICES, ROWS)
    lex_ids, typed_ids = (pick + 1).astype(np.uint32), (pick + 1 + PRICES).astype(np.uint32)
    rowid = np.arange(ROWS, dtype=np.uint32)
    mean_len = float(lens[pick].mean())
    bound = np.float32(5000.0)
    keep_mask = values[pick] < bound

    def dev(cols):
        ts = [torch.from_numpy(np.ascontiguousarray(c).view(np.int32)).cuda() for c in cols]
        return ts, [t.data_ptr() for t in ts]

    lex = lambda c: P.xsd_float(P.xsd_string(ENC_TV(col(c))), lexical=True)
    for label, ids, cast, per_row in (("lex_filter", lex_ids, lex(0), 4 + 4 + 16 + mean_len), ("typed_filter", typed_ids, P.xsd_float(ENC_TV(col(0))), 4 + 16)):
        pb = PlanBuilder()
        st.set_option("FORCE_GENERIC_VM", 1)        # (the typed form has no specialised shape either way: both run in filter_kernel<0>)
        plan = st.plan(pb.build(pb.filter(pb.table(0, 2), EBV(P.LT(cast, P.float32(float(bound)))), projection=[1])))
        st.set_option("FORCE_GENERIC_VM", 0)
        keep, ptrs = dev([ids, rowid])
        plan.bind_table(0, ptrs, ROWS)
        first, ms, ks = timed_plan(plan)
        got = np.sort(plan.fetch()[0])
        assert np.array_equal(got, rowid[keep_mask]), label
        report(label, first, ms, ks, "filter_kernel", ROWS * per_row + 4 * len(got), len(got))
    # the Q8 join shape
    product = rng.integers(1, PRODUCTS + 1, ROWS).astype(np.uint32)
    avg_pick = rng.integers(0, PRICES, PRODUCTS)
    rkey = np.arange(1, PRODUCTS + 1, dtype=np.uint32)
    rval = (avg_pick + 1 + PRICES).astype(np.uint32)
    pb = PlanBuilder()
    left, right = pb.table(0, 2), pb.table(1, 2)
    agg = pb.aggregate(right, [0], [(abi.AGG_AVG, 1)])
    root = pb.hash_join(left, agg, on=[(0, 0)], filter=EBV(P.LT(lex(1), ENC_TV(col(3)))), projection=[0, 1])
    plan = st.plan(pb.build(root, agg_columns=True))
    k1, p1 = dev([product, lex_ids])
    k2, p2 = dev([rkey, rval])
    plan.bind_table(0, p1, ROWS)
    plan.bind_table(1, p2, PRODUCTS)
    first, ms, ks = timed_plan(plan)
    want = int((values[pick] < values[avg_pick][product - 1]).sum())
    n, _ = plan.result_info()
    assert n == want, (n, want)
    host = max((k for k in ks if "join" in k[0]), key=lambda k: k[2])[0]
    report("q8_join", first, ms, ks, host, ROWS * (8 + 4 + 16 + mean_len + 24) + 8 * n, n)
    if OUT:
        with open(OUT, "w") as f:
            json.dump(dict(rows=ROWS, prices=PRICES, products=PRODUCTS, steps=STEPS, mean_literal_bytes=round(mean_len, 3), records=records), f, indent=1)


if __name__ == "__main__":
    main()
