"""SortExec (abi.NODE_SORT, PlanBuilder.sort / sparql_order_by), modelled on extend_bench.py.  One workload, the shape that ends the BSBM
Business Intelligence plans: over a bound table of ROWS rows (2^20) a computed column MUL(ENC_TV(a), ENC_TV(b)) (xsd:integer products,
many of them equal), then ORDER BY (value DESC, id ASC) — with fetch = 10 (`SortExec: TopK(fetch=10)`) and without.

Times are device-event kernel times (rdfgpu_plan_enable_kernel_timing) per kernel class of sort.hip, the median over STEPS steady-state
executions after WARMUP unmeasured ones, with the spread (min .. max of the sort's total).  Beside them two yardsticks, neither a pass mark:
  roofline   the operator's compulsory bytes at 8 TB/s:  N (4 k_id + 28 k_value) + 8 c N_out  — every key entry (and a value key's 24-byte
             value) read once, every output cell read and written once; N rows, N_out output rows, c output columns;
  torch.sort of ROWS int64 keys (one word per key), device-event time, the same warm-up and median.
Every result is checked against numpy."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, MUL

STEPS = int(os.environ.get("STEPS", "15"))
WARMUP = int(os.environ.get("WARMUP", "3"))
ROWS = int(os.environ.get("ROWS", str(1 << 20)))
OUT = os.environ.get("OUT", "")
PEAK_BYTES_PER_MS = 8e9          # 8 TB/s
records = []


def sort_times(plan):
    """per steady-state execution: {kernel class: ms} of the sort's kernels"""
    for _ in range(WARMUP):
        plan.execute()
    plan.enable_kernel_timing(True)
    plan.execute()                # the first timed execution creates the events
    runs = []
    for _ in range(STEPS):
        plan.execute()
        runs.append({k[0]: (k[1], k[2]) for k in plan.kernel_stats() if "sort_" in k[0]})
    return runs


def torch_sort_ms(torch, n):
    keys = torch.from_numpy(np.random.default_rng(2).integers(0, 1 << 62, n)).cuda()
    for _ in range(WARMUP):
        torch.sort(keys)
    ms = []
    for _ in range(STEPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.sort(keys)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)


def main():
    import torch
    tv = np.zeros(1001, TV_DTYPE)
    tv["tag"][1:] = abi.TV_INTEGER
    tv["lo"][1:] = np.arange(1, 1001)
    st = rf.GpuQuadStore()
    st.set_typed_values(tv, np.zeros((0, 2), np.int64))
    rng = np.random.default_rng(1)
    a, b = rng.integers(1, 1001, ROWS).astype(np.uint32), rng.integers(1, 1001, ROWS).astype(np.uint32)
    ids = rng.permutation(ROWS).astype(np.uint32) + 1
    dev = [torch.from_numpy(c.view(np.int32)).cuda() for c in (a, b, ids)]
    prod = a.astype(np.int64) * b.astype(np.int64)
    want = np.lexsort((ids, -prod))
    torch_ms = torch_sort_ms(torch, ROWS)
    for fetch in (10, None):
        pb = PlanBuilder()
        e = pb.sparql_bind(pb.table(0, 3, ["a", "b", "id"]), MUL(ENC_TV(col(0)), ENC_TV(col(1))), "product")
        root = pb.sparql_order_by(e, [(3, True), (2, False)], limit=fetch)
        plan = st.plan(pb.build(root, agg_columns=True))
        plan.bind_table(0, [t.data_ptr() for t in dev], ROWS)
        runs = sort_times(plan)
        n_out = plan.result_info()[0]
        assert n_out == (fetch or ROWS) and np.array_equal(plan.fetch()[2], ids[want[:n_out]])
        assert np.array_equal(plan.fetch_column_values(3)["lo"], prod[want[:n_out]])
        totals = sorted(sum(ms for _, ms in r.values()) for r in runs)
        med = sorted(runs, key=lambda r: sum(ms for _, ms in r.values()))[len(runs) // 2]
        bytes_ = ROWS * (4 * 1 + 28 * 1) + 8 * 4 * n_out
        rec = dict(workload="value DESC, id ASC", rows=ROWS, fetch=fetch or 0, result_rows=int(n_out), sort_ms=round(totals[len(totals) // 2], 4),
                   sort_ms_min=round(totals[0], 4), sort_ms_max=round(totals[-1], 4),
                   kernels={k: dict(launches=int(v[0]), ms=round(v[1], 4)) for k, v in med.items()},
                   compulsory_bytes=int(bytes_), roofline_ms=round(bytes_ / PEAK_BYTES_PER_MS, 5),
                   torch_sort_int64_ms=round(torch_ms[len(torch_ms) // 2], 4), torch_sort_int64_ms_min=round(torch_ms[0], 4), torch_sort_int64_ms_max=round(torch_ms[-1], 4))
        records.append(rec)
        print(json.dumps(rec), flush=True)
        plan.close()
    st.close()
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(dict(steps=STEPS, warmup=WARMUP, records=records), f, indent=1)


if __name__ == "__main__":
    main()
