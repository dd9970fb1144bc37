"""SUM over an expression against SUM over a column (aggregate.hip: agg_accum_expr_kernel against agg_accum_kernel).

N (default 2^24) bound rows {key, a, b} with 1 024 groups; for integer, decimal and double value columns the device-event kernel time of
`SUM(MUL(ENC_TV(a), ENC_TV(b)))` and of `SUM(a)`, the median over STEPS steady-state executions, and their ratio.  There is no target:
the ratio is what an expression input costs over the column input.  Every timed result is checked: integer and decimal sums exactly
(over the per-group counts of the 100 x 100 value pairs), double sums to 1e-9 relative.  OUT=<file> writes JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, MUL, ENC_TV, col

N = int(os.environ.get("N", str(1 << 24)))
STEPS = int(os.environ.get("STEPS", "7"))
GROUPS = 1024
OUT = os.environ.get("OUT", "")


def median_ms(st, aggs, ptrs):
    pb = PlanBuilder()
    plan = st.plan(pb.build(pb.aggregate(pb.table(0, 3), [0], aggs)))
    plan.bind_table(0, ptrs, N)
    plan.execute()
    plan.enable_kernel_timing(True)
    runs = []
    for _ in range(STEPS):
        plan.execute()
        runs.append(sum(k[2] for k in plan.kernel_stats()))
    return sorted(runs)[len(runs) // 2], plan


def main():
    st = rf.GpuQuadStore()
    tv = np.zeros(301, TV_DTYPE)        # ids 1..100 xsd:integer 1..100, 101..200 xsd:decimal k / 4 (k = 1..100), 201..300 xsd:double 0.37 k
    tv["tag"][1:101], tv["lo"][1:101] = abi.TV_INTEGER, np.arange(1, 101)
    tv["tag"][101:201], tv["lo"][101:201] = abi.TV_DECIMAL, np.arange(100)
    tv["tag"][201:], tv["lo"][201:] = abi.TV_DOUBLE, (np.arange(1, 101).astype(np.float64) * np.float64(0.37)).view(np.int64)
    scaled = [k * (10 ** 18 // 4) for k in range(1, 101)]        # Python integers: 25 x 10^18 does not fit an int64
    s64 = lambda x: x - (1 << 64) if x >= 1 << 63 else x
    dec = np.array([[s64(v & ((1 << 64) - 1)), s64(v >> 64)] for v in scaled], np.int64)
    st.set_typed_values(tv, dec)
    rng = np.random.default_rng(1)
    key = (rng.integers(0, GROUPS, N) + 1).astype(np.uint32)
    records = []
    for kind, base in (("integer", 1), ("decimal", 101), ("double", 201)):
        a, b = (rng.integers(base, base + 100, N).astype(np.uint32) for _ in range(2))
        keep = [torch.from_numpy(c.view(np.int32)).cuda() for c in (key, a, b)]
        ptrs = [t.data_ptr() for t in keep]
        col_ms, _ = median_ms(st, [(abi.AGG_SUM, 1)], ptrs)
        expr_ms, plan = median_ms(st, [(abi.AGG_SUM, MUL(ENC_TV(col(1)), ENC_TV(col(2))))], ptrs)
        # per group, how often each (a, b) pair of the 100 x 100 occurs: the expected sum is a sum over at most 10^4 products
        uk, inv = np.unique(key, return_inverse=True)
        pair = (inv.astype(np.int64) * 100 + (a - base)) * 100 + (b - base)
        counts = np.bincount(pair, minlength=len(uk) * 10000).reshape(len(uk), 100, 100)
        order = np.argsort(plan.fetch()[0])
        got = plan.fetch_aggregate(0)[order]
        kk = np.arange(1, 101, dtype=np.int64)
        sum_kk = (counts * np.outer(kk, kk)).sum(axis=(1, 2))            # per group: sum of k_a * k_b, below 2^63
        if kind == "integer":
            assert (got["tag"] == abi.TV_INTEGER).all() and np.array_equal(got["lo"], sum_kk)
        elif kind == "decimal":      # (k_a / 4)(k_b / 4) = k_a k_b / 16: exact in 18 fraction digits
            have = [(int(h) << 64) | (int(l) & ((1 << 64) - 1)) for l, h in zip(got["lo"], got["hi"])]
            assert (got["tag"] == abi.TV_DECIMAL).all() and have == [int(x) * (10 ** 18 // 16) for x in sum_kk]
        else:
            dv = kk.astype(np.float64) * np.float64(0.37)
            want = (counts * np.outer(dv, dv)).sum(axis=(1, 2))
            assert (got["tag"] == abi.TV_DOUBLE).all() and np.allclose(got["lo"].view(np.float64), want, rtol=1e-9, atol=0)
        rec = {"kind": kind, "rows": N, "groups": GROUPS, "sum_column_ms": col_ms, "sum_mul_expr_ms": expr_ms, "ratio": expr_ms / col_ms}
        print(json.dumps(rec))
        records.append(rec)
        del keep
    if OUT:
        json.dump(records, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()
