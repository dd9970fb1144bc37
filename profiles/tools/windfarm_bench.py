"""Wind Farm GroupedProduction, the tail of the plan on bound tables (windfarm.py has the whole plan): N data-point rows
{site label, turbine label, value, timestamp, bucket} through

  wide    ProjectionExec [minute_10, hour, day, month, year of ENC_TV(t)] + AggregateExec by (site, turbine, year, month, day, hour,
          minute_10), AVG(val): one EXTEND (extend_kernel, the VM instantiation with the date parts) and the 7-key aggregate, 2 id + 5
          value keys (agg_groups_wide_kernel, RDFGPU_PLAN_VALUE_KEYS);
  id3     the nearest plan without value keys: the same rows grouped by (site, turbine, bucket), the 10-minute bucket precomputed by the
          host as an object-id column — 3 id keys, agg_groups_kernel.

Rows: N (default 2^24) draws of (turbine, timestamp) from TURBINES turbines and one timestamp per minute of DAYS days; a third of the
timestamps each is written in UTC, at +05:30 and without a timezone (the local time decides the bucket).  Times are device-event kernel
times (rdfgpu_plan_enable_kernel_timing), the median over STEPS steady-state executions.  Checked: both plans give the same number of
groups — numpy's count of distinct (turbine, bucket) — and the same multiset of averages, bit for bit."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, xsd
from rdf_fusion_amd import windfarm as wf
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, YEAR, MONTH, DAY, HOURS

N = int(os.environ.get("N", str(1 << 24)))
STEPS = int(os.environ.get("STEPS", "7"))
TURBINES = int(os.environ.get("TURBINES", "64"))
DAYS = int(os.environ.get("DAYS", "30"))
OUT = os.environ.get("OUT", "")
OFFSETS = (0, 330, None)


def dev(cols):
    t = [torch.from_numpy(np.ascontiguousarray(c).view(np.int32)).cuda() for c in cols]
    return t, [x.data_ptr() for x in t]


def timed_plan(st, desc, ptrs, n):
    plan = st.plan(desc)
    plan.bind_table(0, ptrs, n)
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


def main():
    minutes = DAYS * 1440
    n_sites = max(1, TURBINES // 8)
    site_base, turb_base, val_base = 1, 1 + n_sites, 1 + n_sites + TURBINES
    t_base = val_base + 1000
    bucket_base = t_base + 3 * minutes
    n_ids = bucket_base + minutes // 10 + 200
    tv = np.zeros(n_ids, TV_DTYPE)
    tv["tag"][1:] = abi.TV_NAMED_NODE
    tv["lo"][1:] = np.arange(1, n_ids)
    tv["tag"][val_base:val_base + 1000] = abi.TV_INTEGER
    tv["lo"][val_base:val_base + 1000] = np.arange(1000)
    local0 = xsd.parse_date_time("2022-08-17T00:00:00")[0] // xsd.SCALE
    dec = np.zeros((3 * minutes, 2), np.int64)
    for k, off in enumerate(OFFSETS):                         # timestamp id t_base + k * minutes + m: local minute m, written with offset k
        for m in range(minutes):
            v = (local0 + 60 * m - 60 * (off or 0)) * xsd.SCALE
            j = k * minutes + m
            dec[j] = ((v & ((1 << 63) - 1)) | -(v & (1 << 63)), v >> 64)
            tv[t_base + j] = (j, 0 if off is None else 1, abi.TV_DATE_TIME, 0, off or 0)
    st = rf.GpuQuadStore()
    st.set_typed_values(tv, dec)
    rng = np.random.default_rng(1)
    turbine = rng.integers(0, TURBINES, N)
    stamp = rng.integers(0, 3 * minutes, N)
    site_c = (site_base + turbine // 8 % n_sites).astype(np.uint32)
    turb_c = (turb_base + turbine).astype(np.uint32)
    val_c = (val_base + rng.integers(0, 1000, N)).astype(np.uint32)
    t_c = (t_base + stamp).astype(np.uint32)
    bucket_c = (bucket_base + (stamp % minutes) // 10).astype(np.uint32)      # the host's precomputed 10-minute bucket of the local time
    keep, ptrs = dev([site_c, turb_c, val_c, t_c, bucket_c])
    groups = len(np.unique(turbine.astype(np.int64) << 32 | (stamp % minutes) // 10))

    pb = PlanBuilder()
    t = pb.table(0, 5, names=["site_label", "wtur_label", "val", "t", "bucket"])
    a = ENC_TV(col(3))
    x = pb.extend(t, [wf.minute_10(a), HOURS(a), DAY(a), MONTH(a), YEAR(a)], keep=[0, 1, 2], names=["minute_10", "hour", "day", "month", "year"])
    wide = pb.aggregate(x, [0, 1, 7, 6, 5, 4, 3], [(abi.AGG_AVG, 2)])
    w_first, w_ms, w_ks, w_plan = timed_plan(st, pb.build(wide, agg_columns=True, value_keys=True), ptrs, N)
    pb2 = PlanBuilder()
    id3 = pb2.aggregate(pb2.table(0, 5), [0, 1, 4], [(abi.AGG_AVG, 2)])
    i_first, i_ms, i_ks, i_plan = timed_plan(st, pb2.build(id3, agg_columns=True), ptrs, N)

    assert w_plan.result_info() == (groups, 8) and i_plan.result_info() == (groups, 4), (w_plan.result_info(), i_plan.result_info(), groups)
    avg = lambda plan, q: np.sort(plan.fetch_column_values(q)[["tag", "lo", "hi"]], order=["hi", "lo"])
    assert np.array_equal(avg(w_plan, 7), avg(i_plan, 3))
    assert any(k[0] == "rdfgpu::agg_groups_wide_kernel" for k in w_ks) and any(k[0] == "rdfgpu::agg_groups_kernel" for k in i_ks)
    table = lambda ks: {k[0]: dict(launches=int(k[1]), ms=round(k[2], 4), bytes=int(k[3])) for k in ks if k[1]}
    part = lambda ks, word: round(sum(k[2] for k in ks if word in k[0]), 4)
    rec = dict(rows=N, groups=groups, turbines=TURBINES, days=DAYS, steps=STEPS,
               wide=dict(median_ms=round(w_ms, 4), first_ms=round(w_first, 4), extend_ms=part(w_ks, "extend"), aggregate_ms=part(w_ks, "agg_"), kernels=table(w_ks)),
               id3=dict(median_ms=round(i_ms, 4), first_ms=round(i_first, 4), aggregate_ms=part(i_ks, "agg_"), kernels=table(i_ks)),
               ratio_wide_over_id3=round(w_ms / i_ms, 3))
    print("rows %d groups %d: 7-key plan %.3f ms (EXTEND %.3f + aggregate %.3f), 3-id-key plan %.3f ms, ratio %.2f" % (
        N, groups, w_ms, rec["wide"]["extend_ms"], rec["wide"]["aggregate_ms"], i_ms, w_ms / i_ms), flush=True)
    for name, ks in (("wide", w_ks), ("id3", i_ks)):
        for k in sorted(ks, key=lambda k: -k[2]):
            if k[1]:
                print("  %-5s %-60s %8.4f ms  %12d B" % (name, k[0][-60:], k[2], k[3]))
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(rec, f, indent=1)
    w_plan.close(); i_plan.close(); st.close()
    del keep


if __name__ == "__main__":
    main()
