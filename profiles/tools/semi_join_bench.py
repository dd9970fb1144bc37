"""LeftSemi / LeftAnti joins (semi_join.hip) against the inner join on the same shapes.

Bound tables, the shapes of join_micro.py: 32 M left (probe) rows {key, payload} against right inputs of 1 K, 20 K and 1 M rows
{key, payload}, hit rates 0.1 and 1.0.  Per shape: the semi and the anti join projected onto the left payload, and the inner
join with the same output column (HashJoinExec, the engine choosing its build side).  Times are device-event kernel times
(rdfgpu_plan_enable_kernel_timing), the median over STEPS steady-state executions; the first execution of a fresh plan is
reported on its own (elapsed_compute_ms).  Roofline fraction: DESIGN §6's formula, compulsory bytes = 4·(k + c)·N_probe +
4·c_out·N_out + the build's 4·k·N_build, over 8 TB/s.  Every timed result is checked against numpy: the row count and two
power sums of the (distinct) payload column.

BSBM (BSBM=n products, 0 = skip; BSBM-100M is 285000): offers whose product has / lacks a feature (a semi / anti join of a
store slice against a small slice), offers whose product has / lacks a review (against a 10-per-product slice), and the BSBM
explore Q3 shape NOT EXISTS against its OPTIONAL + FILTER(!BOUND) form.  Checked against each other (anti + semi = all rows,
NOT EXISTS = OPTIONAL + !BOUND)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
from rdf_fusion_amd.plan import PlanBuilder, quad_pattern, col, NOT, BOUND

NP = int(os.environ.get("NP", str(32 << 20)))
STEPS = int(os.environ.get("STEPS", "7"))
OUT = os.environ.get("OUT", "")
ROOF = 8e12
records = []


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


def power_sums(x):
    x = x.astype(np.uint64)
    return int(x.sum()), int((x * x).sum())


def check(plan, want_payload):
    n, _ = plan.result_info()
    got = plan.fetch()[0][:n]
    assert n == len(want_payload), (n, len(want_payload))
    assert power_sums(got) == power_sums(want_payload)
    return n


def bound_tables():
    st = rf.GpuQuadStore()
    rng = np.random.default_rng(1)
    for nb in [int(x) for x in os.environ.get("NB", "1000,20000,1000000").split(",")]:
        for hit in (0.1, 1.0):
            bk = rng.permutation(np.arange(1, nb + 1, dtype=np.uint32))
            B = [bk, (bk * 7 + 1).astype(np.uint32)]
            pk = rng.integers(1, int(nb / hit) + 1, NP).astype(np.uint32)
            P = [pk, np.arange(1, NP + 1, dtype=np.uint32)]
            kp, pp = dev(P); kb, pbp = dev(B)
            tables = [(pp, NP), (pbp, nb)]
            hit_mask = pk <= nb
            for name, jt in (("semi", abi.JOIN_LEFT_SEMI), ("anti", abi.JOIN_LEFT_ANTI), ("inner", abi.JOIN_INNER)):
                pb = PlanBuilder()
                desc = pb.build(pb.hash_join(pb.table(0, 2), pb.table(1, 2), on=[(0, 0)], join_type=jt, projection=[1]))
                first, ms, ks, plan = timed_plan(st, desc, tables)
                want = P[1][~hit_mask] if jt == abi.JOIN_LEFT_ANTI else P[1][hit_mask]
                n_out = check(plan, want)
                byt = 4 * NP + 4 * n_out + 4 * nb
                top = max(ks, key=lambda k: k[2])
                rec = dict(shape="bound", join=name, build_rows=nb, hit=hit, probe_rows=NP, out_rows=n_out, median_ms=round(ms, 4),
                           first_ms=round(first, 4), roofline=round(byt / (ms * 1e-3) / ROOF, 3), top_kernel=top[0], top_ms=round(top[2], 4),
                           kernels={k[0]: round(k[2], 4) for k in ks})
                records.append(rec)
                print("build %8d hit %.1f %-5s %8.3f ms (first %8.3f)  %.3f of 8 TB/s  out %9d  top %s %.3f ms" % (
                    nb, hit, name, ms, first, rec["roofline"], n_out, top[0][-44:], top[2]), flush=True)
                plan.close()
            del kp, kb
    st.close()


def bsbm_store(n):
    ds = bsbm.generate(n)
    st = rf.GpuQuadStore()
    st.extend(ds.g, ds.s, ds.p, ds.o)
    st.set_typed_values(ds.typed_values, ds.decimals)
    return ds, st


def bsbm_cases(n):
    ds, st = bsbm_store(n)
    pr = ds.pred
    pf = pr["bsbm:productFeature"]
    f, c = np.unique(ds.o[ds.p == pf], return_counts=True)
    f1, f2 = (int(x) for x in f[np.argsort(-c)][:2])

    def offers(pb):
        return pb.data_source(quad_pattern("offer", pr["bsbm:product"], "product"))

    def run(label, desc):
        first, ms, ks, plan = timed_plan(st, desc, [])
        n = plan.result_info()[0]
        top = max(ks, key=lambda k: k[2]) if ks else ("(no launch: a zero-copy slice)", 0, 0.0)
        records.append(dict(shape="bsbm%d" % n_products, case=label, out_rows=n, median_ms=round(ms, 4), first_ms=round(first, 4),
                            top_kernel=top[0], kernels={k[0]: round(k[2], 4) for k in ks}))
        print("bsbm %-44s %8.3f ms (first %8.3f)  out %9d  top %s %.3f ms" % (label, ms, first, n, top[0][-44:], top[2]), flush=True)
        plan.close()
        return n
    n_products = n
    counts = {}
    for rname, right in (("feature", lambda pb: pb.data_source(quad_pattern("product", pf, f1))),
                         ("review", lambda pb: pb.data_source(quad_pattern("review", pr["bsbm:reviewFor"], "product")))):
        for jt, nm in ((abi.JOIN_LEFT_SEMI, "has"), (abi.JOIN_LEFT_ANTI, "lacks")):
            pb = PlanBuilder()
            l, r = offers(pb), right(pb)
            counts[(rname, nm)] = run("offers whose product %s a %s" % (nm, rname), pb.build(pb.sparql_exists(l, r, negate=nm == "lacks")))
        pb = PlanBuilder()
        all_offers = run("all offers", pb.build(offers(pb)))
        assert counts[(rname, "has")] + counts[(rname, "lacks")] == all_offers
    # explore Q3 shape: products with feature F1 and a label, but not feature F2
    def q3_left(pb):
        return pb.sparql_join(pb.data_source(quad_pattern("product", pf, f1)), pb.data_source(quad_pattern("product", pr["rdfs:label"], "label")))
    pb = PlanBuilder()
    l = q3_left(pb)
    n_ne = run("Q3 shape: NOT EXISTS", pb.build(pb.sparql_exists(l, pb.data_source(quad_pattern("product", pf, f2)), negate=True)))
    pb = PlanBuilder()
    l = q3_left(pb)
    w = pb.width[l]
    opt = pb.filter(pb.hash_join(l, pb.data_source(quad_pattern("product", pf, f2)), on=[(0, 0)], join_type=abi.JOIN_LEFT), NOT(BOUND(col(w))),
                    projection=list(range(w)))
    n_opt = run("Q3 shape: OPTIONAL + FILTER(!BOUND)", pb.build(opt))
    assert n_ne == n_opt, (n_ne, n_opt)
    st.close()


if __name__ == "__main__":
    print("kernel_source_sha16", rf.kernel_source_sha16(), flush=True)
    if os.environ.get("SKIP_BOUND", "") != "1":
        bound_tables()
    n = int(os.environ.get("BSBM", "285000"))
    if n:
        bsbm_cases(n)
    if OUT:
        with open(OUT, "w") as fh:
            json.dump(dict(kernel_source_sha16=rf.kernel_source_sha16(), probe_rows=NP, steps=STEPS, records=records), fh, indent=1)
