"""The LeftMark join (semi_join.hip: mark_join_kernel) beside the semi and the anti join on the same inputs, and a FILTER with IS_LITERAL, IF
and COALESCE beside the same scan with EBV(GT(ENC_TV, lit)) in the generic VM.

Bound tables, the shapes of semi_join_bench.py: 32 M left (probe) rows {key, payload} against right inputs of 1 K, 20 K and 1 M rows {key,
payload}, hit rates 0.1 and 1.0.  Per shape: the semi and the anti join projected onto the left payload, and the mark join projected onto
{payload, mark}.  The filters scan a bound table of 32 M rows {id, row number} over a typed table of 4096 ids (integers, every eighth a simple
string, every 64th an IRI).  Times are device-event kernel times (rdfgpu_plan_enable_kernel_timing), the median over STEPS steady-state
executions, with the fastest and the slowest beside it (the run-to-run spread).  Every timed result is checked against numpy.

RDF_TREE=<a checkout of another commit, built> runs what that commit has — the semi join, the anti join and the comparison filter — with
that commit's library: the times a change to semi_join.hip or to the VM is held against."""
import json
import os
import sys

TREE = os.environ.get("RDF_TREE", os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, TREE)
import numpy as np
import torch

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, EBV
from rdf_fusion_amd.engine import TV_DTYPE

NP = int(os.environ.get("NP", str(32 << 20)))
STEPS = int(os.environ.get("STEPS", "7"))
OUT = os.environ.get("OUT", "")
HAS_FORMS = hasattr(abi, "JOIN_LEFT_MARK")
records = []


def dev(cols):
    t = [torch.from_numpy(np.ascontiguousarray(c).view(np.int32)).cuda() for c in cols]
    return t, [x.data_ptr() for x in t]


def timed_plan(st, desc, tables, options=()):
    for name in options:          # (a predicate's kernel shape is chosen when the plan is compiled: the store's option, for this plan only)
        st.set_option(name, 1)
    plan = st.plan(desc)
    for name in options:
        st.set_option(name, 0)
    for slot, (ptrs, n) in enumerate(tables):
        plan.bind_table(slot, ptrs, n)
    plan.execute()
    plan.enable_kernel_timing(True)
    runs = []
    for _ in range(STEPS):
        plan.execute()
        ks = plan.kernel_stats()
        runs.append((sum(k[2] for k in ks), ks))
    runs.sort(key=lambda r: r[0])
    return runs[len(runs) // 2][0], runs[0][0], runs[-1][0], runs[len(runs) // 2][1], plan


def power_sums(x):
    x = x.astype(np.uint64)
    return int(x.sum()), int((x * x).sum())


def joins():
    st = rf.GpuQuadStore()
    rng = np.random.default_rng(1)
    kinds = [("semi", abi.JOIN_LEFT_SEMI), ("anti", abi.JOIN_LEFT_ANTI)] + ([("mark", abi.JOIN_LEFT_MARK)] if HAS_FORMS else [])
    for nb in [int(x) for x in os.environ.get("NB", "1000,20000,1000000").split(",")]:
        for hit in (0.1, 1.0):
            bk = rng.permutation(np.arange(1, nb + 1, dtype=np.uint32))
            B = [bk, (bk * 7 + 1).astype(np.uint32)]
            pk = rng.integers(1, int(nb / hit) + 1, NP).astype(np.uint32)
            Pc = [pk, np.arange(1, NP + 1, dtype=np.uint32)]
            kp, pp = dev(Pc); kb, pbp = dev(B)
            tables = [(pp, NP), (pbp, nb)]
            hit_mask = pk <= nb
            for name, jt in kinds:
                pb = PlanBuilder()
                mark = name == "mark"
                j = pb.hash_join(pb.table(0, 2), pb.table(1, 2), on=[(0, 0)], join_type=jt, projection=[1, 2] if mark else [1])
                ms, lo, hi, ks, plan = timed_plan(st, pb.build(j, agg_columns=True) if mark else pb.build(j), tables)
                n, _ = plan.result_info()
                got = plan.fetch()
                if mark:                                  # every left row, in order, entry 2 where the key has a partner
                    assert n == NP and np.array_equal(got[0][:n], Pc[1]) and np.array_equal(got[1][:n] == 2, hit_mask) and int(got[1][:n].min()) >= 1
                else:
                    want = Pc[1][~hit_mask] if jt == abi.JOIN_LEFT_ANTI else Pc[1][hit_mask]
                    assert n == len(want) and power_sums(got[0][:n]) == power_sums(want)
                rec = dict(shape="join", join=name, build_rows=nb, hit=hit, probe_rows=NP, out_rows=n, median_ms=round(ms, 4), min_ms=round(lo, 4),
                           max_ms=round(hi, 4), kernels={k[0]: round(k[2], 4) for k in ks})
                records.append(rec)
                print("build %8d hit %.1f %-5s %8.3f ms (%.3f .. %.3f)  out %9d" % (nb, hit, name, ms, lo, hi, n), flush=True)
                plan.close()
            del kp, kb
    st.close()


def filters():
    n_ids = 4096
    tv = np.zeros(n_ids, TV_DTYPE)
    for i in range(1, n_ids):
        tv[i] = (i, 0, abi.TV_NAMED_NODE, 0, 0) if i % 64 == 0 else (i, 0, abi.TV_STRING, 0, 0) if i % 8 == 0 else (i, 0, abi.TV_INTEGER, 0, 0)
    st = rf.GpuQuadStore()
    st.set_typed_values(tv)
    rng = np.random.default_rng(2)
    ids = rng.integers(0, n_ids + 64, NP).astype(np.uint32)                 # id 0 and ids beyond the table: the null value
    keep, ptrs = dev([ids, np.arange(1, NP + 1, dtype=np.uint32)])
    known = (ids > 0) & (ids < n_ids)
    iri, string = known & (ids % 64 == 0), known & (ids % 8 == 0) & (ids % 64 != 0)
    integer = known & ~iri & ~string
    x = ENC_TV(col(0))
    cases = [("EBV(GT(ENC_TV(x), 2000)) in the generic VM", EBV(P.GT(x, P.integer(2000))), integer & (ids > 2000), ("FORCE_GENERIC_VM",))]
    if HAS_FORMS:
        cases += [
            ("EBV(isLITERAL(ENC_TV(x)))", EBV(P.IS_LITERAL(x)), integer | string, ()),
            ("EBV(IF(isNUMERIC(x), GT(x, 2000), isIRI(x)))", EBV(P.IF(P.IS_NUMERIC(x), P.GT(x, P.integer(2000)), P.IS_IRI(x))), (integer & (ids > 2000)) | iri, ()),
            ("EBV(GT(COALESCE(x, 4000), 2000))", EBV(P.GT(P.COALESCE(x, P.integer(4000)), P.integer(2000))), (integer & (ids > 2000)) | ~known, ()),
            ("EBV(IF(isLITERAL(x), GT(COALESCE(x, 0), 2000), false))", EBV(P.IF(P.IS_LITERAL(x), P.GT(P.COALESCE(x, P.integer(0)), P.integer(2000)), P.boolean(False))),
             integer & (ids > 2000), ()),
        ]
    for name, pred, mask, options in cases:
        pb = PlanBuilder()
        ms, lo, hi, ks, plan = timed_plan(st, pb.build(pb.filter(pb.table(0, 2), pred, projection=[1])), [(ptrs, NP)], options)
        n, _ = plan.result_info()
        want = np.flatnonzero(mask).astype(np.uint32) + 1
        assert n == len(want) and power_sums(plan.fetch()[0][:n]) == power_sums(want), name
        records.append(dict(shape="filter", predicate=name, rows=NP, out_rows=n, median_ms=round(ms, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                            kernels={k[0]: round(k[2], 4) for k in ks}))
        print("filter %-58s %8.3f ms (%.3f .. %.3f)  out %9d  %s" % (name, ms, lo, hi, n, ", ".join(k[0][-28:] for k in ks)), flush=True)
        plan.close()
    del keep
    st.close()


if __name__ == "__main__":
    print("tree", TREE, "kernel_source_sha16", rf.kernel_source_sha16(), flush=True)
    joins()
    filters()
    if OUT:
        with open(OUT, "w") as fh:
            json.dump(dict(kernel_source_sha16=rf.kernel_source_sha16(), has_forms=HAS_FORMS, probe_rows=NP, steps=STEPS, records=records), fh, indent=1)
