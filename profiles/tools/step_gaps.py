"""Summarises a `rocprofv3 --kernel-trace --output-format csv` run of `bench.py --gpus 1 --steps K --warmup W` into the steady Q5 steps' kernel
times, spans and the idle time BETWEEN steps (profiles/rNN_q5_step_gaps_{before,after}.json).

    python profiles/tools/step_gaps.py <trace dir> <out.json> [steps, default 10]

A step ends with its band_emit_kernel; a runtime copy kernel that directly follows emit (the counters' copy of an execute that waits for the whole
stream) belongs to the step it follows.  Only steps whose emit is the list form's and that hold exactly one emit are steady steps; the last `steps`
of them are kept.  idle = start of the next step's first kernel - end of this step's last kernel (the next step being the next one in the trace)."""
import csv
import glob
import json
import os
import statistics
import sys


def short(name):
    for tag in ("OjKeyValues", "OjInPlace"):
        if tag in name:
            return name.split("(")[0] + "(.., " + tag + ")"
    if "rocprim" in name:
        return "rocprim scan"
    return name.split("(")[0] if name.startswith("rdfgpu::") or name.startswith("__amd") else name.split("(rdfgpu::BandArgs")[0]


def main():
    trace_dir, out = sys.argv[1], sys.argv[2]
    keep = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    steps, cur, close_after_next = [], [], False
    for i, k in enumerate(rows):
        cur.append(k)
        if close_after_next:
            steps.append(cur); cur, close_after_next = [], False
        elif "band_emit_kernel" in k[2]:
            if i + 1 < len(rows) and "copyBuffer" in rows[i + 1][2]:
                close_after_next = True
            else:
                steps.append(cur); cur = []
    summary = []
    for n, st in enumerate(steps[:-1]):
        names = [k[2] for k in st]
        if sum("band_emit_kernel" in x for x in names) != 1 or not any("OjKeyValues" in x for x in names):
            continue
        kernels = {}
        for s, e, name in st:
            kernels[short(name)] = round(kernels.get(short(name), 0.0) + (e - s) / 1e3, 2)
        emit_at = next(i for i, x in enumerate(names) if "band_emit_kernel" in x)
        to_host = [i for i, x in enumerate(names) if "copyBuffer" in x or "band_count_point_kernel" in x]
        nxt = steps[n + 1]
        summary.append({"kernels_us": kernels, "kernel_sum_us": round(sum(kernels.values()), 2), "span_us": round((st[-1][1] - st[0][0]) / 1e3, 2),
                        "idle_to_next_step_us": round((nxt[0][0] - st[-1][1]) / 1e3, 2),
                        "counters_to_host": "none" if not to_host else ("before emit" if to_host[-1] < emit_at else "after emit"),
                        "launches": len(st)})
    summary = summary[-keep:]
    med = lambda xs: round(statistics.median(xs), 2) if xs else None
    names = sorted({k for s in summary for k in s["kernels_us"]})
    doc = {"what": "steady Q5 steps of `bench.py --gpus 1 --steps 10 --warmup 3` under rocprofv3 --kernel-trace (kernel tracing only); a step ends with its emit "
                   "kernel (+ the copy kernel that directly follows it); idle = from the end of a step's last kernel to the start of the next step's first; us",
           "steps": len(summary),
           "median": {"kernels_us": {k: med([s["kernels_us"].get(k, 0.0) for s in summary]) for k in names},
                      "kernel_sum_us": med([s["kernel_sum_us"] for s in summary]), "span_us": med([s["span_us"] for s in summary]),
                      "idle_to_next_step_us": med([s["idle_to_next_step_us"] for s in summary]),
                      "period_us": med([s["span_us"] + s["idle_to_next_step_us"] for s in summary])},
           "counters_to_host": sorted({s["counters_to_host"] for s in summary}),
           "per_step": summary}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"steps": doc["steps"], "median": doc["median"], "counters_to_host": doc["counters_to_host"]}))


if __name__ == "__main__":
    main()
