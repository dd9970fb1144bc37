"""bench.py end to end at a small size: a plain run prints the headline line and nothing it does not need, `--steps` sets the
number of timed batches, and --dump-outputs writes the same files for the same arguments — the oracle's bindings."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run_bench(*args):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "bench.py"), *args]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_and_its_dumped_outputs(tmp_path, torch_cuda):
    import rdf_fusion_amd as rf
    from rdf_fusion_amd import bsbm
    from oracle import oracle as orc
    import kat_util as ku
    P, Q, W = 2000, 512, 1
    small = ["--gpus", "1", "--products", str(P), "--queries", str(Q), "--warmup", str(W)]
    a = run_bench(*small, "--steps", "3", "--dump-outputs", str(tmp_path / "a"))
    b = run_bench(*small, "--steps", "2")
    c = run_bench(*small, "--steps", "3", "--dump-outputs", str(tmp_path / "c"))
    for out, steps in ((a, 3), (b, 2), (c, 3)):
        assert out["steps"] == steps and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "bindings/s"
        assert out["higher_is_better"] is True and out["dtype"] and out["metric"]
        assert out["roofline"] is None and out["cpu_baseline"] is None and "scan_roofline" not in out     # --full only
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["bindings_per_instance.npy", "inst.npy", "product.npy", "product_label.npy"]
    dump = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:                                                          # same arguments, same files
        assert dump[n[:-4]].dtype == np.float64
        np.testing.assert_array_equal(dump[n[:-4]], np.load(tmp_path / "c" / n))

    # The batches bench.py draws (W warm-ups, then the timed ones), executed here: the timed bindings of a run add up over
    # exactly the `--steps` batches after the warm-ups
    bench = load_bench()
    ds = bsbm.generate(P)
    rng = np.random.default_rng(bench.BATCH_SEED)
    batches = [bench.draw_batch(rng, ds, Q, Q) for _ in range(W + 3)]
    gs = rf.GpuQuadStore(device=0)
    gs.extend(ds.g, ds.s, ds.p, ds.o)
    gs.set_typed_values(ds.typed_values, ds.decimals)
    plan = gs.plan(bsbm.q5_batch_plan(ds))
    rows = []
    for bt in batches:
        t = torch_cuda.from_numpy(np.stack([np.arange(1, Q + 1, dtype=np.uint32), bt]).view(np.int32)).cuda()
        plan.bind_table(0, [t.data_ptr(), t.data_ptr() + 4 * Q], Q)
        plan.execute()
        rows.append(plan.result_info()[0])
    plan.close(); gs.close()
    assert a["config"]["bindings"] == sum(rows[W:W + 3]) and b["config"]["bindings"] == sum(rows[W:W + 2])

    # The dump against the CPU oracle: the last timed batch's instances, one reference plan each
    counts = dump["bindings_per_instance"]
    assert len(counts) == Q and counts.sum() == rows[W + 2]
    assert len(dump["inst"]) == counts.sum()                                 # Q < the sample size: every binding is dumped
    os_ = orc.OracleStore()
    os_.extend(ds.g, ds.s, ds.p, ds.o)
    os_.set_typed_values(ds.typed_values, ds.decimals)
    checked = 0
    for tag in np.unique(np.linspace(1, Q, 48).astype(int)):
        cols, n, _ = os_.execute(bsbm.q5_plan(ds, int(batches[W + 2][tag - 1])))
        assert counts[tag - 1] == n, tag
        sel = dump["inst"] == tag
        got = [dump["product"][sel].astype(np.uint32), dump["product_label"][sel].astype(np.uint32)]
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(cols, n))
        checked += n
    assert checked > 0
