#!/usr/bin/env python
"""Mixed (k, ef) batches, measured (profiles/r07_scan_mixed.md).  One resident index, one process, one JSON object per line:

  1. device-level cost of the per-query-parameter instantiation: 8192 resident queries, k = 10, ef = 64, through
     lantern_gpu_search_batch_params_device with uniform parameters against lantern_gpu_search_batch_device_strided; and a four-way mix
     (k in {10, 20, 40, 80}, 2048 queries each) as ONE call against four uniform calls.
  2. the scan-side service under paginating backends (lantern-scan-load --pages 4, 256 connections): LANTERN_SCAN_MIXED=1 and =0
     alternating, three repetitions each, against the same resident index; then --pages 1 (the uniform workload) under both.

    python scripts/scan_mixed_ab.py [--rows 1000000 --dim 768] > profiles/r07_scan_mixed.jsonl
"""
import argparse
import json
import os

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")  # a hardware queue per service lane
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--kind", default="clustered")
    p.add_argument("--connections", type=int, default=256)
    p.add_argument("--pages", type=int, default=4)
    p.add_argument("--seconds", type=float, default=3.0)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--max-batch", type=int, default=1024)
    p.add_argument("--max-wait-us", type=int, default=200)
    a = p.parse_args()
    from lantern_amd import capi, hip, synth

    base = synth.base_rows(a.kind, a.rows, a.dim)
    ix = capi.GpuIndex("l2sq", a.dim, M=16, ef_construction=128, ef=64, seed=42)
    ix.reserve(a.rows)
    t0 = time.time()
    ix.add_many(np.arange(a.rows, dtype=np.uint64) + 1, base)
    ix.flush()
    hip.synchronize()
    print(json.dumps({"index": f"{a.rows}x{a.dim} {a.kind} f32 l2sq M=16 efc=128 ef=64", "build_seconds": time.time() - t0}), flush=True)
    del base

    # ---- 1. device-level cost
    nq = 8192
    queries = synth.query_maker(a.kind, a.dim)(np.random.default_rng(4), nq)
    rows = ix.device_query_rows(queries)
    dq = hip.Buffer.from_numpy(rows)
    stride = rows.strides[0]
    lab, dist, slot, cnt = hip.Buffer(nq * 80 * 8), hip.Buffer(nq * 80 * 4), hip.Buffer(nq * 80 * 4), hip.Buffer(nq * 4)

    def timed(fn, reps=10):
        for _ in range(2):
            fn()
        hip.synchronize()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            hip.synchronize()
            ts.append(time.perf_counter() - t)
        ts = np.array(ts) * 1e3
        return {"ms_median": float(np.median(ts)), "ms_min": float(ts.min()), "ms_max": float(ts.max())}

    uni = timed(lambda: ix.search_batch_device(dq.ptr, nq, 10, 64, 0, lab.ptr, dist.ptr, slot.ptr, cnt.ptr, query_stride=stride))
    P = capi.query_params([(10, 64, 0)] * nq)
    each = timed(lambda: ix.search_batch_params_device(dq.ptr, stride, nq, P, 10, lab.ptr, dist.ptr, slot.ptr, cnt.ptr))
    print(json.dumps({"leg": "8192 resident queries, k=10 ef=64", "uniform_call": uni, "params_call_uniform_parameters": each,
                      "params_over_uniform": each["ms_median"] / uni["ms_median"], "params_regime": ix.last_params_launch()}), flush=True)
    ks = (10, 20, 40, 80)
    Pm = capi.query_params([(ks[i // 2048], 64, 0) for i in range(nq)])
    one = timed(lambda: ix.search_batch_params_device(dq.ptr, stride, nq, Pm, 80, lab.ptr, dist.ptr, slot.ptr, cnt.ptr))
    regime = ix.last_params_launch()

    def four():
        for i, k in enumerate(ks):
            ix.search_batch_device(dq.ptr + i * 2048 * stride, 2048, k, 64, 0, lab.ptr, dist.ptr, slot.ptr, cnt.ptr, query_stride=stride)

    sep = timed(four)
    print(json.dumps({"leg": "four-way mix, k in {10, 20, 40, 80} x 2048 queries, ef=64", "one_params_call": one, "four_uniform_calls": sep,
                      "one_over_four": one["ms_median"] / sep["ms_median"], "params_regime": regime}), flush=True)

    # ---- 2. the service: paginating backends, mixed against grouped
    tool = os.path.join(ROOT, "lantern_amd", "lib", "lantern-scan-load")

    def service(mixed, pages):
        os.environ["LANTERN_SCAN_MIXED"] = "1" if mixed else "0"
        srv = capi.ScanServer(index=ix, max_batch=a.max_batch, max_wait_us=a.max_wait_us)
        pr = subprocess.run([tool, "--port", str(srv.port), "--dim", str(a.dim), "--rows", str(a.rows), "--connections", str(a.connections), "--seconds",
                             str(a.seconds), "--warmup-seconds", "1", "--pages", str(pages)], capture_output=True, text=True, timeout=300)
        st, legs = srv.stats(), srv.timing()
        srv.stop()
        line = next((json.loads(l) for l in pr.stdout.splitlines() if l.startswith("{")), {"error": (pr.stderr or pr.stdout)[-300:]})
        line.pop("service", None)
        line.update({"leg": "scan service", "LANTERN_SCAN_MIXED": int(mixed), "pages": pages, "requests_per_s": line.get("queries_per_s"),
                     "service_whole_run": st, "launches_per_batch": st["launches"] / max(st["batches"], 1), "mean_batch": st["requests"] / max(st["batches"], 1),
                     "server_side_us": legs})
        print(json.dumps(line), flush=True)
        return line

    for pages in (a.pages, 1):
        runs = {1: [], 0: []}
        for _ in range(a.reps if pages > 1 else 2):
            for mixed in (1, 0):
                runs[mixed].append(service(mixed, pages))
        summary = {"leg": "scan service summary", "pages": pages, "connections": a.connections}
        for mixed in (1, 0):
            r = np.array([x.get("requests_per_s") or 0 for x in runs[mixed]])
            summary["mixed" if mixed else "grouped"] = {
                "requests_per_s": {"median": float(np.median(r)), "min": float(r.min()), "max": float(r.max())},
                "p50_us": [x.get("latency_us", {}).get("p50") for x in runs[mixed]], "p99_us": [x.get("latency_us", {}).get("p99") for x in runs[mixed]],
                "launches_per_batch": [round(x["launches_per_batch"], 3) for x in runs[mixed]]}
        g = summary["grouped"]["requests_per_s"]
        summary["grouped_spread"] = g["max"] - g["min"]
        summary["mixed_median_minus_grouped_median"] = summary["mixed"]["requests_per_s"]["median"] - g["median"]
        summary["mixed_keeps_default"] = bool(summary["mixed_median_minus_grouped_median"] >= -summary["grouped_spread"])
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
