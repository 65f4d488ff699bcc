#!/usr/bin/env python
"""A/B of the exact k-NN's contraction on quantised indexes: the native f16 / i8 MFMA kernel (LANTERN_GPU_DENSE_NATIVE=1,
dense_native.hip) against the dequantised f32 path (=0: the baseline), on one index and one query batch per case.

    python scripts/dense_native_ab.py [--n 1000000] [--d 768] [--nq 1024] [--k 10] [--reps 3] [--out FILE]

Cases: f16 and i8 storage, each under l2sq and cos; Gaussian rows (scaled 0.3 for i8, as bench.py --data-scale advises).  Per
case the two settings alternate in one process after one warm-up call each; per call: wall time, the sum of the contraction
launches' durations (lantern_gpu_dense_profile) and the certificate's counters.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lantern_amd import capi  # noqa: E402


def empty_graph(n):
    return {"levels": np.zeros(n, np.uint8), "nbr0": np.full((n, 8), 0xFFFFFFFF, np.uint32), "upper_off": np.full(n, 0xFFFFFFFF, np.uint32),
            "upper_nbr": np.zeros((0, 4), np.uint32), "labels": None, "entry_slot": 0, "max_level": 0}


def one_call(ix, queries, k, native):
    os.environ["LANTERN_GPU_DENSE_NATIVE"] = native
    before, kinds = capi.exact_knn_stats(), capi.dense_kind_stats()
    capi.dense_profile(True)
    t0 = time.perf_counter()
    slots, dists = ix.exact_search(queries, k)
    wall = (time.perf_counter() - t0) * 1e3
    launches = capi.dense_profile(False)
    after = capi.exact_knn_stats()
    return {"wall_ms": wall, "dense_ms": sum(r["ms"] for r in launches), "launches": len(launches),
            "kinds": [a - b for a, b in zip(capi.dense_kind_stats(), kinds)], **{key: after[key] - before[key] for key in after}}, slots, dists


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert capi.device_count() > 0, "no HIP device"
    rng = np.random.default_rng(0)
    rows, queries = rng.standard_normal((a.n, a.d), dtype=np.float32), rng.standard_normal((a.nq, a.d), dtype=np.float32)
    line = {"script": "scripts/dense_native_ab.py", "command": " ".join(sys.argv), "n": a.n, "d": a.d, "nq": a.nq, "k": a.k, "reps": a.reps, "cases": {}}
    for storage in ("f16", "i8"):
        scale = np.float32(0.3) if storage == "i8" else np.float32(1.0)
        if storage == "i8":  # the integers an i8 index stores: trunc(clamp(100 x, -100, 100))
            stored = np.trunc(np.clip(rows * (scale * np.float32(100.0)), -100.0, 100.0)).astype(np.float32)
        else:
            stored = rows
        for metric in ("l2sq", "cos"):
            ix = capi.GpuIndex(metric, a.d, M=4, ef_construction=8, seed=1, quantization=storage)
            ix.import_graph(stored, empty_graph(a.n))
            q = queries * scale
            runs, answers = {"1": [], "0": []}, {}
            for native in ("1", "0"):  # one warm-up call each
                _, s, dd = one_call(ix, q, a.k, native)
                answers[native] = (s, dd)
            same = bool(np.array_equal(answers["1"][0], answers["0"][0]) and np.array_equal(answers["1"][1].view(np.uint32), answers["0"][1].view(np.uint32)))
            for _ in range(a.reps):
                for native in ("1", "0"):
                    runs[native].append(one_call(ix, q, a.k, native)[0])
            ix.close()
            med = {m: statistics.median(r["wall_ms"] for r in runs[m]) for m in runs}
            base = [r["wall_ms"] for r in runs["0"]]
            line["cases"][f"{storage}_{metric}"] = {
                "native": runs["1"], "dequantised": runs["0"], "identical_answers": same,
                "median_wall_ms": {"native": med["1"], "dequantised": med["0"]},
                "median_dense_ms": {m2: statistics.median(r["dense_ms"] for r in runs[m]) for m, m2 in (("1", "native"), ("0", "dequantised"))},
                "dequantised_spread_ms": max(base) - min(base), "ratio_dequantised_over_native": med["0"] / med["1"],
                "native_within_rule": bool(med["1"] <= med["0"] + (max(base) - min(base)))}
    line["native_default_by_rule"] = all(c["native_within_rule"] for c in line["cases"].values())
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
