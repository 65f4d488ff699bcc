#!/usr/bin/env python
"""Compacting after deletes on one MI355X: what lantern_gpu_compact_deleted costs, what it frees, and that nothing else changes.

    python scripts/bench_compact.py [--n 1000000] [--dim 768] [--nq 4096] [--reps 3] [--out profiles/compact_1Mx768_clustered.json]

Clustered rows (lantern_amd/synth.py), f32 L2sq, M = 16, ef_construction = 128, ef = 64, k = 10.  Cases: a random 10 % and 30 % of the
rows deleted, and one whole cluster.  Per case, on a fresh copy of the built index (usearch_load_buffer), after remove_labels and
unlink_deleted:
  * queries/s (search_batch_device, best of --reps) and recall@10 against exact_search over the live rows, before and after the
    compaction; the two label arrays must be equal;
  * compact_ms / compact_wall_ms: HIP events and the wall clock around the call; kernels_ms and rows_kernel_ms: the call's own events
    around all its kernels and around k_compact_rows over the vector block (lantern_gpu_last_compact_ms);
  * the call's stats (bytes_before / after / moved) and lantern_gpu_memory_usage before and after;
  * THE CEILING: a hipMemcpy device-to-device of the vector block's live bytes (rows_bytes = rows_after * row bytes, what the row
    kernel moves), timed with events in the same process, best of --reps; rows_kernel_over_copy = rows_kernel_ms / that.  Target: <= 1.5.
The case's record is written to --out as soon as it is complete; the whole result is printed as ONE JSON line at the end.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_filtered import cluster_ids  # noqa: E402
from bench_unlink import EF, EFC, K, M, new_index, recall, searcher, timed  # noqa: E402
from lantern_amd import hip, synth  # noqa: E402

D2D = 3  # hipMemcpyDeviceToDevice


def copy_ms(nbytes, reps):
    """best-of-reps event time of one device-to-device hipMemcpy of nbytes"""
    src, dst = hip.Buffer(nbytes), hip.Buffer(nbytes)
    src.zero(), dst.zero()
    best = float("inf")
    for _ in range(reps + 1):  # (the first one warms up)
        a, b = hip.Event(), hip.Event()
        a.record()
        hip.check(hip.rt().hipMemcpy(C.c_void_p(dst.ptr), C.c_void_p(src.ptr), C.c_size_t(nbytes), C.c_int(D2D)), "hipMemcpy D2D")
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_ms(b))
    src.free(), dst.free()
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    base = synth.base_rows("clustered", a.n, a.dim)
    queries = synth.query_maker("clustered", a.dim)(np.random.default_rng(9), a.nq)
    labels = np.arange(a.n, dtype=np.uint64) + 1
    cluster = cluster_ids(a.n, a.dim)
    built = new_index(a.dim)
    t = time.perf_counter()
    built.add_many(labels, base)
    built.flush()
    result = {"n": a.n, "dim": a.dim, "M": M, "ef_construction": EFC, "ef": EF, "k": K, "nq": a.nq, "reps": a.reps,
              "build_s": time.perf_counter() - t, "cases": []}
    blob = built.save_buffer()
    built.close()
    rng = np.random.default_rng(13)
    cases = [("random 10 %", rng.random(a.n) < 0.10), ("random 30 %", rng.random(a.n) < 0.30), ("one cluster", cluster == 0)]
    for name, dead in cases:
        rec = {"case": name, "deleted": int(dead.sum())}
        ix = new_index(a.dim)
        ix.load_buffer(blob)
        assert ix.remove_labels(labels[dead]) == rec["deleted"]
        ix.unlink_deleted()
        live = np.flatnonzero(~dead)
        rec["memory_before"] = ix.memory_usage()
        qps, lab_before = searcher(ix, queries, a.reps)
        (st, slot_map), ev, wall = timed(ix.compact_deleted)
        rec["compact_ms"], rec["compact_wall_ms"] = ev, wall
        rec["kernels_ms"], rec["rows_kernel_ms"] = ix.last_compact_ms()
        rec["stats"] = st
        rec["memory_after"] = ix.memory_usage()
        t_slots, _ = ix.exact_search(queries, K)  # the exact search over the live rows
        truth = labels[live][t_slots.astype(np.int64)]
        rec["before"] = {"qps": qps, "recall": recall(lab_before, truth)}
        qps, lab_after = searcher(ix, queries, a.reps)
        rec["after"] = {"qps": qps, "recall": recall(lab_after, truth)}
        rec["answers_identical"] = bool(np.array_equal(lab_before, lab_after))
        rec["slot_map_ok"] = bool(np.array_equal(slot_map[live], np.arange(live.size)) and (slot_map[dead] == 0xFFFFFFFF).all())
        rec["rows_bytes"] = int(st["rows_after"]) * ix.row_bytes()
        ix.close()
        rec["copy_ms"] = copy_ms(rec["rows_bytes"], a.reps)
        rec["rows_kernel_over_copy"] = rec["rows_kernel_ms"] / rec["copy_ms"]
        rec["rows_kernel_GBps_read_plus_write"] = 2 * rec["rows_bytes"] / rec["rows_kernel_ms"] / 1e6
        rec["memory_ratio"] = sum(rec["memory_after"]) / sum(rec["memory_before"])
        result["cases"].append(rec)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(result, fh, indent=1)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
