#!/usr/bin/env python
"""Deleting rows on one MI355X: what lantern_gpu_remove_labels and lantern_gpu_unlink_deleted cost and what the unlinked graph is worth.

    python scripts/bench_unlink.py [--n 1000000] [--dim 768] [--nq 4096] [--reps 3] [--out profiles/unlink_1Mx768_clustered.json]

Clustered rows (lantern_amd/synth.py), f32 L2sq, M = 16, ef_construction = 128, ef = 64, k = 10.  Cases: a random 10 % and 30 % of the
rows deleted, and one whole cluster.  Per case:
  * remove_ms / unlink_ms: HIP events around the call (it waits for its own device work), the median of --reps runs on fresh copies of
    the index (usearch_load_buffer of the built index), every run listed; the unlink's stats;
  * queries/s (search_batch_device, best of --reps) and recall@10 against the exact search over the live rows, in four states:
    "tombstoned" (labels removed; label 0 dropped from each page of 10), "unlinked", "filtered" (the tombstoned graph under an
    all-live filter, walk path), "fresh" (a new build of the live rows).
The case's record is appended to --out as soon as it is complete; the whole result is printed as ONE JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_filtered import cluster_ids  # noqa: E402
from lantern_amd import capi, hip, synth  # noqa: E402

M, EFC, EF, K = 16, 128, 64, 10


def new_index(dim):
    return capi.GpuIndex("l2sq", dim, M=M, ef_construction=EFC, ef=EF, seed=42)


def timed(fn):
    a, b = hip.Event(), hip.Event()
    a.record()
    t = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t) * 1e3
    b.record()
    b.synchronize()
    return out, a.elapsed_ms(b), wall


def searcher(ix, queries, reps, filt=None):
    """(best queries/s, labels [nq][K]) of the device-resident batch."""
    nq = queries.shape[0]
    rows = ix.device_query_rows(queries)
    dq = hip.Buffer.from_numpy(rows)
    lab, dist = hip.Buffer(nq * K * 8), hip.Buffer(nq * K * 4)

    def run():
        if filt is None:
            ix.search_batch_device(dq.ptr, nq, K, 0, 0, lab.ptr, dist.ptr, query_stride=rows.strides[0])
        else:
            ix.search_batch_filtered_device(filt, dq.ptr, rows.strides[0], nq, K, 0, 0, lab.ptr, dist.ptr)
        hip.synchronize()

    run()
    best = 0.0
    for _ in range(reps):
        t = time.perf_counter()
        run()
        best = max(best, nq / (time.perf_counter() - t))
    out = lab.download((nq, K), np.uint64)
    for b in (dq, lab, dist):
        b.free()
    return best, out


def recall(labels, truth_labels):
    hit = sum(len(set(int(x) for x in row if x != 0) & set(t)) for row, t in zip(labels, truth_labels.tolist()))
    return hit / truth_labels.size


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
        live = np.flatnonzero(~dead)
        rec = {"case": name, "deleted": int(dead.sum()), "remove_ms": [], "remove_wall_ms": [], "unlink_ms": [], "unlink_wall_ms": []}
        fresh = new_index(a.dim)
        fresh.add_many(labels[live], base[live])
        t_slots, _ = fresh.exact_search(queries, K)  # the exact search over the live rows
        truth = labels[live][t_slots.astype(np.int64)]
        qps, lab = searcher(fresh, queries, a.reps)
        rec["fresh"] = {"qps": qps, "recall": recall(lab, truth)}
        fresh.close()
        for r in range(a.reps):
            ix = new_index(a.dim)
            ix.load_buffer(blob)
            removed, ev, wall = timed(lambda: ix.remove_labels(labels[dead]))
            assert removed == rec["deleted"]
            rec["remove_ms"].append(ev), rec["remove_wall_ms"].append(wall)
            if r == 0:
                qps, lab = searcher(ix, queries, a.reps)
                rec["tombstoned"] = {"qps": qps, "recall": recall(lab, truth)}
                f = ix.filter_from_bitmap(~dead)
                ix.set_filter_policy("walk")
                qps, lab = searcher(ix, queries, a.reps, f)
                rec["filtered"] = {"qps": qps, "recall": recall(lab, truth)}
                f.close()
            st, ev, wall = timed(ix.unlink_deleted)
            rec["unlink_ms"].append(ev), rec["unlink_wall_ms"].append(wall)
            if r == 0:
                rec["stats"] = st
                qps, lab = searcher(ix, queries, a.reps)
                assert not (lab == 0).any()
                rec["unlinked"] = {"qps": qps, "recall": recall(lab, truth)}
            ix.close()
        rec["remove_ms_median"], rec["unlink_ms_median"] = float(np.median(rec["remove_ms"])), float(np.median(rec["unlink_ms"]))
        result["cases"].append(rec)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(result, fh, indent=1)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
