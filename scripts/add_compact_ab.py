"""A/B of adding to a compact pq index (lantern_gpu_set_add_compact; DESIGN.md 4.7 "Compact pq indexes: adding").  The first
n - tail rows are built once, expanded, and saved; every repeat loads that buffer again, so all legs continue from the same state.
  bulk  vectors/s and walk_ms (build profile) of adding the last `tail` rows in one call
          a  to the compacted index, the switch on: served from the code rows
          b  to the expanded twin
  lone  wall of ONE usearch_add + flush, in every leg after one untimed warm-up add on the freshly loaded index
          a  compact, the switch on   b  compact, the switch off (today: the add expands the index; the warm-up add expanded it too and
          it was compacted again, untimed, before the timed add)   c  expanded
alternated in one process.  Prints ONE JSON document (and writes it to --out).  Needs an MI355X.

    python scripts/add_compact_ab.py --out profiles/add_compact_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lantern_amd import capi, synth  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--tail", type=int, default=100_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--subvectors", type=int, default=96)
    p.add_argument("--centroids", type=int, default=256)
    p.add_argument("--m", type=int, default=16)
    p.add_argument("--efc", type=int, default=128)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert capi.device_count() > 0, "no HIP device"
    S, C, sub, n0 = a.subvectors, a.centroids, a.dim // a.subvectors, a.n - a.tail
    base = synth.base_rows("clustered", a.n + 2, a.dim)  # (the last two rows: the lone adds)
    labels = np.arange(a.n + 2, dtype=np.uint64) + 1
    crng = np.random.default_rng(5)
    cb = np.zeros((C, a.dim), dtype=np.float32)
    for sv in range(S):
        cb[:, sv * sub:(sv + 1) * sub] = base[crng.choice(a.n, size=C, replace=False), sv * sub:(sv + 1) * sub]
    make = lambda: capi.GpuIndex("l2sq", a.dim, M=a.m, ef_construction=a.efc, ef=64, seed=42, pq_codebook=cb, num_subvectors=S)
    t0 = time.time()
    first = make()
    first.reserve(n0)
    first.add_many(labels[:n0], base[:n0])
    first.flush()
    blob = first.save_buffer()
    del first
    print(f"first {n0} rows built and saved in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)

    def loaded(compact, on):
        ix = make()
        ix.load_buffer(blob)
        if compact:
            ix.pq_compact()
        ix.set_add_compact(int(on))
        return ix

    def bulk(compact):
        ix = loaded(compact, compact)
        ix.set_profiling(True)
        t = time.perf_counter()
        ix.add_many(labels[n0:a.n], base[n0:a.n])
        ix.flush()  # (returns after the device drained)
        wall = time.perf_counter() - t
        return {"vectors_per_s": a.tail / wall, "walk_ms": ix.build_profile()["walk_ms"], "row_bytes_after": ix.memory_usage()[0], "checksum": ix.checksum()}

    def lone(compact, on):
        ix = loaded(compact, on)
        # EVERY leg: one untimed warm-up add on the freshly loaded index (its first-use allocations: scratch, visited bitmaps, the staging
        # block).  Leg b's warm-up expands the index; it is compacted again, untimed, so that the timed add pays the expansion and nothing else
        ix.add(labels[a.n], base[a.n])
        ix.flush()
        if compact and not on:
            ix.pq_compact()
        t = time.perf_counter()
        ix.add(labels[a.n + 1], base[a.n + 1])
        ix.flush()
        return (time.perf_counter() - t) * 1e3

    bulk(True), bulk(False)  # warm-up of both legs: code objects, scratch sizes
    legs = {"bulk_a": [], "bulk_b": [], "lone_a": [], "lone_b": [], "lone_c": []}
    for _ in range(a.reps):  # alternated
        legs["bulk_a"].append(bulk(True))
        legs["bulk_b"].append(bulk(False))
        legs["lone_a"].append(lone(True, True))
        legs["lone_b"].append(lone(True, False))
        legs["lone_c"].append(lone(False, False))
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    out = {"command": "python scripts/add_compact_ab.py " + " ".join(sys.argv[1:]),
           "workload": f"clustered {a.n}x{a.dim} l2sq pq {S} subvectors x {C} centroids, M={a.m} efc={a.efc}: the last {a.tail} rows added to the saved first {n0}",
           "reps": a.reps, "unit": "median of reps (min, max)"}
    for leg in ("bulk_a", "bulk_b"):
        out[leg] = {k: stat([r[k] for r in legs[leg]]) for k in ("vectors_per_s", "walk_ms")}
        out[leg]["row_bytes_after"] = legs[leg][0]["row_bytes_after"]
    out["bulk_same_graph"] = len({r["checksum"] for r in legs["bulk_a"] + legs["bulk_b"]}) == 1
    for leg in ("lone_a", "lone_b", "lone_c"):
        out[leg] = {"wall_ms": stat(legs[leg])}
    # the rule for a default flip: a's median not below the twin's by more than the twin's own min-max spread
    b = out["bulk_b"]["vectors_per_s"]
    out["bulk_a_within_b_spread"] = out["bulk_a"]["vectors_per_s"]["median"] >= b["median"] - (b["max"] - b["min"])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
