"""A/B of quantising rows in one launch (lantern_gpu_set_pq_encode_fused; DESIGN.md 4.7 "Encoding in one launch").  The first n - tail rows
are built once, expanded, and saved with their graph; every leg starts from that state.
  load  wall of import_graph of the first n - tail RAW rows under the saved graph: the upload and the bulk encode of a load
          a  the switch on: one k_pq_encode launch + one decode     b  the switch off: one nearest-centroid pass per subvector
  add   wall of adding the last `tail` rows in one call to the compacted index under lantern_gpu_set_add_compact
          a  the switch on: one launch per staging piece            b  the switch off
alternated in one process.  Prints ONE JSON document (and writes it to --out).  Needs an MI355X.

    python scripts/pq_encode_ab.py --out profiles/pq_encode_ab.json
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
    base = synth.base_rows("clustered", a.n, a.dim)
    labels = np.arange(a.n, dtype=np.uint64) + 1
    crng = np.random.default_rng(5)
    cb = np.zeros((C, a.dim), dtype=np.float32)
    for sv in range(S):
        cb[:, sv * sub:(sv + 1) * sub] = base[crng.choice(a.n, size=C, replace=False), sv * sub:(sv + 1) * sub]
    make = lambda: capi.GpuIndex("l2sq", a.dim, M=a.m, ef_construction=a.efc, ef=64, seed=42, pq_codebook=cb, num_subvectors=S)
    plan = capi.plan_pq_encode("l2sq", a.dim, S, C)
    t0 = time.time()
    first = make()
    first.reserve(n0)
    first.add_many(labels[:n0], base[:n0])
    first.flush()
    blob, graph, codes = first.save_buffer(), first.export_graph(), first.export_codes()
    del first
    print(f"first {n0} rows built and saved in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)

    def load(on):
        ix = make()
        ix.set_pq_encode_fused(int(on))
        t = time.perf_counter()
        ix.import_graph(base[:n0], graph)  # (returns after the device drained)
        wall = time.perf_counter() - t
        return {"wall_ms": wall * 1e3, "record": capi.last_pq_encode(), "same_codes": bool(np.array_equal(ix.export_codes(), codes))}

    def add(on):
        ix = make()
        ix.load_buffer(blob)
        ix.pq_compact()
        ix.set_add_compact(1)
        ix.set_pq_encode_fused(int(on))
        t = time.perf_counter()
        ix.add_many(labels[n0:], base[n0:])
        ix.flush()
        wall = time.perf_counter() - t
        return {"wall_ms": wall * 1e3, "record": capi.last_pq_encode(), "checksum": ix.checksum(), "codes": ix.export_codes()[n0:]}

    load(True), load(False), add(True), add(False)  # warm-up of every leg: code objects, pools
    legs = {"load_a": [], "load_b": [], "add_a": [], "add_b": []}
    for _ in range(a.reps):  # alternated
        legs["load_a"].append(load(True))
        legs["load_b"].append(load(False))
        legs["add_a"].append(add(True))
        legs["add_b"].append(add(False))
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    out = {"command": "python scripts/pq_encode_ab.py " + " ".join(sys.argv[1:]),
           "workload": f"clustered {a.n}x{a.dim} l2sq pq {S} subvectors x {C} centroids, M={a.m} efc={a.efc}: the first {n0} rows loaded raw under their graph; "
                       f"the last {a.tail} added to the compacted index",
           "reps": a.reps, "unit": "median of reps (min, max)", "plan": plan}
    for leg, runs in legs.items():
        out[leg] = {"wall_ms": stat([r["wall_ms"] for r in runs]), "record": runs[0]["record"]}
    out["load_same_codes"] = all(r["same_codes"] for r in legs["load_a"] + legs["load_b"])
    out["add_same_index"] = len({r["checksum"] for r in legs["add_a"] + legs["add_b"]}) == 1 and all(
        np.array_equal(r["codes"], legs["add_b"][0]["codes"]) for r in legs["add_a"])
    # the rule for a default flip: the fused median not above the switch-off median by more than the switch-off runs' own spread
    for leg in ("load", "add"):
        b = out[leg + "_b"]["wall_ms"]
        out[leg + "_a_within_b_spread"] = out[leg + "_a"]["wall_ms"]["median"] <= b["median"] + (b["max"] - b["min"])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
