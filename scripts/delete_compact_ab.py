"""A/B of unlinking and compacting a compact pq index (lantern_gpu_set_delete_compact; DESIGN.md 4.11, 4.12 "Compact pq indexes").  The
index is built once, expanded, a random share of its labels removed, and saved; every repeat loads that buffer again, so all legs start
from the same state.
  a  compact, the switch on: unlink_deleted, then compact_deleted, on the code rows
  b  compact, the switch off -- what a caller must do today: pq_expand, the two calls, pq_compact
  c  the expanded twin's two calls
alternated in one process.  Per leg and call: wall, the peak of device memory in use while it ran (hipMemGetInfo sampled from a second
thread every millisecond), and after the leg recall@10 against the exact answers over the live rows.  The request kernel's own time is
not in this document: no entry point reports it; take it from a kernel trace of this script run on its own.  Prints ONE JSON document
(and writes it to --out).  Needs an MI355X.

    python scripts/delete_compact_ab.py --out profiles/delete_compact_ab.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lantern_amd import capi, hip, synth  # noqa: E402


def in_use():
    free, total = C.c_size_t(), C.c_size_t()
    hip.check(hip.rt().hipMemGetInfo(C.byref(free), C.byref(total)), "hipMemGetInfo")
    return total.value - free.value


def timed(call):
    """(wall ms, peak bytes in use while `call` ran, its result)"""
    peak, done = [in_use()], threading.Event()

    def watch():
        while not done.wait(0.001):
            peak[0] = max(peak[0], in_use())

    t = threading.Thread(target=watch)
    t.start()
    t0 = time.perf_counter()
    try:
        out = call()
    finally:
        wall = (time.perf_counter() - t0) * 1e3
        done.set()
        t.join()
    return wall, peak[0], out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--subvectors", type=int, default=96)
    p.add_argument("--centroids", type=int, default=256)
    p.add_argument("--m", type=int, default=16)
    p.add_argument("--efc", type=int, default=128)
    p.add_argument("--share", type=float, default=0.10)
    p.add_argument("--queries", type=int, default=1000)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert capi.device_count() > 0, "no HIP device"
    S, Cn, sub = a.subvectors, a.centroids, a.dim // a.subvectors
    base = synth.base_rows("clustered", a.n + a.queries, a.dim)
    queries, base = base[a.n:], base[:a.n]
    labels = np.arange(a.n, dtype=np.uint64) + 1
    rng = np.random.default_rng(5)
    cb = np.zeros((Cn, a.dim), dtype=np.float32)
    for sv in range(S):
        cb[:, sv * sub:(sv + 1) * sub] = base[rng.choice(a.n, size=Cn, replace=False), sv * sub:(sv + 1) * sub]
    make = lambda: capi.GpuIndex("l2sq", a.dim, M=a.m, ef_construction=a.efc, ef=64, seed=42, pq_codebook=cb, num_subvectors=S)
    t0 = time.time()
    first = make()
    first.reserve(a.n)
    first.add_many(labels, base)
    first.flush()
    dead = rng.choice(labels, int(a.n * a.share), replace=False)
    assert first.remove_labels(dead) == dead.size
    blob = first.save_buffer()
    del first
    print(f"{a.n} rows built, {dead.size} removed, saved in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    truth = None  # [nq][10] labels: exact over the live rows, from the first expanded leg (every leg ends with the same rows)

    def leg(kind):
        nonlocal truth
        ix = make()
        ix.load_buffer(blob)
        if kind != "c":
            ix.pq_compact()
        ix.set_delete_compact(int(kind == "a"))
        out = {}
        if kind == "b":
            out["expand_ms"], out["expand_peak"], _ = timed(ix.pq_expand)
        out["unlink_ms"], out["unlink_peak"], _ = timed(ix.unlink_deleted)
        out["compact_ms"], out["compact_peak"], _ = timed(ix.compact_deleted)
        if kind == "b":
            out["recompact_ms"], out["recompact_peak"], _ = timed(ix.pq_compact)
        out["wall_ms"] = sum(v for k, v in out.items() if k.endswith("_ms"))
        out["peak_bytes"] = max(v for k, v in out.items() if k.endswith("_peak"))
        out["row_bytes_after"], out["checksum"] = ix.memory_usage()[0], ix.checksum()
        if kind == "c" and truth is None:
            slots, _ = ix.exact_search(queries, 10)
            truth = ix.export_graph()["labels"][slots.astype(np.int64)]
        out["labels"] = ix.search_batch(queries, 10)[0]
        return out

    leg("c"), leg("a")  # warm-up: code objects, scratch sizes; the exact answers
    legs = {"a": [], "b": [], "c": []}
    for _ in range(a.reps):  # alternated
        for kind in legs:
            legs[kind].append(leg(kind))
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    out = {"command": "python scripts/delete_compact_ab.py " + " ".join(sys.argv[1:]),
           "workload": f"clustered {a.n}x{a.dim} l2sq pq {S} subvectors x {Cn} centroids, M={a.m} efc={a.efc}: a random {a.share:.0%} of the labels removed",
           "reps": a.reps, "unit": "ms and bytes: median of reps (min, max)"}
    for kind, runs in legs.items():
        out[kind] = {k: stat([r[k] for r in runs]) for k in runs[0] if k.endswith("_ms") or k.endswith("_peak") or k == "peak_bytes"}
        out[kind]["row_bytes_after"] = runs[0]["row_bytes_after"]
        out[kind]["recall_at_10"] = float(np.mean([len(set(g) & set(t)) / 10 for g, t in zip(runs[0]["labels"].tolist(), truth.tolist())]))
    out["same_graph"] = len({r["checksum"] for runs in legs.values() for r in runs}) == 1
    # the rule for a default flip: a's median wall not above the twin's by more than the twin's own min-max spread
    c = out["c"]["wall_ms"]
    out["a_within_c_spread"] = out["a"]["wall_ms"]["median"] <= c["median"] + (c["max"] - c["min"])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
