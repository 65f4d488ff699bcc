#!/usr/bin/env python
"""Same-box A/B of the int8 screen in the insertion walk (lantern_gpu_set_insert_screen): the benchmark's build --
rows x dim f32, M, ef_construction, bench.py's batch plan -- with mode 0 and mode 1, alternated inside every repetition, on the
Gaussian and the clustered set (l2sq) and on the clustered set under cosine.  Per build: vectors/s, the build profile (walk_ms is
the figure the screen can move), the rejected share of the rows put to the screen test, and the graph checksum, which must not
depend on the mode.  One JSON document; the verdict applies the rule that sets kInsertScreenByDefault (csrc/insert_batch.cpp):

    on  iff  on both l2sq sets median(mode 1) >= median(mode 0) - spread(mode 0)
        and  on at least one of them median(mode 1) > median(mode 0) + spread(mode 0),     spread = max - min of the mode-0 runs

    python scripts/insert_screen_ab.py --out profiles/insert_screen_build_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def one_build(capi, hip, a, metric, base, labels, mode):
    ix = capi.GpuIndex(metric, a.dim, M=a.M, ef_construction=a.efc, ef=64, seed=42)
    ix.reserve(len(base))
    ix.set_add_batch(a.add_batch, 16)
    ix.set_insert_screen(mode)
    ix.set_profiling(True)
    hip.synchronize()
    t0 = time.time()
    ix.add_many(labels, base)
    ix.flush()
    hip.synchronize()
    t = time.time() - t0
    st, c = ix.insert_screen_stats(), ix.counters()
    out = {"mode": mode, "seconds": t, "vectors_per_s": len(base) / t, "build_profile": ix.build_profile(), "checksum": ix.checksum(),
           "screened_launches": st[0], "unscreened_launches": st[1], "rows_tested": st[2], "rows_rejected": st[3],
           "rejected_share": st[3] / st[2] if st[2] else None, "walk_evals": c["add_walk_evals"],
           "rejected_share_of_walk_evals": st[3] / c["add_walk_evals"] if c["add_walk_evals"] else None}
    ix.close()
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--M", type=int, default=16)
    p.add_argument("--efc", type=int, default=128)
    p.add_argument("--add-batch", type=int, default=32768, help="bench.py's insertion batch")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--sets", default="gaussian:l2sq,clustered:l2sq,clustered:cos")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    from lantern_amd import capi, hip, synth

    labels = np.arange(a.rows, dtype=np.uint64) + 1
    doc = {"workload": f"build {a.rows}x{a.dim} f32, M={a.M}, ef_construction={a.efc}, batches of up to {a.add_batch} rows (a sixteenth of the graph at most)",
           "library": capi.version() if hasattr(capi, "version") else None, "reps": a.reps, "sets": {}}
    for spec in a.sets.split(","):
        kind, metric = spec.split(":")
        base = synth.base_rows(kind, a.rows, a.dim)
        runs = []
        one_build(capi, hip, a, metric, base[: a.rows // 8], labels[: a.rows // 8], 0)  # warm the allocator and the code objects
        for rep in range(a.reps):
            for mode in ((0, 1) if rep % 2 == 0 else (1, 0)):
                r = one_build(capi, hip, a, metric, base, labels, mode)
                r["rep"] = rep
                runs.append(r)
                print(f"[{spec}] rep {rep} mode {mode}: {r['vectors_per_s']:.0f} vectors/s, walk {r['build_profile']['walk_ms']:.0f} ms, "
                      f"rejected {r['rejected_share']}", file=sys.stderr, flush=True)
        off, on = [r for r in runs if r["mode"] == 0], [r for r in runs if r["mode"] == 1]
        v0, v1 = [r["vectors_per_s"] for r in off], [r["vectors_per_s"] for r in on]
        doc["sets"][spec] = {"runs": runs, "checksums_equal": len({r["checksum"] for r in runs}) == 1,
                             "median_vectors_per_s": {"mode0": statistics.median(v0), "mode1": statistics.median(v1)},
                             "mode0_spread": max(v0) - min(v0),
                             "median_walk_ms": {"mode0": statistics.median(r["build_profile"]["walk_ms"] for r in off),
                                                "mode1": statistics.median(r["build_profile"]["walk_ms"] for r in on)}}
        del base
    l2 = [s for k, s in doc["sets"].items() if k.endswith(":l2sq")]
    not_below = all(s["median_vectors_per_s"]["mode1"] >= s["median_vectors_per_s"]["mode0"] - s["mode0_spread"] for s in l2)
    above = any(s["median_vectors_per_s"]["mode1"] > s["median_vectors_per_s"]["mode0"] + s["mode0_spread"] for s in l2)
    doc["verdict"] = {"not_below_on_both_l2sq_sets": not_below, "above_on_one_l2sq_set": above, "default_on": bool(l2) and not_below and above,
                      "all_checksums_equal": all(s["checksums_equal"] for s in doc["sets"].values())}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc["verdict"]))
    print(json.dumps({k: {"median_vectors_per_s": s["median_vectors_per_s"], "mode0_spread": s["mode0_spread"], "median_walk_ms": s["median_walk_ms"]}
                      for k, s in doc["sets"].items()}))


if __name__ == "__main__":
    main()
