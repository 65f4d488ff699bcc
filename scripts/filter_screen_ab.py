#!/usr/bin/env python
"""Same-box A/B of the screened filtered exact pass (lantern_gpu_set_filter_screen; DESIGN.md 4.9 "Screened exact pass"): clustered
rows x dim f32 under l2sq, M 16, a batch of queries behind ONE filter on the exact path (forced), k = 10 -- with the switch at 0 and at
1, alternated inside every repetition.  Legs: 488, 7 812 and 125 000 random allowed rows, and the rows of one cluster.  Per call: the
wall and the four words of lantern_gpu_last_filtered_screen; per leg the answers of both settings must be equal bit for bit.  One JSON
document; the verdict applies the rule for a later default, as for the other switches:

    in every leg  median(wall, switch 1) <= median(wall, switch 0) + spread(switch 0),     spread = max - min of the switch-0 runs

    python scripts/filter_screen_ab.py --out profiles/filter_screen_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def cluster_ids(synth, n, dim):
    """the cluster of every row of synth.base_rows("clustered", n, dim): its draws replayed chunk by chunk"""
    r = np.random.default_rng(synth.BASE_SEED)
    out = np.empty(n, dtype=np.int64)
    for lo in range(0, n, synth.CLUSTER_CHUNK):
        m = min(synth.CLUSTER_CHUNK, n - lo)
        out[lo:lo + m] = r.integers(0, synth.CLUSTERS, m)
        r.standard_normal((m, synth.CLUSTER_LATENT), dtype=np.float32)
        r.standard_normal((m, dim), dtype=np.float32)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--M", type=int, default=16)
    p.add_argument("--efc", type=int, default=128)
    p.add_argument("--nq", type=int, default=8192)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    from lantern_amd import capi, hip, synth

    base = synth.base_rows("clustered", a.rows, a.dim)
    queries = synth.query_maker("clustered", a.dim)(np.random.default_rng(12345), a.nq)
    ix = capi.GpuIndex("l2sq", a.dim, M=a.M, ef_construction=a.efc, ef=64, seed=42)
    ix.reserve(a.rows)
    ix.add_many(np.arange(a.rows, dtype=np.uint64) + 1, base)
    ix.flush()
    ix.set_filter_policy("exact")
    rows = ix.device_query_rows(queries)
    dq = hip.Buffer.from_numpy(rows)
    nq, k = a.nq, a.k
    slot, dist = hip.Buffer(nq * k * 4), hip.Buffer(nq * k * 4)

    def call(f):
        hip.synchronize()
        t = time.perf_counter()
        ix.search_batch_filtered_device(f, dq.ptr, rows.strides[0], nq, k, d_dists=dist.ptr, d_slots=slot.ptr)
        hip.synchronize()
        wall = time.perf_counter() - t
        return wall, slot.download((nq, k), np.uint32), dist.download((nq, k), np.uint32)

    rng = np.random.default_rng(7)
    sets = []
    for count in (488, 7812, 125000):
        allowed = np.zeros(a.rows, dtype=bool)
        allowed[rng.choice(a.rows, size=min(count, a.rows), replace=False)] = True
        sets.append((f"random {count}", allowed))
    sets.append(("one cluster", cluster_ids(synth, a.rows, a.dim) == 0))
    doc = {"workload": f"clustered {a.rows}x{a.dim} f32 l2sq M={a.M} efc={a.efc}, {nq} queries behind one filter, exact path forced, k={k}",
           "reps": a.reps, "legs": {}}
    for name, allowed in sets:
        f = ix.filter_from_bitmap(allowed)
        answers, runs = {}, []
        for on in (0, 1):  # warm both kernels' code objects and LDS opt-in
            ix.set_filter_screen(on)
            call(f)
        for rep in range(a.reps):
            for on in ((0, 1) if rep % 2 == 0 else (1, 0)):
                ix.set_filter_screen(on)
                wall, s, d = call(f)
                answers[on] = (s, d)
                runs.append({"rep": rep, "switch": on, "wall_s": wall, "queries_per_s": nq / wall, "diagnostics": ix.last_filtered_screen()})
                print(f"[{name}] rep {rep} switch {on}: {wall * 1e3:.2f} ms  {runs[-1]['diagnostics']}", file=sys.stderr, flush=True)
        w0, w1 = [r["wall_s"] for r in runs if r["switch"] == 0], [r["wall_s"] for r in runs if r["switch"] == 1]
        diag = [r["diagnostics"] for r in runs if r["switch"] == 1][-1]
        doc["legs"][name] = {"allowed": int(allowed.sum()), "runs": runs, "median_wall_s": {"switch0": statistics.median(w0), "switch1": statistics.median(w1)},
                             "switch0_spread_s": max(w0) - min(w0), "answers_equal": bool(np.array_equal(answers[0][0], answers[1][0]) and np.array_equal(answers[0][1], answers[1][1])),
                             "rejected_share_of_bounded": diag["rejected"] / diag["bounded"] if diag["bounded"] else None,
                             "ns_per_query_row": {"switch0": statistics.median(w0) / nq / max(int(allowed.sum()), 1) * 1e9,
                                                  "switch1": statistics.median(w1) / nq / max(int(allowed.sum()), 1) * 1e9}}
        f.close()
    ix.set_filter_screen(0)
    legs = doc["legs"].values()
    doc["verdict"] = {"not_above_in_every_leg": all(leg["median_wall_s"]["switch1"] <= leg["median_wall_s"]["switch0"] + leg["switch0_spread_s"] for leg in legs),
                      "all_answers_equal": all(leg["answers_equal"] for leg in legs)}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc["verdict"]))
    print(json.dumps({name: {"median_wall_s": leg["median_wall_s"], "switch0_spread_s": leg["switch0_spread_s"], "ns_per_query_row": leg["ns_per_query_row"],
                             "rejected_share_of_bounded": leg["rejected_share_of_bounded"]} for name, leg in doc["legs"].items()}))
    ix.close()


if __name__ == "__main__":
    main()
