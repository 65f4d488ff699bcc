"""A/B of the pre-selection of lantern_gpu_exact_search on a compact pq index (lantern_gpu_set_exact_adc; DESIGN.md 4.5 "Compact pq
indexes: ADC pre-selection"): wall per call of
  a  the compact index, the scan on: per-query tables + k_scan_adc
  b  the same index, the scan off: k_dense_pq
  c  the expanded twin: stored f32 rows (k_dense_f32)
alternated in one process; a repeat times a window of --calls calls that each end with the answers on the host.  The pre-selection
launches' own time (lantern_gpu_dense_profile: HIP events around every step) comes from a run of its own per leg.
Prints ONE JSON document (and writes it to --out).  Needs an MI355X.

    python scripts/exact_adc_ab.py --out profiles/exact_adc_ab.json
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
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--subvectors", type=int, default=96)
    p.add_argument("--centroids", type=int, default=256)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--nq", default="1,8,64,256,1024")
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--out", default="")
    a = p.parse_args()
    assert capi.device_count() > 0, "no HIP device"
    S, C, sub = a.subvectors, a.centroids, a.dim // a.subvectors
    base = synth.base_rows("clustered", a.n, a.dim)
    nqs = [int(x) for x in a.nq.split(",")]
    queries = synth.query_maker("clustered", a.dim)(np.random.default_rng(12345), max(nqs))
    crng = np.random.default_rng(5)
    cb = np.zeros((C, a.dim), dtype=np.float32)
    for sv in range(S):
        cb[:, sv * sub:(sv + 1) * sub] = base[crng.choice(a.n, size=C, replace=False), sv * sub:(sv + 1) * sub]
    t0 = time.time()
    make = lambda: capi.GpuIndex("l2sq", a.dim, M=4, ef_construction=16, ef=16, seed=42, pq_codebook=cb, num_subvectors=S)
    twin, ix = make(), make()
    twin.reserve(a.n)
    twin.add_many(np.arange(a.n, dtype=np.uint64) + 1, base)
    twin.flush()
    ix.load_buffer(twin.save_buffer())
    ix.pq_compact()
    ix.set_exact_compact(1)
    print(f"built in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    code_bytes = ix.memory_usage()[0]

    def call_a(q):
        ix.set_exact_adc(max(nqs))
        return ix.exact_search(q, a.k)

    def call_b(q):
        ix.set_exact_adc(0)
        return ix.exact_search(q, a.k)

    def call_c(q):
        return twin.exact_search(q, a.k)

    def timed(fn, q):
        t = time.perf_counter()
        for _ in range(a.calls):
            fn(q)  # (returns after the answers are on the host)
        return (time.perf_counter() - t) * 1e3 / a.calls

    def preselection_ms(fn, q):
        capi.dense_profile(True)
        fn(q)
        recs = [r for r in capi.dense_profile(False) if not r["gather"]]
        return {"launches": len(recs), "ms": sum(r["ms"] for r in recs)}

    plan = capi.plan_exact_adc(3, a.dim // 4, a.n, 1, a.k, True, True, 1, ix.memory_usage()[0] // a.n, 1, S, C)
    out = {"command": "python scripts/exact_adc_ab.py " + " ".join(sys.argv[1:]),
           "workload": f"clustered {a.n}x{a.dim} l2sq pq {S} subvectors x {C} centroids, exact k-NN k={a.k}", "reps": a.reps, "calls_per_rep": a.calls,
           "scan": {f: plan[f] for f in ("T", "block", "lds_bytes")},
           "row_bytes": {"compact": code_bytes, "expanded": twin.memory_usage()[0]}, "unit": "ms wall per call (median of reps; min, max)", "nq": {}}
    for nq in nqs:
        q = queries[:nq]
        before = capi.exact_adc_stats()["scans"]
        got, mid, want = call_a(q), call_b(q), call_c(q)  # (also the warm-up of the three legs at this shape)
        same = all(bool(np.array_equal(g[0], want[0]) and np.array_equal(g[1].view(np.uint32), want[1].view(np.uint32))) for g in (got, mid))
        t = {"a": [], "b": [], "c": []}
        for _ in range(a.reps):  # alternated
            for name, fn in (("a", call_a), ("b", call_b), ("c", call_c)):
                t[name].append(timed(fn, q))
        leg = {name: {"median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in t.items()}
        leg["a_and_b_equal_c_slots_and_bits"] = same
        leg["a_scanned"] = capi.exact_adc_stats()["scans"] > before
        leg["index_still_compact"] = ix.memory_usage()[0] == code_bytes
        leg["preselection"] = {"a": preselection_ms(call_a, q), "b": preselection_ms(call_b, q), "c": preselection_ms(call_c, q)}
        # the rule for a default value of max_queries: a's median not above b's by more than b's own min-max spread
        leg["a_within_b_spread"] = leg["a"]["median"] <= leg["b"]["median"] + (leg["b"]["max"] - leg["b"]["min"])
        out["nq"][str(nq)] = leg
        print(f"nq={nq}: {json.dumps(leg)}", file=sys.stderr, flush=True)
    ok = [int(n) for n in out["nq"] if out["nq"][n]["a_within_b_spread"]]
    out["largest_nq_within_rule"] = max(ok) if ok else 0
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
