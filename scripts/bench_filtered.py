#!/usr/bin/env python
"""Filtered search on one MI355X: the filtered walk against k_search, and the walk against the exact pass over the allowed rows.

    python scripts/bench_filtered.py [--n 1000000] [--dim 768] [--nq 8192] [--nq-exact 256] [--reps 3]

Clustered rows (lantern_amd/synth.py), f32 L2sq, M = 16, ef_construction = 128, ef = 64, k = 10.  Prints ONE JSON line:
  * all_allowed: q/s of the filtered walk and of k_search (search_batch_device), same queries, alternated;
  * per filter (random and cluster-correlated at 50 / 10 / 1 / 0.1 %): q/s of the walk and of the exact path, mean D of the walk,
    recall@10 of the walk against the exact path (which is the filtered exact truth, bit for bit);
  * the crossover on the random filters (log-log interpolation of walk / exact q/s between the two legs around 1), as
    exact_factor = allowed^2 / (ef * n) -- the constant of the auto path rule.
The exact path reads allowed x row bytes per query, so it is timed on --nq-exact queries.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lantern_amd import capi, hip, synth  # noqa: E402


def cluster_ids(n, dim):
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
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--nq", type=int, default=8192)
    p.add_argument("--nq-exact", type=int, default=256)
    p.add_argument("--reps", type=int, default=3)
    a = p.parse_args()
    M, efc, ef, k = 16, 128, 64, 10
    t0 = time.time()
    base = synth.base_rows("clustered", a.n, a.dim)
    cluster = cluster_ids(a.n, a.dim)
    queries = synth.query_maker("clustered", a.dim)(np.random.default_rng(12345), a.nq)
    ix = capi.GpuIndex("l2sq", a.dim, M=M, ef_construction=efc, ef=ef, seed=42)
    ix.reserve(a.n)
    ix.add_many(np.arange(a.n, dtype=np.uint64) + 1, base)
    ix.flush()
    build_s = time.time() - t0
    rows = ix.device_query_rows(queries)
    dq = hip.Buffer.from_numpy(rows)
    nq = a.nq
    lab, dist, slot = hip.Buffer(nq * k * 8), hip.Buffer(nq * k * 4), hip.Buffer(nq * k * 4)
    cnt, D, E = hip.Buffer(nq * 4), hip.Buffer(nq * 8), hip.Buffer(nq * 8)

    def timed(fn, n_q):
        best = None
        for _ in range(a.reps):
            s, e = hip.Event(), hip.Event()
            s.record()
            fn(n_q)
            e.record()
            hip.synchronize()
            ms = s.elapsed_ms(e)
            best = ms if best is None else min(best, ms)
        return n_q / (best / 1e3)

    def plain(n_q):
        ix.search_batch_device(dq.ptr, n_q, k, ef, 0, lab.ptr, dist.ptr, slot.ptr, cnt.ptr, D.ptr, E.ptr, query_stride=rows.strides[0])

    def filtered(f):
        return lambda n_q: ix.search_batch_filtered_device(f, dq.ptr, rows.strides[0], n_q, k, ef, 0, lab.ptr, dist.ptr, slot.ptr, cnt.ptr,
                                                           D.ptr, E.ptr)

    out = {"workload": f"clustered {a.n}x{a.dim} f32 l2sq M={M} efc={efc} ef={ef} k={k}", "queries": nq, "queries_exact": a.nq_exact,
           "build_seconds": build_s}
    everyone = ix.filter_from_bitmap(np.ones(a.n, dtype=bool))
    ix.set_filter_policy("walk")
    walk_qps, plain_qps = [], []
    for _ in range(3):  # alternated
        plain(nq)
        plain_qps.append(timed(plain, nq))
        walk_qps.append(timed(filtered(everyone), nq))
    out["all_allowed"] = {"k_search_qps": plain_qps, "filtered_walk_qps": walk_qps}
    everyone.close()

    rng = np.random.default_rng(7)
    legs, crossings = [], []
    member = cluster == 0  # cluster-correlated filters: rows of cluster 0 (6.25 % of the rows; larger sets fall back to random rows)
    for kind in ("random", "cluster"):
        for sel in (0.5, 0.1, 0.01, 0.001):
            if kind == "random":
                allowed = rng.random(a.n) < sel
            else:
                pool = np.flatnonzero(member) if sel * a.n <= member.sum() else np.arange(a.n)
                allowed = np.zeros(a.n, dtype=bool)
                allowed[rng.choice(pool, size=min(pool.size, max(1, int(sel * a.n))), replace=False)] = True
            f = ix.filter_from_bitmap(allowed)
            ix.set_filter_policy("exact")
            exact_qps = timed(filtered(f), a.nq_exact)
            filtered(f)(a.nq_exact)
            hip.synchronize()
            truth = slot.download((a.nq_exact, k), np.uint32).copy()
            ix.set_filter_policy("walk")
            walk_q = timed(filtered(f), nq)
            hip.synchronize()
            got = slot.download((nq, k), np.uint32)[: a.nq_exact]
            d_mean = float(D.download(nq, np.uint64).mean())
            rec = float(np.mean([len(set(got[i].tolist()) & set(t for t in truth[i].tolist() if t != capi.EMPTY)) /
                                 max(1, sum(1 for t in truth[i].tolist() if t != capi.EMPTY)) for i in range(a.nq_exact)]))
            legs.append({"filter": kind, "selectivity": sel, "allowed": int(f.count), "walk_qps": walk_q, "exact_qps": exact_qps,
                         "walk_mean_D": d_mean, "walk_recall_at_10": rec})
            crossings.append((int(f.count), walk_q > exact_qps))
            f.close()
    out["filters"] = legs
    # the crossover on the random filters: log(walk / exact q/s) interpolated linearly in log(allowed) between the two legs around zero
    pts = sorted((np.log(l["allowed"]), np.log(l["walk_qps"] / l["exact_qps"])) for l in legs if l["filter"] == "random")
    cross = None
    for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
        if y0 <= 0 < y1:
            cross = float(np.exp(x0 + (x1 - x0) * (-y0) / (y1 - y0)))
    out["crossover_allowed"] = cross
    out["crossover_exact_factor"] = cross ** 2 / (ef * a.n) if cross else None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
