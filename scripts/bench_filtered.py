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

    python scripts/bench_filtered.py --each [--nq-each 256]

measures the per-query-filter call instead (lantern_gpu_search_batch_filtered_each_device) and prints ONE JSON line:
  * distinct_filters: --nq-each queries, each with its OWN random filter, at 10 % (walk path) and at 0.1 % (exact path): one per-query
    call against the only way the single-filter API answers them -- one one-query call per filter; wall-clock queries/s of both,
    alternated, every repeat listed;
  * shared_filter: ONE 10 % filter for --nq queries through the per-query call against search_batch_filtered_device (the same walks;
    the per-query form pays the descriptor reads and the selection list): queries/s of both, alternated, and their ratio.

    python scripts/bench_filtered.py --each-params [--nq-each 256]

measures the per-query-filter call with per-query (k, ef) (lantern_gpu_search_batch_filtered_each_params_device) and prints
ONE JSON line: --nq-each queries, each with its OWN random filter, four distinct (k, ef) among them, at 10 % (walk path) and at 0.1 %
(exact path): ONE call against the only way the uniform per-query-filter API answers the batch -- one
lantern_gpu_search_batch_filtered_each_device call per distinct (k, ef); wall-clock queries/s of both, alternated, every repeat listed.

    python scripts/bench_filtered.py --seeds 0,64,256

measures the seeded walk (lantern_gpu_set_filter_seeds) and prints ONE JSON line: per filter -- the random and
cluster-correlated ones above, and the rows of one whole cluster (1/16), of half a cluster and of four clusters -- and per seeds value,
the walk forced: q/s (the seeds values alternated within every repeat, every repeat listed), mean D, and recall@10 against the exact
path on the first --nq-exact queries.

    python scripts/bench_filtered.py --compact [--pq-subvectors 96] [--pq-centroids 256]

measures filtered search on a COMPACT pq index (lantern_gpu_set_filter_compact; DESIGN.md 4.9 "Compact pq indexes") and prints ONE JSON
line: the same pq index twice, expanded and compact; per filter (all rows, random 50 / 10 / 1 / 0.1 %) and per row routine -- "expanded"
(the decodings in HBM), "decode" (rows decoded on the fly) and "adc" (LANTERN_GPU_PQ_ADC=1) -- q/s of the forced walk and of the forced
exact path (the routines alternated within every repeat, every repeat listed), mean D of the walk, recall@10 of the walk against the
same routine's exact path, and per routine the interpolated walk / exact crossover as exact_factor = allowed^2 / (ef * n).

    python scripts/bench_filtered.py --dense

measures the exact path's DENSE ROUTE (lantern_gpu_set_filter_dense; DESIGN.md 4.9 "Dense exact path") and prints ONE JSON line: per filter
(random 50 / 10 / 1 / 0.1 % and the rows of one whole cluster) and per batch size (8192, 1024, 256, 64 queries behind the one filter) the
wall-clock milliseconds per call of the forced walk, of today's exact pass (setting 0) and of the dense route, alternated within each of
--reps repeats, every repeat listed, with their medians; recall@10 of the walk against the exact answer; whether the dense route's slots
equal the exact pass's; the gather and contraction launches of one more dense call (lantern_gpu_dense_profile) and its certified /
recomputed queries.  Then: a filter of 18 900 rows (today's walk / exact crossover) at 1 .. 256 queries, exact against dense, and the
smallest batch at which the dense route is not slower; per batch size the allowed count at which the dense route meets the walk
(log-log interpolation over the random filters) as exact_factor = allowed^2 / (ef * n); one f16 and one i8 index over the same graph
at 10 %.

    python scripts/bench_filtered.py --each-dense

measures the dense route of the PER-QUERY-FILTER call (lantern_gpu_set_filter_dense_each; DESIGN.md 4.9 "Dense exact path, per-query
filters") and prints ONE JSON line: the rows imported under an empty graph (the exact path reads none), the path forced exact, --nq
queries interleaved over disjoint filters -- 8 filters x 1024 queries (n / 8 rows each), 128 x 64 (n / 128 rows), 2048 x 4 (500 rows) and
one filter of n / 10 rows behind every query -- and per case the wall-clock milliseconds of the same per-query call (device synchronised)
with the setting at 0 and at 2, alternated within each of --reps repeats after one warming repeat (and each timed call behind one untimed
call of its own mode), every repeat listed, with their medians; for the one-filter case also the single-filter dense route (fused) on
the same group; the dense run's diagnostic; whether the slots equal those of the setting at 0.  Run from a checkout of an earlier
commit, the same script times that build's call ("setting_0" only): the A/B against the parent commit is two processes, alternated by the caller; --setting-0-only makes this build's process do the
same (no dense call between its timed calls).  scripts/merge_each_dense_ab.py assembles the processes' lines into the profile file.
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


def each_legs(a, ix, rows, dq, bufs, k, ef):
    """The per-query-filter call against the single-filter API (module docstring)."""
    lab, dist, slot, cnt, D, E = bufs
    stride = rows.strides[0]

    def wall(fn, n_q):
        hip.synchronize()
        t = time.perf_counter()
        fn()
        hip.synchronize()
        return n_q / (time.perf_counter() - t)

    def each(filters, n_q):
        filters = capi.GpuIndex._filter_array(filters, n_q)  # (the handle array built once: the call is timed, not the list walk)
        return lambda: ix.search_batch_filtered_each_device(filters, dq.ptr, stride, n_q, k, ef, 0, lab.ptr, dist.ptr, slot.ptr, cnt.ptr, D.ptr, E.ptr)

    def one_by_one(filters):
        def fn():
            for i, f in enumerate(filters):  # one query, one filter, one launch: the rows of query i
                ix.search_batch_filtered_device(f, dq.ptr + i * stride, stride, 1, k, ef, 0, lab.ptr + i * k * 8, dist.ptr + i * k * 4,
                                                slot.ptr + i * k * 4, cnt.ptr + i * 4, D.ptr + i * 8, E.ptr + i * 8)
        return fn

    out = {"distinct_filters": [], "reps": a.reps}
    ix.set_filter_policy("auto")
    rng = np.random.default_rng(11)
    m = a.nq_each
    for sel in (0.1, 0.001):
        filters = [ix.filter_from_bitmap(rng.random(a.n) < sel) for _ in range(m)]
        call = each(filters, m)
        call()
        one_by_one(filters[:8])()
        together, alone = [], []
        for _ in range(a.reps):  # alternated
            together.append(wall(call, m))
            alone.append(wall(one_by_one(filters), m))
        out["distinct_filters"].append({"selectivity": sel, "queries": m, "filters": m, "regime": ix.last_filtered_each(),
                                        "per_query_call_qps": together, "one_call_per_filter_qps": alone,
                                        "speedup_best": max(together) / max(alone)})
        for f in filters:
            f.close()
    f = ix.filter_from_bitmap(rng.random(a.n) < 0.1)
    nq = a.nq
    single = lambda: ix.search_batch_filtered_device(f, dq.ptr, stride, nq, k, ef, 0, lab.ptr, dist.ptr, slot.ptr, cnt.ptr, D.ptr, E.ptr)  # noqa: E731
    shared = each([f] * nq, nq)
    single()
    shared()
    s_qps, e_qps = [], []
    for _ in range(max(a.reps, 3)):
        s_qps.append(wall(single, nq))
        e_qps.append(wall(shared, nq))
    out["shared_filter"] = {"selectivity": 0.1, "queries": nq, "single_filter_qps": s_qps, "per_query_call_qps": e_qps,
                            "ratio_best": max(e_qps) / max(s_qps), "single_filter_spread": (max(s_qps) - min(s_qps)) / max(s_qps)}
    return out


EACH_PARAMS_ROWS = [(10, 64), (20, 64), (10, 128), (40, 200)]  # the four (k, ef) of --each-params: query i takes row i % 4


def each_params_legs(a, ix, rows, k_stride):
    """One per-query-filter call with per-query (k, ef) against one uniform per-query-filter call per distinct (k, ef) (module docstring)."""
    stride, m = rows.strides[0], a.nq_each
    classes = [[i for i in range(m) if i % 4 == c] for c in range(4)]
    params = capi.query_params([EACH_PARAMS_ROWS[i % 4] + (0,) for i in range(m)])
    dq = hip.Buffer.from_numpy(np.ascontiguousarray(rows[:m]))
    dq_c = [hip.Buffer.from_numpy(np.ascontiguousarray(rows[:m][idx])) for idx in classes]  # (each class's queries side by side)
    lab, dist, slot = hip.Buffer(m * k_stride * 8), hip.Buffer(m * k_stride * 4), hip.Buffer(m * k_stride * 4)
    cnt, D, E = hip.Buffer(m * 4), hip.Buffer(m * 8), hip.Buffer(m * 8)

    def wall(fn):
        hip.synchronize()
        t = time.perf_counter()
        fn()
        hip.synchronize()
        return m / (time.perf_counter() - t)

    out = {"each_params": [], "reps": a.reps, "rows": EACH_PARAMS_ROWS}
    ix.set_filter_policy("auto")
    rng = np.random.default_rng(11)
    for sel in (0.1, 0.001):
        filters = [ix.filter_from_bitmap(rng.random(a.n) < sel) for _ in range(m)]
        F = capi.GpuIndex._filter_array(filters, m)
        F_c = [capi.GpuIndex._filter_array([filters[i] for i in idx], len(idx)) for idx in classes]

        def one_call():
            ix.search_batch_filtered_each_params_device(F, dq.ptr, stride, m, params, k_stride, lab.ptr, dist.ptr, slot.ptr, cnt.ptr, D.ptr, E.ptr)

        def four_calls():
            at = q0 = 0
            for c, idx in enumerate(classes):  # class c's answers behind those of the classes before it
                k, ef = EACH_PARAMS_ROWS[c]
                ix.search_batch_filtered_each_device(F_c[c], dq_c[c].ptr, stride, len(idx), k, ef, 0, lab.ptr + at * 8, dist.ptr + at * 4,
                                                     slot.ptr + at * 4, cnt.ptr + q0 * 4, D.ptr + q0 * 8, E.ptr + q0 * 8)
                at += len(idx) * k
                q0 += len(idx)

        one_call()
        regime, carve = ix.last_filtered_each(), ix.last_filtered_each_params()
        mean_D = float(D.download(m, np.uint64).mean())
        four_calls()
        together, apart = [], []
        for _ in range(a.reps):  # alternated
            together.append(wall(one_call))
            apart.append(wall(four_calls))
        out["each_params"].append({"selectivity": sel, "queries": m, "filters": m, "regime": regime, "carve": carve, "mean_D": mean_D,
                                   "one_call_qps": together, "one_call_per_k_ef_qps": apart, "ratio_best": max(together) / max(apart)})
        for f in filters:
            f.close()
    return out


def seeds_legs(a, ix, cluster, filtered, timed_once, slot, D, k):
    """The seeded walk per filter and seeds value (module docstring)."""
    values = [int(x) for x in a.seeds.split(",")]
    rng = np.random.default_rng(7)
    member = cluster == 0
    sets = []
    for kind in ("random", "cluster"):  # the filters of the standing set, drawn as main() draws them
        for sel in (0.5, 0.1, 0.01, 0.001):
            if kind == "random":
                allowed = rng.random(a.n) < sel
            else:
                pool = np.flatnonzero(member) if sel * a.n <= member.sum() else np.arange(a.n)
                allowed = np.zeros(a.n, dtype=bool)
                allowed[rng.choice(pool, size=min(pool.size, max(1, int(sel * a.n))), replace=False)] = True
            sets.append((kind, sel, allowed))
    half = member & (np.random.default_rng(8).random(a.n) < 0.5)
    sets += [("one_cluster", 1 / 16, member), ("half_cluster", 1 / 32, half), ("four_clusters", 1 / 4, cluster < 4)]
    legs = []
    for kind, sel, allowed in sets:
        f = ix.filter_from_bitmap(allowed)
        ix.set_filter_seeds(0)
        ix.set_filter_policy("exact")
        filtered(f)(a.nq_exact)
        hip.synchronize()
        truth = [set(t for t in row.tolist() if t != capi.EMPTY) for row in slot.download((a.nq_exact, k), np.uint32)]
        ix.set_filter_policy("walk")
        leg = {"filter": kind, "selectivity": sel, "allowed": int(f.count), "seeds": {}}
        for v in values:
            ix.set_filter_seeds(v)
            filtered(f)(a.nq)  # warm, and the answers
            hip.synchronize()
            got = slot.download((a.nq, k), np.uint32)[: a.nq_exact]
            rec = float(np.mean([len(set(got[i].tolist()) & truth[i]) / max(1, len(truth[i])) for i in range(a.nq_exact)]))
            leg["seeds"][str(v)] = {"walk_qps": [], "walk_mean_D": float(D.download(a.nq, np.uint64).mean()), "walk_recall_at_10": rec,
                                    "regime": ix.last_filtered_seeds()}
        for _ in range(a.reps):  # alternated
            for v in values:
                ix.set_filter_seeds(v)
                leg["seeds"][str(v)]["walk_qps"].append(timed_once(filtered(f), a.nq))
        legs.append(leg)
        f.close()
    ix.set_filter_seeds(0)
    ix.set_filter_policy("auto")
    return {"seeds_values": values, "reps": a.reps, "filters": legs}


def compact_legs(a, base, queries, M, efc, ef, k):
    """Filtered search on the expanded and on the compact form of one pq index (module docstring)."""
    S, C = a.pq_subvectors, a.pq_centroids
    sub = a.dim // S
    crng = np.random.default_rng(5)
    cb = np.zeros((C, a.dim), dtype=np.float32)
    for sv in range(S):
        cb[:, sv * sub:(sv + 1) * sub] = base[crng.choice(a.n, size=C, replace=False), sv * sub:(sv + 1) * sub]
    index = {}
    t0 = time.time()
    for form in ("expanded", "compact"):
        ix = capi.GpuIndex("l2sq", a.dim, M=M, ef_construction=efc, ef=ef, seed=42, pq_codebook=cb, num_subvectors=S)
        ix.reserve(a.n)
        ix.add_many(np.arange(a.n, dtype=np.uint64) + 1, base)
        ix.flush()
        index[form] = ix
    assert index["expanded"].checksum() == index["compact"].checksum()
    index["compact"].pq_compact()
    index["compact"].set_filter_compact(1)
    build_s = time.time() - t0
    routines = {"expanded": (index["expanded"], "0"), "decode": (index["compact"], "0"), "adc": (index["compact"], "1")}
    rows = index["expanded"].device_query_rows(queries)
    stride, nq = rows.strides[0], a.nq
    dq = hip.Buffer.from_numpy(rows)
    lab, dist, slot = hip.Buffer(nq * k * 8), hip.Buffer(nq * k * 4), hip.Buffer(nq * k * 4)
    cnt, D, E = hip.Buffer(nq * 4), hip.Buffer(nq * 8), hip.Buffer(nq * 8)

    def run(name, f, path, n_q):
        ix, env = routines[name]
        os.environ["LANTERN_GPU_PQ_ADC"] = env
        ix.set_filter_policy(path)
        s, e = hip.Event(), hip.Event()
        s.record()
        ix.search_batch_filtered_device(f, dq.ptr, stride, n_q, k, ef, 0, lab.ptr, dist.ptr, slot.ptr, cnt.ptr, D.ptr, E.ptr)
        e.record()
        hip.synchronize()
        return n_q / (s.elapsed_ms(e) / 1e3)

    rng = np.random.default_rng(7)
    legs = []
    for sel in (1.0, 0.5, 0.1, 0.01, 0.001):
        allowed = np.ones(a.n, dtype=bool) if sel == 1.0 else rng.random(a.n) < sel
        filt = {"expanded": index["expanded"].filter_from_bitmap(allowed), "compact": index["compact"].filter_from_bitmap(allowed)}
        leg = {"selectivity": sel, "allowed": int(allowed.sum()), "routines": {}}
        for name in routines:
            f = filt["expanded" if name == "expanded" else "compact"]
            run(name, f, "exact", a.nq_exact)  # warm, and the truth of this routine
            truth = [set(t for t in row.tolist() if t != capi.EMPTY) for row in slot.download((a.nq_exact, k), np.uint32)]
            run(name, f, "walk", nq)
            got = slot.download((nq, k), np.uint32)[: a.nq_exact]
            rec = float(np.mean([len(set(got[i].tolist()) & truth[i]) / max(1, len(truth[i])) for i in range(a.nq_exact)]))
            leg["routines"][name] = {"walk_qps": [], "exact_qps": [], "walk_mean_D": float(D.download(nq, np.uint64).mean()), "walk_recall_at_10": rec,
                                     "launch": routines[name][0].last_filtered_launch()}
        for _ in range(a.reps):  # alternated
            for name in routines:
                f = filt["expanded" if name == "expanded" else "compact"]
                leg["routines"][name]["walk_qps"].append(run(name, f, "walk", nq))
                leg["routines"][name]["exact_qps"].append(run(name, f, "exact", a.nq_exact))
        legs.append(leg)
        for f in filt.values():
            f.close()
    os.environ.pop("LANTERN_GPU_PQ_ADC", None)
    # per routine the crossover: log(walk / exact q/s, best of the repeats) interpolated linearly in log(allowed) between the two legs around zero
    cross = {}
    for name in routines:
        pts = sorted((np.log(l["allowed"]), np.log(max(l["routines"][name]["walk_qps"]) / max(l["routines"][name]["exact_qps"]))) for l in legs)
        at = None
        for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
            if y0 <= 0 < y1:
                at = float(np.exp(x0 + (x1 - x0) * (-y0) / (y1 - y0)))
        cross[name] = {"allowed": at, "exact_factor": at ** 2 / (ef * a.n) if at else None}
    return {"workload": f"clustered {a.n}x{a.dim} pq {S} subvectors x {C} centroids, l2sq M={M} efc={efc} ef={ef} k={k}", "queries": nq,
            "queries_exact": a.nq_exact, "build_seconds_both": build_s, "reps": a.reps, "memory_rows_bytes": {n_: index[n_].memory_usage()[0] for n_ in index},
            "filters": legs, "crossover": cross}


def dense_legs(a, ix, base, cluster, queries, k, ef):
    """--dense: the exact path's dense route (lantern_gpu_set_filter_dense) against the walk and today's exact pass"""
    def bench_index(index, q, filters, batches, walk=True):
        rows = index.device_query_rows(q)
        dq = hip.Buffer.from_numpy(rows)
        nq = rows.shape[0]
        slot, D = hip.Buffer(nq * k * 4), hip.Buffer(nq * 8)

        def call(f, n_q):
            index.search_batch_filtered_device(f, dq.ptr, rows.strides[0], n_q, k, ef, 0, None, None, slot.ptr, None, D.ptr, None)
            hip.synchronize()

        modes = {"walk": ("walk", 0), "exact": ("exact", 0), "dense": ("exact", 1)}
        out = []
        for name, allowed in filters:
            f = index.filter_from_bitmap(allowed)
            for n_q in batches:
                wall = {m: [] for m in modes if walk or m != "walk"}
                answers = {}
                for _ in range(a.reps):  # the legs alternated within every repeat
                    for m in wall:
                        index.set_filter_policy(modes[m][0])
                        index.set_filter_dense(modes[m][1])
                        slot.upload(np.full(slot.nbytes, 0xA5, dtype=np.uint8))  # (untimed: the answers compared below are this call's own)
                        hip.synchronize()
                        t = time.perf_counter()
                        call(f, n_q)
                        wall[m].append((time.perf_counter() - t) * 1e3)
                        answers[m] = slot.download((nq, k), np.uint32)[:min(n_q, a.nq_exact)].copy()
                leg = {"filter": name, "allowed": int(f.count), "queries": n_q, "wall_ms": wall,
                       "median_ms": {m: float(np.median(v)) for m, v in wall.items()}}
                leg["qps"] = {m: n_q / (v / 1e3) for m, v in leg["median_ms"].items()}
                leg["dense_equals_exact"] = bool(np.array_equal(answers["dense"], answers["exact"]))
                if walk:
                    truth = answers["exact"]
                    leg["walk_recall_at_10"] = float(np.mean([len(set(answers["walk"][i].tolist()) & set(t for t in truth[i].tolist() if t != capi.EMPTY)) /
                                                              max(1, sum(1 for t in truth[i].tolist() if t != capi.EMPTY)) for i in range(truth.shape[0])]))
                # one more dense call under the launch profile: the gather and the contraction launch by launch, and the certificate
                index.set_filter_policy("exact")
                index.set_filter_dense(1)
                s0 = index.filter_dense_stats()
                capi.dense_profile(True)
                call(f, n_q)
                prof = capi.dense_profile(False)
                s1 = index.filter_dense_stats()
                index.set_filter_dense(0)
                leg["gather_ms"] = [float(l["ms"]) for l in prof if l["gather"]]
                leg["gather_rows"] = [int(l["cols"]) for l in prof if l["gather"]]
                leg["contraction_ms"] = [float(l["ms"]) for l in prof if not l["gather"]]
                leg["certified"], leg["recomputed"] = s1["certified"] - s0["certified"], s1["recomputed"] - s0["recomputed"]
                out.append(leg)
            f.close()
        index.set_filter_policy("auto")
        return out

    rng = np.random.default_rng(7)
    filters = [(f"random {sel}", rng.random(a.n) < sel) for sel in (0.5, 0.1, 0.01, 0.001)] + [("cluster 0", cluster == 0)]
    batches = [b for b in (8192, 1024, 256, 64) if b <= a.nq]
    out = {"legs": bench_index(ix, queries, filters, batches)}
    # where today's crossover lies (18.9 k allowed rows): the smallest batch at which the dense route is not slower than the exact pass
    at_cross = np.zeros(a.n, dtype=bool)
    at_cross[rng.choice(a.n, size=min(a.n, 18900), replace=False)] = True
    out["at_crossover"] = bench_index(ix, queries, [("random 18900 rows", at_cross)], [1, 2, 4, 8, 16, 32, 64, 128, 256], walk=False)
    ok = [l["queries"] for l in out["at_crossover"] if l["median_ms"]["dense"] <= l["median_ms"]["exact"]]
    out["smallest_nq_dense_not_slower_at_crossover"] = min(ok) if ok else None
    # per batch size: the allowed count at which the dense route meets the walk (log-log interpolation over the random filters)
    meets = {}
    for b in batches:
        pts = sorted((np.log(l["allowed"]), np.log(l["median_ms"]["dense"] / l["median_ms"]["walk"])) for l in out["legs"]
                     if l["queries"] == b and l["filter"].startswith("random"))
        cross = None
        for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
            if y0 <= 0 < y1:
                cross = float(np.exp(x0 + (x1 - x0) * (-y0) / (y1 - y0)))
        if cross is None and pts:
            cross = "above the largest filter" if pts[-1][1] <= 0 else "below the smallest filter"
        meets[str(b)] = {"allowed": cross, "exact_factor": cross ** 2 / (ef * a.n) if isinstance(cross, float) else None}
    out["dense_meets_walk"] = meets
    # quantised rows: the same graph over f16 / i8 rows (the exact path reads no graph; the walk's is the f32 build's), 10 %
    g = ix.export_graph()
    tenth = [filters[1]]
    for storage in ("f16", "i8"):
        scale = np.float32(1.0)
        if storage == "i8":  # i8 storage keeps trunc(100 x) in [-100, 100]: rows scaled to fill that range
            scale = np.float32(0.99 / float(np.abs(base).max()))
        qix = capi.GpuIndex("l2sq", a.dim, M=ix.M, ef_construction=128, ef=ef, seed=42, quantization=storage)
        stored = base * scale
        qix.import_graph(np.trunc(np.clip(stored * np.float32(100), -100, 100)) if storage == "i8" else stored, g)
        out[storage] = bench_index(qix, queries * scale, tenth, [b for b in (8192, 256) if b <= a.nq])
        qix.close()
    return out


def each_dense_legs(a, base, queries, k, ef):
    """--each-dense: the per-query-filter call with groups of queries behind shared filters, path forced exact (module docstring)"""
    n, nq = a.n, a.nq
    # the exact path reads no graph: the rows are imported under an empty one (no build)
    g = {"levels": np.zeros(n, np.uint8), "nbr0": np.full((n, 8), 0xFFFFFFFF, np.uint32), "upper_off": np.full(n, 0xFFFFFFFF, np.uint32),
         "upper_nbr": np.zeros((0, 4), np.uint32), "labels": np.arange(n, dtype=np.uint64) + 1, "entry_slot": 0, "max_level": 0}
    ix = capi.GpuIndex("l2sq", a.dim, M=4, ef_construction=8, ef=ef, seed=42)
    ix.import_graph(base, g)
    ix.set_filter_policy("exact")
    # (the same script times a build from before the setting: "setting_0" only; --setting-0-only: this build, the setting never touched)
    has_setting = hasattr(ix, "set_filter_dense_each") and not a.setting_0_only
    rows = ix.device_query_rows(queries)
    dq = hip.Buffer.from_numpy(rows)
    slot, D = hip.Buffer(nq * k * 4), hip.Buffer(nq * 8)
    perm = np.random.default_rng(7).permutation(n)
    cases = [("8 filters x 1024 queries", 8, n // 8), ("128 filters x 64 queries", 128, n // 128), ("2048 filters x 4 queries", 2048, min(500, n // 2048)),
             ("1 filter x 8192 queries at 10 %", 1, n // 10)]
    out = []
    for name, parts, rows_each in cases:
        filters = []
        for p in range(parts):  # disjoint sets, as tenants are
            allowed = np.zeros(n, dtype=bool)
            allowed[perm[p * rows_each:(p + 1) * rows_each]] = True
            filters.append(ix.filter_from_bitmap(allowed))
        F = capi.GpuIndex._filter_array([filters[i % parts] for i in range(nq)], nq)  # interleaved: query i stands behind filter i mod parts

        def each_call():
            ix.search_batch_filtered_each_device(F, dq.ptr, rows.strides[0], nq, k, ef, 0, None, None, slot.ptr, None, D.ptr, None)
            hip.synchronize()

        def single_call():
            ix.search_batch_filtered_device(filters[0], dq.ptr, rows.strides[0], nq, k, ef, 0, None, None, slot.ptr, None, D.ptr, None)
            hip.synchronize()

        modes = {"setting_0": (0, 0, each_call)}
        if has_setting:
            modes["setting_on"] = (2, 0, each_call)
            if parts == 1:
                modes["single_filter_dense"] = (0, 1, single_call)  # the fused single-filter route on the same group: the price of running unfused
        wall, answers, diag = {m: [] for m in modes}, {}, {}
        for rep in range(a.reps + 1):  # (repeat 0 warms every mode -- the pooled blocks are allocated there -- and is not listed)
            for m, (each_min, single_min, call) in modes.items():
                if has_setting:
                    ix.set_filter_dense_each(each_min)
                ix.set_filter_dense(single_min)
                if rep:
                    call()  # (untimed: every timed call follows a call of its own mode, whatever the modes alternated with are)
                slot.upload(np.full(slot.nbytes, 0xA5, dtype=np.uint8))
                hip.synchronize()
                t = time.perf_counter()
                call()
                ms = (time.perf_counter() - t) * 1e3
                if rep:
                    wall[m].append(ms)
                answers[m] = slot.download((nq, k), np.uint32)[:a.nq_exact].copy()
                if m == "setting_on":
                    diag = ix.last_filtered_each_dense()
        ix.set_filter_dense(0)
        if has_setting:
            ix.set_filter_dense_each(0)
        leg = {"case": name, "filters": parts, "rows_per_filter": int(filters[0].count), "queries": nq, "wall_ms": wall,
               "median_ms": {m: float(np.median(v)) for m, v in wall.items()}, "dense_run": diag,
               "answers_equal": {m: bool(np.array_equal(answers[m], answers["setting_0"])) for m in modes}}
        out.append(leg)
        for f in filters:
            f.close()
    ix.close()
    return {"each_dense": out, "reps": a.reps, "has_setting": has_setting, "min_group": 2}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--nq", type=int, default=8192)
    p.add_argument("--nq-exact", type=int, default=256)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--each", action="store_true", help="the legs of the per-query-filter call")
    p.add_argument("--each-params", action="store_true", help="the legs of the per-query-filter call with per-query (k, ef)")
    p.add_argument("--nq-each", type=int, default=256)
    p.add_argument("--seeds", default="", help="comma-separated seeds values: the legs of the seeded walk")
    p.add_argument("--compact", action="store_true", help="the legs of filtered search on a compact pq index against its expanded form")
    p.add_argument("--dense", action="store_true", help="the legs of the exact path's dense route against the walk and today's exact pass")
    p.add_argument("--each-dense", action="store_true", help="the legs of the per-query-filter call's dense route (groups of queries behind shared filters)")
    p.add_argument("--setting-0-only", action="store_true", help="--each-dense: time the setting at 0 only and never touch it, as a build without it does")
    p.add_argument("--pq-subvectors", type=int, default=96)
    p.add_argument("--pq-centroids", type=int, default=256)
    a = p.parse_args()
    M, efc, ef, k = 16, 128, 64, 10
    t0 = time.time()
    base = synth.base_rows("clustered", a.n, a.dim)
    cluster = cluster_ids(a.n, a.dim)
    queries = synth.query_maker("clustered", a.dim)(np.random.default_rng(12345), a.nq)
    if a.compact:
        out = {"command": "python scripts/bench_filtered.py " + " ".join(sys.argv[1:])}
        out.update(compact_legs(a, base, queries, M, efc, ef, k))
        print(json.dumps(out))
        return
    if a.each_dense:
        out = {"command": "python scripts/bench_filtered.py " + " ".join(sys.argv[1:]), "workload": f"clustered {a.n}x{a.dim} f32 l2sq k={k}, path forced exact"}
        out.update(each_dense_legs(a, base, queries, k, ef))
        print(json.dumps(out))
        return
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
    if a.dense:
        out["command"] = "python scripts/bench_filtered.py " + " ".join(sys.argv[1:])
        out.update(dense_legs(a, ix, base, cluster, queries, k, ef))
        print(json.dumps(out))
        return
    if a.each_params:
        out["command"] = "python scripts/bench_filtered.py " + " ".join(sys.argv[1:])
        out.update(each_params_legs(a, ix, rows, max(r[0] for r in EACH_PARAMS_ROWS)))
        print(json.dumps(out))
        return
    if a.each:
        out["command"] = "python scripts/bench_filtered.py " + " ".join(sys.argv[1:])
        out.update(each_legs(a, ix, rows, dq, (lab, dist, slot, cnt, D, E), k, ef))
        print(json.dumps(out))
        return
    if a.seeds:
        def timed_once(fn, n_q):
            s, e = hip.Event(), hip.Event()
            s.record()
            fn(n_q)
            e.record()
            hip.synchronize()
            return n_q / (s.elapsed_ms(e) / 1e3)

        out["command"] = "python scripts/bench_filtered.py " + " ".join(sys.argv[1:])
        out.update(seeds_legs(a, ix, cluster, filtered, timed_once, slot, D, k))
        print(json.dumps(out))
        return
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
