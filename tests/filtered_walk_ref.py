"""CPU restatement of filtered k-NN search (include/lantern_gpu.h "Filtered search") over an exported graph.

Test infrastructure, not part of the product.  `graph` is the dict of OracleIndex.export_graph() / GpuIndex.export_graph();
`dist` is the [nq][n] matrix of every (query, row) distance in the device's summation order (distance_matrix below, from
oracle.bruteforce over all n rows), so every key here has the bits the device gives it.  Keys are ordered by (distance, slot).
"""
from __future__ import annotations

import bisect

import numpy as np

EMPTY = 0xFFFFFFFF


def distance_matrix(oracle, base, queries, metric, sum_mode, nthreads=1):
    """[nq][n] float32: oracle.bruteforce with k = n, scattered back to slot order.

    Quantised storage: pass the rows and queries AS STORED and the matching summation order -- oracle.round_f16 of both with
    SUM_WAVE64_F16, oracle.quantize_i8 of both with SUM_I8, and for a b1 index the packed sign-bit words with metric "hamming" (index
    metric l2sq) or "cos_b1" (index metric cos) and SUM_SEQ, as tests/test_gpu_quantized_indexes.py does."""
    n = base.shape[0]
    ids, d = oracle.bruteforce(base, queries, n, metric, sum_mode, nthreads)
    assert all(np.array_equal(np.sort(row), np.arange(n, dtype=ids.dtype)) for row in ids), "bruteforce with k = n returns every row once"
    out = np.empty((ids.shape[0], n), dtype=np.float32)
    np.put_along_axis(out, ids.astype(np.int64), d, axis=1)
    return out


def _list(graph, slot, level, M):
    if level == 0:
        row = graph["nbr0"][slot]
    else:
        row = graph["upper_nbr"][int(graph["upper_off"][slot]) + level - 1]
    out = []
    for x in row[: (2 * M if level == 0 else M)]:
        if int(x) == EMPTY:
            break
        out.append(int(x))
    return out


def greedy_descent(graph, drow, M):
    """search_for_one_ over levels max_level .. 1: (start slot, D)."""
    cur = int(graph["entry_slot"])
    best = float(drow[cur])
    D = 1
    for level in range(int(graph["max_level"]), 0, -1):
        while True:
            nbrs = _list(graph, cur, level, M)
            D += len(nbrs)
            changed = False
            for x in nbrs:  # first strictly-closer wins, in list order
                if drow[x] < best:
                    best, cur, changed = float(drow[x]), x, True
            if not changed:
                break
    return cur, D


def walk(graph, drow, allowed, M, k, ef, skip=0, cand_cap=None):
    """The WALK path for one query: (slots, distances, D, E).  allowed: bool[n]; cand_cap None = max(4 expansion, 256)."""
    exp = max(ef, k + skip)
    C = max(cand_cap, exp) if cand_cap else max(4 * exp, 256)
    start, D = greedy_descent(graph, drow, M)
    key = lambda s: (float(drow[s]), s)
    top, nxt = [], []  # sorted lists of keys
    visited = {start}
    D += 1
    nxt.append(key(start))
    if allowed[start]:
        top.append(key(start))
    E = 0
    while nxt:
        c = nxt[0]
        if len(top) == exp and top[-1] < c:
            break
        nxt.pop(0)
        E += 1
        for x in _list(graph, c[1], 0, M):
            if x in visited:
                continue
            visited.add(x)
            D += 1
            kx = key(x)
            if len(top) < exp or kx < top[-1]:
                if len(nxt) < C:
                    bisect.insort(nxt, kx)
                elif kx < nxt[-1]:
                    nxt.pop()
                    bisect.insort(nxt, kx)
                if allowed[x]:
                    bisect.insort(top, kx)
                    if len(top) > exp:
                        top.pop()
    ans = top[skip: skip + k]
    return [s for _, s in ans], [d for d, _ in ans], D, E


def exact(drow, allowed, k, skip=0):
    """The EXACT path for one query: (slots, distances, D, E = 0)."""
    idx = np.flatnonzero(allowed)
    keys = sorted((float(drow[s]), int(s)) for s in idx)
    ans = keys[skip: skip + k]
    return [s for _, s in ans], [d for d, _ in ans], int(idx.size), 0


def search(graph, dist, allowed, M, k, ef, skip=0, cand_cap=None, path="walk"):
    """Every query: (slots [nq][k] EMPTY-padded, dists [nq][k] +inf-padded, counts, D, E)."""
    nq = dist.shape[0]
    slots = np.full((nq, k), EMPTY, dtype=np.uint32)
    dists = np.full((nq, k), np.inf, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    D = np.zeros(nq, dtype=np.uint64)
    E = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        if path == "walk":
            s, d, D[q], E[q] = walk(graph, dist[q], allowed, M, k, ef, skip, cand_cap)
        else:
            s, d, D[q], E[q] = exact(dist[q], allowed, k, skip)
        counts[q] = len(s)
        slots[q, : len(s)] = s
        dists[q, : len(d)] = np.array(d, dtype=np.float32)
    return slots, dists, counts, D, E
