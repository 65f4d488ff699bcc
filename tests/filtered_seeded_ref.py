"""CPU restatement of the SEEDED filtered walk (include/lantern_gpu.h "Filtered search" 5) over an exported graph.

Test infrastructure, not part of the product.  Arguments as tests/filtered_walk_ref.py: `graph` an exported graph, `drow` one query's
row of distance_matrix (the device's bits), `allowed` bool[n].  Everything is taken one slot at a time, as the definition states it;
the kernel's rounds and hops must give the same keys, D and E.
"""
from __future__ import annotations

import bisect

import numpy as np

from tests.filtered_walk_ref import EMPTY, _list, distance_matrix, exact, greedy_descent  # noqa: F401  (re-exported for the tests)


def seed_slots(allowed, seeds):
    """The seeds of a filter in the order the walk takes them: allow_slots[(j * count) // S'], j = 0 .. S'-1, S' = min(seeds, count)."""
    slots = np.flatnonzero(allowed)
    count = int(slots.size)
    S = min(int(seeds), count)
    return [int(slots[(j * count) // S]) for j in range(S)]


def seeded_walk(graph, drow, allowed, M, k, ef, seeds, skip=0, cand_cap=None):
    """The WALK path for one query with `seeds` seeds: (slots, distances, D, E).  seeds = 0 is filtered_walk_ref.walk."""
    exp = max(ef, k + skip)
    C = max(cand_cap, exp) if cand_cap else max(4 * exp, 256)
    start, D = greedy_descent(graph, drow, M)
    key = lambda s: (float(drow[s]), s)  # noqa: E731
    top, nxt = [], []  # sorted lists of keys
    visited = set()
    E = 0

    def admit(x, into_top):
        kx = key(x)
        if len(top) < exp or kx < top[-1]:
            if len(nxt) < C:
                bisect.insort(nxt, kx)
            elif kx < nxt[-1]:
                nxt.pop()
                bisect.insort(nxt, kx)
            if into_top:
                bisect.insort(top, kx)
                if len(top) > exp:
                    top.pop()

    def loop(allowed_only):
        nonlocal D, E
        while nxt:
            c = nxt[0]
            if len(top) == exp and top[-1] < c:
                break
            nxt.pop(0)
            E += 1
            for x in _list(graph, c[1], 0, M):
                if allowed_only and not allowed[x]:
                    continue  # neither marked, counted nor evaluated
                if x in visited:
                    continue
                visited.add(x)
                D += 1
                admit(x, bool(allowed[x]))

    sds = seed_slots(allowed, seeds) if seeds > 0 else []
    if sds:
        for x in sds:  # seeding
            if x in visited:
                continue
            visited.add(x)
            D += 1
            admit(x, True)
        loop(True)  # the allowed-only stage
        nxt[:] = list(top)  # hand-over
    if start not in visited:
        visited.add(start)
        D += 1
        if sds:
            admit(start, bool(allowed[start]))
        else:  # today's walk pushes its start node unconditionally (top and next are empty)
            nxt.append(key(start))
            if allowed[start]:
                top.append(key(start))
    loop(False)
    ans = top[skip: skip + k]
    return [s for _, s in ans], [d for d, _ in ans], D, E


def search(graph, dist, allowed, M, k, ef, seeds, skip=0, cand_cap=None):
    """Every query on the seeded walk path: (slots [nq][k] EMPTY-padded, dists [nq][k] +inf-padded, counts, D, E)."""
    nq = dist.shape[0]
    slots = np.full((nq, k), EMPTY, dtype=np.uint32)
    dists = np.full((nq, k), np.inf, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    D = np.zeros(nq, dtype=np.uint64)
    E = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        s, d, D[q], E[q] = seeded_walk(graph, dist[q], allowed, M, k, ef, seeds, skip, cand_cap)
        counts[q] = len(s)
        slots[q, : len(s)] = s
        dists[q, : len(d)] = np.array(d, dtype=np.float32)
    return slots, dists, counts, D, E
