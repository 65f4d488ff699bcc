"""CPU restatement of lantern_gpu_unlink_deleted (include/lantern_gpu.h "Deleting rows") over an exported graph.

Test infrastructure, not part of the product.  `graph` is the dict of OracleIndex.export_graph() / GpuIndex.export_graph();
`dist` is the [n][n] matrix of every (row, row) distance in the storage's device summation order (pair_matrix below: one
oracle.bruteforce call), or a callable slot -> that row of it, so every request's d and every re-prune decision has the bits the
device gives it.  tie_mix, refine and reverse_link restate oracle/hnsw.c:332-382.
"""
from __future__ import annotations

import numpy as np

EMPTY = 0xFFFFFFFF
STATS = ("tombstones_unlinked", "lists_repaired", "offers", "lists_cut", "request_evals", "entry_moved")  # what the restatement defines


def pair_matrix(oracle, rows, metric, sum_mode, nthreads=1):
    """[n][n] float32, rows AS STORED (tests/filtered_walk_ref.py distance_matrix says which sum mode goes with which storage)."""
    from tests.filtered_walk_ref import distance_matrix

    return distance_matrix(oracle, rows, rows, metric, sum_mode, nthreads)


def tie_mix(slot: int, centre: int) -> int:
    return ((slot ^ ((centre * 0x9E3779B1) & 0xFFFFFFFF)) * 0x85EBCA6B) & 0xFFFFFFFF


def cap_of(level: int, M: int) -> int:
    return 2 * M if level == 0 else M


def cut_of(level: int, M: int) -> int:
    return max(256, 8 * cap_of(level, M))


def get_list(graph, slot, level, M):
    row = graph["nbr0"][slot] if level == 0 else graph["upper_nbr"][int(graph["upper_off"][slot]) + level - 1]
    out = []
    for x in row[: cap_of(level, M)]:
        if int(x) == EMPTY:
            break
        out.append(int(x))
    return out


def set_list(graph, slot, level, M, lst):
    row = graph["nbr0"][slot] if level == 0 else graph["upper_nbr"][int(graph["upper_off"][slot]) + level - 1]
    row[: cap_of(level, M)] = EMPTY
    row[: len(lst)] = lst


def reverse_link(lst, cap, close, new_slot, d_new_close, drow):
    """oracle/hnsw.c reverse_link + refine on a Python list; returns 1 if it re-pruned."""
    if len(lst) < cap:
        lst.append(new_slot)
        return 0
    dc = drow(close)
    cand = [(float(d_new_close), new_slot)] + [(float(dc[x]), x) for x in lst]
    cand.sort(key=lambda t: (t[0], tie_mix(t[1], close)))
    kept = [cand[0]]
    for cd, cid in cand[1:]:
        if len(kept) >= cap:
            break
        row = drow(cid)
        if not any(float(row[k]) < cd for _, k in kept):
            kept.append((cd, cid))
    lst[:] = [x for _, x in kept]
    return 1


def unlink(graph, dist, M):
    """(the unlinked graph -- a deep copy --, stats)."""
    drow = dist if callable(dist) else (lambda a: dist[a])
    out = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in graph.items()}
    stats = {k: 0 for k in STATS}
    stats["reprunes"] = stats["max_kept"] = 0
    labels, levels = graph["labels"], graph["levels"]
    n = len(labels)
    dead = np.asarray(labels) == 0
    if not dead.any() or dead.all():
        return out, stats
    for p in range(n):
        if dead[p]:
            continue
        for level in range(int(levels[p]) + 1):
            L = get_list(graph, p, level, M)
            if not any(dead[x] for x in L):
                continue
            cap, cut = cap_of(level, M), cut_of(level, M)
            keep = [x for x in L if not dead[x]]
            offers, seen = [], set(keep) | {p}
            for t in L:
                if not dead[t] or len(offers) == cut or int(levels[t]) < level:
                    continue
                for c in get_list(graph, t, level, M):
                    if dead[c] or c in seen:
                        continue
                    offers.append(c)
                    seen.add(c)
                    if len(offers) == cut:
                        break
            new = list(keep)
            dp = drow(p)
            for c in offers:
                if reverse_link(new, cap, p, c, dp[c], drow):
                    stats["reprunes"] += 1
                    stats["max_kept"] = max(stats["max_kept"], len(new))  # the longest list a re-prune left
            set_list(out, p, level, M, new)
            stats["lists_repaired"] += 1
            stats["offers"] += len(offers)
            stats["lists_cut"] += len(offers) == cut
    for t in np.flatnonzero(dead):
        had = False
        for level in range(int(levels[t]) + 1):
            had = had or bool(get_list(graph, int(t), level, M))
            set_list(out, int(t), level, M, [])
        stats["tombstones_unlinked"] += had
    stats["request_evals"] = stats["offers"]
    if dead[int(graph["entry_slot"])]:
        live = np.flatnonzero(~dead)
        top = int(levels[live].max())
        out["entry_slot"], out["max_level"] = int(live[levels[live] == top][0]), top
        stats["entry_moved"] = 1
    return out, stats


def strip(graph, M):
    """Tombstones taken out of every list and their own lists emptied, nothing offered (the table's middle column)."""
    out = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in graph.items()}
    dead = np.asarray(graph["labels"]) == 0
    for p in range(len(dead)):
        for level in range(int(graph["levels"][p]) + 1):
            set_list(out, p, level, M, [] if dead[p] else [x for x in get_list(graph, p, level, M) if not dead[x]])
    if dead[int(graph["entry_slot"])] and not dead.all():
        live = np.flatnonzero(~dead)
        top = int(graph["levels"][live].max())
        out["entry_slot"], out["max_level"] = int(live[graph["levels"][live] == top][0]), top
    return out


def check_invariants(before, after, M):
    """What holds after every unlink: no list holds a tombstone, itself, a duplicate or a hole; a list that had no tombstone is
    byte-identical; every tombstone's lists are empty."""
    dead = np.asarray(before["labels"]) == 0
    if not dead.any() or dead.all():
        assert np.array_equal(before["nbr0"], after["nbr0"]) and np.array_equal(before["upper_nbr"], after["upper_nbr"])
        return
    for p in range(len(dead)):
        for level in range(int(before["levels"][p]) + 1):
            cap = cap_of(level, M)
            raw = (after["nbr0"][p] if level == 0 else after["upper_nbr"][int(after["upper_off"][p]) + level - 1])[:cap]
            lst = get_list(after, p, level, M)
            assert all(int(x) == EMPTY for x in raw[len(lst):]), ("hole", p, level)
            if dead[p]:
                assert not lst, ("tombstone keeps a list", p, level)
                continue
            assert p not in lst and len(set(lst)) == len(lst) and not any(dead[x] for x in lst), (p, level, lst)
            old = get_list(before, p, level, M)
            if not any(dead[x] for x in old):
                raw_old = (before["nbr0"][p] if level == 0 else before["upper_nbr"][int(before["upper_off"][p]) + level - 1])[:cap]
                assert np.array_equal(raw, raw_old), ("untouched list changed", p, level)
