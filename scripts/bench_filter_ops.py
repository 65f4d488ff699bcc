#!/usr/bin/env python
"""What building, extending and combining a filter costs (DESIGN.md 4.9 "Filter life cycle"): wall time through the host ABI.

Part 1 uses filter_from_labels / filter_from_bitmap only, so it runs on any checkout that has filters: `--tree DIR` measures the
lantern_amd of another checkout (built there) with this script -- the before / after of the device list pass.  On an index of
--rows rows (and again of --small rows), at 1 %, 10 % and 50 % of the rows allowed: three warm-up calls, then the median and
min - max of --reps calls of each constructor.
Part 2 (a checkout with lantern_gpu_filter_extend / _combine): the filter of 10 % of the rows extended after the index grew by 1 %
against filter_from_labels of the union; `a & b` on the device against the AND of the two host bitmaps and filter_from_bitmap.

    python scripts/bench_filter_ops.py [--tree DIR] [--label NAME] [--rows 1000000 --small 3000 --reps 11] >> profiles/filter_ops_build.json
One JSON line per run.  Alternate the checkouts on one box.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

DIM = 16  # (a filter's cost does not depend on the rows' width; a narrow index builds quickly)


def timed(fn, reps, warmup=3):
    """ms of fn() -- which returns what to close outside the clock"""
    out = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        made = fn()
        dt = (time.perf_counter() - t0) * 1e3
        made.close()
        if i >= warmup:
            out.append(dt)
    return {"median": round(statistics.median(out), 4), "min": round(min(out), 4), "max": round(max(out), 4), "reps": reps}


def grow(ix, n_old, n_new):
    rng = np.random.default_rng(7 + n_old)
    ix.add_many(np.arange(n_old, n_new, dtype=np.uint64) + 1, rng.standard_normal((n_new - n_old, DIM), dtype=np.float32))
    ix.flush()


def pack(allowed):
    w = np.packbits(allowed.astype(np.uint8), bitorder="little")
    return np.concatenate([w, np.zeros((-w.size) % 4, dtype=np.uint8)]).view(np.uint32)


def constructors(capi, ix, n, reps):
    rows = []
    for frac in (0.01, 0.1, 0.5):
        allowed = np.random.default_rng(int(frac * 1000)).random(n) < frac
        labels = np.random.default_rng(1).permutation(np.flatnonzero(allowed).astype(np.uint64) + 1)  # a heap scan's TIDs: any order
        words = pack(allowed)
        rows.append({"n": n, "allowed": int(allowed.sum()), "frac": frac,
                     "from_labels_ms": timed(lambda: ix.filter_from_labels(labels), reps),
                     "from_bitmap_ms": timed(lambda: ix.filter_from_bitmap(words), reps)})
    return rows


def life_cycle(capi, ix, n, reps):
    a_set, b_set = np.random.default_rng(2).random(n) < 0.1, np.random.default_rng(3).random(n) < 0.5
    wa, wb = pack(a_set), pack(b_set)
    fa, fb = ix.filter_from_bitmap(wa), ix.filter_from_bitmap(wb)
    out = {"n": n, "combine": {"device_and_ms": timed(lambda: fa & fb, reps), "host_and_then_from_bitmap_ms": timed(lambda: ix.filter_from_bitmap(wa & wb), reps),
                               "allowed": int((a_set & b_set).sum())}}
    L1 = np.flatnonzero(a_set).astype(np.uint64) + 1
    more = max(1, n // 100)
    grow(ix, n, n + more)
    L2 = np.flatnonzero(np.random.default_rng(4).random(more) < 0.1).astype(np.uint64) + n + 1
    union = np.concatenate([L1, L2])
    out["extend"] = {"grown_by": more, "new_labels": int(L2.size), "extend_ms": timed(lambda: fa.extend(L2), reps),
                     "fresh_from_labels_of_the_union_ms": timed(lambda: ix.filter_from_labels(union), reps)}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose lantern_amd is measured")
    p.add_argument("--label", default="tree")
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--small", type=int, default=3000)
    p.add_argument("--reps", type=int, default=11)
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from lantern_amd import capi

    line = {"what": "filter build / extend / combine, wall ms through the host ABI", "label": a.label, "dim": DIM, "constructors": [], "life_cycle": []}
    has_ops = hasattr(capi.Filter, "extend")
    for n in (a.rows, a.small):
        ix = capi.GpuIndex("l2sq", DIM, M=4, ef_construction=8, ef=8, seed=3)
        ix.reserve(n + n // 100 + 1)
        grow(ix, 0, n)
        line["constructors"] += constructors(capi, ix, n, a.reps)
        if has_ops:
            line["life_cycle"].append(life_cycle(capi, ix, n, a.reps))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
