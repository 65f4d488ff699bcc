#!/usr/bin/env python
"""The int8 screen at size: the share of a launch's row evaluations that still read the f32 row, and the physical
row bytes per query that follow from it, on the bench's own sets.

    python scripts/experiments/screen_share.py [--rows 1000000] [--dim 768] [--data gaussian|clustered] [--queries 8192] [--metric l2sq|cos]

Builds the bench's index (bench.py defaults: M=16, ef_construction=128, add batches of 32768), searches one launch of resident-size
queries at ef=64 and prints one JSON line: logical evaluations (D, also the oracle's), evaluations that read the f32 row, the share,
and row bytes per query -- f32 rows for the exact evaluations plus the screen row (16 B per 16 dims + 8 B of (s, r)) for every
evaluation of a screened hop (an upper bound: hops before the list is full read no screen row).  --metric cos: the cosine screen
(the table has the same size; its per-row pair is (s / norm, rho)).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lantern_amd import capi, synth  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--data", default="gaussian", choices=["gaussian", "clustered"])
    p.add_argument("--queries", type=int, default=8192)
    p.add_argument("--ef", type=int, default=64)
    p.add_argument("--metric", default="l2sq", choices=["l2sq", "cos"])
    a = p.parse_args()
    base = synth.base_rows(a.data, a.rows, a.dim)
    queries = synth.query_maker(a.data, a.dim)(np.random.default_rng(4), a.queries)
    ix = capi.GpuIndex(a.metric, a.dim, M=16, ef_construction=128, ef=a.ef, seed=42)
    ix.set_add_batch(32768, 16)
    ix.add_many(np.arange(a.rows, dtype=np.uint64) + 1, base)
    ix.flush()
    del base
    ix.search_batch(queries, 10, a.ef)
    logical, exact = ix.screen_stats()
    nq = a.queries
    row = 4 * a.dim
    screen_row = 16 * ((a.dim + 15) // 16) + 8
    out = {"rows": a.rows, "dim": a.dim, "data": a.data, "metric": a.metric, "ef": a.ef, "queries": nq,
           "dist_evals_per_query": logical / nq, "exact_evals_per_query": exact / nq,
           "exact_share": exact / logical if logical else None,
           "f32_row_bytes_per_query_without_screen": logical / nq * row,
           "row_bytes_per_query_with_screen_upper_bound": (exact * row + logical * screen_row) / nq}
    out["row_bytes_ratio_upper_bound"] = out["row_bytes_per_query_with_screen_upper_bound"] / out["f32_row_bytes_per_query_without_screen"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
