"""The [nq][n] matrix of ADC distances of a compact pq index, with the oracle's own bits (oracle/hnsw.c lo_set_pq_view), for the CPU
restatements of filtered search (tests/filtered_walk_ref.py, tests/filtered_seeded_ref.py).

Test infrastructure, not part of the product.  The oracle has no brute force over code rows, so its SEARCH is made to visit every row:
a ring graph (level 0 only, row i's one neighbour is row i + 1) over the decoded rows, the pq view set, and k = ef = n.  The walk then
pops every row once, so the answer holds every (slot, ADC distance); scattered back by slot it is the matrix.
"""
from __future__ import annotations

import numpy as np

EMPTY = 0xFFFFFFFF


def make_codebook(rng, base, S, C):
    """[C][d], row c = centroid c of every subvector, concatenated (pqtable.c:194-240): sampled data points per subvector."""
    n, d = base.shape
    sub = d // S
    cb = np.zeros((C, d), dtype=np.float32)
    for s in range(S):
        pick = rng.choice(n, size=C, replace=False)
        cb[:, s * sub:(s + 1) * sub] = base[pick, s * sub:(s + 1) * sub]
    return cb


def quantize(oracle, base, cb, S, metric, nthreads=4):
    """product_quantization.c:207-240: per subvector the first centroid of smallest distance under the index metric -> (codes, decoded)."""
    n, d = base.shape
    sub = d // S
    codes = np.zeros((n, S), dtype=np.uint8)
    dec = np.zeros_like(base)
    for s in range(S):
        cols = slice(s * sub, (s + 1) * sub)
        ids, _ = oracle.bruteforce(np.ascontiguousarray(cb[:, cols]), np.ascontiguousarray(base[:, cols]), 1, metric, oracle.SUM_WAVE64, nthreads)
        codes[:, s] = ids[:, 0]
        dec[:, cols] = cb[codes[:, s], cols]
    return codes, dec


def ring_graph(n, M):
    """level 0 only: nbr0[i] = [(i + 1) % n], entry 0, max_level 0"""
    nbr0 = np.full((n, 2 * M), EMPTY, dtype=np.uint32)
    nbr0[:, 0] = (np.arange(n, dtype=np.uint32) + 1) % n
    return {"levels": np.zeros(n, dtype=np.uint8), "nbr0": nbr0, "upper_off": np.zeros(n, dtype=np.uint32),
            "upper_nbr": np.full((1, M), EMPTY, dtype=np.uint32), "labels": np.arange(n, dtype=np.uint64) + 1, "entry_slot": 0, "max_level": 0}


def distance_matrix(oracle, decoded, codebook, codes, queries, metric, nthreads=1, M=2):
    """[nq][n] float32: the oracle's ADC distance of every (query, row)."""
    n = decoded.shape[0]
    ora = oracle.OracleIndex.from_graph(metric, decoded, ring_graph(n, M), M, 8, n, 1, oracle.SUM_WAVE64)
    ora.set_pq_view(codebook, codes)
    _, d, slots, D, E = ora.search_batch(queries, n, n, nthreads)
    assert all(np.array_equal(np.sort(row), np.arange(n, dtype=slots.dtype)) for row in slots), "the ring walk returns every row once"
    assert np.all(D == n + 1) and np.all(E == n), "... having evaluated (the entry twice: descent, then start) and expanded every row once"
    out = np.empty((slots.shape[0], n), dtype=np.float32)
    np.put_along_axis(out, slots.astype(np.int64), d, axis=1)
    return out
