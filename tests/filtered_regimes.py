"""The large indexes, filters and regime conditions of the filtered-search regime tests, shared by tests/test_filtered_walk_ref.py (which
proves the conditions on the CPU restatement alone) and tests/test_gpu_filtered_regimes.py (which runs the kernels in them).

Test infrastructure, not part of the product.  The conditions are about the walk's HBM visited bitmap and its undo log (walk.hpp VisUndo):
the LDS visited set holds VIS_SLOTS ids and spills to the bitmap at three quarters; from then on every new id is also appended to an undo log
of UNDO_WORDS ids; a walk that records more than that clears the whole bitmap at its end.  So a walk that evaluates D rows
  * spills and keeps its log           if VIS_SLOTS < D < UNDO_WORDS,
  * overflows its log for certain      if D > UNDO_WORDS + VIS_SLOTS (at most VIS_SLOTS of its ids never reached the log),
and a D between the two bounds proves neither, so no condition uses it.
"""
from __future__ import annotations

import functools
import os

import numpy as np

from lantern_amd import synth
from tests import filtered_walk_ref as ref

UNDO_WORDS = 8192  # device_common.hpp kVisUndoWords
VIS_SLOTS = 2048   # filter.hip filtered_search_locked: the LDS visited set of a walk that fits its LDS target
N, DIM, M, EFC, EF, K, NQ = 30000, 64, 16, 64, 64, 10, 48
BITMAP_ONLY_CAP = 4096  # a candidate cap whose `next` list alone (64 KiB) pushes the LDS visited set out: vis_slots == 0
PLAIN_EF = 400          # an unfiltered search that visits more rows than its own LDS set holds (it reads the bitmap too)
REGIMES = ("within", "overflow", "mixed")
THREADS = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1))


@functools.lru_cache(maxsize=None)
def big_index(kind):
    """kind "gauss" | "clustered": {base, queries, cluster, ora, g, dist} of an oracle-built N x DIM f32 l2sq index."""
    from oracle import binding as oracle

    if kind == "gauss":
        rng = np.random.default_rng(1)
        base = rng.standard_normal((N, DIM), dtype=np.float32)
        queries = rng.standard_normal((NQ, DIM), dtype=np.float32)
        cluster = None
    else:
        base = synth.base_rows("clustered", N, DIM)
        cluster = np.random.default_rng(synth.BASE_SEED).integers(0, synth.CLUSTERS, N)  # the draw base_rows makes first
        qall = synth.query_maker("clustered", DIM)(np.random.default_rng(99), 16 * NQ)
        qcl = np.random.default_rng(99).integers(0, synth.CLUSTERS, 16 * NQ)
        per = NQ // synth.CLUSTERS  # queries from all 16 clusters, interleaved so that neighbours in a batch differ in cluster
        pick = np.stack([np.flatnonzero(qcl == c)[:per] for c in range(synth.CLUSTERS)], axis=1).ravel()
        assert pick.size == NQ
        queries = qall[pick]
    ora = oracle.OracleIndex("l2sq", DIM, M=M, ef_construction=EFC, ef=EF, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(N, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64, THREADS)
    return {"base": base, "queries": queries, "cluster": cluster, "ora": ora, "g": g, "dist": dist}


def regime_kind(name):
    return "clustered" if name == "mixed" else "gauss"


def regime_filter(name):
    """bool[N]: the allow-set of a regime."""
    u = np.random.default_rng(20).random(N)
    if name == "within":
        return u < 0.20
    if name == "overflow":
        return u < 0.03
    cluster = big_index("clustered")["cluster"]
    return (cluster < 2) & (u < 0.20)  # a random fifth of clusters 0 and 1: near queries walk a little, far ones a lot


@functools.lru_cache(maxsize=None)
def regime_reference(name, cand_cap=None):
    """ref.search of the regime's NQ queries at the default candidate cap (None) or at `cand_cap`."""
    ix = big_index(regime_kind(name))
    return ref.search(ix["g"], ix["dist"], regime_filter(name), M, K, EF, cand_cap=cand_cap)


def assert_regime(name, D):
    """The condition that makes a batch of walks with evaluation counts D a case of regime `name`.  A miss is a failure."""
    D = np.asarray(D).astype(np.int64)
    if name == "within":
        assert D.min() > VIS_SLOTS and D.max() < UNDO_WORDS, (name, int(D.min()), int(D.max()))
    elif name == "overflow":
        assert D.min() > UNDO_WORDS + VIS_SLOTS, (name, int(D.min()))
    else:
        assert name == "mixed"
        assert (D < UNDO_WORDS).sum() >= 8 and (D > UNDO_WORDS + VIS_SLOTS).sum() >= 8, (name, np.sort(D).tolist())


def stored_rows(oracle, storage, metric, base, queries):
    """(rows, queries, oracle metric, summation order) of what an index of `storage` ("f32" | "f16" | "i8" | "b1") holds and computes on:
    the rounded halves, the quantised integers, or the packed sign bits (l2sq over bits IS hamming; cos over bits is the oracle's cos_b1)."""
    if storage == "f16":
        return oracle.round_f16(base), oracle.round_f16(queries), metric, oracle.SUM_WAVE64_F16
    if storage == "i8":
        return oracle.quantize_i8(base), oracle.quantize_i8(queries), metric, oracle.SUM_I8
    if storage == "b1":
        from tests.test_gpu_quantized_indexes import pack_bits_msb_first

        return pack_bits_msb_first(base), pack_bits_msb_first(queries), "hamming" if metric == "l2sq" else "cos_b1", oracle.SUM_SEQ
    return base, queries, metric, oracle.SUM_WAVE64
