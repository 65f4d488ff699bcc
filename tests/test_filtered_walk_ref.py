"""The CPU restatement of filtered search (tests/filtered_walk_ref.py) against the oracle: with every slot allowed its walk path
is the unfiltered search (ids, distance bits, D, E) on oracle-built graphs; its exact path is the brute force over the allowed
rows.  No device needed."""
import numpy as np
import pytest

from tests import filtered_walk_ref as ref

CASES = [  # the shapes of test_gpu_parity.py::CASES -- metric, n, d, M, efc, ef, k
    ("l2sq", 3000, 128, 16, 64, 64, 10),
    ("cos", 2000, 768, 16, 64, 64, 10),
    ("l2sq", 1500, 100, 8, 40, 32, 5),
    ("l2sq", 800, 3, 2, 10, 4, 1),
    ("hamming", 3000, 24, 16, 64, 64, 10),
    ("cos", 600, 1536, 16, 32, 128, 10),
]


def rows(rng, n, d, metric):
    if metric == "hamming":
        return rng.integers(0, 2**32, size=(n, d), dtype=np.uint32)
    return rng.standard_normal((n, d), dtype=np.float32)


@pytest.mark.parametrize("metric,n,d,M,efc,ef,k", CASES)
def test_all_allowed_walk_is_the_unfiltered_search(oracle, metric, n, d, M, efc, ef, k):
    rng = np.random.default_rng(n + d)
    base, queries = rows(rng, n, d, metric), rows(rng, 16, d, metric)
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=ef, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    _, o_dist, o_slot, o_D, o_E = ora.search_batch(queries, k)
    dist = ref.distance_matrix(oracle, base, queries, metric, oracle.SUM_WAVE64)
    allowed = np.ones(n, dtype=bool)
    for cap in (None, max(ef, k)):  # the default cap, and C = expansion
        slots, dists, counts, D, E = ref.search(g, dist, allowed, M, k, ef, cand_cap=cap)
        assert np.array_equal(slots, o_slot)
        assert np.array_equal(dists.view(np.uint32), o_dist.view(np.uint32))
        assert np.array_equal(D, o_D) and np.array_equal(E, o_E)


@pytest.mark.parametrize("metric", ["l2sq", "cos", "hamming"])
def test_exact_path_is_bruteforce_over_allowed_rows(oracle, metric):
    rng = np.random.default_rng(5)
    n, d, k = 1200, 40, 10
    base, queries = rows(rng, n, d, metric), rows(rng, 8, d, metric)
    dist = ref.distance_matrix(oracle, base, queries, metric, oracle.SUM_WAVE64)
    for sel in (0.5, 0.05, 0.005):
        allowed = rng.random(n) < sel
        idx = np.flatnonzero(allowed)
        kk = min(k, idx.size)
        slots, dists, counts, D, E = ref.search(None, dist, allowed, 16, k, 64, path="exact")
        if kk:
            t_ids, t_d = oracle.bruteforce(base[idx], queries, kk, metric, sum_mode=oracle.SUM_WAVE64)
            assert np.array_equal(slots[:, :kk], idx[t_ids].astype(np.uint32))
            assert np.array_equal(dists[:, :kk].view(np.uint32), t_d.view(np.uint32))
        assert np.all(counts == kk) and np.all(D == idx.size) and np.all(E == 0)
        assert np.all(slots[:, kk:] == ref.EMPTY)


def test_walk_returns_only_allowed_rows_and_drops_under_a_tight_cap(oracle):
    rng = np.random.default_rng(11)
    n, d, M, ef, k = 2000, 32, 8, 32, 10
    base, queries = rows(rng, n, d, "l2sq"), rows(rng, 16, d, "l2sq")
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=64, ef=ef, seed=3, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64)
    allowed = rng.random(n) < 0.1
    wide = ref.search(g, dist, allowed, M, k, ef)
    tight = ref.search(g, dist, allowed, M, k, ef, cand_cap=ef)
    for slots, _, counts, _, _ in (wide, tight):
        for q in range(slots.shape[0]):
            assert allowed[slots[q, : counts[q]]].all()
    assert not np.array_equal(wide[3], tight[3])  # the cap changes the walk: entries were dropped
