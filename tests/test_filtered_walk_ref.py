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


# ------------------------------------------------------------------------------------------------
# identities that do not come from the kernel's definition
# ------------------------------------------------------------------------------------------------
FULL = [  # metric, n, d, M -- with ef >= the allowed count and a candidate cap of n a walk can neither stop early nor drop a candidate
    ("l2sq", 4000, 128, 16),
    ("cos", 2000, 768, 16),
    ("l2sq", 1500, 20, 40),
]


def check_answer_invariants(res, allowed, k, skip, n, g, dist, M):
    """Every returned slot allowed, keys strictly ascending by (distance, slot), the tail padded, count and D within their bounds: the
    base layer evaluates no row twice, so D less the evaluations of the greedy descent (which the filter does not touch) is at most n."""
    slots, dists, counts, D, E = res
    for q in range(slots.shape[0]):
        c = int(counts[q])
        assert c <= min(k, max(0, int(allowed.sum()) - skip))
        assert allowed[slots[q, :c]].all()
        keys = list(zip(dists[q, :c].tolist(), slots[q, :c].tolist()))
        assert all(a < b for a, b in zip(keys, keys[1:])), "keys ascend strictly by (distance, slot)"
        assert np.all(slots[q, c:] == ref.EMPTY) and np.all(np.isinf(dists[q, c:]))
        assert 1 <= int(D[q]) - ref.greedy_descent(g, dist[q], M)[1] <= n and E[q] <= D[q]
    assert not np.isnan(dists).any()


def reachable(graph, start):
    """bool[n]: the slots a base-layer walk from `start` can come to at all (a plain traversal of the level-0 lists; HNSW's lists are
    directed and a few rows of a graph have no list pointing at them)."""
    nbr0 = graph["nbr0"]
    seen = np.zeros(nbr0.shape[0], dtype=bool)
    seen[start] = True
    stack = [int(start)]
    while stack:
        for y in nbr0[stack.pop()]:
            if y == ref.EMPTY:
                break
            if not seen[y]:
                seen[y] = True
                stack.append(int(y))
    return seen


@pytest.mark.parametrize("metric,n,d,M", FULL)
def test_full_exploration_walk_is_the_exact_path(oracle, metric, n, d, M):
    """ef >= allowed count and cand_cap = n: the walk's top never fills before everything is evaluated and next never drops, so every
    allowed row the graph connects to the start is found and the answer is the exact path's over the allowed rows among them."""
    rng = np.random.default_rng(1)
    base, queries = rows(rng, n, d, metric), rows(rng, 8, d, metric)
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=64, ef=64, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    dist = ref.distance_matrix(oracle, base, queries, metric, oracle.SUM_WAVE64)
    reach = [reachable(g, ref.greedy_descent(g, dist[q], M)[0]) for q in range(len(queries))]
    assert all(r.sum() > 0.99 * n for r in reach)  # (all but a handful of rows: the identity is about nearly the whole allow-set)
    for sel in (0.5, 0.1, 0.02):
        allowed = rng.random(n) < sel
        count = int(allowed.sum())
        for k, skip in ((count, 0), (10, 0), (10, 3)):
            w = ref.search(g, dist, allowed, M, k, count, skip=skip, cand_cap=n)
            check_answer_invariants(w, allowed, k, skip, n, g, dist, M)
            for q in range(len(queries)):
                idx = np.flatnonzero(allowed & reach[q])
                kk = min(k, idx.size - skip)
                e = ref.search(None, dist[q:q + 1], allowed & reach[q], M, k, count, skip=skip, path="exact")
                assert np.array_equal(w[0][q], e[0][0]), (sel, k, skip, q)
                assert np.array_equal(w[1][q].view(np.uint32), e[1][0].view(np.uint32))
                assert w[2][q] == e[2][0] == kk
                # ... and against something that is not this module: brute force over those rows
                t_ids, t_d = oracle.bruteforce(base[idx], queries[q:q + 1], kk + skip, metric, sum_mode=oracle.SUM_WAVE64)
                assert np.array_equal(w[0][q, :kk], idx[t_ids[0, skip:]].astype(np.uint32))
                assert np.array_equal(w[1][q, :kk].view(np.uint32), t_d[0, skip:].view(np.uint32))


@pytest.mark.parametrize("cap", [None, 64, 300])
def test_walk_answers_keep_their_invariants_under_any_cap(oracle, cap):
    rng = np.random.default_rng(13)
    n, d, M, ef, k = 2500, 48, 12, 64, 10
    base, queries = rows(rng, n, d, "l2sq"), rows(rng, 16, d, "l2sq")
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=64, ef=ef, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64)
    for sel in (1.0, 0.3, 0.01, 0.002):
        allowed = rng.random(n) < sel
        for skip in (0, 3):
            check_answer_invariants(ref.search(g, dist, allowed, M, k, ef, skip=skip, cand_cap=cap), allowed, k, skip, n, g, dist, M)


@pytest.mark.parametrize("storage,metric,d", [("f16", "l2sq", 33), ("i8", "cos", 200), ("b1", "l2sq", 96), ("b1", "cos", 1000)])
def test_distance_matrix_serves_quantised_storage(oracle, storage, metric, d):
    """distance_matrix over the stored values is the oracle's pair distance of them, row for row (tests/filtered_regimes.py stored_rows)."""
    from tests import filtered_regimes as regimes

    rng = np.random.default_rng(d)
    base = rng.standard_normal((300, d), dtype=np.float32) * np.float32(0.4)
    queries = rng.standard_normal((4, d), dtype=np.float32) * np.float32(0.4)
    sb, sq, ometric, mode = regimes.stored_rows(oracle, storage, metric, base, queries)
    dist = ref.distance_matrix(oracle, sb, sq, ometric, mode)
    for q in range(4):
        for s in (0, 7, 299):
            assert np.float32(oracle.distance(sq[q], sb[s], ometric, mode)).view(np.uint32) == dist[q, s].view(np.uint32)


@pytest.mark.parametrize("name", ["within", "overflow", "mixed"])
def test_regime_conditions_hold_for_the_reference_alone(oracle, name):
    """The evaluation counts that put the large filtered walks of tests/test_gpu_filtered_regimes.py into their undo-log regimes, on the CPU
    restatement: no device needed to know that the data reaches them."""
    from tests import filtered_regimes as regimes

    res = regimes.regime_reference(name)
    regimes.assert_regime(name, res[3])
    allowed = regimes.regime_filter(name)
    ix = regimes.big_index(regimes.regime_kind(name))
    check_answer_invariants(res, allowed, regimes.K, 0, regimes.N, ix["g"], ix["dist"], regimes.M)
    # the bitmap-only launches of the same filters (every id goes to the log): within keeps it, overflow overflows it
    D0 = regimes.regime_reference(name, regimes.BITMAP_ONLY_CAP)[3]
    if name == "within":
        assert D0.max() < regimes.UNDO_WORDS
    elif name == "overflow":
        assert D0.min() > regimes.UNDO_WORDS
    else:
        assert (D0 < regimes.UNDO_WORDS).sum() >= 8 and (D0 > regimes.UNDO_WORDS).sum() >= 8
    # the unfiltered launch that reads the bitmap afterwards goes past its own LDS set on the Gaussian index
    if regimes.regime_kind(name) == "gauss":
        ix = regimes.big_index("gauss")
        _, _, _, D, _ = ix["ora"].search_batch(ix["queries"], regimes.K, regimes.PLAIN_EF, regimes.THREADS)
        assert D.min() > regimes.VIS_SLOTS
