"""The seeded filtered walk on the device (include/lantern_gpu.h "Filtered search" 5).  Needs an MI355X.

Method as tests/test_gpu_filtered_search.py: graphs are built by the oracle and imported, so the CPU restatement
(tests/filtered_seeded_ref.py, one slot at a time) walks the very graph the kernel walks in rounds and hops; ids, distance bits,
counts, D and E are compared exactly, for every query -- never against the device itself.
"""
import numpy as np
import pytest

from lantern_amd import synth
from tests import filtered_regimes as regimes
from tests import filtered_seeded_ref as sref
from tests import filtered_walk_ref as ref
from tests.test_gpu_filtered_each import EachDev
from tests.test_gpu_filtered_regimes import check, instance, plain_reference, shape_is
from tests.test_gpu_filtered_search import Dev, rows, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def built(capi, oracle, metric, n, d, M, ef, nq, efc=64):
    rng = np.random.default_rng(n + d)
    base, queries = rows(rng, n, d, metric), rows(rng, nq, d, metric)
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=ef, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    gpu = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=ef, seed=9)
    gpu.import_graph(base, g)
    dist = ref.distance_matrix(oracle, base, queries, metric, oracle.SUM_WAVE64, regimes.THREADS)
    return {"gpu": gpu, "g": g, "dist": dist, "queries": queries, "base": base}


def seeds_are(gpu, seeds, single, seeded, unseeded):
    assert gpu.last_filtered_seeds() == {"seeds": seeds, "single_seeds": single, "seeded": seeded, "unseeded": unseeded}


# ------------------------------------------------------------------------------------------------
# 1. rounds: below, at and above one round of M0 = 16 seeds, several rounds, more seeds than allowed rows
# ------------------------------------------------------------------------------------------------
R_N, R_D, R_M, R_EF, R_K, R_NQ = 4000, 100, 8, 32, 10, 64


@pytest.fixture(scope="module")
def rounds_index(capi, oracle):
    c = built(capi, oracle, "l2sq", R_N, R_D, R_M, R_EF, R_NQ, efc=40)
    u = np.random.default_rng(31).random(R_N)
    order = np.random.default_rng(32).permutation(R_N)
    span = np.zeros(R_N, dtype=bool)
    span[1700:2100] = True
    one = np.zeros(R_N, dtype=bool)
    one[order[0]] = True
    few = np.zeros(R_N, dtype=bool)
    few[order[1:R_EF]] = True  # expansion - 1 allowed rows: top never fills
    c["filters"] = {"half": u < 0.5, "tenth": u < 0.1, "hundredth": u < 0.01, "span400": span, "one_row": one, "exp_minus_1": few}
    assert few.sum() == R_EF - 1
    return c


@pytest.mark.parametrize("seeds", [1, 15, 16, 17, 35, 4096])
def test_seeding_rounds(rounds_index, seeds):
    c = rounds_index
    gpu, g = c["gpu"], c["g"]
    dev = Dev(gpu, c["queries"], R_K)
    try:
        gpu.set_filter_policy("walk")
        gpu.set_filter_seeds(seeds)
        for name, allowed in c["filters"].items():
            want = sref.search(g, c["dist"], allowed, R_M, R_K, R_EF, seeds)
            f = gpu.filter_from_bitmap(allowed)
            for W in (0, 2):  # one query per workgroup; two workgroups serve 32 queries each
                gpu.set_search_shape(0, max_workgroups=W)
                got = dev.filtered(f)
                shape_is(gpu, "walk", grid=W or R_NQ, expansion=R_EF)
                seeds_are(gpu, seeds, min(seeds, int(allowed.sum())), R_NQ, 0)
                check(got, want, g["labels"])
    finally:
        gpu.set_search_shape(0, 0)
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 2. edges
# ------------------------------------------------------------------------------------------------
def test_k1_ef1_and_skip(rounds_index):
    c = rounds_index
    gpu, g = c["gpu"], c["g"]
    try:
        gpu.set_filter_policy("walk")
        gpu.set_filter_seeds(20)
        for name in ("tenth", "hundredth", "span400"):
            allowed = c["filters"][name]
            f = gpu.filter_from_bitmap(allowed)
            # k = 1, ef = 1: the radius exists after the first seed
            got = Dev(gpu, c["queries"], 1).filtered(f, ef=1)
            shape_is(gpu, "walk", expansion=1)
            check(got, sref.search(g, c["dist"], allowed, R_M, 1, 1, 20), g["labels"])
            # k = 5, skip = 7, ef = 0 (the index's 32)
            got = Dev(gpu, c["queries"], 5).filtered(f, ef=0, skip=7)
            shape_is(gpu, "walk", expansion=R_EF)
            check(got, sref.search(g, c["dist"], allowed, R_M, 5, R_EF, 20, skip=7), g["labels"])
    finally:
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")


def test_every_row_a_seed_counts_the_start_node_once(capi, oracle):
    n, d, M, ef, k, nq = 300, 24, 8, 32, 10, 32
    c = built(capi, oracle, "l2sq", n, d, M, ef, nq)
    gpu, g = c["gpu"], c["g"]
    allowed = np.ones(n, dtype=bool)
    f = gpu.filter_from_bitmap(allowed)
    try:
        gpu.set_filter_policy("walk")
        gpu.set_filter_seeds(n)
        want = sref.search(g, c["dist"], allowed, M, k, ef, n)
        descent = np.array([ref.greedy_descent(g, c["dist"][q], M)[1] for q in range(nq)])
        assert np.all(want[3] == descent + n)  # every row once -- the start node among the seeds, not again at the hand-over
        got = Dev(gpu, c["queries"], k).filtered(f)
        seeds_are(gpu, n, n, nq, 0)
        check(got, want, g["labels"])
    finally:
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")


def test_empty_filter_launches_nothing(rounds_index):
    gpu = rounds_index["gpu"]
    try:
        gpu.set_filter_policy("walk")
        gpu.set_filter_seeds(64)
        empty = gpu.filter_from_bitmap(np.zeros(R_N, dtype=bool))
        before = gpu.filter_stats()
        lab, dist, cnt = gpu.search_batch_filtered(empty, rounds_index["queries"], R_K)
        assert gpu.filter_stats() == before
        assert np.all(lab == 0) and np.all(np.isinf(dist)) and np.all(cnt == 0)
        seeds_are(gpu, 64, 0, 0, 0)
    finally:
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 3. the visited set's regimes: seeding alone spills the LDS set; the bitmap only; an overflowing undo log
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_gauss(capi, oracle):
    ix = regimes.big_index("gauss")
    gpu = capi.GpuIndex("l2sq", regimes.DIM, M=regimes.M, ef_construction=regimes.EFC, ef=regimes.EF, seed=9)
    gpu.import_graph(ix["base"], ix["g"])
    return ix, gpu


@pytest.mark.parametrize("regime", ["seeds_spill", "bitmap_only", "undo_overflow"])
def test_visited_set_regimes_leave_the_bitmap_clean(big_gauss, regime):
    ix, gpu = big_gauss
    g, seeds, nq = ix["g"], 2048, 16
    queries, dist = ix["queries"][:nq], ix["dist"][:nq]
    # 2048 seeds > three quarters of the 2048-slot LDS set: the seeding rounds themselves cross the spill.  The 3 % filter's 900 rows
    # are all seeds; its final stage then walks the disallowed rows around the query as the unseeded walk does
    allowed = regimes.regime_filter("overflow" if regime == "undo_overflow" else "within")
    cap = regimes.BITMAP_ONLY_CAP if regime == "bitmap_only" else 0
    want = sref.search(g, dist, allowed, regimes.M, regimes.K, regimes.EF, seeds, cand_cap=cap or None)
    D = want[3].astype(np.int64)
    print(regime, "allowed", int(allowed.sum()), "D", int(D.min()), int(D.max()))
    if regime == "seeds_spill":
        assert allowed.sum() >= seeds and D.min() > seeds
    elif regime == "undo_overflow":
        assert D.min() > regimes.UNDO_WORDS + regimes.VIS_SLOTS  # more ids than the log and the LDS set hold together
    f = gpu.filter_from_bitmap(allowed)
    dev = Dev(gpu, queries, regimes.K)
    plain_want = tuple(a[:nq] for a in plain_reference(ix))
    try:
        gpu.set_filter_policy("walk", cand_cap=cap)
        gpu.set_filter_seeds(seeds)
        for W in (0, 2):
            gpu.set_search_shape(0, max_workgroups=W)
            got = dev.filtered(f)
            shape_is(gpu, "walk", grid=W or nq, vis_slots=0 if regime == "bitmap_only" else regimes.VIS_SLOTS)
            check(got, want, g["labels"])
            s, d, c, D1, E1, _ = dev.plain(ef=regimes.PLAIN_EF)  # reads the bitmaps: a stale bit shows as a missing row or a smaller D
            same((s, d, c, D1, E1), plain_want)
    finally:
        gpu.set_search_shape(0, 0)
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 4. instantiations: one case per group width, every row kind
# ------------------------------------------------------------------------------------------------
INSTANCES = ([("f32", "l2sq", d) for d in (64, 192, 320, 768)] + [("f32", "cos", 192), ("f16", "l2sq", 200), ("i8", "cos", 200), ("b1", "l2sq", 96)])


@pytest.mark.parametrize("storage,metric,d", INSTANCES, ids=[f"{s}-{m}-{d}" for s, m, d in INSTANCES])
def test_seeded_walk_in_every_instantiation(capi, oracle, storage, metric, d):
    n, nq, ef, k, M, seeds = 2000, 32, 64, 10, 16, 20
    gpu, g, dist, queries = instance(capi, oracle, storage, metric, d, M, None, n, nq, ef)
    dev = Dev(gpu, queries, k)
    rng = np.random.default_rng(7)
    try:
        gpu.set_filter_policy("walk")
        gpu.set_filter_seeds(seeds)
        for sel in (0.1, 0.01):
            allowed = rng.random(n) < sel
            f = gpu.filter_from_bitmap(allowed)
            for skip in (0, 3):
                got = dev.filtered(f, skip=skip)
                check(got, sref.search(g, dist, allowed, M, k, ef, seeds, skip=skip), g["labels"])
    finally:
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 5. the per-query form
# ------------------------------------------------------------------------------------------------
def test_per_query_form_mixes_seeded_and_unseeded_queries(capi, oracle):
    n, d, M, ef, k, nq, seeds = 3000, 64, 16, 64, 10, 64, 1200
    c = built(capi, oracle, "l2sq", n, d, M, ef, nq)
    gpu, g, dist = c["gpu"], c["g"], c["dist"]
    u = np.random.default_rng(3).random(n)
    even = np.arange(n) % 2 == 0
    small = u < 0.01  # ~30 rows: 30^2 <= 5.6 * 64 * 3000 = 1037^2, the exact path under auto
    below = np.zeros(n, dtype=bool)
    below[np.argsort(u)[-1100:]] = True  # 1100 rows: past the rule's 1037 (the walk path) and fewer than the seeds -- every one a seed
    assert 0 < small.sum() < below.sum() < seeds < even.sum()
    assert small.sum() ** 2 <= 5.6 * ef * n < below.sum() ** 2
    sets = [None, np.zeros(n, dtype=bool), small, below, even, ~even]
    which = [q % len(sets) for q in range(nq)]
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    filters = [filt[w] for w in which]
    dev = EachDev(gpu, c["queries"], k)
    try:
        gpu.set_filter_policy("auto")
        gpu.set_filter_seeds(0)
        unseeded = dev.each(filters)
        seeds_are(gpu, 0, 0, 0, sum(1 for w in which if w in (0, 3, 4, 5)))
        plain = dev.plain()
        gpu.set_filter_seeds(seeds)
        for W in (0, 2):  # two workgroups: each serves seeded and unseeded queries of alternating disjoint filters in turn
            gpu.set_search_shape(0, max_workgroups=W)
            got = dev.each(filters)
            each = gpu.last_filtered_each()
            n_null = which.count(0)
            assert each["walk"] == sum(1 for w in which if w in (0, 3, 4, 5)) and each["exact"] == which.count(2), each
            assert each["unfiltered"] == n_null and each["empty"] == which.count(1) and each["launches"] == 2, each
            seeds_are(gpu, seeds, 0, each["walk"] - n_null, n_null)
            for q in range(nq):
                row = tuple(a[q:q + 1] for a in got[:5])
                w = which[q]
                if w == 0:  # NULL: byte for byte the unfiltered search
                    same(row, tuple(a[q:q + 1] for a in plain[:5]))
                elif w == 1:
                    assert got[2][q] == 0 and got[3][q] == 0 and got[4][q] == 0 and np.all(got[0][q] == ref.EMPTY)
                elif w == 2:  # the exact path ignores the setting: byte for byte the call at seeds = 0
                    same(row, tuple(a[q:q + 1] for a in unseeded[:5]))
                    assert got[3][q] == sets[2].sum() and got[4][q] == 0
                else:
                    s, dd, D, E = sref.seeded_walk(g, dist[q], sets[w], M, k, ef, seeds)
                    assert got[2][q] == len(s) == k
                    assert got[0][q].tolist() == s and np.array_equal(got[1][q].view(np.uint32), np.array(dd, dtype=np.float32).view(np.uint32))
                    assert (int(got[3][q]), int(got[4][q])) == (D, E), q
                    assert sets[w][got[0][q]].all()
    finally:
        gpu.set_search_shape(0, 0)
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 6. neutrality
# ------------------------------------------------------------------------------------------------
def test_the_exact_path_ignores_seeds_and_seeds_off_is_the_unseeded_walk(rounds_index):
    c = rounds_index
    gpu, g = c["gpu"], c["g"]
    dev = Dev(gpu, c["queries"], R_K)
    try:
        for name in ("tenth", "span400"):
            allowed = c["filters"][name]
            f = gpu.filter_from_bitmap(allowed)
            gpu.set_filter_policy("exact")
            gpu.set_filter_seeds(0)
            exact0 = dev.filtered(f)
            gpu.set_filter_seeds(256)
            exact256 = dev.filtered(f)
            seeds_are(gpu, 256, 0, 0, 0)
            for a, b in zip(exact0, exact256):
                assert a.tobytes() == b.tobytes()
            check(exact256, ref.search(None, c["dist"], allowed, R_M, R_K, R_EF, path="exact"), g["labels"])
            gpu.set_filter_policy("walk")
            seeded = dev.filtered(f)
            seeds_are(gpu, 256, min(256, int(allowed.sum())), R_NQ, 0)
            gpu.set_filter_seeds(0)
            back = dev.filtered(f)
            seeds_are(gpu, 0, 0, 0, R_NQ)
            check(back, ref.search(g, c["dist"], allowed, R_M, R_K, R_EF), g["labels"])  # the unseeded walk's ids, bits, D and E
            assert not np.array_equal(seeded[3], back[3])  # (the seeded launch was another walk)
    finally:
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 7. the cursor
# ------------------------------------------------------------------------------------------------
def test_cursor_pages_through_a_seeded_walk(rounds_index):
    c = rounds_index
    gpu, g, allowed = c["gpu"], c["g"], c["filters"]["hundredth"]
    f = gpu.filter_from_bitmap(allowed)
    count = int(allowed.sum())
    assert 30 <= count < 64
    try:
        gpu.set_filter_policy("walk")
        gpu.set_filter_seeds(64)
        for qi in (0, 17, 63):
            cur = gpu.cursor()
            seen = []
            for page in range(3):
                labels, dists = cur.search_filtered(f, c["queries"][qi], 10, ef=R_EF, streaming=page > 0)
                kk = min(len(seen) + 10, count)
                s, d, _, _ = sref.seeded_walk(g, c["dist"][qi], allowed, R_M, kk, R_EF, 64)
                assert labels.tolist() == g["labels"][s[len(seen):]].tolist(), (qi, page)
                assert np.array_equal(dists.view(np.uint32), np.array(d[len(seen):], dtype=np.float32).view(np.uint32))
                seen += labels.tolist()
            assert len(seen) == 30 == len(set(seen))
            cur.close()
    finally:
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 8. at size: the cluster-correlated filter that the unseeded walk fails
# ------------------------------------------------------------------------------------------------
def test_one_cluster_filter_at_size(capi, oracle):
    n, d, M, ef, k, nq, seeds = 300000, 48, 16, 64, 10, 8, 256
    base = synth.base_rows("clustered", n, d)
    cluster = np.random.default_rng(synth.BASE_SEED).integers(0, synth.CLUSTERS, n)  # the draw base_rows makes first
    queries = synth.query_maker("clustered", d)(np.random.default_rng(5), nq)
    gpu = capi.GpuIndex("l2sq", d, M=M, ef_construction=128, ef=ef, seed=42)
    gpu.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    gpu.flush()
    g = gpu.export_graph()
    allowed = cluster == 0
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64, regimes.THREADS)
    want = sref.search(g, dist, allowed, M, k, ef, seeds)
    f = gpu.filter_from_bitmap(allowed)
    try:
        gpu.set_filter_policy("walk")
        gpu.set_filter_seeds(seeds)
        got = Dev(gpu, queries, k).filtered(f)
        shape_is(gpu, "walk", grid=nq, expansion=ef)
        seeds_are(gpu, seeds, seeds, nq, 0)
        check(got, want, g["labels"])
        truth = ref.search(None, dist, allowed, M, k, ef, path="exact")[0]
        recall = np.mean([len(set(got[0][q].tolist()) & set(truth[q].tolist())) / k for q in range(nq)])
        print(f"seeded recall@10 over {nq} queries: {recall:.3f}; mean D {got[3].mean():.0f}, mean E {got[4].mean():.0f}")
    finally:
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")
