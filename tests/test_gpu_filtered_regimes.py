"""Filtered search in the states it runs in at size: a workgroup that serves many queries, walks whose visited-bitmap undo
log fills, overflows, or is all there is, every row kind and lanes-per-row width under a selective filter, and filters built from hostile
label lists.  Needs an MI355X.

Method as tests/test_gpu_filtered_search.py: graphs are built by the oracle and imported, so the CPU restatement (tests/filtered_walk_ref.py)
walks the very graph the kernel walks; ids, distance bits, counts, D and E are compared exactly, for every query.  What is new is that each
case PROVES its regime from two sides -- the reference's evaluation counts (tests/filtered_regimes.py assert_regime; also checked without a
device by tests/test_filtered_walk_ref.py) and the launch diagnostic (GpuIndex.last_filtered_launch: grid, candidate cap, LDS visited-set
slots).  A case whose data misses its regime fails.
"""
import numpy as np
import pytest

from lantern_amd import synth
from tests import filtered_regimes as regimes
from tests import filtered_walk_ref as ref
from tests.test_gpu_degenerate_data import few_bit_patterns, lattice, triplicates
from tests.test_gpu_filtered_search import Dev, rows, same

pytestmark = pytest.mark.gpu

DEFAULT_CAP = 256  # filter.hip: max(4 expansion, 256) at ef = 64


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def check(got, want, labels):
    """same() on ids, distance bits, counts, D, E -- and the labels: the slot's label, 0 in the unused tail."""
    same(got, want)
    slot, lab = got[0], got[5]
    valid = slot != ref.EMPTY
    assert np.array_equal(lab[valid], labels[slot[valid]]) and np.all(lab[~valid] == 0)


def tiled(res, nq):
    """a reference answer of m queries repeated to nq rows (query i of the batch is query i % m)"""
    return tuple(np.concatenate([a] * (-(-nq // a.shape[0])))[:nq] for a in res)


def shape_is(gpu, path, **fields):
    got = gpu.last_filtered_launch()
    assert got["path"] == path and got["lds_bytes"] > 0, got
    for name, value in fields.items():
        assert got[name] == value, (name, value, got)
    return got


# ------------------------------------------------------------------------------------------------
# a. many queries per workgroup
# ------------------------------------------------------------------------------------------------
A_N, A_D, A_M, A_EF, A_K, A_NQ = 4000, 64, 16, 64, 10, 64


@pytest.fixture(scope="module")
def clustered_small(capi, oracle):
    """4000 x 64 clustered rows, 64 queries from all 16 clusters interleaved: under a filter on one cluster near and far queries alternate."""
    base = synth.base_rows("clustered", A_N, A_D)
    cluster = np.random.default_rng(synth.BASE_SEED).integers(0, synth.CLUSTERS, A_N)  # the draw base_rows makes first
    qall = synth.query_maker("clustered", A_D)(np.random.default_rng(99), 16 * A_NQ)
    qcl = np.random.default_rng(99).integers(0, synth.CLUSTERS, 16 * A_NQ)
    per = A_NQ // synth.CLUSTERS
    queries = qall[np.stack([np.flatnonzero(qcl == c)[:per] for c in range(synth.CLUSTERS)], axis=1).ravel()]
    assert queries.shape[0] == A_NQ
    ora = oracle.OracleIndex("l2sq", A_D, M=A_M, ef_construction=64, ef=A_EF, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(A_N, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    gpu = capi.GpuIndex("l2sq", A_D, M=A_M, ef_construction=64, ef=A_EF, seed=9)
    gpu.import_graph(base, g)
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64, regimes.THREADS)
    u = np.random.default_rng(31).random(A_N)
    filters = {  # name -> (allow-set, candidate cap of the walk, k)
        # C = expansion drops candidates: walks of a few hundred to a few thousand rows side by side, some losing allowed rows on the way
        "one_cluster_tight_cap": ((cluster == 0) & (u < 0.2), A_EF, A_K),
        # two dozen allowed rows, k just below their number, C = expansion: most walks lose a row or two -- short and full answers alternate
        "sparse_tight_cap": (u < 0.006, A_EF, 22),
        "tenth": (u < 0.1, 0, A_K),
        "seven_rows": (np.isin(np.arange(A_N), np.random.default_rng(32).choice(A_N, 7, replace=False)), 0, A_K),  # fewer rows than k
    }
    return {"gpu": gpu, "g": g, "dist": dist, "queries": queries, "filters": filters}


@pytest.mark.parametrize("path", ["walk", "exact"])
@pytest.mark.parametrize("name", ["one_cluster_tight_cap", "sparse_tight_cap", "tenth", "seven_rows"])
def test_one_workgroup_serves_many_queries(clustered_small, path, name):
    c = clustered_small
    gpu, g = c["gpu"], c["g"]
    allowed, cap, k = c["filters"][name]
    want = ref.search(g, c["dist"], allowed, A_M, k, A_EF, cand_cap=cap or None, path=path)
    counts, D = want[2], want[3].astype(np.int64)
    short = counts < k
    if name == "seven_rows":
        assert np.all(short)  # every answer ends in padding rows
    if path == "walk" and name == "one_cluster_tight_cap":  # long and short walks in one batch, and a short answer behind a full one
        assert D.max() >= 2 * D.min(), (D.min(), D.max())
        assert np.any(short[1:] & ~short[:-1]), counts.tolist()
    if path == "walk" and name == "sparse_tight_cap":  # one batch mixes short and full answers
        assert short.sum() >= 8 and (~short).sum() >= 8 and np.any(short[1:] & ~short[:-1]), counts.tolist()
    f = gpu.filter_from_bitmap(allowed)
    gpu.set_filter_policy(path, cand_cap=cap)
    dev = Dev(gpu, c["queries"], k)
    diag = path
    try:
        base_line = dev.filtered(f)
        default_grid = shape_is(gpu, diag)["grid"]
        assert default_grid == A_NQ  # 64 queries on an MI355X: one query per workgroup, the only state the small suite reaches
        check(base_line, want, g["labels"])
        for W in (1, 3):  # one workgroup serves all 64 queries; three serve 21 - 22 each, handed out by ticket
            gpu.set_search_shape(0, max_workgroups=W)
            got = dev.filtered(f)
            shape_is(gpu, diag, grid=W)
            check(got, want, g["labels"])
            same(got, base_line)
        gpu.set_search_shape(0, 0)
        # more queries than the default grid holds workgroups: every workgroup takes a second and a third query
        probe = Dev(gpu, np.tile(c["queries"], (64, 1)), k)
        probe.filtered(f)
        full_grid = gpu.last_filtered_launch()["grid"]
        nq = 2 * full_grid + 7
        assert full_grid < nq <= probe.nq
        big = Dev(gpu, np.tile(c["queries"], (64, 1))[:nq], k)
        got = big.filtered(f)
        shape_is(gpu, diag, grid=full_grid)
        check(got, tiled(want, nq), g["labels"])
    finally:
        gpu.set_search_shape(0, 0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# b. the undo log of the walk's visited bitmap: within capacity, overflowing, mixed in one launch
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_gpu(capi, oracle):
    made = {}

    def get(kind):
        if kind not in made:
            ix = regimes.big_index(kind)
            gpu = capi.GpuIndex("l2sq", regimes.DIM, M=regimes.M, ef_construction=regimes.EFC, ef=regimes.EF, seed=9)
            gpu.import_graph(ix["base"], ix["g"])
            made[kind] = gpu
        return made[kind]

    return get


def plain_reference(ix):
    lab, dist, slot, D, E = ix["ora"].search_batch(ix["queries"], regimes.K, regimes.PLAIN_EF, regimes.THREADS)
    cnt = np.full(lab.shape[0], regimes.K, dtype=np.uint32)
    return slot, dist, cnt, D, E


@pytest.mark.parametrize("W", [2, 0], ids=["two_workgroups", "default_grid"])
@pytest.mark.parametrize("name", regimes.REGIMES)
def test_undo_log_regimes_leave_the_bitmap_clean(big_gpu, name, W):
    """After every filtered launch the workgroups' HBM bitmaps must be all-zero again.  Proven by launches that READ them: the same launch
    again, a bitmap-only walk (no LDS set: every lookup is a bitmap lookup), and an unfiltered search past its own LDS set.  A bit left
    behind makes a later walk take a row for visited: a smaller D or a missing row."""
    ix = regimes.big_index(regimes.regime_kind(name))
    gpu, g, allowed = big_gpu(regimes.regime_kind(name)), ix["g"], regimes.regime_filter(name)
    want = regimes.regime_reference(name)
    regimes.assert_regime(name, want[3])
    want0 = regimes.regime_reference(name, regimes.BITMAP_ONLY_CAP)
    plain_want = plain_reference(ix)
    f = gpu.filter_from_bitmap(allowed)
    assert f.count == allowed.sum()
    dev = Dev(gpu, ix["queries"], regimes.K)
    grid = W or regimes.NQ
    try:
        gpu.set_search_shape(0, max_workgroups=W)
        for _ in range(2):  # (the second pass starts from whatever the bitmap-only and the unfiltered launches left)
            gpu.set_filter_policy("walk")
            first = dev.filtered(f)
            shape_is(gpu, "walk", grid=grid, vis_slots=regimes.VIS_SLOTS, cand_cap=DEFAULT_CAP, expansion=regimes.EF)
            check(first, want, g["labels"])
            again = dev.filtered(f)
            check(again, want, g["labels"])
            same(again, first)
            gpu.set_filter_policy("walk", cand_cap=regimes.BITMAP_ONLY_CAP)
            only = dev.filtered(f)
            shape_is(gpu, "walk", grid=grid, vis_slots=0, cand_cap=regimes.BITMAP_ONLY_CAP)
            check(only, want0, g["labels"])
            s, d, c, D, E, lab = dev.plain(ef=regimes.PLAIN_EF)
            same((s, d, c, D, E), plain_want)
    finally:
        gpu.set_search_shape(0, 0)
        gpu.set_filter_policy("auto")


def test_cursor_pages_over_the_large_filters(big_gpu):
    k = 10
    for name in regimes.REGIMES:
        ix = regimes.big_index(regimes.regime_kind(name))
        gpu, allowed = big_gpu(regimes.regime_kind(name)), regimes.regime_filter(name)
        f = gpu.filter_from_bitmap(allowed)
        gpu.set_filter_policy("walk")
        picks = [0, regimes.NQ // 2, regimes.NQ - 1]
        want = ref.search(ix["g"], ix["dist"][picks], allowed, regimes.M, 5 * k, regimes.EF)
        cur = gpu.cursor()
        for i, qi in enumerate(picks):
            q = ix["queries"][qi]
            pages = [cur.search_filtered(f, q, k, ef=regimes.EF, streaming=j > 0) for j in range(5)]
            labels = np.concatenate([p[0] for p in pages])
            dists = np.concatenate([p[1] for p in pages])
            assert labels.size == 5 * k == len(set(labels.tolist()))
            one_l, one_d, one_c = gpu.search_batch_filtered(f, q[None, :], 5 * k, ef=regimes.EF)
            assert np.array_equal(labels, one_l[0]) and np.array_equal(dists.view(np.uint32), one_d[0].view(np.uint32))
            assert one_c[0] == want[2][i] == 5 * k
            assert np.array_equal(labels, ix["g"]["labels"][want[0][i]]) and np.array_equal(dists.view(np.uint32), want[1][i].view(np.uint32))
        cur.close()
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# c. the bitmap-only walk, and full exploration: two kernels that must agree
# ------------------------------------------------------------------------------------------------
def reachable(graph, start):
    """bool[n]: what a base-layer walk from `start` can come to (HNSW's lists are directed; a few rows have none pointing at them)"""
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


def test_bitmap_only_walk_and_full_exploration(capi, oracle):
    n, d, M, ef, k, nq = 4000, 128, 16, 64, 10, 32
    rng = np.random.default_rng(1)
    base, queries = rows(rng, n, d, "l2sq"), rows(rng, nq, d, "l2sq")
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=64, ef=ef, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    gpu = capi.GpuIndex("l2sq", d, M=M, ef_construction=64, ef=ef, seed=9)
    gpu.import_graph(base, g)
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64, regimes.THREADS)
    connected = np.ones(n, dtype=bool)
    for start in {ref.greedy_descent(g, dist[q], M)[0] for q in range(nq)}:
        connected &= reachable(g, start)
    assert connected.sum() > 0.99 * n
    dev = Dev(gpu, queries, k)
    for sel in (0.5, 0.1, 0.02):
        allowed = rng.random(n) < sel
        f = gpu.filter_from_bitmap(allowed)
        gpu.set_filter_policy("walk", cand_cap=n)  # 64 KB of `next` alone: no room for an LDS visited set
        for W in (0, 2):
            gpu.set_search_shape(0, max_workgroups=W)
            got = dev.filtered(f)
            shape_is(gpu, "walk", vis_slots=0, cand_cap=n, grid=W or nq)
            want = ref.search(g, dist, allowed, M, k, ef, cand_cap=n)
            assert want[3].max() < regimes.UNDO_WORDS  # (every id of a bitmap-only walk goes to the log: these keep it)
            check(got, want, g["labels"])
        gpu.set_search_shape(0, 0)
        # full exploration: ef = the allowed count and nothing dropped -- the walk finds every allowed row the graph connects, so over
        # those rows the walk kernel and the exact kernel give one answer, and it is the brute force's
        both = allowed & connected
        idx = np.flatnonzero(both)
        f2 = gpu.filter_from_bitmap(both)
        assert f2.count == idx.size
        wide = Dev(gpu, queries, idx.size)
        gpu.set_filter_policy("walk", cand_cap=n)
        w = wide.filtered(f2, ef=idx.size)
        shape_is(gpu, "walk", vis_slots=0, cand_cap=n, expansion=idx.size)
        gpu.set_filter_policy("exact")
        e = wide.filtered(f2)
        shape_is(gpu, "exact", expansion=idx.size, cand_cap=0, vis_slots=0)
        for i in (0, 1, 2, 5):  # slots, distance bits, counts, labels (D and E are each path's own)
            assert np.array_equal(w[i].view(np.uint32) if i == 1 else w[i], e[i].view(np.uint32) if i == 1 else e[i]), i
        t_ids, t_d = oracle.bruteforce(base[idx], queries, idx.size, "l2sq", sum_mode=oracle.SUM_WAVE64)
        assert np.array_equal(w[0], idx[t_ids].astype(np.uint32)) and np.array_equal(w[1].view(np.uint32), t_d.view(np.uint32))
        assert np.all(w[2] == idx.size) and np.all(e[3] == idx.size) and np.all(e[4] == 0)
        check(w, ref.search(g, dist, both, M, idx.size, idx.size, cand_cap=n), g["labels"])
    gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# d. every row kind and every lanes-per-row width under a selective filter
# ------------------------------------------------------------------------------------------------
INSTANCES = (  # storage, metric, d (f32 scalars, or u32 words for hamming), M, data maker
    [("f32", m, d, 16, None) for m in ("l2sq", "cos") for d in (3, 20, 48, 100, 128, 255, 256, 510, 768, 1536, 2000)]
    + [("f32", "hamming", w, 16, None) for w in (8, 24, 64, 160)]
    + [(s, m, d, 16, None) for s in ("f16", "i8") for m in ("l2sq", "cos") for d in (33, 200, 768)]
    + [("b1", m, d, 16, None) for m in ("l2sq", "cos") for d in (96, 1000)]
    + [("f32", "l2sq", 20, 40, None)]  # M0 = 80: a neighbour list longer than one wave
    + [("f32", "l2sq", 6, 8, lattice), ("f32", "l2sq", 130, 16, lattice), ("f32", "l2sq", 64, 8, triplicates), ("f32", "hamming", 4, 8, few_bit_patterns)]
)


def instance(capi, oracle, storage, metric, d, M, maker, n, nq, ef=64):
    """An oracle-built (b1: device-built and exported) index of the kind, its queries, graph and distance matrix in the device's bits."""
    rng = np.random.default_rng(1000 * M + d)
    if maker is not None:
        base = maker(rng, n, d)
        queries = np.concatenate([base[rng.integers(0, n, nq // 2)], maker(rng, nq - nq // 2, d)])
    else:
        base, queries = rows(rng, n, d, metric), rows(rng, nq, d, metric)
    if storage == "i8":
        base, queries = base * np.float32(0.4), queries * np.float32(0.4)
    if storage == "b1":
        base, queries = base - np.float32(0.1), queries - np.float32(0.1)
    sb, sq, ometric, mode = regimes.stored_rows(oracle, storage, metric, base, queries)
    labels = np.arange(n, dtype=np.uint64) + 1
    if storage == "b1":  # (the graph importer takes f32 rows for a float metric: a b1 index is built on the device and its graph exported)
        gpu = capi.GpuIndex(metric, d, M=M, ef_construction=64, ef=ef, seed=9, quantization="b1")
        gpu.add_many(labels, base)
        gpu.flush()
        g = gpu.export_graph(with_vectors=True)
        assert np.array_equal(g["vectors"], sb)
    else:
        ora = oracle.OracleIndex(ometric, d, M=M, ef_construction=64, ef=ef, seed=9, sum_mode=mode)
        ora.add_many(labels, sb)
        g = ora.export_graph()
        gpu = capi.GpuIndex(metric, d, M=M, ef_construction=64, ef=ef, seed=9, quantization=storage)
        gpu.import_graph(sb, g)
    dist = ref.distance_matrix(oracle, sb, sq, ometric, mode, regimes.THREADS)
    assert not np.isnan(dist).any()
    return gpu, g, dist, queries


@pytest.mark.parametrize("storage,metric,d,M,maker", INSTANCES,
                         ids=[f"{s}-{m}-{d}-M{M}" + (f"-{mk.__name__}" if mk else "") for s, m, d, M, mk in INSTANCES])
def test_selective_filter_in_every_instantiation(capi, oracle, storage, metric, d, M, maker):
    n, nq, ef, k = (1500 if d <= 256 else 1000), 32, 64, 10
    gpu, g, dist, queries = instance(capi, oracle, storage, metric, d, M, maker, n, nq, ef)
    dev = Dev(gpu, queries, k)
    rng = np.random.default_rng(7)
    for sel in (0.1, 0.01):
        allowed = rng.random(n) < sel
        f = gpu.filter_from_bitmap(allowed)
        assert f.count == allowed.sum() > 0
        gpu.set_filter_policy("walk")
        for skip in (0, 3):
            got = dev.filtered(f, skip=skip)
            shape_is(gpu, "walk", cand_cap=DEFAULT_CAP, expansion=ef, grid=nq)
            check(got, ref.search(g, dist, allowed, M, k, ef, skip=skip), g["labels"])
        gpu.set_filter_policy("exact")
        for skip in (0, 3):
            got = dev.filtered(f, skip=skip)
            shape_is(gpu, "exact", expansion=k + skip, grid=nq)
            check(got, ref.search(None, dist, allowed, M, k, ef, skip=skip, path="exact"), g["labels"])
    gpu.set_filter_policy("auto")


@pytest.mark.parametrize("d,R", [(48, 64), (768, 8)])  # 8 and 64 lanes per row: R = 2 * 256 / G rows per round of the exact kernel
def test_exact_path_round_boundaries(capi, oracle, d, R):
    n, nq, k = 1200, 32, 10
    gpu, g, dist, queries = instance(capi, oracle, "f32", "l2sq", d, 16, None, n, nq)
    gpu.set_filter_policy("exact")
    dev = Dev(gpu, queries, k)
    order = np.random.default_rng(3).permutation(n)
    for count in (1, R - 1, R, R + 1, 3 * R + 1):
        allowed = np.zeros(n, dtype=bool)
        allowed[order[:count]] = True
        f = gpu.filter_from_bitmap(allowed)
        assert f.count == count
        for skip in (0, 3):
            got = dev.filtered(f, skip=skip)
            shape_is(gpu, "exact", expansion=k + skip)
            check(got, ref.search(None, dist, allowed, 16, k, 64, skip=skip, path="exact"), g["labels"])
            assert np.all(got[3] == count) and np.all(got[2] == max(0, min(k, count - skip)))
    gpu.set_filter_policy("auto")


def test_exact_path_with_a_thousand_keys(capi, oracle):
    n, d, nq, k, skip = 2500, 48, 32, 997, 3
    gpu, g, dist, queries = instance(capi, oracle, "f32", "l2sq", d, 16, None, n, nq)
    allowed = np.zeros(n, dtype=bool)
    allowed[np.random.default_rng(4).permutation(n)[:1500]] = True
    f = gpu.filter_from_bitmap(allowed)
    gpu.set_filter_policy("exact")
    for W in (0, 2):
        gpu.set_search_shape(0, max_workgroups=W)
        got = Dev(gpu, queries, k).filtered(f, skip=skip)
        shape_is(gpu, "exact", expansion=k + skip, grid=W or nq)
        check(got, ref.search(None, dist, allowed, 16, k, 64, skip=skip, path="exact"), g["labels"])
    gpu.set_search_shape(0, 0)
    gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# e. building filters
# ------------------------------------------------------------------------------------------------
def read_back(gpu, f, queries, n):
    """The allow-set of a filter as the exact path sees it: with k = count every allowed slot comes back, once."""
    count = f.count
    assert 0 < count <= 1500
    gpu.set_filter_policy("exact")
    s, d, c, D, E, lab = Dev(gpu, queries, count).filtered(f)
    gpu.set_filter_policy("auto")
    assert np.all(c == count) and np.all(D == count)
    got = np.zeros(n, dtype=bool)
    for row in s:
        assert len(set(row.tolist())) == count and row.max() < n
        got[:] = False
        got[row] = True
        yield got.copy()


def test_filters_from_hostile_label_lists(capi, big_gpu):
    ix = regimes.big_index("gauss")
    n = regimes.N
    rng = np.random.default_rng(41)
    labels = rng.integers(0, 2**64, size=n, dtype=np.uint64, endpoint=False)
    top = np.uint64(1) << np.uint64(63)
    labels[: n // 2] |= top                      # half of them with the top bit set: an unsigned order, not a signed one
    labels[n // 2:] &= ~top
    labels[labels == 0] = 5
    perm = rng.permutation(n)
    twins_a, twins_b, zeros = perm[:50], perm[50:100], perm[100:300]
    labels[twins_a] = labels[twins_b]            # 50 slots share their label with another slot
    labels[zeros] = 0                            # 200 deleted rows
    g = dict(ix["g"])
    g["labels"] = labels
    gpu = capi.GpuIndex("l2sq", regimes.DIM, M=regimes.M, ef_construction=regimes.EFC, ef=regimes.EF, seed=9)
    gpu.import_graph(ix["base"], g)
    queries = ix["queries"][:2]
    present = set(labels.tolist())
    absent = np.array([x for x in rng.integers(0, 2**64, size=12000, dtype=np.uint64, endpoint=False).tolist() if x not in present][:10000], dtype=np.uint64)
    assert absent.size == 10000
    chosen = np.concatenate([perm[300:1200], twins_a[:20], twins_b[20:40]])  # 940 slots, among them one side of 40 shared labels
    for with_zero in (False, True):
        wanted = labels[chosen]
        wanted = np.concatenate([wanted, wanted[:300], absent, np.zeros(3 if with_zero else 0, dtype=np.uint64)])  # duplicates, strangers
        rng.shuffle(wanted)
        for skip_deleted in (False, True):
            expect = np.isin(labels, wanted)
            if skip_deleted:
                expect &= labels != 0
            f = gpu.filter_from_labels(wanted, skip_deleted=skip_deleted)
            assert f.count == expect.sum(), (with_zero, skip_deleted)
            assert expect[twins_a[:40]].all() and expect[twins_b[:40]].all()  # both slots of a shared label are in
            for got in read_back(gpu, f, queries, n):
                assert np.array_equal(got, expect)
    # a list three times as long as the index: every label three times (all rows; SKIP_DELETED drops the 200), and 1000 labels among strangers
    everything = np.tile(labels, 3)
    assert gpu.filter_from_labels(everything).count == n
    assert gpu.filter_from_labels(everything, skip_deleted=True).count == n - zeros.size
    strangers = rng.integers(0, 2**64, size=3 * n, dtype=np.uint64, endpoint=False)
    strangers = strangers[~np.isin(strangers, labels)]
    long_list = np.concatenate([labels[perm[2000:3000]], strangers])[: 3 * n]
    rng.shuffle(long_list)
    expect = np.isin(labels, long_list)
    f = gpu.filter_from_labels(long_list)
    assert long_list.size > 2.9 * n and f.count == expect.sum() == 1000
    for got in read_back(gpu, f, queries, n):
        assert np.array_equal(got, expect)
    # the empty list: nothing allowed, nothing launched, the diagnostic says so
    empty = gpu.filter_from_labels(np.zeros(0, dtype=np.uint64))
    assert empty.count == 0
    lab, dist, cnt = gpu.search_batch_filtered(empty, queries, 10)
    assert np.all(lab == 0) and np.all(np.isinf(dist)) and np.all(cnt == 0)
    assert gpu.last_filtered_launch() == {"path": None, "grid": 0, "expansion": 0, "cand_cap": 0, "vis_slots": 0, "lds_bytes": 0}
    # a slot bitmap whose last word has bits past n (n = 30000 is not a multiple of 32): masked as k_filter_mask says
    assert n % 32 != 0
    allowed = np.zeros(n, dtype=bool)
    allowed[perm[5000:6200]] = True
    allowed[[0, n - 1]] = True
    for skip_deleted in (False, True):
        words = np.packbits(allowed.astype(np.uint8), bitorder="little")
        words = np.concatenate([words, np.zeros((-words.size) % 4, dtype=np.uint8)]).view(np.uint32).copy()
        assert words.size == (n + 31) // 32
        words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32)  # stray bits at slots n .. 32 * words - 1
        expect = allowed & (labels != 0) if skip_deleted else allowed
        f = gpu.filter_from_bitmap(words, skip_deleted=skip_deleted)
        assert f.count == expect.sum()
        for got in read_back(gpu, f, queries, n):
            assert np.array_equal(got, expect)
    with pytest.raises(capi.LanternGpuError, match="slot bitmap has"):
        gpu.filter_from_bitmap(np.ones((n + 31) // 32 + 1, dtype=np.uint32))
