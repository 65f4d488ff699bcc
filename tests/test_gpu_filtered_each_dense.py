"""The dense route of the per-query-filter calls on the device (lantern_gpu_set_filter_dense_each; include/lantern_gpu.h "THE DENSE
ROUTE FOR PER-QUERY-FILTER CALLS", DESIGN.md 4.9 "Dense exact path, per-query filters").  Needs an MI355X.

The referee of every row is the single-filter answer of that query's filter (the device's, with both dense settings at 0; on the
exact path also tests/filtered_walk_ref.py::exact over the distance matrix in the device's summation order); the same call with the
setting at 0 is compared as well.  Slots, distance bits, labels, counts, D and E equal, for every query.  The output buffers are filled
with a pattern before each call.
"""
import numpy as np
import pytest

from tests import filtered_walk_ref as ref
from tests.test_gpu_exact_knn import FAMILIES
from tests.test_gpu_filtered_dense import gauss_case, index_of, poison, random_set
from tests.test_gpu_filtered_search import Dev, oracle_index, same

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def each(dev, filters, skip=0, ef=0):
    dev.gpu.search_batch_filtered_each_device(filters, dev.dq.ptr, dev.rows.strides[0], dev.nq, dev.k, ef, skip, dev.lab.ptr, dev.dist.ptr, dev.slot.ptr,
                                              dev.cnt.ptr, dev.D.ptr, dev.E.ptr)
    return dev._out()


def same6(a, b):
    same(a, b)
    assert np.array_equal(a[5], b[5]), "labels differ"


def single_filter_rows(ix, dev, filters, skip):
    """row i: what the single-filter call gives query i with filters[i] (None: the unfiltered search), both dense settings at 0"""
    ix.set_filter_dense(0)
    ix.set_filter_dense_each(0)
    want, done = None, {}
    for i, f in enumerate(filters):
        key = id(f)
        if key not in done:
            poison(dev)
            done[key] = dev.plain() if f is None else dev.filtered(f, skip=skip)
        if want is None:
            want = tuple(np.empty_like(x) for x in done[key])
        for w, x in zip(want, done[key]):
            w[i] = x[i]
    return want


def moved(ix, call):
    d0, f0, t0 = ix.filter_dense_stats(), ix.filter_stats(), ix.counters()
    out = call()
    d1, f1, t1 = ix.filter_dense_stats(), ix.filter_stats(), ix.counters()
    delta = {key: d1[key] - d0[key] for key in d1}
    delta.update(exact=f1["exact"] - f0["exact"], walk=f1["walk"] - f0["walk"], evals=t1["search_dist_evals"] - t0["search_dist_evals"],
                 expansions=t1["search_expansions"] - t0["search_expansions"], searched=t1["search_queries"] - t0["search_queries"])
    return out, delta


def check_each(ix, dev, filters, m, skip=0, exact_ref=None):
    """one per-query call with the setting at 0 and at m: both equal the single-filter rows (and exact_ref = (dist, {query: allowed})
    where given); returns (last_filtered_each of both, the dense diagnostic, the counters' moves of both)"""
    want = single_filter_rows(ix, dev, filters, skip)
    if exact_ref:
        dist, sets = exact_ref
        for q, allowed in sets.items():
            r = ref.search(None, dist[q:q + 1], allowed, 0, dev.k, 0, skip=skip, path="exact")
            same(tuple(x[q:q + 1] for x in want), r)
    poison(dev)
    off, d_off = moved(ix, lambda: each(dev, filters, skip=skip))
    last_off, none = ix.last_filtered_each(), ix.last_filtered_each_dense()
    assert none == dict(groups=0, queries=0, certified=0, recomputed=0, rows=0, steps=0)
    assert (d_off["calls"], d_off["queries"]) == (0, 0)
    ix.set_filter_dense_each(m)
    poison(dev)  # (the buffers held the answer: what is compared below is what this call wrote)
    on, d_on = moved(ix, lambda: each(dev, filters, skip=skip))
    last_on, dense = ix.last_filtered_each(), ix.last_filtered_each_dense()
    ix.set_filter_dense_each(0)
    same6(off, want)
    same6(on, want)
    # the cumulative counters move as without the setting: D = the query's own filter's count, E as before
    assert (d_on["evals"], d_on["expansions"], d_on["searched"]) == (d_off["evals"], d_off["expansions"], d_off["searched"])
    assert d_on["calls"] == (1 if dense["groups"] else 0) and d_on["queries"] == dense["queries"]
    assert d_on["certified"] == dense["certified"] and d_on["recomputed"] == dense["recomputed"] and dense["certified"] + dense["recomputed"] == dense["queries"]
    return last_off, last_on, dense, d_off, d_on


# ---- the mixed call ---------------------------------------------------------------------------------------------------------------
def test_mixed_call_on_a_built_graph_under_the_auto_policy(capi, oracle, cores):
    n, d, k = 1500, 16, 10
    base, queries, g, ix = oracle_index(capi, oracle, "l2sq", n, d, 8, 40, 64, 9)
    rng = np.random.default_rng(77)
    queries = queries[:24]
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64, cores)
    # auto: exact iff count^2 <= 5.6 * 64 * 1500, count <= 733
    sets = {name: random_set(rng, n, c) for name, c in (("walk_a", 1200), ("walk_b", 900), ("small", 300), ("third", 500), ("g37", 37), ("g1", 1))}
    sets["empty"] = np.zeros(n, dtype=bool)
    f = {name: ix.filter_from_bitmap(a) for name, a in sets.items()}
    # interleaved, not sorted by group: `small` stands behind 2 queries (below min_group = 3), the three dense groups behind 6, 3 and 3
    names = ["third", "walk_a", None, "g37", "small", "third", "g1", "empty", "walk_b", "third", "g37", None, "g1", "third", "small", "walk_a", "third",
             "g1", "g37", "third", "empty", None, "walk_b", "walk_a"]
    filters = [None if x is None else f[x] for x in names]
    dev = Dev(ix, queries, k)
    exact_sets = {q: sets[x] for q, x in enumerate(names) if x in ("small", "third", "g37", "g1")}
    last_off, last_on, dense, d_off, d_on = check_each(ix, dev, filters, 3, exact_ref=(dist, exact_sets))
    assert last_off == last_on == dict(walk=8, exact=14, unfiltered=3, empty=2, distinct_filters=7, launches=2)
    assert dense == dict(groups=3, queries=12, certified=12, recomputed=0, rows=538, steps=3)
    assert (d_off["walk"], d_off["exact"]) == (1, 1) and (d_on["walk"], d_on["exact"]) == (1, 1)
    ix.close()


# ---- the edges of the plan --------------------------------------------------------------------------------------------------------
def test_chunk_edge(capi, oracle, cores):
    """65 530 + 20 rows: the second segment straddles position 65 536 of the concatenated list"""
    n = 70000
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", n, 8, 6, 21)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    perm = rng.permutation(n)
    a, b = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    a[perm[:65530]] = True
    b[perm[65530:65550]] = True
    fa, fb = ix.filter_from_bitmap(a), ix.filter_from_bitmap(b)
    filters = [fa, fb, fb, fa, fb, fa]
    _, _, dense, _, d_on = check_each(ix, Dev(ix, queries, 10), filters, 2, exact_ref=(dist, {q: (a if f is fa else b) for q, f in enumerate(filters)}))
    assert dense == dict(groups=2, queries=6, certified=6, recomputed=0, rows=65550, steps=3) and d_on["exact"] == 0
    ix.close()


def test_query_tile_edge(capi, oracle, cores):
    """a group of 1025 queries (two tiles) beside a group of 2"""
    n, nq = 1000, 1027
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", n, 4, nq, 22)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    a, b = random_set(rng, n, 300), random_set(rng, n, 45)
    fa, fb = ix.filter_from_bitmap(a), ix.filter_from_bitmap(b)
    filters = [fa] * nq
    filters[5] = filters[900] = fb
    _, _, dense, _, _ = check_each(ix, Dev(ix, queries, 10), filters, 2, exact_ref=(dist, {q: (a if f is fa else b) for q, f in enumerate(filters)}))
    assert dense == dict(groups=2, queries=nq, certified=nq, recomputed=0, rows=345, steps=3)
    ix.close()


# ---- row kinds --------------------------------------------------------------------------------------------------------------------
def row_kind_case(capi, oracle, cores, metric, storage, n, d, scale, seed):
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, metric, storage, n, d, 9, seed, scale)
    ix = index_of(capi, oracle, metric, storage, rows)
    a, b = random_set(rng, n, n // 2), random_set(rng, n, 60)
    fa, fb = ix.filter_from_bitmap(a), ix.filter_from_bitmap(b)
    filters = [fa, fb, fa, fa, fb, fa, fb, fa, fb]
    sets = {q: (a if f is fa else b) for q, f in enumerate(filters)}
    _, _, dense, _, _ = check_each(ix, Dev(ix, queries, 10), filters, 4, skip=3, exact_ref=(dist, sets))
    assert (dense["groups"], dense["queries"], dense["recomputed"], dense["rows"]) == (2, 9, 0, n // 2 + 60)
    ix.close()


@pytest.mark.parametrize("metric,storage,n,d,scale", [
    ("l2sq", "f32", 900, 3, 1.0), ("cos", "f32", 900, 3, 1.0),            # G = 8
    ("l2sq", "f32", 900, 128, 1.0), ("cos", "f32", 900, 128, 1.0),        # G = 16
    ("l2sq", "f32", 700, 768, 1.0), ("cos", "f32", 700, 768, 1.0),        # G = 64
    ("l2sq", "f32", 600, 1536, 1.0), ("cos", "f32", 600, 1536, 1.0),      # G = 64, two blocks of chunks per lane
    ("l2sq", "f16", 900, 200, 1.0), ("cos", "f16", 900, 200, 1.0),        # native f16 contraction
    ("l2sq", "i8", 900, 200, 0.3), ("cos", "i8", 900, 200, 0.3),          # native i8 contraction: exact keys
    ("hamming", "f32", 900, 24, 1.0),                                      # bit rows: popcounts, no norms
])
def test_row_kinds(capi, oracle, cores, metric, storage, n, d, scale):
    row_kind_case(capi, oracle, cores, metric, storage, n, d, scale, 5)


@pytest.mark.parametrize("storage", ["f16", "i8"])
def test_quantised_rows_on_the_f32_copy(capi, oracle, cores, monkeypatch, storage):
    monkeypatch.setenv("LANTERN_GPU_DENSE_NATIVE", "0")
    row_kind_case(capi, oracle, cores, "l2sq", storage, 900, 100, 0.3, 6)


@pytest.mark.parametrize("metric,d", [("cos", 1000), ("l2sq", 96)])
def test_bit_rows_of_a_b1_index(capi, oracle, cores, metric, d):
    """a b1 index (sign bits of f32 rows): cosine over b1 is k_dense_ham's other variant, l2sq over b1 is Hamming; built on the device
    and exported, as tests/test_gpu_filtered_regimes.py does, the referee the oracle's cos_b1 / hamming in sequential order"""
    from tests.test_gpu_filtered_regimes import instance

    n = 900
    ix, g, dist, queries = instance(capi, oracle, "b1", metric, d, 8, None, n, 9)
    assert np.array_equal(g["labels"], np.arange(n, dtype=np.uint64) + 1)
    ix.set_filter_policy("exact")
    rng = np.random.default_rng([31, d])
    a, b = random_set(rng, n, n // 2), random_set(rng, n, 60)
    fa, fb = ix.filter_from_bitmap(a), ix.filter_from_bitmap(b)
    filters = [fa, fb, fa, fa, fb, fa, fb, fa, fb]
    sets = {q: (a if f is fa else b) for q, f in enumerate(filters)}
    _, _, dense, _, d_on = check_each(ix, Dev(ix, queries, 10), filters, 4, skip=3, exact_ref=(dist, sets))
    assert dense == dict(groups=2, queries=9, certified=9, recomputed=0, rows=n // 2 + 60, steps=2) and d_on["exact"] == 0
    ix.close()


# ---- the certificate's refusals: answered by the call's exact launch ------------------------------------------------------------------
def test_recomputed_queries(capi, oracle, cores):
    """tests/test_gpu_filtered_dense.py's offset10 input (its certificate refuses queries) beside its 900 x 128 Gaussian input (all
    certified there, fused and unfused), as two groups of one index"""
    n1, n2, d, k, skip = 4000, 900, 128, 10, 3
    r1, q1 = FAMILIES["offset10"](np.random.default_rng([0, n1, d, 16, 10]), n1, d, 16)
    r2, q2, _, rng2 = gauss_case(capi, oracle, cores, "l2sq", "f32", n2, d, 9, 5)
    rows, queries = np.concatenate([r1, r2]).astype(F32), np.concatenate([q1, q2]).astype(F32)
    dist = ref.distance_matrix(oracle, rows, queries, "l2sq", oracle.SUM_WAVE64, cores)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    a, b = np.zeros(n1 + n2, dtype=bool), np.zeros(n1 + n2, dtype=bool)
    a[:n1] = np.random.default_rng(7).random(n1) < 0.5
    b[n1:] = random_set(rng2, n2, n2 // 2)
    fa, fb = ix.filter_from_bitmap(a), ix.filter_from_bitmap(b)
    filters = [fa] * 16 + [fb] * 9
    sets = {q: (a if f is fa else b) for q, f in enumerate(filters)}
    _, last_on, dense, _, d_on = check_each(ix, Dev(ix, queries, k), filters, 2, skip=skip, exact_ref=(dist, sets))
    assert dense["groups"] == 2 and dense["queries"] == 25 and 0 < dense["recomputed"] <= 16, dense
    assert d_on["exact"] == 1 and last_on["launches"] == 1 and last_on["exact"] == 25
    # the Gaussian group alone: every query certified, no per-query launch at all
    _, last_on, dense, _, d_on = check_each(ix, Dev(ix, queries[16:], k), [fb] * 9, 2, skip=skip)
    assert dense == dict(groups=1, queries=9, certified=9, recomputed=0, rows=n2 // 2, steps=1)
    assert d_on["exact"] == 0 and last_on["launches"] == 0 and last_on["exact"] == 9
    ix.close()


# ---- paging, width, routing -------------------------------------------------------------------------------------------------------
def test_paging_and_width(capi, oracle, cores):
    n, nq = 1200, 8
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", n, 24, nq, 23)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    a, b = random_set(rng, n, 400), random_set(rng, n, 25)
    fa, fb = ix.filter_from_bitmap(a), ix.filter_from_bitmap(b)
    filters = [fa, fb, fa, fb, fa, fb, fa, fa]
    sets = {q: (a if f is fa else b) for q, f in enumerate(filters)}
    dev = Dev(ix, queries, 10)
    for skip in (10, 20, 30, 230):  # (20, 30: the page of the small group runs out; 230: k + skip = 240)
        _, _, dense, _, _ = check_each(ix, dev, filters, 3, skip=skip, exact_ref=(dist, sets))
        assert dense["groups"] == 2 and dense["queries"] == 8
    # k + skip = 241: today's kernel
    _, _, dense, _, d_on = check_each(ix, dev, filters, 3, skip=231)
    assert dense["groups"] == 0 and (d_on["calls"], d_on["exact"]) == (0, 1)
    ix.close()


def test_routing(capi, oracle, cores):
    n, nq, k = 1500, 8, 10
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", n, 16, nq, 24)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    allowed = random_set(rng, n, 500)
    f, twin = ix.filter_from_bitmap(allowed), ix.filter_from_bitmap(allowed)
    want = ref.search(None, dist, allowed, 0, k, 0, path="exact")
    want_host = (want[0].astype(np.uint64) + 1, want[1], want[2])

    def host_same(got):
        lab, dd, cnt = got
        assert np.array_equal(lab, want_host[0]) and np.array_equal(dd.view(np.uint32), want_host[1].view(np.uint32)) and np.array_equal(cnt, want_host[2])

    assert ix.filter_dense_each() == 0
    # the single-filter switch alone leaves the per-query call alone
    ix.set_filter_dense(1)
    got, d = moved(ix, lambda: ix.search_batch_filtered_each([f] * nq, queries, k))
    assert (d["calls"], d["exact"]) == (0, 1) and ix.filter_dense_each() == 0
    host_same(got)
    ix.set_filter_dense(0)
    ix.set_filter_dense_each(4)
    assert ix.filter_dense_each() == 4 and ix.filter_dense() == 0
    # the host form takes the route
    got, d = moved(ix, lambda: ix.search_batch_filtered_each([f] * nq, queries, k))
    assert (d["calls"], d["queries"], d["exact"]) == (1, nq, 0) and ix.last_filtered_each_dense()["groups"] == 1
    host_same(got)
    # ... and the single-filter call does not, under this switch
    _, d = moved(ix, lambda: ix.search_batch_filtered(f, queries, k))
    assert (d["calls"], d["exact"]) == (0, 1)
    # the lane form, the per-query-parameter form and a cursor leave it alone
    got, d = moved(ix, lambda: ix.search_batch_filtered_each_lane(0, [f] * nq, queries, k))
    assert (d["calls"], d["exact"]) == (0, 1) and ix.last_filtered_each_dense()["groups"] == 0
    host_same(got)
    ix.search_batch_filtered_each([f] * nq, queries, k)  # (a dense run's numbers stand in the diagnostic: the next call must clear them)
    assert ix.last_filtered_each_dense()["groups"] == 1
    got, d = moved(ix, lambda: ix.search_batch_filtered_each_params([f] * nq, queries, [(k, 0)] * nq))
    assert (d["calls"], d["exact"]) == (0, 1) and ix.last_filtered_each_dense()["groups"] == 0
    host_same(got)
    cur = ix.cursor()
    (lab, dd), d = moved(ix, lambda: cur.search_filtered(f, queries[0], k))
    cur.close()
    assert (d["calls"], d["exact"]) == (0, 1) and np.array_equal(lab, want_host[0][0])
    # two handles over one set are two groups (of 4 queries each: dense at 4, not at 5) with equal answers
    got, d = moved(ix, lambda: ix.search_batch_filtered_each([f, twin] * 4, queries, k))
    assert (d["calls"], d["queries"], d["exact"]) == (1, nq, 0) and ix.last_filtered_each_dense()["groups"] == 2 and ix.last_filtered_each_dense()["rows"] == 1000
    host_same(got)
    ix.set_filter_dense_each(5)
    got, d = moved(ix, lambda: ix.search_batch_filtered_each([f, twin] * 4, queries, k))
    assert (d["calls"], d["exact"]) == (0, 1)
    host_same(got)
    # a query on the walk path is not grouped
    ix.set_filter_dense_each(1)
    ix.set_filter_policy("walk")
    _, d = moved(ix, lambda: ix.search_batch_filtered_each([f] * nq, queries, k))
    assert (d["calls"], d["exact"], d["walk"]) == (0, 0, 1)
    ix.close()


def test_callers_stream_and_null_outputs(capi, oracle, cores):
    from lantern_amd import hip

    n, nq, k = 2500, 6, 10
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", n, 64, nq, 25)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    a, b = random_set(rng, n, 900), random_set(rng, n, 40)
    fa, fb = ix.filter_from_bitmap(a), ix.filter_from_bitmap(b)
    filters = [fa, fb, fb, fa, fa, fb]
    want = [ref.search(None, dist[q:q + 1], a if f is fa else b, 0, k, 0, path="exact") for q, f in enumerate(filters)]
    qrows = ix.device_query_rows(queries)
    dq = hip.Buffer.from_numpy(qrows)
    slot, cnt, D = hip.Buffer(nq * k * 4), hip.Buffer(nq * 4), hip.Buffer(nq * 8)
    for buf in (slot, cnt, D):
        buf.upload(np.full(buf.nbytes, 0xA5, dtype=np.uint8))
    stream = hip.Stream()
    ix.set_filter_dense_each(3)
    ix.search_batch_filtered_each_device(filters, dq.ptr, qrows.strides[0], nq, k, 0, 0, None, None, slot.ptr, cnt.ptr, D.ptr, None, stream=stream.handle)
    assert ix.last_filtered_each_dense()["groups"] == 2
    stream.synchronize()
    assert np.array_equal(slot.download((nq, k), np.uint32), np.concatenate([w[0] for w in want]))
    assert np.array_equal(cnt.download(nq, np.uint32), np.concatenate([w[2] for w in want]))
    assert np.array_equal(D.download(nq, np.uint64), np.concatenate([w[3] for w in want]))
    # every output NULL: the route runs and still makes its additions to the cumulative counters
    _, d = moved(ix, lambda: (ix.search_batch_filtered_each_device(filters, dq.ptr, qrows.strides[0], nq, k, 0, 0, None, None, None, None, None, None,
                                                                   stream=stream.handle), stream.synchronize()))
    assert (d["calls"], d["queries"], d["exact"]) == (1, nq, 0)
    assert d["evals"] == 3 * 900 + 3 * 40 and d["searched"] == nq and d["expansions"] == 0
    ix.close()


def test_tombstones(capi, oracle, cores):
    n, nq = 2000, 6
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", n, 32, nq, 26)
    labels = np.arange(n, dtype=np.uint64) + 1
    labels[rng.random(n) < 0.4] = 0
    ix = index_of(capi, oracle, "l2sq", "f32", rows, labels=labels)
    allowed, other = rng.random(n) < 0.5, random_set(rng, n, 300)
    live = allowed & (labels != 0)
    f_live, f_other = ix.filter_from_bitmap(allowed, skip_deleted=True), ix.filter_from_bitmap(other)  # (f_other allows tombstones: label-0 rows come back)
    assert f_live.count == live.sum() and (labels[other] == 0).any()
    filters = [f_live, f_other, f_live, f_other, f_live, f_other]
    sets = {q: (live if f is f_live else other) for q, f in enumerate(filters)}
    dev = Dev(ix, queries, 10)
    _, _, dense, _, _ = check_each(ix, dev, filters, 3, exact_ref=(dist, sets))
    assert dense["groups"] == 2 and dense["recomputed"] == 0
    ix.set_filter_dense_each(3)
    got = each(dev, filters)
    assert np.all(got[5][0::2] != 0)
    ix.close()
