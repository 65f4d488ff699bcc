"""The dense route of the filtered exact path on the device (lantern_gpu_set_filter_dense; include/lantern_gpu.h "THE EXACT PATH'S DENSE
ROUTE", DESIGN.md 4.9 "Dense exact path").  Needs an MI355X.

The referee of every answer is tests/filtered_walk_ref.py::exact over the distance matrix in the device's summation order
(ref.distance_matrix); the same call with the setting at 0 -- today's k_search_exact_allowed -- is compared as well.  Slots, distance
bits, counts, D, E and labels equal, for every query.  The graph plays no part on the exact path: the rows are imported under an
empty graph, as tests/test_gpu_exact_knn.py does.
"""
import numpy as np
import pytest

from tests import filtered_walk_ref as ref
from tests.test_gpu_exact_knn import FAMILIES, empty_graph
from tests.test_gpu_filtered_search import Dev, same

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def stored_form(oracle, storage, metric, rows, queries):
    """(rows as stored, queries as stored, the oracle's summation order) of a storage kind"""
    if metric == "hamming":
        return rows, queries, oracle.SUM_WAVE64
    if storage == "f16":
        return oracle.round_f16(rows), oracle.round_f16(queries), oracle.SUM_WAVE64_F16
    if storage == "i8":
        return oracle.quantize_i8(rows), oracle.quantize_i8(queries), oracle.SUM_I8
    return rows, queries, oracle.SUM_WAVE64


def index_of(capi, oracle, metric, storage, rows, labels=None):
    g = empty_graph(rows.shape[0])
    g["labels"] = np.arange(rows.shape[0], dtype=np.uint64) + 1 if labels is None else labels
    ix = capi.GpuIndex(metric, rows.shape[1], M=4, ef_construction=8, seed=1, quantization=storage)
    ix.import_graph(oracle.quantize_i8(rows) if storage == "i8" else rows, g)
    ix.set_filter_policy("exact")
    return ix


def with_labels(got, labels, n):
    """the labels an answer must carry: the row's own, 0 in the tail"""
    slots, lab = got[0], got[5]
    want = np.where(slots == ref.EMPTY, 0, labels[np.minimum(slots, n - 1)]).astype(np.uint64)
    assert np.array_equal(lab, want), "labels differ"


def poison(dev):
    """every output buffer of `dev` filled with a pattern no answer holds: a cell the next call fails to write shows in the comparison"""
    for b in (dev.lab, dev.dist, dev.slot, dev.cnt, dev.D, dev.E):
        b.upload(np.full(b.nbytes, 0xA5, dtype=np.uint8))


def check(capi, oracle, cores, ix, dist, queries, allowed, k, skip=0, labels=None, recomputed=0, dev=None):
    """one filter, one (k, skip): the dense route == the referee == today's kernel; returns the dense stats of the call"""
    n = allowed.size
    labels = np.arange(n, dtype=np.uint64) + 1 if labels is None else labels
    dev = dev or Dev(ix, queries, k)
    f = ix.filter_from_bitmap(allowed)
    want = ref.search(None, dist, allowed, 0, k, 0, skip=skip, path="exact")
    ix.set_filter_dense(0)
    s0, e0 = ix.filter_dense_stats(), ix.filter_stats()
    poison(dev)
    today = dev.filtered(f, skip=skip)
    assert ix.filter_dense_stats() == s0 and ix.filter_stats()["exact"] == e0["exact"] + 1
    same(today, want)
    with_labels(today, labels, n)
    ix.set_filter_dense(1)
    tot0 = ix.counters()
    poison(dev)  # (the buffers held today's answer: what is compared below is what the dense route wrote)
    got = dev.filtered(f, skip=skip)
    tot1, s1 = ix.counters(), ix.filter_dense_stats()
    ix.set_filter_dense(0)
    same(got, want)
    same(got, today)
    assert np.array_equal(got[5], today[5]), "labels differ from today's kernel"
    with_labels(got, labels, n)
    st = {key: s1[key] - s0[key] for key in s1}
    assert st["calls"] == 1 and st["queries"] == dev.nq and st["certified"] + st["recomputed"] == dev.nq, st
    assert ix.last_filtered_launch() == {"path": "dense", "grid": 0, "expansion": k + skip, "cand_cap": 0, "vis_slots": 0, "lds_bytes": 0}
    # the cumulative counters move as under today's kernel: D = allowed per query, E = 0
    assert tot1["search_dist_evals"] - tot0["search_dist_evals"] == dev.nq * int(allowed.sum())
    assert tot1["search_expansions"] == tot0["search_expansions"] and tot1["search_queries"] - tot0["search_queries"] == dev.nq
    if recomputed == 0:
        assert st["recomputed"] == 0, ("the certificate refused queries of an input chosen to certify", st)
    elif recomputed == "some":
        assert st["recomputed"] > 0, st
    f.close()
    return st


def gauss_case(capi, oracle, cores, metric, storage, n, d, nq, seed, scale=1.0):
    rng = np.random.default_rng([seed, n, d, nq])
    if metric == "hamming":
        rows, queries = rng.integers(0, 2 ** 32, size=(n, d), dtype=np.uint32), rng.integers(0, 2 ** 32, size=(nq, d), dtype=np.uint32)
    else:
        rows, queries = (rng.standard_normal((n, d), dtype=F32) * F32(scale)).astype(F32), (rng.standard_normal((nq, d), dtype=F32) * F32(scale)).astype(F32)
    sr, sq, mode = stored_form(oracle, storage, metric, rows, queries)
    dist = ref.distance_matrix(oracle, sr, sq, metric, mode, cores)
    return rows, queries, dist, rng


def random_set(rng, n, count):
    allowed = np.zeros(n, dtype=bool)
    allowed[rng.choice(n, size=count, replace=False)] = True
    return allowed


# ---- the edges of the plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ["1", "0"])
def test_chunk_edge(capi, oracle, cores, monkeypatch, fused):
    """65 537 allowed rows: a second gathered chunk of one row; again with the fused epilogue off (the switch is read per call)"""
    monkeypatch.setenv("LANTERN_GPU_DENSE_FUSED", fused)
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", 70000, 8, 3, 1)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    check(capi, oracle, cores, ix, dist, queries, random_set(rng, 70000, 65537), 10)
    ix.close()


def test_seed_column_edge(capi, oracle, cores):
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", 6000, 16, 5, 2)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    dev = Dev(ix, queries, 10)
    for count in (4095, 4096, 4097):
        check(capi, oracle, cores, ix, dist, queries, random_set(rng, 6000, count), 10, dev=dev)
    ix.close()


def test_query_tile_edge(capi, oracle, cores):
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", 1000, 4, 1025, 3)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    check(capi, oracle, cores, ix, dist, queries, random_set(rng, 1000, 300), 10)
    ix.close()


def test_short_answers_and_paging(capi, oracle, cores):
    n, d, nq = 1200, 24, 7
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", n, d, nq, 4)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    dev10 = Dev(ix, queries, 10)
    # allowed = 1; allowed < k + 16; allowed < k + skip; skip >= allowed (count 0)
    for count, skip in ((1, 0), (20, 0), (25, 20), (12, 5), (12, 12), (12, 40)):
        check(capi, oracle, cores, ix, dist, queries, random_set(rng, n, count), 10, skip=skip, dev=dev10)
    # k + skip = 240, with more and with fewer allowed rows than that
    dev200 = Dev(ix, queries, 200)
    check(capi, oracle, cores, ix, dist, queries, random_set(rng, n, 700), 200, skip=40, dev=dev200)
    check(capi, oracle, cores, ix, dist, queries, random_set(rng, n, 230), 200, skip=40, dev=dev200)
    # pages skip = 0, 10, 20 of k = 10 join to one call of k = 30
    allowed = random_set(rng, n, 400)
    f = ix.filter_from_bitmap(allowed)
    ix.set_filter_dense(1)
    pages = []
    for s in (0, 10, 20):
        poison(dev10)
        pages.append(dev10.filtered(f, skip=s))
    whole = Dev(ix, queries, 30).filtered(f)
    assert ix.last_filtered_launch()["path"] == "dense"
    ix.set_filter_dense(0)
    for i, name in ((0, "slots"), (1, "distances"), (5, "labels")):
        joined = np.concatenate([p[i] for p in pages], axis=1)
        assert np.array_equal(joined.view(np.uint32) if i == 1 else joined, whole[i].view(np.uint32) if i == 1 else whole[i]), name
    same(whole, ref.search(None, dist, allowed, 0, 30, 0, path="exact"))
    ix.close()


# ---- row kinds and group widths -------------------------------------------------------------------------------------------------
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
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, metric, storage, n, d, 9, 5, scale)
    ix = index_of(capi, oracle, metric, storage, rows)
    dev = Dev(ix, queries, 10)
    for count in (n // 2, 60):
        check(capi, oracle, cores, ix, dist, queries, random_set(rng, n, count), 10, skip=3, dev=dev)
    ix.close()


@pytest.mark.parametrize("storage", ["f16", "i8"])
def test_quantised_rows_on_the_f32_copy(capi, oracle, cores, monkeypatch, storage):
    """LANTERN_GPU_DENSE_NATIVE=0: the gathered chunk is dequantised and its norms taken on the copy"""
    monkeypatch.setenv("LANTERN_GPU_DENSE_NATIVE", "0")
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", storage, 900, 100, 9, 6, 0.3)
    ix = index_of(capi, oracle, "l2sq", storage, rows)
    check(capi, oracle, cores, ix, dist, queries, random_set(rng, 900, 450), 10)
    ix.close()


def pq_twin(capi, metric="l2sq", n=1500, d=96, S=4, C=200):
    from tests import filtered_adc_ref as adc

    rng = np.random.default_rng(n + d + S)
    base = rng.standard_normal((n, d), dtype=F32)
    queries = rng.standard_normal((9, d), dtype=F32)
    cb = adc.make_codebook(rng, base, S, C)
    make = lambda: capi.GpuIndex(metric, d, M=8, ef_construction=48, ef=64, seed=5, pq_codebook=cb, num_subvectors=S)
    twin = make()
    twin.set_add_batch(256, 16)
    twin.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    twin.flush()
    return twin, make, queries, rng


def test_expanded_pq_index_and_compact_routing(capi, oracle, cores):
    twin, make, queries, rng = pq_twin(capi)
    n = 1500
    decoded = twin.export_graph(with_vectors=True)["vectors"]
    dist = ref.distance_matrix(oracle, decoded, queries, "l2sq", oracle.SUM_WAVE64, cores)
    twin.set_filter_policy("exact")
    allowed = random_set(rng, n, 700)
    check(capi, oracle, cores, twin, dist, queries, allowed, 10)
    # the same index, compact and served (set_filter_compact): today's kernels, whatever the setting
    ix = make()
    ix.load_buffer(twin.save_buffer())
    ix.pq_compact()
    ix.set_filter_compact(1)
    ix.set_filter_policy("exact")
    ix.set_filter_dense(1)
    f = ix.filter_from_bitmap(allowed)
    before, e0 = ix.filter_dense_stats(), ix.filter_stats()["exact"]
    got = Dev(ix, queries, 10).filtered(f)
    assert ix.filter_dense_stats() == before and ix.filter_stats()["exact"] == e0 + 1 and ix.last_filtered_launch()["path"] == "exact"
    same(got, ref.search(None, dist, allowed, 0, 10, 0, path="exact"))
    ix.close()
    twin.close()


# ---- the certificate's refusals: answered by today's kernel ---------------------------------------------------------------------
@pytest.mark.parametrize("family,recomputed", [("offset10", "some"), ("dupgroups", "any")])
def test_recomputed_queries(capi, oracle, cores, family, recomputed):
    n, d, nq = 4000, 128, 16
    rng = np.random.default_rng([0, n, d, nq, 10])
    rows, queries = FAMILIES[family](rng, n, d, nq)
    dist = ref.distance_matrix(oracle, rows, queries, "l2sq", oracle.SUM_WAVE64, cores)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    e0 = ix.filter_stats()["exact"]
    st = check(capi, oracle, cores, ix, dist, queries, np.random.default_rng(7).random(n) < 0.5, 10, skip=2, recomputed=recomputed)
    # today's call, and the per-query launch over the refused queries if there were any
    assert ix.filter_stats()["exact"] - e0 == 1 + (1 if st["recomputed"] else 0)
    ix.close()


# ---- state ----------------------------------------------------------------------------------------------------------------------
def test_nothing_carried_over_between_filters(capi, oracle, cores):
    n = 3000
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "cos", "f32", n, 40, 6, 8)
    ix = index_of(capi, oracle, "cos", "f32", rows)
    dev = Dev(ix, queries, 10)
    u = rng.random(n)
    for allowed in (u < 0.6, u > 0.97, (u > 0.6) & (u < 0.8)):  # disjoint, of different sizes: the pooled buffers and norms are the call's own
        check(capi, oracle, cores, ix, dist, queries, allowed, 10, dev=dev)
    ix.close()


def test_tombstones(capi, oracle, cores):
    n = 2000
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", n, 32, 6, 9)
    labels = np.arange(n, dtype=np.uint64) + 1
    labels[rng.random(n) < 0.4] = 0
    ix = index_of(capi, oracle, "l2sq", "f32", rows, labels=labels)
    allowed = rng.random(n) < 0.5
    assert (labels[allowed] == 0).any()
    check(capi, oracle, cores, ix, dist, queries, allowed, 10, labels=labels)  # a filter that allows tombstones: label-0 rows come back
    f = ix.filter_from_bitmap(allowed, skip_deleted=True)
    live = allowed & (labels != 0)
    assert f.count == live.sum()
    ix.set_filter_dense(1)
    got = Dev(ix, queries, 10).filtered(f)
    assert ix.last_filtered_launch()["path"] == "dense"
    ix.set_filter_dense(0)
    same(got, ref.search(None, dist, live, 0, 10, 0, path="exact"))
    assert np.all(got[5] != 0)
    ix.close()


def test_routing(capi, oracle, cores):
    n, m = 1500, 8
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", n, 16, m, 10)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    assert ix.filter_dense() == 0
    ix.set_filter_dense(m)
    assert ix.filter_dense() == m
    allowed = random_set(rng, n, 500)
    f = ix.filter_from_bitmap(allowed)
    want = ref.search(None, dist, allowed, 0, 10, 0, path="exact")

    def moved(call):
        d0, f0 = ix.filter_dense_stats(), ix.filter_stats()
        out = call()
        d1, f1 = ix.filter_dense_stats(), ix.filter_stats()
        return out, d1["calls"] - d0["calls"], f1["exact"] - f0["exact"], f1["walk"] - f0["walk"]

    # nq = m - 1: today's exact launch; nq = m: the dense route, path 3
    got, dense, exact, walk = moved(lambda: Dev(ix, queries[: m - 1], 10).filtered(f))
    assert (dense, exact, walk) == (0, 1, 0) and ix.last_filtered_launch()["path"] == "exact"
    same(got, tuple(x[: m - 1] for x in want))
    got, dense, exact, walk = moved(lambda: Dev(ix, queries, 10).filtered(f))
    assert (dense, exact, walk) == (1, 0, 0) and ix.last_filtered_launch()["path"] == "dense"
    same(got, want)
    # the host form takes it too
    (lab, dd, cnt), dense, exact, walk = moved(lambda: ix.search_batch_filtered(f, queries, 10))
    assert (dense, exact, walk) == (1, 0, 0)
    assert np.array_equal(lab, want[0].astype(np.uint64) + 1) and np.array_equal(dd.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(cnt, want[2])
    # k + skip = 241: today's kernel
    got, dense, exact, walk = moved(lambda: Dev(ix, queries, 10).filtered(f, skip=231))
    assert (dense, exact, walk) == (0, 1, 0)
    same(got, ref.search(None, dist, allowed, 0, 10, 0, skip=231, path="exact"))
    # a query on the walk path: the walk
    ix.set_filter_policy("walk")
    _, dense, exact, walk = moved(lambda: Dev(ix, queries, 10).filtered(f))
    assert (dense, exact, walk) == (0, 0, 1)
    ix.set_filter_policy("exact")
    # a per-query call and a cursor search leave the dense route alone
    ix.set_filter_dense(1)
    _, dense, exact, walk = moved(lambda: ix.search_batch_filtered_each([f] * m, queries, 10))
    assert (dense, exact, walk) == (0, 1, 0)
    cur = ix.cursor()
    (lab, dd), dense, exact, walk = moved(lambda: cur.search_filtered(f, queries[0], 10))
    cur.close()
    assert (dense, exact, walk) == (0, 1, 0) and np.array_equal(lab, want[0][0].astype(np.uint64) + 1)
    ix.close()


def test_callers_stream_and_null_outputs(capi, oracle, cores):
    from lantern_amd import hip

    n, nq, k = 2500, 5, 10
    rows, queries, dist, rng = gauss_case(capi, oracle, cores, "l2sq", "f32", n, 64, nq, 11)
    ix = index_of(capi, oracle, "l2sq", "f32", rows)
    allowed = random_set(rng, n, 900)
    f = ix.filter_from_bitmap(allowed)
    want = ref.search(None, dist, allowed, 0, k, 0, path="exact")
    qrows = ix.device_query_rows(queries)
    dq = hip.Buffer.from_numpy(qrows)
    slot, cnt, D = hip.Buffer(nq * k * 4), hip.Buffer(nq * 4), hip.Buffer(nq * 8)
    stream = hip.Stream()
    ix.set_filter_dense(1)
    ix.search_batch_filtered_device(f, dq.ptr, qrows.strides[0], nq, k, 0, 0, None, None, slot.ptr, cnt.ptr, D.ptr, None, stream=stream.handle)
    assert ix.last_filtered_launch()["path"] == "dense"
    stream.synchronize()
    assert np.array_equal(slot.download((nq, k), np.uint32), want[0]) and np.array_equal(cnt.download(nq, np.uint32), want[2])
    assert np.array_equal(D.download(nq, np.uint64), want[3])
    s0, t0 = ix.filter_dense_stats(), ix.counters()
    ix.search_batch_filtered_device(f, dq.ptr, qrows.strides[0], nq, k, 0, 0, None, None, None, None, None, None, stream=stream.handle)  # every output NULL
    stream.synchronize()
    s1, t1 = ix.filter_dense_stats(), ix.counters()
    # the route ran and still made its additions to the cumulative counters
    assert s1["calls"] - s0["calls"] == 1 and s1["queries"] - s0["queries"] == nq and ix.last_filtered_launch()["path"] == "dense"
    assert t1["search_dist_evals"] - t0["search_dist_evals"] == nq * 900 and t1["search_queries"] - t0["search_queries"] == nq
    ix.close()
