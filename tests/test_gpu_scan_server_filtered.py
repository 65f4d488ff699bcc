"""Filtered scans through the scan-side service on a device index (scan_server.cpp "LSRF").  Needs an MI355X.

Concurrent backends, each with its own WHERE clause -- its own label filter on its connection -- share launches: the filtered requests
of a batch go out in one lantern_gpu_search_batch_filtered_each_lane call.  Every answer is compared with what the same index gives a
lone backend: lantern_gpu_cursor_search_filtered with a filter built from the same labels (the plain cursor for unfiltered clients)."""
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K, EF = 20000, 64, 10, 64


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


@pytest.fixture(scope="module")
def served(capi):
    rng = np.random.default_rng(5)
    base = rng.standard_normal((N, D), dtype=np.float32)
    ix = capi.GpuIndex("l2sq", D, M=16, ef_construction=64, ef=EF, seed=3)
    ix.add_many(np.arange(N, dtype=np.uint64) + 1, base)
    ix.flush()
    return ix, rng.standard_normal((64, D), dtype=np.float32)


def labels_of(t):
    """client t's WHERE clause as a label list (labels are slot + 1), or None: a quarter of the clients is unfiltered.  Selectivities
    from a half to one row: at n = 20000, ef = 64 the rule's threshold is 2677 allowed rows, so both paths are taken."""
    if t % 4 == 3:
        return None
    u = np.random.default_rng(1000 + t).random(N)
    sel = (0.5, 0.3, 0.1, 0.01, 0.001, 1.5 / N)[(t // 4 + t) % 6]
    rows = np.flatnonzero(u < sel)
    return (rows if rows.size else np.array([t])).astype(np.uint64) + 1


def test_concurrent_backends_with_their_own_filters_share_launches(capi, served):
    ix, queries = served
    nthreads, pages = 32, 3
    srv = capi.ScanServer(index=ix, max_batch=64, max_wait_us=20000)
    start = threading.Barrier(nthreads)
    got, errs = {}, []

    def session(t):
        try:
            c = capi.ScanClient(srv.host, srv.port)
            lab = labels_of(t)
            allowed = None if lab is None else c.set_filter(lab)
            start.wait()
            out = []
            for r in range(2):  # two scans per backend, paged with the continuation
                q = queries[(2 * t + r) % 64]
                rows = [c.search(q, K, EF)]
                for _ in range(pages - 1):
                    rows.append(c.search_next(q, K, EF))
                out.append(rows)
            got[t] = (allowed, out)
            c.close()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=session, args=(t,)) for t in range(nthreads)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    st, fst = srv.stats(), srv.filter_stats()
    assert not errs, errs
    n_f = sum(1 for t in range(nthreads) if labels_of(t) is not None)
    paths = set()
    for t in range(nthreads):
        lab = labels_of(t)
        allowed, out = got[t]
        f = None if lab is None else ix.filter_from_labels(lab)
        if f is not None:
            assert allowed == f.count == lab.size
            paths.add("exact" if f.count ** 2 <= 5.6 * EF * N else "walk")
        cur = ix.cursor()
        for r in range(2):
            q = queries[(2 * t + r) % 64]
            seen = []
            for p in range(pages):
                want = cur.search(q, K, EF, streaming=p > 0) if f is None else cur.search_filtered(f, q, K, EF, streaming=p > 0)
                have = out[r][p]
                assert np.array_equal(have[0], want[0]) and np.array_equal(have[1].view(np.uint32), want[1].view(np.uint32)), (t, r, p)
                seen += have[0].tolist()
            assert len(set(seen)) == len(seen)  # paging never repeats a row
            if lab is not None:
                assert set(seen) <= set(lab.tolist())  # allowed rows only
        cur.close()
    assert paths == {"walk", "exact"}
    assert fst["filters_set"] == n_f and fst["filtered_requests"] == n_f * 2 * pages
    assert fst["each_calls"] < fst["filtered_requests"] and fst["most_distinct_filters"] >= 2, fst  # different filters shared a call
    assert st["requests"] == nthreads * 2 * pages and st["launches"] > fst["each_calls"]  # the unfiltered ones: the old path
    t0 = time.perf_counter()
    while srv.filter_stats()["resident_bytes"] and time.perf_counter() - t0 < 5:
        time.sleep(0.01)
    assert srv.filter_stats()["resident_bytes"] == 0  # every connection closed with its filter set: all released
    srv.stop()


def test_replace_clear_empty_and_stale_filters_on_a_connection(capi):
    rng = np.random.default_rng(7)
    n = 3000
    base = rng.standard_normal((n + 1, D), dtype=np.float32)
    ix = capi.GpuIndex("l2sq", D, M=16, ef_construction=64, ef=EF, seed=3)
    ix.add_many(np.arange(n, dtype=np.uint64) + 1, base[:n])
    ix.flush()
    q = rng.standard_normal(D, dtype=np.float32)
    srv = capi.ScanServer(index=ix, max_wait_us=200)
    c = capi.ScanClient(srv.host, srv.port)
    plain = c.search(q, K)[0]
    evens = np.arange(2, n + 1, 2, dtype=np.uint64)
    assert c.set_filter(evens) == evens.size
    f = ix.filter_from_labels(evens)
    assert srv.filter_stats()["resident_bytes"] == capi._call("lantern_gpu_filter_resident_bytes", f.h) > 0
    a = c.search(q, K)[0]
    assert np.all(a % 2 == 0) and np.array_equal(a, ix.search_batch_filtered(f, q[None, :], K)[0][0])
    odds = evens - 1
    assert c.set_filter(odds) == odds.size  # replaced mid-connection
    b = c.search_next(q, K)[0]  # (the scan ended with the old filter: a fresh one)
    assert np.all(b % 2 == 1) and b.size == K
    assert c.set_filter([]) == 0  # an empty filter: nothing is allowed
    assert c.search(q, K)[0].size == 0
    c.clear_filter()
    assert srv.filter_stats()["resident_bytes"] == 0
    assert np.array_equal(c.search(q, K)[0], plain)
    # the served index grows: the filter is stale, the library's message comes back, the connection survives and sets it again
    assert c.set_filter(evens) == evens.size
    ix.add(10**6, base[n])
    with pytest.raises(capi.LanternGpuError, match="stale filter: built when the index held 3000 rows, it now holds 3001"):
        c.search(q, K)
    assert c.set_filter(evens) == evens.size
    assert np.all(c.search(q, K)[0] % 2 == 0)
    c.close()
    srv.stop()


def test_the_scan_shim_over_a_filtered_connection(capi, served):
    ix, queries = served
    lab = labels_of(2)
    srv = capi.ScanServer(index=ix, max_wait_us=200)
    c = capi.ScanClient(srv.host, srv.port)
    assert c.set_filter(lab) == lab.size
    f = ix.filter_from_labels(lab)
    for q in queries[:3]:
        scan = capi.Scan(client=c, init_k=10, ef=EF, metric="l2sq", dims=D)
        with pytest.raises(capi.LanternGpuError, match="lantern_scan_client_set_filter"):
            scan.set_filter(f)  # a handle is local to a process: the connection's filter is the way
        scan.rescan(q)
        rows = scan.fetch(50)
        local = capi.Scan(ix, init_k=10, ef=EF)
        local.set_filter(f)
        local.rescan(q)
        assert rows == local.fetch(50) and len(rows) == 50
        assert set(rows) <= set(lab.tolist())  # every gettuple label is allowed
        assert scan.trace() == local.trace() == [10, 20, 40]  # the reference's doubling (scan.c:240-292)
        scan.end()
        local.end()
    c.close()
    srv.stop()
