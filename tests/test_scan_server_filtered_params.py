"""Filtered requests with several (k, ef) through the scan-side service (lantern_amd/csrc/scan_server.cpp): with a back end that takes a
filter AND (k, ef, skip) per query (lantern_scan_server_start_filtered_params_fn; on a device index under LANTERN_SCAN_MIXED=1,
lantern_gpu_search_batch_filtered_each_params_lane) the filtered requests of a batch go out in ONE call whatever their (k, ef).  CPU tests
over the real server, sockets, dispatcher and client code with an injected back end."""
import threading

import numpy as np
import pytest

from tests.test_scan_server_filtered import ROWS, FakeFilters, q


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


class FakeFiltersParams(FakeFilters):
    """... that also takes a filter and a parameter row per query; a request with ef = fail_ef makes the mixed call fail."""

    def __init__(self, fail_ef=None):
        super().__init__()
        self.mixed_calls, self.each_k_ef, self.fail_ef = [], [], fail_ef

    def each(self, filters, queries, k, ef):
        with self.lock:
            self.each_k_ef.append((len(filters), k, ef))
        if self.fail_ef is not None and ef == self.fail_ef:
            raise RuntimeError("the back end refuses ef = %d" % ef)
        return super().each(filters, queries, k, ef)

    def each_params(self, filters, queries, params, k_stride):
        nq = queries.shape[0]
        first = queries.view(np.float32)[:, 0]
        assert len(filters) == nq == len(params) and not params["reserved"].any() and not params["skip"].any() and k_stride >= params["k"].max()
        lab, dst, cnt = np.zeros((nq, k_stride), dtype=np.uint64), np.full((nq, k_stride), np.inf, dtype=np.float32), np.zeros(nq, dtype=np.uint32)
        with self.lock:
            self.mixed_calls.append((list(filters), [(int(p["k"]), int(p["ef"])) for p in params], [int(x) for x in first], k_stride))
            if self.fail_ef is not None and (params["ef"] == self.fail_ef).any():
                raise RuntimeError("the back end refuses ef = %d" % self.fail_ef)
            for i, h in enumerate(filters):
                assert h in self.live, "a request searched through a filter that is not resident"
                js = self.live[h][: int(params["k"][i])]
                cnt[i] = len(js)
                lab[i, : len(js)] = [int(first[i]) * 1000 + j for j in js]
                dst[i, : len(js)] = js
        return lab, dst, cnt

    def fns(self):
        return (self.make, self.free, self.each, self.each_params)


def allowed_of(t):
    return [j for j in range(ROWS) if j % (t % 5 + 2) == t % 2]


def sessions(capi, srv, nthreads, pages, page_k_of, ef_of, unfiltered=()):
    """nthreads connections, each with its own filter, paginating with its own page size and ef: {t: (ident, [page, ...])}"""
    start = threading.Barrier(nthreads)
    got, errs = {}, []

    def session(t):
        try:
            c = capi.ScanClient(srv.host, srv.port)
            if t not in unfiltered:
                assert c.set_filter(np.array(allowed_of(t), dtype=np.uint64)) == len(allowed_of(t))
            start.wait()
            ident = t + 1
            rows = []
            for p in range(pages):
                rows.append((c.search if p == 0 else c.search_next)(q(ident), page_k_of(t), ef_of(t))[0].tolist())
            got[t] = (ident, rows)
            c.close()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=session, args=(t,)) for t in range(nthreads)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    return got


def check_scans(got, pages, page_k_of, unfiltered=()):
    for t, (ident, rows) in got.items():
        js = (list(range(ROWS)) if t in unfiltered else allowed_of(t))[: pages * page_k_of(t)]
        flat = [x for p in rows for x in p]
        assert flat == [ident * 1000 + j for j in js], t  # allowed rows only, in order, never one twice


def test_filtered_requests_with_several_k_ef_arrive_in_one_call(capi):
    be = FakeFiltersParams()
    srv = be.server(capi, max_batch=64, max_wait_us=20000)
    nthreads, pages = 24, 4
    page_k_of, ef_of = (lambda t: 3 + t % 4), (lambda t: (0, 40, 90)[t % 3])
    unfiltered = {5, 17}
    got = sessions(capi, srv, nthreads, pages, page_k_of, ef_of, unfiltered)
    st, fst = srv.stats(), srv.filter_stats()
    srv.stop()
    check_scans(got, pages, page_k_of, unfiltered)
    assert be.mixed_calls and max(len(set(c[1])) for c in be.mixed_calls) >= 3, be.mixed_calls  # calls that carry several distinct (k, ef)
    assert all(len(set(c[1])) >= 2 for c in be.mixed_calls)  # a call with one (k, ef) never goes to the per-query-parameter function
    # the right filter and the right parameters for every query: query `ident` belongs to connection ident - 1
    for filters, k_ef, idents, k_stride in be.mixed_calls:
        assert k_stride == max(k for k, _ in k_ef)
        for h, (k, ef), ident in zip(filters, k_ef, idents):
            t = ident - 1
            assert t not in unfiltered and ef == ef_of(t) and k % page_k_of(t) == 0 and k <= pages * page_k_of(t), (t, k, ef)
    n_f = nthreads - len(unfiltered)
    assert fst["filtered_requests"] == n_f * pages == sum(len(c[0]) for c in be.mixed_calls) + sum(c[0] for c in be.each_k_ef)
    assert fst["each_calls"] == len(be.mixed_calls) + len(be.each_k_ef)
    assert sum(c[0] for c in be.plain_calls) == len(unfiltered) * pages  # the unfiltered requests took the path they always took
    assert st["launches"] == len(be.mixed_calls) + len(be.each_k_ef) + len(be.plain_calls)
    assert st["requests"] == nthreads * pages


def test_filtered_requests_with_one_shared_k_ef_take_the_each_function(capi):
    be = FakeFiltersParams()
    srv = be.server(capi, max_batch=64, max_wait_us=20000)
    got = sessions(capi, srv, 16, 1, lambda t: 7, lambda t: 50)
    st = srv.stats()
    srv.stop()
    check_scans(got, 1, lambda t: 7)
    assert not be.mixed_calls and be.each_k_ef and {(c[1], c[2]) for c in be.each_k_ef} == {(7, 50)}
    assert st["launches"] == len(be.each_k_ef) == st["batches"]


def test_without_the_new_function_filtered_requests_stay_grouped_by_k_ef(capi):
    be = FakeFiltersParams()
    srv = capi.ScanServer(batch_fn=lambda queries, k, ef: (_ for _ in ()).throw(AssertionError("no unfiltered request here")),
                          filter_fns=(be.make, be.free, be.each), vec_bytes=8, max_batch=64, max_wait_us=20000)
    nthreads, pages = 16, 3
    page_k_of, ef_of = (lambda t: 3 + t % 4), (lambda t: (0, 40)[t % 2])
    got = sessions(capi, srv, nthreads, pages, page_k_of, ef_of)
    st = srv.stats()
    srv.stop()
    check_scans(got, pages, page_k_of)
    assert not be.mixed_calls
    assert st["launches"] == len(be.each_k_ef) > st["batches"]  # several (k, ef) in a batch: several calls
    assert sum(c[0] for c in be.each_k_ef) == st["requests"] == nthreads * pages


def test_a_failing_mixed_call_is_repeated_per_request_and_the_connections_survive(capi):
    be = FakeFiltersParams(fail_ef=666)
    srv = be.server(capi, max_batch=64, max_wait_us=30000)
    nthreads = 12
    errs, ok, failed = [], [], []
    start = threading.Barrier(nthreads)

    def session(t):
        try:
            c = capi.ScanClient(srv.host, srv.port)
            c.set_filter(np.array(allowed_of(t), dtype=np.uint64))
            start.wait()
            k = 4 + t % 3
            try:  # only the request that carries ef = 666 gets the error frame: the others of its batch are asked again, alone
                lab, _ = c.search(q(t + 1), k, 666 if t == 0 else 30 + t % 2)
                assert lab.tolist() == [(t + 1) * 1000 + j for j in allowed_of(t)[:k]]
            except capi.LanternGpuError as e:
                assert "refuses ef = 666" in str(e)
                failed.append(t)
            lab, _ = c.search(q(t + 1), 5, 20 + t % 2)  # the connection survived
            assert lab.tolist() == [(t + 1) * 1000 + j for j in allowed_of(t)[:5]]
            ok.append(t)
            c.close()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=session, args=(t,)) for t in range(nthreads)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    srv.stop()
    assert not errs, errs
    assert failed == [0] and sorted(ok) == list(range(nthreads))
    # the batch that carried the offender: one mixed call of several requests that failed, then one call per request of it
    bad = [c for c in be.mixed_calls if 666 in [ef for _, ef in c[1]]]
    assert bad and len(bad[0][0]) > 1 and all(len(c[0]) == 1 for c in bad[1:]) and len(bad) == 2


def test_the_start_function_refuses_a_missing_back_end(capi):
    import ctypes as C

    err = C.c_char_p()
    fn = capi.BATCH_SEARCH_FN(lambda *a: 1)
    mk, fr = capi.FILTER_MAKE_FN(lambda *a: None), capi.FILTER_FREE_FN(lambda *a: None)
    each = capi.BATCH_SEARCH_EACH_FN(lambda *a: 1)
    none = C.cast(None, capi.BATCH_SEARCH_EACH_PARAMS_FN)
    assert capi.lib().lantern_scan_server_start_filtered_params_fn(fn, mk, fr, each, none, None, 16, b"127.0.0.1", 0, 8, 100, C.byref(err)) is None
    assert b"bad scan server arguments" in err.value
