"""Mixed batches through the scan-side service (lantern_amd/csrc/scan_server.cpp): with a back end that takes (k, ef) per query
(lantern_scan_server_start_params_fn; on a device index, lantern_gpu_search_batch_params_lane*) the unfiltered requests of a batch go
out in ONE call whatever their (k, ef).  CPU tests over the real server, sockets, dispatcher and client code with an injected back
end: coalescing, routing, pagination, the uniform batch's path, the plain back end's grouping, error frames."""
import threading

import numpy as np
import pytest


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


TABLE = np.random.default_rng(3).standard_normal((400, 4)).astype(np.float32)


def rank(q, k):
    """rows of TABLE by squared distance to q: labels = row + 1, ascending; at most len(TABLE)"""
    d = ((q[None, :] - TABLE) ** 2).sum(-1)
    order = np.argsort(d, kind="stable")[:k]
    return (order + 1).astype(np.uint64), d[order].astype(np.float32)


def backends(plain_calls, mixed_calls, fail_ef=None):
    """The plain function and the per-query one over the same ranking; each records (nq, distinct (k, ef) it carried)."""
    def plain(queries, k, ef):
        q = queries.view(np.float32).reshape(queries.shape[0], -1)
        plain_calls.append((len(q), k, ef))
        if fail_ef is not None and ef == fail_ef:
            raise RuntimeError("the back end refuses ef = %d" % ef)
        lab, dst, cnt = np.zeros((len(q), k), np.uint64), np.full((len(q), k), np.inf, np.float32), np.zeros(len(q), np.uint32)
        for i in range(len(q)):
            l, d = rank(q[i], k)
            lab[i, :len(l)], dst[i, :len(l)], cnt[i] = l, d, len(l)
        return lab, dst, cnt

    def mixed(queries, params, k_stride):
        q = queries.view(np.float32).reshape(queries.shape[0], -1)
        mixed_calls.append((len(q), sorted({(int(p["k"]), int(p["ef"])) for p in params}), k_stride))
        assert not params["reserved"].any() and not params["skip"].any() and k_stride == params["k"].max()
        if fail_ef is not None and (params["ef"] == fail_ef).any():
            raise RuntimeError("the back end refuses ef = %d" % fail_ef)
        lab, dst, cnt = np.zeros((len(q), k_stride), np.uint64), np.full((len(q), k_stride), np.inf, np.float32), np.zeros(len(q), np.uint32)
        for i in range(len(q)):
            l, d = rank(q[i], int(params["k"][i]))
            lab[i, :len(l)], dst[i, :len(l)], cnt[i] = l, d, len(l)
        return lab, dst, cnt

    return plain, mixed


def paginate(capi, srv, t, pages, page_k, ef, out, errs, start):
    try:
        c = capi.ScanClient(srv.host, srv.port)
        q = np.random.default_rng(100 + t).standard_normal(4).astype(np.float32)
        start.wait()
        rows = []
        for p in range(pages):
            lab, dst = (c.search if p == 0 else c.search_next)(q, page_k, ef)
            rows.append((lab.copy(), dst.copy()))
        out[t] = (q, rows)
        c.close()
    except Exception as e:  # noqa: BLE001
        errs.append(repr(e))


def run_clients(capi, srv, nthreads, pages, page_k_of, ef_of):
    out, errs = {}, []
    start = threading.Barrier(nthreads)
    ts = [threading.Thread(target=paginate, args=(capi, srv, t, pages, page_k_of(t), ef_of(t), out, errs, start)) for t in range(nthreads)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    return out


def check_scans(out, pages, page_k_of):
    for t, (q, rows) in out.items():
        k = page_k_of(t)
        lab, dst = rank(q, pages * k)
        got = np.concatenate([r[0] for r in rows])
        assert len(set(got.tolist())) == len(got), "a scan saw a row twice"
        assert got.tolist() == lab.tolist(), t  # page after page: the scan's ranking, each row once
        assert np.array_equal(np.concatenate([r[1] for r in rows]), dst)


def test_mixed_requests_are_coalesced_into_calls_with_several_k_ef(capi):
    plain_calls, mixed_calls = [], []
    plain, mixed = backends(plain_calls, mixed_calls)
    srv = capi.ScanServer(batch_fn=plain, params_fn=mixed, vec_bytes=16, max_batch=64, max_wait_us=20000)
    nthreads, pages = 24, 5
    page_k_of, ef_of = (lambda t: 3 + t % 4), (lambda t: (0, 40, 90)[t % 3])
    out = run_clients(capi, srv, nthreads, pages, page_k_of, ef_of)
    st = srv.stats()
    srv.stop()
    check_scans(out, pages, page_k_of)  # every answer went to its connection; pagination never repeats a row
    assert st["requests"] == nthreads * pages
    assert st["launches"] == len(plain_calls) + len(mixed_calls)
    assert sum(c[0] for c in plain_calls) + sum(c[0] for c in mixed_calls) == st["requests"]
    assert mixed_calls and max(len(c[1]) for c in mixed_calls) >= 3, mixed_calls  # calls that carry several distinct (k, ef)
    assert all(len(c[1]) >= 2 for c in mixed_calls)  # a call with one (k, ef) never goes to the per-query function
    assert st["launches"] <= st["batches"], st  # one back-end call per batch, whatever its (k, ef)


def test_a_batch_with_one_shared_k_ef_goes_to_the_plain_function(capi):
    plain_calls, mixed_calls = [], []
    plain, mixed = backends(plain_calls, mixed_calls)
    srv = capi.ScanServer(batch_fn=plain, params_fn=mixed, vec_bytes=16, max_batch=64, max_wait_us=20000)
    out = run_clients(capi, srv, 16, 1, lambda t: 7, lambda t: 50)
    st = srv.stats()
    srv.stop()
    check_scans(out, 1, lambda t: 7)
    assert not mixed_calls and plain_calls and {(c[1], c[2]) for c in plain_calls} == {(7, 50)}
    assert st["launches"] == len(plain_calls) == st["batches"]


def test_a_plain_back_end_still_sees_one_call_per_k_ef(capi):
    plain_calls, mixed_calls = [], []
    plain, _ = backends(plain_calls, mixed_calls)
    srv = capi.ScanServer(batch_fn=plain, vec_bytes=16, max_batch=64, max_wait_us=20000)
    nthreads, pages = 16, 3
    page_k_of, ef_of = (lambda t: 3 + t % 4), (lambda t: (0, 40)[t % 2])
    out = run_clients(capi, srv, nthreads, pages, page_k_of, ef_of)
    st = srv.stats()
    srv.stop()
    check_scans(out, pages, page_k_of)
    assert st["launches"] == len(plain_calls) > st["batches"]  # several (k, ef) in a batch: several calls
    assert sum(c[0] for c in plain_calls) == st["requests"] == nthreads * pages


def test_a_failing_mixed_call_answers_with_error_frames_and_the_connections_survive(capi):
    plain_calls, mixed_calls = [], []
    plain, mixed = backends(plain_calls, mixed_calls, fail_ef=666)
    srv = capi.ScanServer(batch_fn=plain, params_fn=mixed, vec_bytes=16, max_batch=64, max_wait_us=30000)
    nthreads = 12
    errs, ok, failed = [], [], []
    start = threading.Barrier(nthreads)

    def session(t):
        try:
            c = capi.ScanClient(srv.host, srv.port)
            q = np.random.default_rng(t).standard_normal(4).astype(np.float32)
            start.wait()
            try:  # every request of the batch that carries ef = 666 gets the error frame, whatever its own ef
                c.search(q, 4 + t % 3, 666 if t == 0 else 30 + t % 2)
            except capi.LanternGpuError as e:
                assert "refuses ef = 666" in str(e)
                failed.append(t)
            lab, dst = c.search(q, 5, 20 + t % 2)  # the connection survived
            assert lab.tolist() == rank(q, 5)[0].tolist()
            ok.append(t)
            c.close()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=session, args=(t,)) for t in range(nthreads)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    srv.stop()
    assert not errs, errs
    assert 0 in failed and sorted(ok) == list(range(nthreads))
