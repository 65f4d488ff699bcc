"""Filters through the scan-side service (lantern_amd/csrc/scan_server.cpp "LSRF"): a connection sets its filter from a list of labels,
and the filtered requests of a batch -- whatever their filters -- go out in ONE per-query-filter call.  As tests/test_scan_server.py, the
CPU tests drive the REAL server, sockets, I/O threads, filter thread, dispatcher and client code over an injected back end -- here one that
also makes / frees filters and receives a filter per query (lantern_scan_server_start_filtered_fn)."""
import socket
import struct
import threading
import time

import numpy as np
import pytest

from tests.test_scan_server import _raw_reply, _raw_request, fake_backend

ROWS = 200  # the fake index: every query `ident` has the rows ident * 1000 + j, j < ROWS, at distance j; a filter is a set of j


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


class FakeFilters:
    """A filter-aware back end.  make: the labels are the allowed j (those >= ROWS are not in the index); label 666666 makes it fail."""

    def __init__(self):
        self.live, self.next, self.made, self.freed, self.each_calls, self.plain_calls = {}, 1, [], [], [], []
        self.lock = threading.Lock()

    def make(self, labels, flags):
        if 666666 in labels.tolist():
            raise RuntimeError("fake back end: cannot build this filter")
        allowed = sorted({int(x) for x in labels.tolist() if x < ROWS and not (flags & 1 and x == 0)})
        with self.lock:
            h = self.next
            self.next += 1
            self.live[h] = allowed
            self.made.append(h)
        return h, len(allowed), 128 + 4 * len(allowed)

    def free(self, h):
        with self.lock:
            assert h in self.live, "a filter freed twice, or never made"
            del self.live[h]
            self.freed.append(h)

    def each(self, filters, queries, k, ef):
        nq = queries.shape[0]
        first = queries.view(np.float32)[:, 0]
        lab, dst, cnt = np.zeros((nq, k), dtype=np.uint64), np.full((nq, k), np.inf, dtype=np.float32), np.zeros(nq, dtype=np.uint32)
        with self.lock:
            self.each_calls.append(list(filters))
            for i, h in enumerate(filters):
                assert h in self.live, "a request searched through a filter that is not resident"
                js = self.live[h][:k]
                cnt[i] = len(js)
                lab[i, : len(js)] = [int(first[i]) * 1000 + j for j in js]
                dst[i, : len(js)] = js
        return lab, dst, cnt

    def fns(self):
        return (self.make, self.free, self.each)

    def server(self, capi, **kw):
        return capi.ScanServer(batch_fn=fake_backend(self.plain_calls), filter_fns=self.fns(), vec_bytes=8, **kw)


def q(ident):
    return np.array([ident, 0], dtype=np.float32)


def wait_for(cond, seconds=5.0):
    t0 = time.perf_counter()
    while not cond():
        assert time.perf_counter() - t0 < seconds, "timed out"
        time.sleep(0.01)


def raw_filter(labels, flags=0, count=None):
    labels = np.asarray(labels, dtype=np.uint64)
    return struct.pack("<IIQ", 0x4652534C, flags, labels.size if count is None else count) + labels.tobytes()


def raw_filter_reply(sock):
    buf = b""
    while len(buf) < 12:
        chunk = sock.recv(12 - len(buf))
        assert chunk, "the server closed the connection"
        buf += chunk
    magic, status, n = struct.unpack("<III", buf)
    assert magic == 0x5052534C
    want, body = (n if status else 8), b""
    while len(body) < want:
        chunk = sock.recv(want - len(body))
        assert chunk
        body += chunk
    return (status, body.decode()) if status else (0, struct.unpack("<Q", body)[0])


def test_filters_are_routed_to_the_right_queries_of_a_coalesced_batch(capi):
    be = FakeFilters()
    srv = be.server(capi, max_batch=64, max_wait_us=20000)
    nthreads, per = 32, 6
    start = threading.Barrier(nthreads)
    got, errs = {}, []

    def allowed_of(t):
        return None if t % 4 == 0 else [j for j in range(ROWS) if j % (t % 7 + 2) == t % 2]

    def session(t):
        try:
            c = capi.ScanClient(srv.host, srv.port)
            a = allowed_of(t)
            if a is not None:
                assert c.set_filter(np.array(a[::-1] + [ROWS + 5], dtype=np.uint64)) == len(a)  # any order; a stranger among them
            start.wait()
            for i in range(per):
                ident = t * 10 + i + 1
                rows = [c.search(q(ident), 5)[0].tolist()]
                for _ in range(2):
                    rows.append(c.search_next(q(ident), 5)[0].tolist())
                got[(t, ident)] = rows
            c.close()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=session, args=(t,)) for t in range(nthreads)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    st, fst = srv.stats(), srv.filter_stats()
    assert not errs, errs
    for (t, ident), pages in got.items():
        a = allowed_of(t)
        js = (a if a is not None else list(range(ROWS)))[:15]
        flat = [x for p in pages for x in p]
        assert flat == [ident * 1000 + j for j in js], (t, ident)  # allowed rows only, in order, never one twice
    n_f = sum(1 for t in range(nthreads) if allowed_of(t) is not None)
    assert fst["filters_set"] == n_f and fst["filtered_requests"] == n_f * per * 3
    assert fst["each_calls"] == len(be.each_calls) < fst["filtered_requests"]  # coalescing happened ...
    assert fst["most_distinct_filters"] == max(len(set(c)) for c in be.each_calls) >= 2  # ... across connections with different filters
    assert sum(len(c) for c in be.each_calls) == fst["filtered_requests"]
    assert sum(c[0] for c in be.plain_calls) == (nthreads - n_f) * per * 3  # the unfiltered requests took the old path
    assert st["requests"] == nthreads * per * 3 and st["launches"] == len(be.each_calls) + len(be.plain_calls)
    # every connection closed: its filter is released
    wait_for(lambda: srv.filter_stats()["resident_bytes"] == 0)
    assert sorted(be.freed) == sorted(be.made) and not be.live
    srv.stop()


def test_replace_clear_and_empty_filters(capi):
    be = FakeFilters()
    srv = be.server(capi, max_wait_us=100)
    c = capi.ScanClient(srv.host, srv.port)
    assert c.search(q(1), 3)[0].tolist() == [1000, 1001, 1002]
    assert c.set_filter([5, 7, 9, 11]) == 4
    assert srv.filter_stats()["resident_bytes"] == 128 + 16
    assert c.search(q(1), 3)[0].tolist() == [1005, 1007, 1009]
    assert c.search_next(q(1), 3)[0].tolist() == [1011]
    # replaced in the middle of a scan: the scan is over (a continuation starts afresh), the old filter is released
    assert c.set_filter([0, 7, 8], skip_deleted=True) == 2
    assert be.freed == [1] and srv.filter_stats()["resident_bytes"] == 128 + 8
    assert c.search_next(q(1), 3)[0].tolist() == [1007, 1008]
    # an empty list is a filter that allows nothing -- not "clear"
    assert c.set_filter([]) == 0
    assert c.search(q(2), 3)[0].tolist() == []
    assert srv.filter_stats()["resident_bytes"] == 128
    c.clear_filter()
    assert srv.filter_stats()["resident_bytes"] == 0 and be.freed == [1, 2, 3]
    assert c.search(q(2), 3)[0].tolist() == [2000, 2001, 2002]
    assert len(be.plain_calls) == 2 and srv.filter_stats()["filters_set"] == 3
    # a back end that cannot build the filter: its message comes back, the previous filter stays in force
    assert c.set_filter([1, 2]) == 2
    with pytest.raises(capi.LanternGpuError, match="cannot build this filter"):
        c.set_filter([3, 666666])
    assert c.search(q(3), 3)[0].tolist() == [3001, 3002]
    with pytest.raises(capi.LanternGpuError, match="unknown filter flags"):
        capi._call("lantern_scan_client_set_filter", c.c, None, 0, 6)
    c.close()
    wait_for(lambda: srv.filter_stats()["resident_bytes"] == 0)
    srv.stop()
    assert not be.live


def test_filter_frames_in_pieces_and_back_to_back_with_a_request(capi):
    be = FakeFilters()
    srv = be.server(capi, max_wait_us=500)
    s = socket.create_connection((srv.host, srv.port))
    s.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
    other = capi.ScanClient(srv.host, srv.port)
    msg = raw_filter([3, 4, 50, 60])
    for i in range(0, len(msg), 7):  # 48 bytes in seven pieces; another connection is served meanwhile
        s.sendall(msg[i:i + 7])
        assert other.search(q(9), 1)[0].tolist() == [9000]
        time.sleep(0.01)
    assert raw_filter_reply(s) == (0, 4)
    # a filter message and a request in one write: the request waits in the socket until the filter stands, and is searched through it
    s.sendall(raw_filter([10, 20]) + _raw_request(7, 3) + _raw_request(7, 1, magic=0x4352534C))
    assert raw_filter_reply(s) == (0, 2)
    assert _raw_reply(s, 3) == (0, [7010, 7020])
    assert _raw_reply(s, 1) == (0, [])  # the continuation: nothing is left
    # a large message (1.6 MB: several visits of its I/O thread) while the other connection keeps being answered
    big = raw_filter(np.arange(200000, dtype=np.uint64)[::-1])
    t = threading.Thread(target=lambda: s.sendall(big))
    t.start()
    for _ in range(20):
        assert other.search(q(9), 1)[0].tolist() == [9000]
    t.join()
    assert raw_filter_reply(s) == (0, ROWS)
    # bad flags: an error frame, the connection survives; clear with labels is one of them
    s.sendall(raw_filter([], flags=4))
    status, text = raw_filter_reply(s)
    assert status == 1 and "bad filter flags" in text
    s.sendall(raw_filter([1], flags=0x80000000))
    status, text = raw_filter_reply(s)
    assert status == 1 and "bad filter flags" in text
    s.sendall(raw_filter([], flags=0x80000000) + _raw_request(4, 2))
    assert raw_filter_reply(s) == (0, 0)
    assert _raw_reply(s, 2) == (0, [4000, 4001])
    # a client that dies in the middle of a filter message
    gone = socket.create_connection((srv.host, srv.port))
    gone.sendall(raw_filter(np.arange(100))[:200])
    gone.close()
    assert other.search(q(9), 1)[0].tolist() == [9000]
    s.close()
    other.close()
    wait_for(lambda: srv.filter_stats()["resident_bytes"] == 0)
    srv.stop()
    assert not be.live


def test_label_cap_closes_the_connection_and_byte_budget_does_not(capi, monkeypatch):
    monkeypatch.setenv("LANTERN_SCAN_FILTER_BYTES", "1000")
    be = FakeFilters()
    srv = be.server(capi, max_wait_us=100)
    # above the per-message label cap (2^24): the error frame goes out on the head alone and the connection is closed
    s = socket.create_connection((srv.host, srv.port))
    s.sendall(raw_filter([1, 2, 3], count=(1 << 24) + 1))
    status, text = raw_filter_reply(s)
    assert status == 1 and "at most 16777216 labels" in text and "closed" in text
    assert s.recv(1) == b""
    s.close()
    with pytest.raises(capi.LanternGpuError, match="too many labels"):  # (the client refuses before it sends)
        capi._call("lantern_scan_client_set_filter", capi.ScanClient(srv.host, srv.port).c, np.zeros(1, dtype=np.uint64).ctypes.data, (1 << 24) + 1, 0)
    # the byte budget (1000 here; the fake filter takes 128 + 4 per allowed row): refused after its payload was read, the connection
    # survives, its previous filter stays, and what others hold counts
    a, b = capi.ScanClient(srv.host, srv.port), capi.ScanClient(srv.host, srv.port)
    assert a.set_filter(list(range(100))) == 100  # 528 bytes
    with pytest.raises(capi.LanternGpuError, match=r"needs 528 bytes; 528 of the server's budget of 1000 are in use \(LANTERN_SCAN_FILTER_BYTES\)"):
        b.set_filter(list(range(100, 200)))
    assert b.search(q(1), 2)[0].tolist() == [1000, 1001]  # b: in step, unfiltered
    assert b.set_filter(list(range(100, 150))) == 50  # 328 bytes: fits
    assert srv.filter_stats()["resident_bytes"] == 528 + 328
    with pytest.raises(capi.LanternGpuError, match="budget of 1000"):
        a.set_filter(list(range(200)))  # 928 - 528 + 328 > 1000: refused ...
    assert a.search(q(2), 2)[0].tolist() == [2000, 2001] and srv.filter_stats()["resident_bytes"] == 528 + 328  # ... and a keeps its filter
    assert a.set_filter(list(range(130))) == 130  # replacing counts the difference: 648 + 328 fits
    assert srv.filter_stats()["resident_bytes"] == 648 + 328
    a.close()
    b.close()
    wait_for(lambda: srv.filter_stats()["resident_bytes"] == 0)
    srv.stop()


def test_a_back_end_without_filters_answers_with_an_error_frame(capi):
    srv = capi.ScanServer(batch_fn=fake_backend([]), vec_bytes=8, max_wait_us=100)
    c = capi.ScanClient(srv.host, srv.port)
    with pytest.raises(capi.LanternGpuError, match="this back end has no filters"):
        c.set_filter([1, 2, 3])
    with pytest.raises(capi.LanternGpuError, match="this back end has no filters"):
        c.clear_filter()
    assert c.search(q(5), 2)[0].tolist() == [5000, 5001]  # the connection survives, in step
    assert srv.filter_stats() == {"filters_set": 0, "filtered_requests": 0, "each_calls": 0, "most_distinct_filters": 0, "resident_bytes": 0}
    c.close()
    srv.stop()


def test_a_failing_call_is_asked_again_one_by_one(capi):
    """One stale filter refuses a whole per-query call; only ITS connection may see the error."""
    be = FakeFilters()
    stale = set()
    inner = be.each

    def each(filters, queries, k, ef):
        bad = [i for i, h in enumerate(filters) if h in stale]
        if bad:
            raise RuntimeError("lantern_gpu: stale filter: built when the index held 10 rows, it now holds 11 (filters[%d])" % bad[0])
        return inner(filters, queries, k, ef)

    srv = capi.ScanServer(batch_fn=fake_backend([]), filter_fns=(be.make, be.free, each), vec_bytes=8, max_batch=8, max_wait_us=200000)
    cs = [capi.ScanClient(srv.host, srv.port) for _ in range(4)]
    for i, c in enumerate(cs):
        assert c.set_filter([i, i + 10]) == 2
    stale.add(be.made[2])
    out = {}

    def session(i):
        try:
            out[i] = cs[i].search(q(i + 1), 2)[0].tolist()
        except capi.LanternGpuError as e:
            out[i] = str(e)

    ts = [threading.Thread(target=session, args=(i,)) for i in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert "stale filter" in out[2] and "now holds 11" in out[2]
    for i in (0, 1, 3):
        assert out[i] == [(i + 1) * 1000 + i, (i + 1) * 1000 + i + 10], out
    # the connection survives and may send its filter again
    assert cs[2].set_filter([2, 12]) == 2
    assert cs[2].search(q(3), 2)[0].tolist() == [3002, 3012]
    [c.close() for c in cs]
    srv.stop()


def test_stop_with_filters_resident_does_not_hang_or_leak(capi):
    be = FakeFilters()
    srv = be.server(capi, max_wait_us=100)
    clients = [capi.ScanClient(srv.host, srv.port) for _ in range(6)]
    for i, c in enumerate(clients[:4]):
        assert c.set_filter(list(range(i + 1))) == i + 1
    assert clients[0].search(q(1), 1)[0].tolist() == [1000]
    t0 = time.perf_counter()
    srv.stop()
    assert time.perf_counter() - t0 < 5
    assert not be.live and sorted(be.freed) == sorted(be.made) and len(be.made) == 4
    with pytest.raises(capi.LanternGpuError, match="went away|not connected"):
        clients[1].set_filter([1])
    [c.close() for c in clients]
