"""Filtered, paginating backends through the scan-side service on a device index (scan_server.cpp).  Needs an MI355X.

Every connection carries its own filter, is on its own page of its scan and has its own ef: the filtered requests of a batch differ in
(k, ef).  Under LANTERN_SCAN_MIXED=1 the service sends them out in ONE lantern_gpu_search_batch_filtered_each_params_lane call;
LANTERN_SCAN_MIXED=0 is one per-query-filter call per distinct (k, ef).  Every page is compared with the direct filtered cursor search of
the same scan, under both settings, and the mixed service makes fewer back-end calls for the same request sequence.  (The shape of
tests/test_gpu_scan_server_params.py.)"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, EF = 20000, 64, 64
NTHREADS, ROUNDS = 12, 6


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
    return ix, rng.standard_normal((NTHREADS, D), dtype=np.float32)


def plan(t):
    """backend t: its page size, its ef, the rounds at which it begins a fresh scan (the others continue) and its filter's labels: a
    tenth to a half of the rows (walk path), or one row in 150 (exact path); backend 7 is unfiltered"""
    step = (2, 150, 10, 3, 150, 5)[t % 6]
    labels = None if t == 7 else np.arange(t % step, N, step, dtype=np.uint64) + 1
    return 4 + t % 5, (0, 100, 30)[t % 3], {0, 2 + t % 3}, labels


def run_service(capi, ix, queries):
    """ROUNDS requests per backend, the backends released together at every round (so that a round is a batch or two whatever the
    setting, and both settings see the same request sequence)."""
    srv = capi.ScanServer(index=ix, max_batch=64, max_wait_us=30000)
    gate = threading.Barrier(NTHREADS)
    got, errs = {}, []

    def session(t):
        try:
            c = capi.ScanClient(srv.host, srv.port)
            k, ef, fresh, labels = plan(t)
            if labels is not None:
                assert c.set_filter(labels) == len(labels)
            pages = []
            for r in range(ROUNDS):
                gate.wait()
                pages.append((c.search if r in fresh else c.search_next)(queries[t], k, ef))
            got[t] = pages
            c.close()
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))
            gate.abort()

    ts = [threading.Thread(target=session, args=(t,)) for t in range(NTHREADS)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    st, fst = srv.stats(), srv.filter_stats()
    srv.stop()
    assert not errs, errs
    return got, st, fst


def check_against_cursor(ix, queries, got):
    for t in range(NTHREADS):
        k, ef, fresh, labels = plan(t)
        f = None if labels is None else ix.filter_from_labels(labels)
        cur = ix.cursor()
        seen = []
        for r in range(ROUNDS):
            if r in fresh:
                seen = []
            streaming = r not in fresh
            want = cur.search(queries[t], k, ef, streaming=streaming) if f is None else cur.search_filtered(f, queries[t], k, ef, streaming=streaming)
            have = got[t][r]
            assert len(have[0]) == k
            assert np.array_equal(have[0], want[0]) and np.array_equal(have[1].view(np.uint32), want[1].view(np.uint32)), (t, r)
            if labels is not None:
                assert np.isin(have[0], labels).all()
            seen += have[0].tolist()
            assert len(set(seen)) == len(seen)  # paging never repeats a row
        cur.close()
        if f is not None:
            f.close()


def test_filtered_paginating_backends_share_one_call_per_batch(capi, served, monkeypatch):
    ix, queries = served
    monkeypatch.setenv("LANTERN_SCAN_MIXED", "1")
    before = ix.last_filtered_each_params()
    mixed, st_mixed, fst_mixed = run_service(capi, ix, queries)
    regime, carve = ix.last_filtered_each(), ix.last_filtered_each_params()
    # the per-query-parameter call was made (how many requests the calls carried: the call counts below)
    assert carve != before and (carve["largest_expansion"] >= EF or carve["largest_exact_keys"] > 0), carve
    assert regime["walk"] + regime["exact"] >= 1, regime
    monkeypatch.setenv("LANTERN_SCAN_MIXED", "0")
    grouped, st_grouped, fst_grouped = run_service(capi, ix, queries)
    assert ix.last_filtered_each_params() == carve  # (the switch off: the uniform per-query-filter calls, as before)
    check_against_cursor(ix, queries, mixed)
    check_against_cursor(ix, queries, grouped)
    for t in range(NTHREADS):  # identical answers under both settings
        for a, b in zip(mixed[t], grouped[t]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert st_mixed["requests"] == st_grouped["requests"] == NTHREADS * ROUNDS
    assert fst_mixed["filtered_requests"] == fst_grouped["filtered_requests"] == (NTHREADS - 1) * ROUNDS
    print("back-end calls mixed / grouped:", st_mixed["launches"], st_grouped["launches"], "per-query-filter calls:", fst_mixed["each_calls"],
          fst_grouped["each_calls"], "batches:", st_mixed["batches"], st_grouped["batches"])
    assert fst_mixed["each_calls"] < fst_grouped["each_calls"], (fst_mixed, fst_grouped)
    assert st_mixed["launches"] < st_grouped["launches"], (st_mixed, st_grouped)
    assert fst_mixed["each_calls"] <= st_mixed["batches"]  # at most one filtered call per batch
