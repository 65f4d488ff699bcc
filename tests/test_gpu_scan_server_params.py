"""Paginating backends through the scan-side service on a device index (scan_server.cpp).  Needs an MI355X.

Backends on different pages of their scans, with different page sizes and ef, ask for different (k, ef): a continuation is a search for
handed-out + k rows.  Under LANTERN_SCAN_MIXED=1 the service sends the unfiltered requests of a batch out in ONE per-query-parameter
call (lantern_gpu_search_batch_params_lane_notify); LANTERN_SCAN_MIXED=0 is one call per distinct (k, ef).  Every page is compared
with the direct cursor search of the same scan, under both settings, and the mixed service makes fewer back-end calls for the same
request sequence."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, EF = 20000, 64, 64
NTHREADS, ROUNDS = 40, 6


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
    """backend t: its page size, its ef, and the rounds at which it begins a fresh scan (the others continue): out of step"""
    return 4 + t % 5, (0, 100, 30)[t % 3], {0, 2 + t % 3}


def run_service(capi, ix, queries, notify):
    """ROUNDS requests per backend, the backends released together at every round (so that a round is a batch or two whatever the
    setting, and both settings see the same request sequence)."""
    srv = capi.ScanServer(index=ix, max_batch=64, max_wait_us=30000)
    gate = threading.Barrier(NTHREADS)
    got, errs = {}, []

    def session(t):
        try:
            c = capi.ScanClient(srv.host, srv.port)
            k, ef, fresh = plan(t)
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
    st = srv.stats()
    srv.stop()
    assert not errs, errs
    return got, st


def check_against_cursor(ix, queries, got):
    for t in range(NTHREADS):
        k, ef, fresh = plan(t)
        cur = ix.cursor()
        seen = []
        for r in range(ROUNDS):
            if r in fresh:
                seen = []
            want = cur.search(queries[t], k, ef, streaming=r not in fresh)
            have = got[t][r]
            assert np.array_equal(have[0], want[0]) and np.array_equal(have[1].view(np.uint32), want[1].view(np.uint32)), (t, r)
            seen += have[0].tolist()
            assert len(set(seen)) == len(seen)  # paging never repeats a row
        cur.close()


@pytest.mark.parametrize("notify", ["1", "0"])
def test_paginating_backends_share_one_call_per_batch(capi, served, notify, monkeypatch):
    ix, queries = served
    monkeypatch.setenv("LANTERN_SCAN_NOTIFY", notify)
    monkeypatch.setenv("LANTERN_SCAN_MIXED", "1")
    mixed, st_mixed = run_service(capi, ix, queries, notify)
    regime = ix.last_params_launch()
    assert regime["launches"] >= 1 and sum(regime["classes"]) > 1, regime  # the per-query call was made, for several requests at once
    monkeypatch.setenv("LANTERN_SCAN_MIXED", "0")
    grouped, st_grouped = run_service(capi, ix, queries, notify)
    check_against_cursor(ix, queries, mixed)
    check_against_cursor(ix, queries, grouped)
    for t in range(NTHREADS):  # identical answers under both settings
        for a, b in zip(mixed[t], grouped[t]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert st_mixed["requests"] == st_grouped["requests"] == NTHREADS * ROUNDS
    print("launches mixed / grouped:", st_mixed["launches"], st_grouped["launches"], "batches:", st_mixed["batches"], st_grouped["batches"])
    assert st_mixed["launches"] < st_grouped["launches"], (st_mixed, st_grouped)
    assert st_mixed["launches"] <= st_mixed["batches"]  # at most one call per batch: no filtered requests here
