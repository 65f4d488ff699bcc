"""A filter PER QUERY in one call (include/lantern_gpu.h "PER-QUERY FILTERS").  Needs an MI355X.

Method as tests/test_gpu_filtered_search.py: graphs are built by the oracle and imported, so the CPU restatement
(tests/filtered_walk_ref.py) walks the very graph the kernels walk.  The arbiter of every answer is that restatement, run per query with
that query's OWN allow-set and the path the rule gives that query: slots, distance bits, counts, D and E equal.  Equality with the
single-filter call is a second, cheaper check.  Each case proves its regime with GpuIndex.last_filtered_each (how many queries took which
path) and GpuIndex.filter_stats (launches).
"""
import threading

import numpy as np
import pytest

from tests import filtered_regimes as regimes
from tests import filtered_walk_ref as ref
from tests.test_gpu_filtered_regimes import check, instance
from tests.test_gpu_filtered_search import CASES, NQ, Dev, oracle_index, same

pytestmark = pytest.mark.gpu

FACTOR = 5.6  # the default exact_factor: exact iff allowed^2 <= FACTOR * ef * n


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


class EachDev(Dev):
    def plain_skip(self, skip):
        self.gpu.search_batch_device(self.dq.ptr, self.nq, self.k, 0, skip, self.lab.ptr, self.dist.ptr, self.slot.ptr, self.cnt.ptr, self.D.ptr,
                                     self.E.ptr, query_stride=self.rows.strides[0])
        return self._out()

    def each(self, filters, ef=0, skip=0):
        self.gpu.search_batch_filtered_each_device(filters, self.dq.ptr, self.rows.strides[0], self.nq, self.k, ef, skip, self.lab.ptr, self.dist.ptr,
                                                   self.slot.ptr, self.cnt.ptr, self.D.ptr, self.E.ptr)
        return self._out()


def mixed_sets(n, seed=11):
    """The allow-sets a mixed batch cycles over: all rows, 50 %, 10 %, 1 %, one row, none, and None (no filter)."""
    u = np.random.default_rng(seed).random(n)
    one = np.zeros(n, dtype=bool)
    one[np.random.default_rng(seed + 1).integers(0, n)] = True
    return [np.ones(n, dtype=bool), u < 0.5, u < 0.1, u < 0.01, one, np.zeros(n, dtype=bool), None]


def rule_exact(count, n, ef, forced, factor=FACTOR):
    if forced != "auto":
        return forced == "exact"
    return count * count <= factor * ef * n


def want_each(g, dist, sets, which, n, M, k, ef, skip=0, forced="auto", cand_cap=None, factor=FACTOR):
    """The restatement of a per-query call: query q with allow-set sets[which[q]] on the path the rule gives it.  Returns the
    (slots, dists, counts, D, E) arrays and the number of queries on the walk path, on the exact path, unfiltered and empty."""
    nq = len(which)
    slots = np.full((nq, k), ref.EMPTY, dtype=np.uint32)
    dists = np.full((nq, k), np.inf, dtype=np.float32)
    counts, D, E = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint64), np.zeros(nq, dtype=np.uint64)
    tally = {"walk": 0, "exact": 0, "unfiltered": 0, "empty": 0}
    for q in range(nq):
        allowed = sets[which[q]]
        if allowed is None:
            allowed, path = np.ones(n, dtype=bool), "walk"
            tally["unfiltered"] += 1
        elif not allowed.any():
            tally["empty"] += 1
            continue
        else:
            path = "exact" if rule_exact(int(allowed.sum()), n, ef, forced, factor) else "walk"
        tally[path] += 1
        s, d, c, D1, E1 = ref.search(g, dist[q:q + 1], allowed, M, k, ef, skip=skip, cand_cap=cand_cap, path=path)
        slots[q], dists[q], counts[q], D[q], E[q] = s[0], d[0], c[0], D1[0], E1[0]
    return (slots, dists, counts, D, E), tally


def launches(gpu, before):
    after = gpu.filter_stats()
    return after["walk"] - before["walk"], after["exact"] - before["exact"]


def regime_is(gpu, tally, distinct):
    got = gpu.last_filtered_each()
    for name in ("walk", "exact", "unfiltered", "empty"):
        assert got[name] == tally[name], (name, tally, got)
    assert got["distinct_filters"] == distinct, got
    return got


# ------------------------------------------------------------------------------------------------
# 1. mixed batch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,n,d,M,efc,ef,k", CASES)
def test_mixed_batch_matches_restatement_per_query(capi, oracle, metric, n, d, M, efc, ef, k):
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    dist = ref.distance_matrix(oracle, base, queries, metric, oracle.SUM_WAVE64, regimes.THREADS)
    sets = mixed_sets(n)
    which = [q % len(sets) for q in range(NQ)]
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    filters = [filt[w] for w in which]
    dev = EachDev(gpu, queries, k)
    threshold = int(np.floor(np.sqrt(FACTOR * ef * n)))
    try:
        for forced in ("auto", "walk", "exact"):
            gpu.set_filter_policy(forced)
            for skip in (0, 3):
                want, tally = want_each(g, dist, sets, which, n, M, k, ef, skip=skip, forced=forced)
                before = gpu.filter_stats()
                got = dev.each(filters, skip=skip)
                check(got, want, g["labels"])
                regime_is(gpu, tally, distinct=len(sets) - 1)
                assert tally["walk"] > 0  # (the None entries walk whatever the policy)
                if forced == "auto":
                    # the rule, per query: real filters at or below the threshold take the exact path, the others (and None) walk
                    n_exact = sum(1 for w in which if sets[w] is not None and 0 < sets[w].sum() <= threshold)
                    assert tally["exact"] == n_exact > 0, (tally, threshold)
                    if n <= FACTOR * ef:  # even an all-allowed filter is below the threshold: the None entries alone walk
                        assert tally["walk"] == tally["unfiltered"]
                # one launch per non-empty group, whatever the filters; the empty filters ride in the exact launch if there is one
                assert launches(gpu, before) == (1, 1 if tally["exact"] or (tally["empty"] and not tally["walk"]) else 0)
                assert gpu.last_filtered_each()["launches"] == sum(launches(gpu, before))
                s, _, c = got[0], got[1], got[2]
                for q in range(NQ):
                    a = sets[which[q]]
                    if a is not None:
                        assert a[s[q, : c[q]]].all(), q
                    if a is not None and not a.any():
                        assert c[q] == 0 and got[3][q] == 0 and got[4][q] == 0 and np.all(np.isinf(got[1][q])) and np.all(got[5][q] == 0)
            # the cheaper check (got: this policy at skip = 3): each query as the single-filter call, or the unfiltered search, answers it
            for w, f in enumerate(filt):
                qs = [q for q in range(NQ) if which[q] == w]
                one = dev.plain_skip(3) if f is None else dev.filtered(f, skip=3)
                same(tuple(a[qs] for a in one), tuple(a[qs] for a in got))
    finally:
        gpu.set_filter_policy("auto")


def test_host_form_equals_device_form(capi, oracle):
    metric, n, d, M, efc, ef, k = CASES[0]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    sets = mixed_sets(n)
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    filters = [filt[q % len(sets)] for q in range(NQ)]
    dev = EachDev(gpu, queries, k)
    s, dd, c, D, E, lab = dev.each(filters)
    for lab2, d2, c2 in (gpu.search_batch_filtered_each(filters, queries, k), gpu.search_batch_filtered_each_lane(3, filters, queries, k)):
        assert np.array_equal(lab2, lab) and np.array_equal(d2.view(np.uint32), dd.view(np.uint32)) and np.array_equal(c2, c)


# ------------------------------------------------------------------------------------------------
# 2. many queries per workgroup: a descriptor must not survive a ticket
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", ["walk", "exact"])
def test_two_workgroups_alternating_disjoint_filters(capi, oracle, forced):
    n, d, M, ef, k, nq = 3000, 64, 16, 64, 10, 320
    rng = np.random.default_rng(5)
    base = rng.standard_normal((n, d), dtype=np.float32)
    q48 = rng.standard_normal((48, d), dtype=np.float32)
    queries = np.tile(q48, (7, 1))[:nq]
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=64, ef=ef, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    gpu = capi.GpuIndex("l2sq", d, M=M, ef_construction=64, ef=ef, seed=9)
    gpu.import_graph(base, g)
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64, regimes.THREADS)
    even = np.arange(n) % 2 == 0
    sets = [even, ~even]
    which = [q % 2 for q in range(nq)]
    filt = [gpu.filter_from_bitmap(a) for a in sets]
    filters = [filt[w] for w in which]
    want, tally = want_each(g, dist, sets, which, n, M, k, ef, forced=forced)
    dev = EachDev(gpu, queries, k)
    try:
        gpu.set_filter_policy(forced)
        gpu.set_search_shape(0, max_workgroups=2)
        before = gpu.filter_stats()
        got = dev.each(filters)
        assert launches(gpu, before) == ((1, 0) if forced == "walk" else (0, 1))
        regime_is(gpu, tally, distinct=2)
        s, c = got[0], got[2]
        assert np.all(c == k)
        for q in range(nq):  # every returned slot lies in its own query's set
            assert np.all(s[q] % 2 == which[q]), (q, s[q])
        check(got, want, g["labels"])
    finally:
        gpu.set_search_shape(0, 0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 3. unfiltered entries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,n,d,M,efc,ef,k", CASES[:3])
def test_all_null_filters_equal_the_unfiltered_search(capi, oracle, metric, n, d, M, efc, ef, k):
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    dev = EachDev(gpu, queries, k)
    before = gpu.filter_stats()
    got = dev.each([None] * NQ)
    assert launches(gpu, before) == (1, 0)
    assert gpu.last_filtered_each() == {"walk": NQ, "exact": 0, "unfiltered": NQ, "empty": 0, "distinct_filters": 0, "launches": 1}
    same(got, dev.plain())
    for e in (10, 200):
        same(dev.each([None] * NQ, ef=e), dev.plain(ef=e))


# ------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_name_the_position_and_touch_nothing(capi, oracle):
    import ctypes as C

    metric, n, d, M, efc, ef, k = CASES[2]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    other = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=ef, seed=9)
    other.import_graph(base, g)
    good = gpu.filter_from_bitmap(np.arange(n) % 3 == 0)
    foreign = other.filter_from_bitmap(np.ones(n, dtype=bool))
    junk = C.create_string_buffer(4096)
    dev = EachDev(gpu, queries, k)
    marker = np.full(NQ * k, 0xABABABAB, dtype=np.uint32)

    def refused(filters, pattern):
        for buf in (dev.slot, dev.dist):
            buf.upload(marker)
        dev.cnt.upload(marker[:NQ])
        before, shape = gpu.filter_stats(), gpu.last_filtered_each()
        with pytest.raises(capi.LanternGpuError, match=pattern):
            dev.each(filters)
        dev.hip.synchronize()
        assert gpu.filter_stats() == before and gpu.last_filtered_each() == shape  # no launch
        assert np.array_equal(dev.slot.download(NQ * k, np.uint32), marker) and np.array_equal(dev.dist.download(NQ * k, np.uint32), marker)
        assert np.array_equal(dev.cnt.download(NQ, np.uint32), marker[:NQ])
        for call in (lambda: gpu.search_batch_filtered_each(filters, queries, k), lambda: gpu.search_batch_filtered_each_lane(0, filters, queries, k)):
            with pytest.raises(capi.LanternGpuError, match=pattern):
                call()
        assert gpu.filter_stats() == before

    valid = [good if q % 2 else None for q in range(NQ)]
    dev.each(valid)  # (the array is fine without the offender)
    refused(valid[:17] + [foreign] + valid[18:], r"another index .*\(filters\[17\]\)")
    refused(valid[:30] + [C.addressof(junk)] + valid[31:], r"not a filter handle .*\(filters\[30\]\)")
    refused(valid[:5] + [foreign] + valid[6:40] + [C.addressof(junk)] + valid[41:], r"\(filters\[5\]\)")  # the first offender
    gpu.add(10**6, base[0] * np.float32(0.5))
    fresh = gpu.filter_from_bitmap(np.ones(n + 1, dtype=bool))
    refused([fresh] * 22 + [good] + [fresh] * (NQ - 23), r"stale filter: built when the index held 1500 rows, it now holds 1501 .*\(filters\[22\]\)")
    dev.each([fresh if q % 2 else None for q in range(NQ)])
    # a compact pq index is refused as by the single-filter call
    rng = np.random.default_rng(8)
    pn, pd, S, Cn = 1000, 64, 8, 32
    pbase = rng.standard_normal((pn, pd), dtype=np.float32)
    cb = np.zeros((Cn, pd), dtype=np.float32)
    for s in range(S):
        cb[:, s * 8:(s + 1) * 8] = pbase[rng.choice(pn, size=Cn, replace=False), s * 8:(s + 1) * 8]
    pq = capi.GpuIndex("l2sq", pd, M=8, ef_construction=48, ef=40, seed=3, pq_codebook=cb, num_subvectors=S)
    pq.add_many(np.arange(pn, dtype=np.uint64) + 1, pbase)
    pq.flush()
    pf = pq.filter_from_bitmap(np.ones(pn, dtype=bool))
    _, _, cnt = pq.search_batch_filtered_each([pf, None, pf, None], pbase[:4], 10)  # expanded: served
    assert np.all(cnt == 10)
    pq.pq_compact()
    for filters in ([pf, None, pf, None], [None] * 4):
        with pytest.raises(capi.LanternGpuError, match="expand it first"):
            pq.search_batch_filtered_each(filters, pbase[:4], 10)


# ------------------------------------------------------------------------------------------------
# 5. visited-bitmap hygiene
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [2, 0], ids=["two_workgroups", "default_grid"])
def test_mixed_batch_at_30000_rows_leaves_the_bitmap_clean(capi, oracle, W):
    """The walks of the "within" filter spill and keep their undo log, those of "overflow" overflow it (tests/filtered_regimes.py); a
    one-in-a-thousand filter (exact path under a factor that keeps the other two walking), unfiltered and empty entries share the batch.
    A bit left behind shows in the unfiltered search after."""
    ix = regimes.big_index("gauss")
    g = ix["g"]
    gpu = capi.GpuIndex("l2sq", regimes.DIM, M=regimes.M, ef_construction=regimes.EFC, ef=regimes.EF, seed=9)
    gpu.import_graph(ix["base"], g)
    u = np.random.default_rng(21).random(regimes.N)
    sets = [regimes.regime_filter("within"), regimes.regime_filter("overflow"), u < 0.001, None, np.zeros(regimes.N, dtype=bool)]
    regimes.assert_regime("within", regimes.regime_reference("within")[3])
    regimes.assert_regime("overflow", regimes.regime_reference("overflow")[3])
    which = [q % len(sets) for q in range(regimes.NQ)]
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    factor = 0.01  # exact at or below sqrt(0.01 * 64 * 30000) = 138 allowed rows: the 900-row "overflow" filter walks
    want, tally = want_each(g, ix["dist"], sets, which, regimes.N, regimes.M, regimes.K, regimes.EF, factor=factor)
    assert tally["walk"] > tally["unfiltered"] > 0 and tally["exact"] > 0 and tally["empty"] > 0
    lab, dist, slot, D, E = ix["ora"].search_batch(ix["queries"], regimes.K, regimes.PLAIN_EF, regimes.THREADS)
    plain_want = (slot, dist, np.full(regimes.NQ, regimes.K, dtype=np.uint32), D, E)
    dev = EachDev(gpu, ix["queries"], regimes.K)
    try:
        gpu.set_filter_policy("auto", exact_factor=factor)
        gpu.set_search_shape(0, max_workgroups=W)
        for _ in range(2):
            got = dev.each([filt[w] for w in which])
            regime_is(gpu, tally, distinct=4)
            check(got, want, g["labels"])
            same(dev.plain(ef=regimes.PLAIN_EF), plain_want)
    finally:
        gpu.set_search_shape(0, 0)


# ------------------------------------------------------------------------------------------------
# 6. storage kinds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,metric,d", [("f16", "l2sq", 200), ("f16", "cos", 33), ("i8", "l2sq", 200), ("i8", "cos", 768), ("b1", "l2sq", 96),
                                              ("b1", "cos", 1000)])
def test_mixed_batch_on_quantised_storage(capi, oracle, storage, metric, d):
    n, nq, ef, k, M = 1500, 32, 64, 10, 16
    gpu, g, dist, queries = instance(capi, oracle, storage, metric, d, M, None, n, nq, ef)
    sets = mixed_sets(n)
    which = [q % len(sets) for q in range(nq)]
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    dev = EachDev(gpu, queries, k)
    for skip in (0, 3):
        want, tally = want_each(g, dist, sets, which, n, M, k, ef, skip=skip)
        assert tally["walk"] > tally["unfiltered"] and tally["exact"] > 0
        got = dev.each([filt[w] for w in which], skip=skip)
        regime_is(gpu, tally, distinct=len(sets) - 1)
        check(got, want, g["labels"])


# ------------------------------------------------------------------------------------------------
# 7. the lane form
# ------------------------------------------------------------------------------------------------
def test_two_lanes_with_different_filter_arrays(capi, oracle):
    metric, n, d, M, efc, ef, k = CASES[0]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    sets = mixed_sets(n)
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    arrays = [[filt[q % len(sets)] for q in range(NQ)], [filt[(3 * q + 1) % len(sets)] for q in range(NQ)]]
    qs = [queries, queries[::-1].copy()]
    alone = [gpu.search_batch_filtered_each_lane(lane, arrays[lane], qs[lane], k) for lane in (0, 1)]
    assert not all(np.array_equal(a, b) for a, b in zip(alone[0], alone[1]))
    rounds, barrier, out, errors = 8, threading.Barrier(2), [[], []], []

    def run(lane):
        try:
            for _ in range(rounds):
                barrier.wait()
                out[lane].append(gpu.search_batch_filtered_each_lane(lane, arrays[lane], qs[lane], k))
        except Exception as exc:  # noqa: BLE001 -- reported by the main thread
            errors.append(exc)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(lane,)) for lane in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for lane in (0, 1):
        assert len(out[lane]) == rounds
        for lab, dist, cnt in out[lane]:
            assert np.array_equal(lab, alone[lane][0]) and np.array_equal(dist.view(np.uint32), alone[lane][1].view(np.uint32))
            assert np.array_equal(cnt, alone[lane][2])


def test_a_filter_may_be_freed_when_the_call_has_returned(capi, oracle):
    metric, n, d, M, efc, ef, k = CASES[2]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    rng = np.random.default_rng(12)
    first = None
    for _ in range(3):
        filt = [gpu.filter_from_bitmap(np.random.default_rng(100 + i).random(n) < 0.3) for i in range(8)]
        got = gpu.search_batch_filtered_each([filt[q % 8] for q in range(NQ)], queries, k)
        for f in filt:
            f.close()
        junk = [gpu.filter_from_bitmap(rng.random(n) < 0.5) for _ in range(8)]  # (likely to reuse the freed blocks)
        if first is None:
            first = got
        assert all(np.array_equal(a, b) for a, b in zip(first, got))
        del junk
