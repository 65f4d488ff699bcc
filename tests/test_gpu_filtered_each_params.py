"""A filter AND (k, ef, skip) per query in one call (include/lantern_gpu.h "PER-QUERY FILTERS WITH PER-QUERY k, ef AND skip", DESIGN.md
4.9).  Needs an MI355X.

Method as tests/test_gpu_filtered_each.py: graphs are built by the oracle and imported, so the CPU restatement (tests/filtered_walk_ref.py)
walks the very graph the kernels walk.  The arbiter of every answer is that restatement, run per query with that query's OWN allow-set,
path, k, ef, skip and C_i: slots, distance bits, counts, D and E equal.  Equality with the library's single-filter uniform call is the
second check.  Each case proves its regime with last_filtered_each, last_filtered_each_params and filter_stats.
"""
import threading

import numpy as np
import pytest

from tests import filtered_regimes as regimes
from tests import filtered_seeded_ref as sref
from tests import filtered_walk_ref as ref
from tests.test_gpu_filtered_each import FACTOR, EachDev, launches, mixed_sets, rule_exact
from tests.test_gpu_filtered_regimes import check, instance
from tests.test_gpu_filtered_search import CASES, NQ, Dev, oracle_index, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


class ParamsDev(Dev):
    """device buffers for nq rows of k_stride answers"""

    def each_params(self, filters, params):
        self.gpu.search_batch_filtered_each_params_device(filters, self.dq.ptr, self.rows.strides[0], self.nq, params, self.k, self.lab.ptr,
                                                          self.dist.ptr, self.slot.ptr, self.cnt.ptr, self.D.ptr, self.E.ptr)
        return self._out()


def rows_for(n):
    """the parameter rows (k, ef, skip) a mixed batch cycles over: ef 1, the defaults, a skip, the step of the automatic cap, ef 0 (the
    index's), a long answer, no answer, a skip of the whole index"""
    return [(1, 1, 0), (10, 64, 0), (10, 64, 10), (5, 65, 0), (10, 0, 0), (300, 64, 0), (0, 64, 0), (10, 64, n)]


def plan_fields(gpu, g, n, ef, forced="auto", cand_cap=0, factor=FACTOR, seeds=0):
    return {"chunks": gpu.row_bytes() // 16, "M0": g["nbr0"].shape[1], "n": n, "ef_default": ef, "path": {"auto": 0, "walk": 1, "exact": 2}[forced],
            "cand_cap": cand_cap, "exact_factor": factor, "seeds": seeds}


_REF = {}  # (tag, dist row, allow-set, k, ef, skip, path, C, seeds) -> one query's reference answer: computed once


def want_params(capi, tag, fields, g, dist, sets, which, params, M, kw, forced="auto", seeds=0, dist_row=None):
    """The restatement of a call: query q with allow-set sets[which[q]] and params[q], on the path the rule gives it from ITS ef, with the
    C_i of the plan.  Returns the (slots, dists, counts, D, E) arrays kw wide, the tally of last_filtered_each and the carve of
    last_filtered_each_params."""
    nq, n, ef_default = len(which), fields["n"], fields["ef_default"]
    counts_in = [-1 if sets[w] is None else int(sets[w].sum()) for w in which]
    per, launch, why = capi.plan_filtered_params(fields, counts_in, params)
    assert why is None, why
    slots = np.full((nq, kw), ref.EMPTY, dtype=np.uint32)
    dists = np.full((nq, kw), np.inf, dtype=np.float32)
    counts, D, E = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint64), np.zeros(nq, dtype=np.uint64)
    tally = {"walk": 0, "exact": 0, "unfiltered": 0, "empty": 0}
    carve = {"largest_expansion": 0, "largest_cand_cap": 0, "largest_exact_keys": 0, "k_zero": 0}
    for q in range(nq):
        k, ef, skip = params[q]
        allowed = sets[which[q]]
        carve["k_zero"] += k == 0
        if k == 0 or (allowed is not None and not allowed.any()):
            tally["empty"] += 1
            assert per[q]["path"] == 0
            continue
        ef_sel = ef or ef_default
        if allowed is None:
            path = "walk"
            tally["unfiltered"] += 1
        else:
            path = "exact" if rule_exact(int(allowed.sum()), n, ef_sel, forced, fields["exact_factor"]) else "walk"
        tally[path] += 1
        assert per[q]["path"] == (1 if path == "walk" else 2), (q, per[q], path)
        C = per[q]["cand_cap"]
        if path == "walk":
            assert per[q]["expansion"] == max(ef_sel, k + skip)
            carve["largest_expansion"] = max(carve["largest_expansion"], per[q]["expansion"])
            carve["largest_cand_cap"] = max(carve["largest_cand_cap"], C)
        else:
            carve["largest_exact_keys"] = max(carve["largest_exact_keys"], k + skip)
        row = q if dist_row is None else dist_row[q]
        key = (tag, row, which[q], k, ef_sel, skip, path, C, seeds if allowed is not None else 0)
        if key not in _REF:
            a = np.ones(n, dtype=bool) if allowed is None else allowed
            if path == "walk" and seeds and allowed is not None:
                _REF[key] = sref.search(g, dist[row:row + 1], a, M, k, ef_sel, seeds, skip=skip, cand_cap=C)
            else:
                _REF[key] = ref.search(g, dist[row:row + 1], a, M, k, ef_sel, skip=skip, cand_cap=C, path=path)
        s, d, c, D1, E1 = _REF[key]
        slots[q, :k], dists[q, :k], counts[q], D[q], E[q] = s[0], d[0], c[0], D1[0], E1[0]
    return (slots, dists, counts, D, E), tally, carve


def regime_is(gpu, tally, carve, distinct):
    got = gpu.last_filtered_each()
    for name in ("walk", "exact", "unfiltered", "empty"):
        assert got[name] == tally[name], (name, tally, got)
    assert got["distinct_filters"] == distinct, got
    assert gpu.last_filtered_each_params() == carve
    return got


def launches_are(gpu, before, tally):
    """one launch per non-empty group; the queries without a path ride in the exact launch if there is one, else in the walk launch"""
    want = (1 if tally["walk"] else 0, 1 if tally["exact"] else 0)
    assert launches(gpu, before) == want
    assert gpu.last_filtered_each()["launches"] == sum(want)


def tails_are_empty(got, params):
    s, d, c, lab = got[0], got[1], got[2], got[5]
    for q, (k, _, _) in enumerate(params):
        assert c[q] <= k
        assert np.all(s[q, c[q]:] == ref.EMPTY) and np.all(np.isinf(d[q, c[q]:])) and np.all(lab[q, c[q]:] == 0), q


# ------------------------------------------------------------------------------------------------
# 1. mixed batch: seven allow-sets x eight parameter rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,n,d,M,efc,ef,k", [CASES[0], CASES[1], CASES[4]], ids=["l2sq", "cos", "hamming"])
def test_mixed_batch_matches_restatement_per_query(capi, oracle, metric, n, d, M, efc, ef, k):
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    dist = ref.distance_matrix(oracle, base, queries, metric, oracle.SUM_WAVE64, regimes.THREADS)
    sets, rows = mixed_sets(n), rows_for(n)
    which = [q % len(sets) for q in range(NQ)]  # (7 and 8 are coprime: 56 of the 64 queries are the 56 combinations)
    params = [rows[q % len(rows)] for q in range(NQ)]
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    filters = [filt[w] for w in which]
    kmax = max(r[0] for r in rows)
    try:
        for forced in ("auto", "walk", "exact"):
            gpu.set_filter_policy(forced)
            fields = plan_fields(gpu, g, n, ef, forced)
            for kw in (kmax, kmax + 7):
                want, tally, carve = want_params(capi, metric, fields, g, dist, sets, which, params, M, kw, forced)
                dev = ParamsDev(gpu, queries, kw)
                before = gpu.filter_stats()
                got = dev.each_params(filters, params)
                check(got, want, g["labels"])
                tails_are_empty(got, params)
                regime_is(gpu, tally, carve, distinct=len(sets) - 1)
                launches_are(gpu, before, tally)
                assert tally["walk"] > 0 and tally["empty"] >= NQ // 8 and carve["k_zero"] == NQ // 8
                assert carve["largest_expansion"] == n + 10  # the skip of the whole index
                if forced == "auto":
                    assert tally["exact"] > 0 and tally["walk"] > tally["unfiltered"]
                    assert carve["largest_exact_keys"] == n + 10
                for q in range(NQ):  # every answer lies in its own query's set
                    a = sets[which[q]]
                    if a is not None:
                        assert a[got[0][q, : got[2][q]]].all(), q
            # the second check (got: this policy, the wider rows): each query as the single-filter uniform call answers it
            for r, (k_i, ef_i, skip_i) in enumerate(rows):
                if k_i == 0:
                    continue
                one = EachDev(gpu, queries, k_i)
                for w, f in enumerate(filt):
                    qs = [q for q in range(NQ) if which[q] == w and q % len(rows) == r]
                    uniform = one.each([None] * NQ, ef=ef_i, skip=skip_i) if f is None else one.filtered(f, ef=ef_i, skip=skip_i)
                    same(tuple(a[qs] for a in uniform), tuple(a[qs][:, :k_i] if a.ndim == 2 else a[qs] for a in got))
    finally:
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 2. many queries per workgroup: nothing of one query's parameters survives a ticket
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", ["walk", "exact"])
def test_two_workgroups_alternating_disjoint_filters_and_parameters(capi, oracle, forced):
    n, d, M, ef, nq = 3000, 64, 16, 64, 320
    rng = np.random.default_rng(5)
    base = rng.standard_normal((n, d), dtype=np.float32)
    q48 = rng.standard_normal((48, d), dtype=np.float32)
    queries = np.tile(q48, (7, 1))[:nq]
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=64, ef=ef, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    gpu = capi.GpuIndex("l2sq", d, M=M, ef_construction=64, ef=ef, seed=9)
    gpu.import_graph(base, g)
    dist = ref.distance_matrix(oracle, base, q48, "l2sq", oracle.SUM_WAVE64, regimes.THREADS)
    even = np.arange(n) % 2 == 0
    sets = [even, ~even]
    which = [q % 2 for q in range(nq)]
    rows = [(1, 4, 0), (20, 300, 100), (10, 40, 0)]  # k, expansion and skip an order of magnitude apart from one ticket to the next
    params = [rows[q % 3] for q in range(nq)]
    filt = [gpu.filter_from_bitmap(a) for a in sets]
    filters = [filt[w] for w in which]
    fields = plan_fields(gpu, g, n, ef, forced)
    want, tally, carve = want_params(capi, "two-wg", fields, g, dist, sets, which, params, M, 20, forced, dist_row=[q % 48 for q in range(nq)])
    dev = ParamsDev(gpu, queries, 20)
    try:
        gpu.set_filter_policy(forced)
        gpu.set_search_shape(0, max_workgroups=2)
        before = gpu.filter_stats()
        got = dev.each_params(filters, params)
        assert launches(gpu, before) == ((1, 0) if forced == "walk" else (0, 1))
        regime_is(gpu, tally, carve, distinct=2)
        assert carve["largest_expansion" if forced == "walk" else "largest_exact_keys"] == (300 if forced == "walk" else 120)
        s, c = got[0], got[2]
        assert np.array_equal(c, [p[0] for p in params])
        for q in range(nq):  # every returned slot lies in its own query's set
            assert np.all(s[q, : c[q]] % 2 == which[q]), (q, s[q])
        check(got, want, g["labels"])
        tails_are_empty(got, params)
    finally:
        gpu.set_search_shape(0, 0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 3. one filter on both sides of the path rule, by ef_i alone
# ------------------------------------------------------------------------------------------------
def test_one_filter_two_paths_by_ef(capi, oracle):
    metric, n, d, M, efc, ef, k = CASES[0]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    dist = ref.distance_matrix(oracle, base, queries, metric, oracle.SUM_WAVE64, regimes.THREADS)
    allowed = np.zeros(n, dtype=bool)
    allowed[np.random.default_rng(2).permutation(n)[:1000]] = True
    threshold = 1000 * 1000 / (FACTOR * n)  # exact iff ef >= threshold
    assert 32 < threshold <= 64
    f = gpu.filter_from_bitmap(allowed)
    params = [(10, 32, 0) if q % 2 else (10, 64, 0) for q in range(NQ)]
    fields = plan_fields(gpu, g, n, ef)
    want, tally, carve = want_params(capi, "two-paths", fields, g, dist, [allowed], [0] * NQ, params, M, 10)
    assert tally == {"walk": NQ // 2, "exact": NQ // 2, "unfiltered": 0, "empty": 0}
    dev = ParamsDev(gpu, queries, 10)
    before = gpu.filter_stats()
    got = dev.each_params([f] * NQ, params)
    assert launches(gpu, before) == (1, 1)
    regime_is(gpu, tally, carve, distinct=1)
    check(got, want, g["labels"])
    D = got[3]
    assert np.all(D[0::2] == 1000) and np.all(got[4][0::2] == 0) and np.all(got[4][1::2] > 0)  # the exact pass: D = allowed, E = 0
    one = Dev(gpu, queries, 10)
    for e in (32, 64):
        qs = [q for q in range(NQ) if params[q][1] == e]
        same(tuple(a[qs] for a in one.filtered(f, ef=e)), tuple(a[qs] for a in got))


# ------------------------------------------------------------------------------------------------
# 4. short answers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", ["walk", "exact"])
def test_short_answers(capi, oracle, forced):
    metric, n, d, M, efc, ef, k = CASES[2]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    dist = ref.distance_matrix(oracle, base, queries, metric, oracle.SUM_WAVE64, regimes.THREADS)
    seven = np.zeros(n, dtype=bool)
    seven[np.random.default_rng(4).permutation(n)[:7]] = True
    sets = [seven, np.random.default_rng(5).random(n) < 0.2]
    # k + skip above the allowed count; skip at it and above it; a list far longer than the allowed rows beside k = 1 in one launch
    rows = [(10, 64, 0), (5, 64, 7), (5, 64, 9), (4, 64, 5), (300, 64, 0), (1, 1, 0)]
    which = [0 if q % 3 else 1 for q in range(NQ)]
    params = [rows[q % len(rows)] for q in range(NQ)]
    filt = [gpu.filter_from_bitmap(a) for a in sets]
    fields = plan_fields(gpu, g, n, ef, forced)
    want, tally, carve = want_params(capi, "short", fields, g, dist, sets, which, params, M, 300, forced)
    dev = ParamsDev(gpu, queries, 300)
    try:
        gpu.set_filter_policy(forced)
        before = gpu.filter_stats()
        got = dev.each_params([filt[w] for w in which], params)
        assert launches(gpu, before) == ((1, 0) if forced == "walk" else (0, 1))
        regime_is(gpu, tally, carve, distinct=2)
        check(got, want, g["labels"])
        tails_are_empty(got, params)
        c = got[2]
        if forced == "exact":  # every allowed row is found: the counts are what is left of the seven behind the skip
            for q in range(NQ):
                if which[q] == 0:
                    k_i, _, skip_i = params[q]
                    assert c[q] == min(k_i, max(0, 7 - skip_i)), q
            assert carve["largest_exact_keys"] == 300
    finally:
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 5. an explicit candidate cap below some expansions of the batch and above others
# ------------------------------------------------------------------------------------------------
def test_explicit_cand_cap_between_the_expansions(capi, oracle):
    metric, n, d, M, efc, ef, k = CASES[0]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    dist = ref.distance_matrix(oracle, base, queries, metric, oracle.SUM_WAVE64, regimes.THREADS)
    sets = [np.random.default_rng(6).random(n) < 0.1, None]
    rows = [(10, 64, 0), (10, 300, 0), (5, 20, 0), (10, 64, 90)]  # C = 100, 300, 100, 100
    which = [q % 2 for q in range(NQ)]
    params = [rows[(q // 2) % len(rows)] for q in range(NQ)]
    filt = [gpu.filter_from_bitmap(sets[0]), None]
    fields = plan_fields(gpu, g, n, ef, "walk", cand_cap=100)
    want, tally, carve = want_params(capi, "cap", fields, g, dist, sets, which, params, M, 10, "walk")
    assert carve["largest_cand_cap"] == 300 and carve["largest_expansion"] == 300
    uncapped, _, _ = want_params(capi, "cap", plan_fields(gpu, g, n, ef, "walk"), g, dist, sets, which, params, M, 10, "walk")
    assert not np.array_equal(want[3], uncapped[3])  # the cap drops candidates: the walks differ
    dev = ParamsDev(gpu, queries, 10)
    try:
        gpu.set_filter_policy("walk", cand_cap=100)
        got = dev.each_params([filt[w] for w in which], params)
        regime_is(gpu, tally, carve, distinct=1)
        check(got, want, g["labels"])
    finally:
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 6. the seeded walk with mixed parameters
# ------------------------------------------------------------------------------------------------
def test_seeded_walk_with_mixed_parameters(capi, oracle):
    metric, n, d, M, efc, ef, k = CASES[0]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    dist = ref.distance_matrix(oracle, base, queries, metric, oracle.SUM_WAVE64, regimes.THREADS)
    span = np.zeros(n, dtype=bool)
    span[1200:1500] = True
    sets = [span, np.random.default_rng(7).random(n) < 0.3, None, np.zeros(n, dtype=bool)]
    rows = [(1, 1, 0), (10, 64, 0), (10, 64, 10), (5, 65, 0), (10, 0, 0), (100, 64, 0), (0, 64, 0)]
    which = [q % len(sets) for q in range(NQ)]
    params = [rows[q % len(rows)] for q in range(NQ)]
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    fields = plan_fields(gpu, g, n, ef, "walk", seeds=8)
    want, tally, carve = want_params(capi, "seeded", fields, g, dist, sets, which, params, M, 100, "walk", seeds=8)
    plain, _, _ = want_params(capi, "seeded", plan_fields(gpu, g, n, ef, "walk"), g, dist, sets, which, params, M, 100, "walk")
    assert not np.array_equal(want[3], plain[3])  # the seeds change D
    dev = ParamsDev(gpu, queries, 100)
    try:
        gpu.set_filter_policy("walk")
        gpu.set_filter_seeds(8)
        got = dev.each_params([filt[w] for w in which], params)
        regime_is(gpu, tally, carve, distinct=3)
        seeded = tally["walk"] - tally["unfiltered"]
        assert gpu.last_filtered_seeds() == {"seeds": 8, "single_seeds": 0, "seeded": seeded, "unseeded": tally["unfiltered"]}
        check(got, want, g["labels"])
    finally:
        gpu.set_filter_seeds(0)
        gpu.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 7. row kinds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,metric,d", [("f16", "l2sq", 200), ("i8", "cos", 768), ("b1", "l2sq", 96)])
def test_mixed_batch_on_quantised_storage(capi, oracle, storage, metric, d):
    n, nq, ef, M = 1500, 32, 64, 16
    gpu, g, dist, queries = instance(capi, oracle, storage, metric, d, M, None, n, nq, ef)
    sets = mixed_sets(n)
    rows = [(1, 1, 0), (10, 64, 10), (5, 65, 0), (40, 0, 0), (0, 64, 0)]
    which = [q % len(sets) for q in range(nq)]
    params = [rows[q % len(rows)] for q in range(nq)]
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    fields = plan_fields(gpu, g, n, ef)
    want, tally, carve = want_params(capi, (storage, metric), fields, g, dist, sets, which, params, M, 40)
    assert tally["walk"] > tally["unfiltered"] and tally["exact"] > 0
    dev = ParamsDev(gpu, queries, 40)
    before = gpu.filter_stats()
    got = dev.each_params([filt[w] for w in which], params)
    launches_are(gpu, before, tally)
    regime_is(gpu, tally, carve, distinct=len(sets) - 1)
    check(got, want, g["labels"])


# ------------------------------------------------------------------------------------------------
# 8. the three forms; two lanes at once
# ------------------------------------------------------------------------------------------------
def test_host_lane_and_device_forms_give_the_same_rows(capi, oracle):
    metric, n, d, M, efc, ef, k = CASES[2]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    sets, rows = mixed_sets(n), rows_for(n)
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    arrays = [[filt[q % len(sets)] for q in range(NQ)], [filt[(3 * q + 1) % len(sets)] for q in range(NQ)]]
    params = [[rows[q % len(rows)] for q in range(NQ)], [rows[(5 * q + 2) % len(rows)] for q in range(NQ)]]
    qs = [queries, queries[::-1].copy()]
    alone = []
    for i in (0, 1):
        s, dd, c, D, E, lab = ParamsDev(gpu, qs[i], 300).each_params(arrays[i], params[i])
        host = gpu.search_batch_filtered_each_params(arrays[i], qs[i], params[i])
        lane = gpu.search_batch_filtered_each_params_lane(3, arrays[i], qs[i], params[i], k_stride=300)
        for lab2, d2, c2 in (host, lane):
            assert lab2.shape == (NQ, 300)
            assert np.array_equal(lab2, lab) and np.array_equal(d2.view(np.uint32), dd.view(np.uint32)) and np.array_equal(c2, c)
        alone.append(host)
    assert not all(np.array_equal(a, b) for a, b in zip(alone[0], alone[1]))
    rounds, barrier, out, errors = 6, threading.Barrier(2), [[], []], []

    def run(lane):
        try:
            for _ in range(rounds):
                barrier.wait()
                out[lane].append(gpu.search_batch_filtered_each_params_lane(lane, arrays[lane], qs[lane], params[lane]))
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


# ------------------------------------------------------------------------------------------------
# 9. degenerate inputs
# ------------------------------------------------------------------------------------------------
def test_an_empty_index_and_a_batch_without_answers_make_no_launch(capi, oracle):
    empty = capi.GpuIndex("l2sq", 16, M=8, ef_construction=32, ef=32, seed=1)
    q = np.random.default_rng(1).standard_normal((5, 16), dtype=np.float32)
    lab, dist, cnt = empty.search_batch_filtered_each_params([None] * 5, q, [(3, 0, 0), (0, 0, 0), (7, 9, 2), (1, 1, 0), (7, 0, 0)])
    assert lab.shape == (5, 7) and np.all(lab == 0) and np.all(np.isinf(dist)) and np.all(cnt == 0)
    assert empty.filter_stats() == {"walk": 0, "exact": 0}
    assert empty.last_filtered_each() == {"walk": 0, "exact": 0, "unfiltered": 0, "empty": 5, "distinct_filters": 0, "launches": 0}

    metric, n, d, M, efc, ef, k = CASES[2]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    some = gpu.filter_from_bitmap(np.arange(n) % 3 == 0)
    none = gpu.filter_from_bitmap(np.zeros(n, dtype=bool))
    filters = [some if i % 2 else None for i in range(NQ)]
    dev = ParamsDev(gpu, queries, 4)
    marker = np.full(NQ * 4, 0xABABABAB, dtype=np.uint32)
    for params, fl in (([(0, 64, 0)] * NQ, filters), ([(0, 0, 5)] * NQ, [none] * NQ), ([(3, 64, 0)] * NQ, [none] * NQ)):
        for buf in (dev.slot, dev.dist):
            buf.upload(marker)
        dev.cnt.upload(marker[:NQ])
        before = gpu.filter_stats()
        s, dd, c, D, E, lab = dev.each_params(fl, params)
        assert gpu.filter_stats() == before  # no launch
        k0 = NQ if params[0][0] == 0 else 0
        assert gpu.last_filtered_each_params() == {"largest_expansion": 0, "largest_cand_cap": 0, "largest_exact_keys": 0, "k_zero": k0}
        assert gpu.last_filtered_each()["empty"] == NQ and gpu.last_filtered_each()["launches"] == 0
        assert np.all(s == ref.EMPTY) and np.all(np.isinf(dd)) and np.all(lab == 0) and np.all(c == 0) and np.all(D == 0) and np.all(E == 0)
    # rows of width zero: the counts are still written
    lab, dist, cnt = gpu.search_batch_filtered_each_params(filters, queries, [(0, 64, 0)] * NQ)
    assert lab.shape == (NQ, 0) and np.all(cnt == 0)
    cnt = np.full(NQ, 9, dtype=np.uint32)
    P = capi.query_params([(0, 64, 0)] * NQ)
    F = gpu._filter_array(filters, NQ)
    Q = np.ascontiguousarray(queries, dtype=np.float32)
    capi._call("lantern_gpu_search_batch_filtered_each_params_lane", gpu.h, 2, capi._ptr(F), capi._ptr(Q), NQ, capi.SCALAR_F32, capi._ptr(P), 0, None, None,
               capi._ptr(cnt))
    assert np.all(cnt == 0)
    # one query with an answer among them: one launch, the others ride in it and touch no row
    params = [(0, 64, 0)] * NQ
    params[17] = (4, 64, 0)
    before = gpu.filter_stats()
    got = dev.each_params(filters, params)
    assert launches(gpu, before) == (0, 1) and gpu.last_filtered_each()["empty"] == NQ - 1
    assert got[2][17] == 4 and got[2].sum() == 4 and got[3].sum() == got[3][17] == (np.arange(n) % 3 == 0).sum()


# ------------------------------------------------------------------------------------------------
# 10. refusals: for the whole call, in the documented order, nothing queued or written
# ------------------------------------------------------------------------------------------------
def test_refusals_in_the_documented_order_touch_nothing(capi, oracle):
    import ctypes as C

    metric, n, d, M, efc, ef, k = CASES[2]
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    other = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=ef, seed=9)
    other.import_graph(base, g)
    good = gpu.filter_from_bitmap(np.arange(n) % 3 == 0)
    foreign = other.filter_from_bitmap(np.ones(n, dtype=bool))
    junk = C.create_string_buffer(4096)
    kw = 10
    dev = ParamsDev(gpu, queries, kw)
    marker = np.full(NQ * kw, 0xABABABAB, dtype=np.uint32)
    valid = [good if q % 2 else None for q in range(NQ)]
    fine = [(10, 64, 0)] * NQ
    dev.each_params(valid, fine)

    def refused(filters, params, pattern, k_stride=kw):
        for buf in (dev.slot, dev.dist):
            buf.upload(marker)
        dev.cnt.upload(marker[:NQ])
        before, shape, carve = gpu.filter_stats(), gpu.last_filtered_each(), gpu.last_filtered_each_params()
        with pytest.raises(capi.LanternGpuError, match=pattern):
            gpu.search_batch_filtered_each_params_device(filters, dev.dq.ptr, dev.rows.strides[0], NQ, params, k_stride, dev.lab.ptr, dev.dist.ptr,
                                                         dev.slot.ptr, dev.cnt.ptr, dev.D.ptr, dev.E.ptr)
        dev.hip.synchronize()
        assert gpu.filter_stats() == before and gpu.last_filtered_each() == shape and gpu.last_filtered_each_params() == carve
        assert np.array_equal(dev.slot.download(NQ * kw, np.uint32), marker) and np.array_equal(dev.dist.download(NQ * kw, np.uint32), marker)
        assert np.array_equal(dev.cnt.download(NQ, np.uint32), marker[:NQ])
        for call in (lambda: gpu.search_batch_filtered_each_params(filters, queries, params, k_stride=k_stride),
                     lambda: gpu.search_batch_filtered_each_params_lane(0, filters, queries, params, k_stride=k_stride)):
            with pytest.raises(capi.LanternGpuError, match=pattern):
                call()
        assert gpu.filter_stats() == before

    def with_row(i, row, base_rows=fine):
        return base_rows[:i] + [row] + base_rows[i + 1:]

    bad_filters = valid[:17] + [foreign] + valid[18:]
    reserved = capi.query_params(fine)
    reserved["reserved"][9] = 1
    huge = with_row(40, (10, 10**5, 0))  # an expansion beyond the LDS budget
    # 2. the parameter array, before the filters (3) and the shapes (5)
    refused(bad_filters, reserved, r"reserved parameter word must be 0 \(params\[9\]\)")
    refused(bad_filters, with_row(12, (11, 64, 0), huge), r"k_stride is smaller than a query's k \(params\[12\]\)")
    # 3. the filters, before the shapes
    refused(bad_filters, huge, r"another index .*\(filters\[17\]\)")
    refused(valid[:30] + [C.addressof(junk)] + valid[31:], fine, r"not a filter handle .*\(filters\[30\]\)")
    # 5. a query's own shape, the first in batch order, whichever path it takes
    refused(valid, huge, r"ef/k exceed the 160 KiB LDS budget of the filtered search kernel \(params\[40\]\)")
    refused(valid, with_row(3, (10, 64, 10**5), huge), r"k \+ skip exceed the 160 KiB LDS budget of the exact filtered search kernel \(params\[3\]\)")
    # ... but not of a query that has no path: an empty filter, as the single-filter call
    none = gpu.filter_from_bitmap(np.zeros(n, dtype=bool))
    got = dev.each_params(valid[:40] + [none] + valid[41:], huge)
    assert got[2][40] == 0 and got[2][39] == 10
    # 6. the joint carve: two long scans that fit one by one
    refused([None] * NQ, with_row(5, (10, 3300, 0), with_row(50, (10, 3010, 0))), r"do not fit together: split the batch$")
    dev.each_params([None] * NQ, with_row(5, (10, 3300, 0)))
    assert gpu.last_filtered_each_params()["largest_expansion"] == 3300
    # 4. a compact pq index is refused as by the single-filter call, behind its filters
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
    four = [(10, 0, 0), (3, 20, 1), (0, 0, 0), (10, 64, 5)]
    _, _, cnt = pq.search_batch_filtered_each_params([pf, None, pf, None], pbase[:4], four)  # expanded: served
    assert cnt.tolist() == [10, 3, 0, 10]
    pq.pq_compact()
    with pytest.raises(capi.LanternGpuError, match="expand it first"):
        pq.search_batch_filtered_each_params([pf, None, pf, None], pbase[:4], with_row(1, (3, 10**5, 0), four))
    with pytest.raises(capi.LanternGpuError, match=r"another index .*\(filters\[2\]\)"):
        pq.search_batch_filtered_each_params([pf, None, good, None], pbase[:4], four)
