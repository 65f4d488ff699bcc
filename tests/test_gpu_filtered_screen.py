"""The screened exact pass of a filtered call on the device (lantern_gpu_set_filter_screen; include/lantern_gpu.h "THE SCREENED EXACT
PASS", DESIGN.md 4.9 "Screened exact pass").  Needs an MI355X.

The referee of every slot is the float64 brute force over the allowed rows, on cases whose float64 gaps around every rank of the answer
exceed the f32 error bound of tests/exact_knn_bound.py (asserted here, so the reference alone pins the slots); the same call with the
switch at 0 -- today's k_search_exact_allowed -- must give the same slots, distance bits, counts, D and E.  The graph plays no part on
the exact path: the rows are imported under an empty graph, as tests/test_gpu_filtered_dense.py does.
"""
import numpy as np
import pytest

from lantern_amd import synth
from tests import exact_knn_bound as bound
from tests.test_gpu_filtered_dense import capi, index_of  # noqa: F401 (capi: the module's fixture)
from tests.test_gpu_filtered_each import EachDev
from tests.test_gpu_filtered_each_params import ParamsDev
from tests.test_gpu_filtered_search import same

pytestmark = pytest.mark.gpu

F32, EMPTY = np.float32, 0xFFFFFFFF
N, NQ, KW = 3000, 2, 10
F32_ROUND = 2 * 512 // 64  # rows of the screened kernel's f32 round
PAIRS = [(10, 0), (5, 7)]  # (k, skip)
NOTHING = {"launches": 0, "bounded": 0, "rejected": 0, "f32_rows": 0}
# The seed of every allow-set, by d, in the order of (pair, count): the first for which every float64 gap of both metrics and every
# query clears the f32 error bound (searched on the CPU; brute() asserts it again whenever a case is built).
SEEDS = {509: [0, 0, 1, 0, 0, 3, 0, 0, 0, 0, 1, 0, 1, 0, 0, 2, 0, 0], 768: [0, 2, 0, 0, 0, 0, 0, 5, 0, 2, 0, 2, 1, 0, 1, 0, 0, 0],
         2000: [1, 3, 5, 2, 5, 30, 24, 6, 6, 0, 2, 1, 2, 11, 21, 50, 5, 5]}


def counts_for(k, skip):
    """around the fill, around a screen round of 64, around an f32 round, and many rounds"""
    return sorted({k + skip - 1, k + skip, k + skip + 1, 63, 64, 65, F32_ROUND - 1, F32_ROUND + 1, 1000})


def fill_rows(count, kk):  # the rows of the filling: whole f32 rounds until the list is full
    return min(count, -(-kk // F32_ROUND) * F32_ROUND)


def distances64(metric, rows, q):
    """float64 distances of one query to rows, with the zero-norm rules of the cosine metric (both zero: 0, one zero: 1)"""
    r, q = rows.astype(np.float64), q.astype(np.float64)
    if metric == "l2sq":
        return ((r - q) ** 2).sum(1)
    rn, qn = np.sqrt((r * r).sum(1)), np.sqrt((q * q).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        d = 1.0 - (r * q).sum(1) / (rn * qn)  # (row by row: a matrix product's sums depend on where a row lies, and equal rows must tie)
    return np.where((rn == 0) & (qn == 0), 0.0, np.where((rn == 0) | (qn == 0), 1.0, d))


def brute(metric, rows, q, allowed, k, skip, gaps=True):
    """slots [skip, skip + k) of the allowed rows by (float64 distance, slot), EMPTY behind them, and the count.  gaps: every pair of
    neighbouring ranks from skip - 1 | skip to k + skip - 1 | k + skip lies further apart than the f32 error of both distances"""
    ids = np.flatnonzero(allowed)
    d = distances64(metric, rows[ids], q)
    order = np.lexsort((ids, d))
    if gaps:
        dims = bound.padded_dims(rows.shape[1])
        qn, rn = np.sqrt((q.astype(np.float64) ** 2).sum()), np.sqrt((rows[ids].astype(np.float64) ** 2).sum(1))
        err = bound.mfma_error_l2(qn, rn, dims) if metric == "l2sq" else np.full(ids.size, bound.mfma_error_cos(dims))
        for i in range(max(skip - 1, 0), min(k + skip, ids.size - 1)):
            a, b = order[i], order[i + 1]
            assert d[b] - d[a] > err[a] + err[b], ("float64 gap inside the f32 error", i, d[a], d[b])
    got = ids[order[skip:skip + k]]
    out = np.full(k, EMPTY, dtype=np.uint32)
    out[:got.size] = got
    return out, got.size


_CASE = {}  # (metric, d) -> rows, queries, {(k, skip, count): allowed}, {(k, skip, count): ([NQ][k] slots, [NQ] counts)}: built once


def case(metric, d):
    if (metric, d) not in _CASE:
        rows = synth.base_rows("clustered", N, d, seed=5)
        queries = synth.query_maker("clustered", d)(np.random.default_rng(d), NQ)
        sets, want, seeds = {}, {}, iter(SEEDS[d])
        for k, skip in PAIRS:
            for count in counts_for(k, skip):
                allowed = np.zeros(N, dtype=bool)
                allowed[np.random.default_rng([d, skip, count, next(seeds)]).choice(N, size=count, replace=False)] = True
                sets[k, skip, count] = allowed
                per = [brute(metric, rows, q, allowed, k, skip) for q in queries]
                want[k, skip, count] = np.stack([p[0] for p in per]), np.array([p[1] for p in per], dtype=np.uint32)
        _CASE[metric, d] = rows, queries, sets, want
    return _CASE[metric, d]


def on_and_off(ix, call):
    """call() with the switch at 1, then at 0: both answers bit for bit equal; returns the answer and the screened call's diagnostics"""
    ix.set_filter_screen(1)
    got, diag = call(), ix.last_filtered_screen()
    ix.set_filter_screen(0)
    off = call()
    assert ix.last_filtered_screen() == NOTHING
    same(got, off)
    return got, diag


@pytest.mark.parametrize("form", ["single", "each", "each_params"])
@pytest.mark.parametrize("d", [509, 768, 2000])  # the narrowest screened row, the headline, the widest with a partial last block
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_parity(capi, metric, d, form):
    rows, queries, sets, want = case(metric, d)
    ix = index_of(capi, None, metric, "f32", rows)
    filters = {key: ix.filter_from_bitmap(a) for key, a in sets.items()}
    # the keys of one call: one filter; every count of a (k, skip), a filter per query; both (k, skip) and every count, rows KW wide
    calls = {"single": [[key] for key in sets], "each": [[key for key in sets if key[:2] == p] for p in PAIRS], "each_params": [list(sets)]}[form]
    for keys in calls:
        per_query = [filters[key] for key in keys for _ in range(NQ)]
        tiled, (k, skip) = np.tile(queries, (len(keys), 1)), keys[0][:2]
        if form == "each_params":
            dev = ParamsDev(ix, tiled, KW)
            got, diag = on_and_off(ix, lambda: dev.each_params(per_query, [(key[0], 0, key[1]) for key in keys for _ in range(NQ)]))
        else:
            dev = EachDev(ix, tiled, k)
            got, diag = on_and_off(ix, (lambda: dev.each(per_query, skip=skip)) if form == "each" else (lambda: dev.filtered(per_query[0], skip=skip)))
        for i, key in enumerate(keys):
            at = slice(i * NQ, (i + 1) * NQ)
            assert np.array_equal(got[0][at, :key[0]], want[key][0]) and np.all(got[0][at, key[0]:] == EMPTY), key
            assert np.array_equal(got[2][at], want[key][1]) and np.all(got[3][at] == key[2]), key
        assert not got[4].any() and diag["launches"] == 1
    ix.close()


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_diagnostics(capi, metric):
    rows, queries, sets, want = case(metric, 768)
    ix = index_of(capi, None, metric, "f32", rows)
    k, skip = PAIRS[0]
    dev, fill = EachDev(ix, queries, k), fill_rows(1000, k + skip)
    f = ix.filter_from_bitmap(sets[k, skip, 1000])
    got, diag = on_and_off(ix, lambda: dev.filtered(f, skip=skip))
    assert np.array_equal(got[0], want[k, skip, 1000][0])
    assert diag["launches"] == 1 and diag["rejected"] > 0 and diag["bounded"] == NQ * (1000 - fill), diag
    assert diag["bounded"] == diag["rejected"] + diag["f32_rows"] - NQ * fill, diag
    f = ix.filter_from_bitmap(sets[k, skip, k + skip - 1])  # the list never fills: nothing is bounded
    got, diag = on_and_off(ix, lambda: dev.filtered(f, skip=skip))
    assert diag == {"launches": 1, "bounded": 0, "rejected": 0, "f32_rows": NQ * (k + skip - 1)}
    ix.close()
    h = index_of(capi, None, metric, "f16", rows)  # an f16 index: today's kernel whatever the switch says
    dev, f = EachDev(h, queries, k), h.filter_from_bitmap(sets[k, skip, 1000])
    h.set_filter_screen(1)
    got = dev.filtered(f)
    assert h.filter_screen() == 1 and h.last_filtered_screen() == NOTHING
    h.set_filter_screen(0)
    same(got, dev.filtered(f))
    h.close()


def edge(capi, metric, rows, queries, allowed, k=10, skip=0):
    """a single-filter call on rows / allowed: == float64 and == the switch-off call; returns the slots and the diagnostics"""
    ix = index_of(capi, None, metric, "f32", rows)
    dev, f = EachDev(ix, queries, k), ix.filter_from_bitmap(allowed)
    got, diag = on_and_off(ix, lambda: dev.filtered(f, skip=skip))
    for i, q in enumerate(queries):
        assert np.array_equal(got[0][i], brute(metric, rows, q, allowed, k, skip, gaps=False)[0]), i
    ix.close()
    return got[0], diag


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_edges(capi, metric):
    rows, queries, sets, want = case(metric, 768)
    k, skip = PAIRS[0]
    # the row at rank k + skip duplicated at a lower and at a higher slot: the three keys differ by their slots only, the lowest enters
    tied, allowed = rows.copy(), sets[k, skip, 1000].copy()
    last, free = int(want[k, skip, 1000][0][0, k - 1]), np.flatnonzero(~allowed)
    lo, hi = int(free[free < last][0]), int(free[free > last][-1])
    tied[lo], tied[hi] = rows[last], rows[last]
    allowed[[lo, hi]] = True
    slots, diag = edge(capi, metric, tied, queries[:1], allowed, k, skip)
    assert slots[0, k - 1] == lo and last not in slots[0] and hi not in slots[0] and diag["rejected"] > 0
    # all-zero rows and a row scaled by 1e30 among rows of scale 1: their screen meta says "not ok", the test is not made for them
    odd, allowed = rows.copy(), sets[k, skip, 1000]
    ids = np.flatnonzero(allowed)
    odd[ids[100:104]] = 0
    odd[ids[200]] *= F32(1e30)
    assert edge(capi, metric, odd, queries, allowed)[1]["rejected"] > 0
    if metric == "cos":  # a query of norm 0: every distance is 1, or 0 to a zero row -- ties by slot throughout, and nothing is rejected
        slots, diag = edge(capi, metric, odd, np.zeros((1, 768), dtype=F32), allowed)
        assert np.array_equal(slots[0, :4], ids[100:104]) and diag["rejected"] == 0 and diag["bounded"] == 1000 - fill_rows(1000, k)


def test_nulls_empties_and_k_zero_in_one_call(capi):
    rows, queries, sets, want = case("l2sq", 768)
    ix = index_of(capi, None, "l2sq", "f32", rows)
    big, none = ix.filter_from_bitmap(sets[10, 0, 1000]), ix.filter_from_bitmap(np.zeros(N, dtype=bool))
    filters = [None, none, big, big, none, big]  # (a NULL entry walks whatever the policy: the switch-off call is its referee)
    params = [(10, 0, 0), (10, 0, 0), (10, 0, 0), (0, 0, 0), (0, 0, 0), (5, 0, 7)]
    dev = ParamsDev(ix, np.tile(queries, (3, 1)), KW)
    got, diag = on_and_off(ix, lambda: dev.each_params(filters, params))
    assert diag["launches"] == 1 and diag["bounded"] == 2 * (1000 - F32_ROUND)
    assert np.array_equal(got[0][2], want[10, 0, 1000][0][0])
    assert np.array_equal(got[0][5, :5], brute("l2sq", rows, queries[1], sets[10, 0, 1000], 5, 7)[0])
    assert np.array_equal(got[2][1:], [0, 10, 0, 0, 5]) and np.array_equal(got[3][1:], [0, 1000, 0, 0, 1000])
    ix.close()
