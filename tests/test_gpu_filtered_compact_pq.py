"""Filtered search on a COMPACT pq index (lantern_gpu_set_filter_compact; include/lantern_gpu.h, DESIGN.md 4.9 "Compact pq indexes").
Needs an MI355X.

The arbiter of every answer is the CPU restatement of filtered search (tests/filtered_walk_ref.py, tests/filtered_seeded_ref.py) over the
graph the index exports and the distance matrix of the index's row routine: rows decoded on the fly -- oracle.bruteforce over the decoded
rows in the f32 kernels' order; ADC -- the oracle's own ADC distances (tests/filtered_adc_ref.py).  Slots, distance bits, counts, D and E
equal, for every query.  On the decode path the expanded twin's answers and launch shape are a second equality, never the arbiter.
"""
import numpy as np
import pytest

from tests import filtered_adc_ref as adc
from tests import filtered_regimes as regimes
from tests import filtered_seeded_ref as sref
from tests import filtered_walk_ref as ref
from tests.test_gpu_filtered_each import EachDev, mixed_sets, regime_is, want_each
from tests.test_gpu_filtered_each_params import ParamsDev
from tests.test_gpu_filtered_regimes import check
from tests.test_gpu_filtered_search import same

pytestmark = pytest.mark.gpu

REFUSAL = "filtered search does not run on a compact pq index: expand it first"
NQ, K = 16, 10
# name -> metric, n, d, num_subvectors, num_centroids, M, ef, row routine ("decode" / "adc"; True: under LANTERN_GPU_PQ_ADC=1)
SHAPES = {
    "decode_g8": ("l2sq", 1500, 96, 4, 200, 8, 64, "decode", False),       # a 16-byte code row
    "decode_g16": ("l2sq", 3000, 128, 32, 256, 8, 40, "decode", False),
    "decode_g32": ("l2sq", 1200, 320, 20, 16, 5, 33, "decode", False),
    "decode_g64": ("cos", 2000, 768, 96, 64, 16, 64, "decode", False),      # 96-byte rows at the 128-byte stride
    "adc_1": ("l2sq", 1500, 60, 6, 10, 4, 100, "adc", False),               # 1 code chunk, subvectors of 10 dimensions
    "adc_8": ("cos", 1200, 256, 128, 256, 16, 48, "adc", False),            # 8 code chunks: the 128 KiB table
    "adc_2_env": ("l2sq", 3000, 128, 32, 256, 8, 40, "adc", True),
    "adc_6_env": ("cos", 2000, 768, 96, 64, 16, 64, "adc", True),
}


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


_BUILT, _DIST = {}, {}


def built(capi, oracle, name):
    """The index of a shape, built once: `twin` keeps its decodings, `ix` is the same index loaded again, compact, the switch on."""
    metric, n, d, S, C, M, ef = SHAPES[name][:7]
    key = (metric, n, d, S, C, M, ef)
    if key not in _BUILT:
        rng = np.random.default_rng(n + d + S)
        base = rng.standard_normal((n, d), dtype=np.float32)
        queries = rng.standard_normal((2 * NQ, d), dtype=np.float32)
        cb = adc.make_codebook(rng, base, S, C)
        twin = capi.GpuIndex(metric, d, M=M, ef_construction=48, ef=ef, seed=5, pq_codebook=cb, num_subvectors=S)
        twin.set_add_batch(256, 16)
        twin.add_many(np.arange(n, dtype=np.uint64) + 1, base)
        twin.flush()
        g = twin.export_graph(with_vectors=True)
        codes = twin.export_codes()
        ix = capi.GpuIndex(metric, d, M=M, ef_construction=48, ef=ef, seed=5, pq_codebook=cb, num_subvectors=S)
        ix.load_buffer(twin.save_buffer())
        assert ix.checksum() == twin.checksum()
        ix.pq_compact()
        assert ix.memory_usage()[0] < n * d  # code bytes only
        ix.set_filter_compact(1)
        _BUILT[key] = {"metric": metric, "n": n, "d": d, "M": M, "ef": ef, "queries": queries, "cb": cb, "codes": codes, "g": g, "twin": twin, "ix": ix, "key": key}
    return _BUILT[key]


def matrix(oracle, b, routine):
    """the [2 NQ][n] reference distances of the index's row routine, computed once"""
    key = (b["key"], routine)
    if key not in _DIST:
        if routine == "adc":
            _DIST[key] = adc.distance_matrix(oracle, b["g"]["vectors"], b["cb"], b["codes"], b["queries"], b["metric"], regimes.THREADS)
        else:
            _DIST[key] = ref.distance_matrix(oracle, b["g"]["vectors"], b["queries"], b["metric"], oracle.SUM_WAVE64, regimes.THREADS)
    return _DIST[key]


@pytest.fixture
def shape(request, capi, oracle, monkeypatch):
    """a built shape with the environment of its row routine; restores the index's policy afterwards"""
    name = request.param
    routine, env = SHAPES[name][7:]
    if env:
        monkeypatch.setenv("LANTERN_GPU_PQ_ADC", "1")
    else:
        monkeypatch.delenv("LANTERN_GPU_PQ_ADC", raising=False)
    b = dict(built(capi, oracle, name))
    b["routine"] = routine
    b["dist"] = matrix(oracle, b, routine)
    assert b["ix"].filter_compact() == routine
    yield b
    for index in (b["ix"], b["twin"]):
        index.set_filter_policy("auto")
        index.set_filter_seeds(0)
        index.set_search_shape(0, 0)


def code_row_bytes(S):
    """num_subvectors padded to 16; rows of 65 .. 127 bytes sit at the 128-byte stride (so 96 subvectors build the 128 KiB table too)"""
    s16 = (S + 15) // 16 * 16
    return 128 if 64 < s16 < 128 else s16


class CompactDev(EachDev):
    """device buffers for nq rows of k answers: the single-filter, per-query and per-query-parameter device forms"""
    each_params = ParamsDev.each_params


def sweep_sets(n):
    """all rows, random 50 % / 10 % / 2 %, one row, none"""
    u = np.random.default_rng(17).random(n)
    one = np.zeros(n, dtype=bool)
    one[n // 3] = True
    return {"all": np.ones(n, dtype=bool), "half": u < 0.5, "tenth": u < 0.1, "fiftieth": u < 0.02, "one": one, "none": np.zeros(n, dtype=bool)}


def is_empty_answer(got):
    slots, dists, counts, D, E, labels = got
    assert np.all(counts == 0) and np.all(D == 0) and np.all(E == 0)
    assert np.all(slots == ref.EMPTY) and np.all(np.isinf(dists)) and np.all(labels == 0)


# ------------------------------------------------------------------------------------------------
# 1. the switch
# ------------------------------------------------------------------------------------------------
def test_the_switch_is_off_by_default_and_takes_0_or_1(capi, oracle, monkeypatch):
    monkeypatch.delenv("LANTERN_GPU_PQ_ADC", raising=False)
    b = built(capi, oracle, "decode_g8")
    ix, twin, n, q = b["ix"], b["twin"], b["n"], b["queries"]
    f = ix.filter_from_bitmap(np.arange(n) % 3 == 0)
    # a fresh index: the switch is off, and its compact form is refused with the text of old
    metric, _, d, S, _, M, ef = SHAPES["decode_g8"][:7]
    fresh = capi.GpuIndex(metric, d, M=M, ef_construction=48, ef=ef, seed=5, pq_codebook=b["cb"], num_subvectors=S)
    fresh.load_buffer(twin.save_buffer())
    assert fresh.filter_compact() is None
    ff = fresh.filter_from_bitmap(np.arange(n) % 3 == 0)
    assert np.all(fresh.search_batch_filtered(ff, q[:4], K)[2] == K)  # expanded: served
    fresh.pq_compact()
    assert fresh.filter_compact() is None
    with pytest.raises(capi.LanternGpuError, match=REFUSAL):
        fresh.search_batch_filtered(ff, q[:4], K)
    try:
        ix.set_filter_compact(0)
        assert ix.filter_compact() is None
        with pytest.raises(capi.LanternGpuError, match=REFUSAL):
            ix.search_batch_filtered(f, q[:4], K)
        with pytest.raises(capi.LanternGpuError, match=REFUSAL):
            ix.search_batch_filtered_each([f, None, f, None], q[:4], K)
        with pytest.raises(capi.LanternGpuError, match=REFUSAL):
            ix.search_batch_filtered_each_params([f, None], q[:2], [(3, 0, 0), (5, 20, 1)])
        cur = ix.cursor()
        with pytest.raises(capi.LanternGpuError, match=REFUSAL):
            cur.search_filtered(f, q[0], K)
        cur.close()
        for bad in (2, -1, 7):
            with pytest.raises(capi.LanternGpuError, match="filter_compact must be 0"):
                ix.set_filter_compact(bad)
        assert ix.filter_compact() is None  # a refused value changes nothing
        ix.set_filter_compact(1)
        assert ix.filter_compact() == "decode"
        lab, _, cnt = ix.search_batch_filtered(f, q[:4], K)
        assert np.all(cnt == K) and np.all((lab - 1) % 3 == 0)
        monkeypatch.setenv("LANTERN_GPU_PQ_ADC", "1")
        assert ix.filter_compact() == "adc"
        monkeypatch.delenv("LANTERN_GPU_PQ_ADC")
        # an index that is not compact: the setting changes nothing
        ft = twin.filter_from_bitmap(np.arange(n) % 3 == 0)
        before = twin.search_batch_filtered(ft, q[:4], K)
        twin.set_filter_compact(1)
        assert twin.filter_compact() == "stored"
        after = twin.search_batch_filtered(ft, q[:4], K)
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
    finally:
        ix.set_filter_compact(1)
        twin.set_filter_compact(0)


# ------------------------------------------------------------------------------------------------
# 2. 3. every shape, both paths, filters from all rows to none
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["walk", "exact"])
@pytest.mark.parametrize("shape", list(SHAPES), indirect=True)
def test_filters_of_every_selectivity_match_the_restatement(capi, oracle, shape, path):
    b = shape
    ix, twin, g, n, M, ef = b["ix"], b["twin"], b["g"], b["n"], b["M"], b["ef"]
    queries, dist = b["queries"][:NQ], b["dist"][:NQ]
    ix.set_filter_policy(path)
    twin.set_filter_policy(path)
    dev, tdev = CompactDev(ix, queries, K), CompactDev(twin, queries, K)
    code_chunks = code_row_bytes(b["codes"].shape[1]) // 16
    for name, allowed in sweep_sets(n).items():
        f = ix.filter_from_bitmap(allowed)
        got = dev.filtered(f)
        if name == "none":
            is_empty_answer(got)
            assert ix.last_filtered_launch()["path"] is None
            continue
        want = ref.search(g, dist, allowed, M, K, ef, path=path)
        check(got, want, g["labels"])
        shape_got = ix.last_filtered_launch()
        assert shape_got["path"] == path
        # the launch is the pure plan's
        fields = {"chunks": twin.row_bytes() // 16, "M0": g["nbr0"].shape[1], "n": n, "ef_default": ef, "path": {"walk": 1, "exact": 2}[path], "cand_cap": 0,
                  "exact_factor": 5.6, "seeds": 0, "code_chunks": code_chunks if b["routine"] == "adc" else 0}
        _, launch, why = capi.plan_filtered_compact(fields, [int(allowed.sum())], [(K, 0, 0)])
        assert why is None
        planned = launch[path]
        assert shape_got["lds_bytes"] == planned["lds"] and shape_got["expansion"] == planned["expansion"]
        if path == "walk":
            assert shape_got["vis_slots"] == planned["vis_slots_or_rows"] and shape_got["cand_cap"] == planned["cand_cap"]
        assert planned["table_bytes"] == (code_chunks * 16384 if b["routine"] == "adc" else 0)
        if b["routine"] == "decode":  # the expanded twin: the same answers and the same launch
            same(tdev.filtered(twin.filter_from_bitmap(allowed)), got)
            assert twin.last_filtered_launch() == shape_got
        if name == "all" and path == "walk":  # the all-allowed walk IS the unfiltered compact search
            plain = dev.plain()
            same(got, plain)
            if b["routine"] == "adc":
                ora = oracle.OracleIndex.from_graph(b["metric"], g["vectors"], g, M, 48, ef, 5, oracle.SUM_WAVE64)
                ora.set_pq_view(b["cb"], b["codes"])
                _, o_dist, o_slot, o_D, o_E = ora.search_batch(queries, K, ef, regimes.THREADS)
                assert np.array_equal(got[0], o_slot) and np.array_equal(got[1].view(np.uint32), o_dist.view(np.uint32))
                assert np.array_equal(got[3], o_D) and np.array_equal(got[4], o_E)


def test_the_128_kib_table_leaves_a_small_visited_set_and_long_walks_still_match(capi, oracle, monkeypatch):
    """adc_8: walks that visit the whole graph (D about n) with whatever visited set fits beside the table, and with none"""
    monkeypatch.delenv("LANTERN_GPU_PQ_ADC", raising=False)
    b = built(capi, oracle, "adc_8")
    ix, g, n, M = b["ix"], b["g"], b["n"], b["M"]
    queries, dist = b["queries"][:NQ], matrix(oracle, b, "adc")[:NQ]
    allowed = sweep_sets(n)["fiftieth"]
    f = ix.filter_from_bitmap(allowed)
    try:
        ix.set_filter_policy("walk")
        seen = set()
        for ef in (48, 700):  # beside expansion 700 and its next list no visited set fits: the HBM bitmap alone
            want = ref.search(g, dist, allowed, M, K, ef, path="walk")
            assert want[3].min() >= n, "the walk evaluates every row"
            dev = EachDev(ix, queries, K)
            check(dev.filtered(f, ef=ef), want, g["labels"])
            got = ix.last_filtered_launch()
            assert got["lds_bytes"] > 8 * 16384 and got["lds_bytes"] <= 160 * 1024
            seen.add(got["vis_slots"])
        assert seen == {2048, 0}, seen
    finally:
        ix.set_filter_policy("auto")


# ------------------------------------------------------------------------------------------------
# 4. a workgroup that serves many queries keeps nothing of the last one
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["walk", "exact"])
@pytest.mark.parametrize("shape", ["decode_g16", "adc_2_env", "adc_8"], indirect=True)
def test_reused_workgroups_rebuild_everything_per_query(capi, shape, path):
    b = shape
    ix, g, n, M, ef = b["ix"], b["g"], b["n"], b["M"], b["ef"]
    nq = 2 * NQ
    queries, dist = b["queries"], b["dist"]
    evens = np.arange(n) % 2 == 0
    sets = [evens & (np.arange(n) % 10 < 4), ~evens]  # disjoint, of different sizes
    which = [q % 2 for q in range(nq)]
    ix.set_search_shape(0, 2)
    ix.set_filter_policy(path)
    filt = [ix.filter_from_bitmap(a) for a in sets]
    dev = CompactDev(ix, queries, K)
    dev.filtered(filt[0])
    assert ix.last_filtered_launch()["grid"] == 2  # 32 queries through two workgroups
    want, tally = want_each(g, dist, sets, which, n, M, K, ef, forced=path)
    check(dev.each([filt[w] for w in which]), want, g["labels"])
    regime_is(ix, tally, distinct=2)
    # ... with per-query parameters, a query that wants nothing (no table is built for it) between two that do
    params = [(K, 0, 0)] * nq
    for at in (5, 6, 20):
        params[at] = (0, 0, 0)
    got = dev.each_params([filt[w] for w in which], params)
    slots, dists, counts, D, E = want
    for at in (5, 6, 20):
        slots[at], dists[at], counts[at], D[at], E[at] = ref.EMPTY, np.inf, 0, 0, 0
    check(got, want, g["labels"])
    assert ix.last_filtered_each_params()["k_zero"] == 3


# ------------------------------------------------------------------------------------------------
# 5. the per-query forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["decode_g8", "decode_g64", "adc_1", "adc_6_env"], indirect=True)
def test_a_filter_per_query_mixes_paths_in_one_call(capi, shape):
    b = shape
    ix, g, n, M, ef = b["ix"], b["g"], b["n"], b["M"], b["ef"]
    nq = 2 * NQ
    sets = mixed_sets(n)  # all rows, 50 %, 10 %, 1 %, one row, none, NULL
    which = [q % len(sets) for q in range(nq)]
    filt = [None if a is None else ix.filter_from_bitmap(a) for a in sets]
    dev = EachDev(ix, b["queries"], K)
    want, tally = want_each(g, b["dist"], sets, which, n, M, K, ef)
    assert tally["walk"] and tally["exact"] and tally["empty"] and tally["unfiltered"]
    before = ix.filter_stats()
    check(dev.each([filt[w] for w in which]), want, g["labels"])
    got = regime_is(ix, tally, distinct=len(sets) - 1)
    after = ix.filter_stats()
    assert got["launches"] == 2 and (after["walk"] - before["walk"], after["exact"] - before["exact"]) == (1, 1)


@pytest.mark.parametrize("shape", ["decode_g16", "adc_1", "adc_8"], indirect=True)
def test_parameters_per_query_equal_each_querys_own_call(capi, shape):
    b = shape
    ix, g, n, M, ef = b["ix"], b["g"], b["n"], b["M"], b["ef"]
    nq = 2 * NQ
    sets = mixed_sets(n)
    rows = [(1, 0, 0), (10, 16, 0), (40, 200, 0), (10, 0, 7), (25, 16, 7), (0, 200, 0), (40, 0, 0), (3, 200, 7)]  # k 1 .. 40, ef 0 / 16 / 200, skip 0 / 7
    which = [q % len(sets) for q in range(nq)]  # (7 and 8 are coprime)
    params = [rows[q % len(rows)] for q in range(nq)]
    filt = [None if a is None else ix.filter_from_bitmap(a) for a in sets]
    kw = 40
    dev = CompactDev(ix, b["queries"], kw)
    got = dev.each_params([filt[w] for w in which], params)
    largest = {"largest_expansion": 0, "largest_cand_cap": 0, "largest_exact_keys": 0, "k_zero": 0}
    for q in range(nq):
        k, e, skip = params[q]
        allowed = sets[which[q]]
        largest["k_zero"] += k == 0
        if k == 0 or (allowed is not None and not allowed.any()):
            assert got[2][q] == 0 and got[3][q] == 0 and got[4][q] == 0 and np.all(got[0][q] == ref.EMPTY), q
            continue
        ef_sel = e or ef
        exact = allowed is not None and int(allowed.sum()) ** 2 <= 5.6 * ef_sel * n
        a = np.ones(n, dtype=bool) if allowed is None else allowed
        s, d, c, D, E = ref.search(g, b["dist"][q:q + 1], a, M, k, ef_sel, skip=skip, path="exact" if exact else "walk")
        assert c[0] == got[2][q] and np.array_equal(got[0][q, :k], s[0]) and np.array_equal(got[1][q, :k].view(np.uint32), d[0].view(np.uint32)), q
        assert (D[0], E[0]) == (got[3][q], got[4][q]), q
        assert np.all(got[0][q, k:] == ref.EMPTY) and np.all(np.isinf(got[1][q, k:])) and np.all(got[5][q, k:] == 0), q
        if exact:
            largest["largest_exact_keys"] = max(largest["largest_exact_keys"], k + skip)
        else:
            exp = max(ef_sel, k + skip)
            largest["largest_expansion"] = max(largest["largest_expansion"], exp)
            largest["largest_cand_cap"] = max(largest["largest_cand_cap"], max(4 * exp, 256))
        # ... and is its own single-filter call
        if q < 8 and allowed is not None:
            one = CompactDev(ix, b["queries"][q:q + 1], k)
            mine = one.filtered(filt[which[q]], ef=e, skip=skip)
            assert np.array_equal(mine[0][0], got[0][q, :k]) and np.array_equal(mine[1][0].view(np.uint32), got[1][q, :k].view(np.uint32))
            assert (mine[2][0], mine[3][0], mine[4][0]) == (got[2][q], got[3][q], got[4][q])
    assert ix.last_filtered_each_params() == largest


@pytest.mark.parametrize("shape", ["decode_g16", "adc_2_env", "adc_8"], indirect=True)
def test_the_seeded_walk_under_a_cluster_shaped_filter(capi, shape):
    b = shape
    ix, g, n, M, ef = b["ix"], b["g"], b["n"], b["M"], b["ef"]
    queries, dist = b["queries"][:NQ], b["dist"][:NQ]
    allowed = np.zeros(n, dtype=bool)
    allowed[n // 2: n // 2 + n // 8] = True  # one contiguous block of slots
    ix.set_filter_policy("walk")
    ix.set_filter_seeds(16)
    f = ix.filter_from_bitmap(allowed)
    want = sref.search(g, dist, allowed, M, K, ef, 16)
    dev = EachDev(ix, queries, K)
    check(dev.filtered(f), want, g["labels"])
    assert ix.last_filtered_seeds()["single_seeds"] == 16
    check(dev.each([f] * NQ), want, g["labels"])
    assert ix.last_filtered_seeds()["seeded"] == NQ


# ------------------------------------------------------------------------------------------------
# 6. paging
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["decode_g8", "adc_1", "adc_8"], indirect=True)
def test_cursor_pages_are_the_skip_forms_and_the_scan_service_serves_them(capi, shape):
    b = shape
    ix, n = b["ix"], b["n"]
    allowed = np.random.default_rng(23).random(n) < 0.3
    labels = (np.flatnonzero(allowed) + 1).astype(np.uint64)
    f = ix.filter_from_labels(labels)
    assert f.count == labels.size
    ef = 64  # >= 40: every page is a slice of one list
    srv = capi.ScanServer(index=ix, max_wait_us=200)
    c = capi.ScanClient(srv.host, srv.port)
    assert c.set_filter(labels) == labels.size
    try:
        for at in range(3):
            q = b["queries"][at]
            cur = ix.cursor()
            pages = [cur.search_filtered(f, q, 10, ef), cur.search_filtered(f, q, 10, ef, streaming=True), cur.search_filtered(f, q, 20, ef, streaming=True)]
            cur.close()
            seen = np.concatenate([p[0] for p in pages])
            assert seen.size == 40 and np.unique(seen).size == 40 and set(seen.tolist()) <= set(labels.tolist())
            for (k, skip), page in zip(((10, 0), (10, 10), (20, 20)), pages):
                one = EachDev(ix, b["queries"][at:at + 1], k)
                got = one.filtered(f, ef=ef, skip=skip)
                assert np.array_equal(got[5][0], page[0]) and np.array_equal(got[1][0].view(np.uint32), page[1].view(np.uint32)), (k, skip)
            served = [c.search(q, 10, ef), c.search_next(q, 10, ef), c.search_next(q, 20, ef)]
            for have, want in zip(served, pages):
                assert np.array_equal(have[0], want[0]) and np.array_equal(have[1].view(np.uint32), want[1].view(np.uint32))
    finally:
        c.close()
        srv.stop()


# ------------------------------------------------------------------------------------------------
# 7. 8. refusals: the stride of device-resident queries, and shapes beyond the LDS budget -- before any row is written
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["decode_g64", "adc_8"], indirect=True)
def test_refusals_come_before_any_row_is_written(capi, shape):
    from lantern_amd import hip

    b = shape
    ix, twin, n = b["ix"], b["twin"], b["n"]
    queries = b["queries"][:4]
    f = ix.filter_from_bitmap(np.arange(n) % 2 == 0)
    few = ix.filter_from_bitmap(np.arange(n) < 5)
    dev = CompactDev(ix, queries, K)
    assert dev.rows.strides[0] == twin.row_bytes() == ix.row_bytes()  # the unfiltered compact call's rule: the raw f32 row
    poison = {name: np.full(buf_shape, 0xA5, dtype=np.uint8) for name, buf_shape in
              (("lab", 4 * K * 8), ("dist", 4 * K * 4), ("slot", 4 * K * 4), ("cnt", 4 * 4), ("D", 4 * 8), ("E", 4 * 8))}

    def refused(call, text):
        for name, bytes_ in poison.items():
            getattr(dev, name).upload(bytes_)
        with pytest.raises(capi.LanternGpuError, match=text):
            call()
        hip.synchronize()
        for name, bytes_ in poison.items():
            assert np.array_equal(getattr(dev, name).download(bytes_.shape, np.uint8), bytes_), name

    code_row = code_row_bytes(b["codes"].shape[1])
    for stride in (code_row, dev.rows.strides[0] + 16, 0):
        refused(lambda: ix.search_batch_filtered_device(f, dev.dq.ptr, stride, 4, K, 0, 0, dev.lab.ptr, dev.dist.ptr, dev.slot.ptr, dev.cnt.ptr, dev.D.ptr, dev.E.ptr),
                "query row stride does not match")
        refused(lambda: ix.search_batch_filtered_each_device([f, None, f, None], dev.dq.ptr, stride, 4, K, 0, 0, dev.lab.ptr, dev.dist.ptr, dev.slot.ptr, dev.cnt.ptr,
                                                             dev.D.ptr, dev.E.ptr), "query row stride does not match")
    ix.set_filter_policy("walk")
    refused(lambda: dev.filtered(f, ef=20000), "ef/k exceed the 160 KiB LDS budget of the filtered search kernel$")
    refused(lambda: dev.each([f, None, f, None], ef=20000), "ef/k exceed the 160 KiB LDS budget of the filtered search kernel$")
    refused(lambda: dev.each_params([f, None, f, None], [(K, 0, 0), (K, 64, 0), (K, 20000, 0), (K, 0, 0)]),
            r"ef/k exceed the 160 KiB LDS budget of the filtered search kernel \(params\[2\]\)$")
    ix.set_filter_policy("exact")
    refused(lambda: dev.filtered(few, skip=30000), "k \\+ skip exceed the 160 KiB LDS budget of the exact filtered search kernel$")
    refused(lambda: dev.each_params([few, few, few, few], [(K, 0, 0), (K, 0, 30000), (K, 0, 0), (K, 0, 0)]),
            r"k \+ skip exceed the 160 KiB LDS budget of the exact filtered search kernel \(params\[1\]\)$")
    if b["routine"] == "adc":  # beside the 128 KiB table two expansions that fit alone do not fit together
        ix.set_filter_policy("walk")
        for row in ((K, 800, 0), (K, 400, 0)):
            dev.each_params([None] * 4, [row] * 4)
        refused(lambda: dev.each_params([None, f, None, f], [(K, 800, 0), (K, 400, 0), (K, 0, 0), (K, 0, 0)]), "do not fit together: split the batch$")
