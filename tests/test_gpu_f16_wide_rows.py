"""f16 storage on rows of 1017 .. 2000 dimensions: the 64-lane instantiations of every kernel on halves.  Needs an MI355X.

An f16 row holds 8 scalars per 16-byte chunk; device_common.hpp group_lanes_for gives a row of >= 128 chunks to 64 lanes, which for f16
storage is every d from 1017 up to Lantern's cap of 2000 (250 chunks).  The f32 rows of 128 .. 385 chunks and the f16 rows below 128
chunks are pinned elsewhere (tests/test_gpu_parity.py BLOCK_BOUNDARY_CHUNKS and the quantised twin of that test); this file pins their
product: builds through every reverse-link kernel, every search launch shape and list placement, per-query parameters, the filtered
walk and exact path, the exact k-NN behind k_dequant_f16, gathers in both launch shapes, denormal halves, and the file round trip.

The contract has no tolerance.  The referee is the oracle fed oracle.round_f16 of rows and queries in SUM_WAVE64_F16 order (which
tests/test_f16_wide_rows_ref.py holds to float64 at these widths): slots, distance bits, D, E and adjacency are compared exactly.
Every case that is here for a launch shape states that shape through lantern_gpu_plan_search on the launch's own fields and holds the
plan's grid to the grid the launch really had, so that a change to the plan cannot silently empty the case."""
import numpy as np
import pytest

from tests import filtered_walk_ref as ref
from tests import value_range as vr
from tests.test_f16_wide_rows_ref import F16, M_COS, M_L2SQ, PATH_CLASSIC, PATH_SPEC2, WIDE, f16_chunks
from tests.test_gpu_search_params import Case, check, check_uniform, classes, small_mix

pytestmark = pytest.mark.gpu

LABEL0 = 1
PATH_SPEC1 = 3
M_HAMMING = 8
NUM_CUS = 256  # an MI355X; every planned grid below is held to the launch's own (last_search_grid), so another chip fails loudly
S_SCALARS = 28  # walk.hpp


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def halves(rng, n, d):
    return (rng.standard_normal((n, d), dtype=np.float32) * np.float32(0.4)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def mcode_of(metric):
    return (M_L2SQ if metric == "l2sq" else M_COS) + F16


def assert_same_graph(gg, go):
    assert gg["entry_slot"] == go["entry_slot"] and gg["max_level"] == go["max_level"]
    assert np.array_equal(gg["levels"], go["levels"])
    assert np.array_equal(gg["labels"], go["labels"])
    assert np.array_equal(gg["upper_off"], go["upper_off"])
    assert np.array_equal(gg["nbr0"], go["nbr0"]), ("level-0 adjacency differs", int(np.sum(np.any(gg["nbr0"] != go["nbr0"], axis=1))))
    assert np.array_equal(gg["upper_nbr"], go["upper_nbr"]), "upper-level adjacency differs"


def gathers(ix, query, slots, monkeypatch):
    """distance_gather through the plain kernel and through the walk's launch shape"""
    out = []
    for walkshape in ("0", "1"):
        monkeypatch.setenv("LANTERN_GPU_GATHER_WALKSHAPE", walkshape)
        out.append(ix.distance_gather(query, slots))
    monkeypatch.delenv("LANTERN_GPU_GATHER_WALKSHAPE")
    return out


def has_no_screen(gpu):
    return gpu.export_screen(0, 1)["row_bytes"] == 0 and gpu.screen_stats() == (0, 0)


class Answers:
    """device buffers for nq x k answers of one index, through lantern_gpu_search_batch_device"""

    def __init__(self, gpu, queries, k):
        from lantern_amd import hip

        self.hip, self.gpu, self.k = hip, gpu, k
        self.rows = gpu.device_query_rows(queries)
        self.dq = hip.Buffer.from_numpy(self.rows)
        nq = self.rows.shape[0]
        self.lab, self.dist, self.slot = hip.Buffer(nq * k * 8), hip.Buffer(nq * k * 4), hip.Buffer(nq * k * 4)
        self.D, self.E = hip.Buffer(nq * 8), hip.Buffer(nq * 8)

    def search(self, nq, ef=0):
        """(slots, distances, labels, D, E) of the first nq queries"""
        k = self.k
        for b in (self.lab, self.dist, self.slot, self.D, self.E):  # whatever the launch leaves unwritten shows
            b.upload(np.full(b.nbytes, 0xA5, dtype=np.uint8))
        self.gpu.search_batch_device(self.dq.ptr, nq, k, ef, 0, self.lab.ptr, self.dist.ptr, self.slot.ptr, None, self.D.ptr, self.E.ptr,
                                     query_stride=self.rows.strides[0])
        self.hip.synchronize()
        return (self.slot.download((nq, k), np.uint32), self.dist.download((nq, k), np.float32), self.lab.download((nq, k), np.uint64),
                self.D.download(nq, np.uint64), self.E.download(nq, np.uint64))


def assert_answers(got, want, nq, what):
    """want: the oracle's search_batch tuple (labels, distances, slots, D, E) of at least nq queries"""
    o_lab, o_dist, o_slot, o_D, o_E = (a[:nq] for a in want)
    slot, dist, lab, D, E = got
    assert np.array_equal(slot, o_slot), f"slots differ: {what}, first query {np.flatnonzero(np.any(slot != o_slot, axis=1))[:4]}"
    assert np.array_equal(lab, o_lab), f"labels differ: {what}"
    assert np.array_equal(bits(dist), bits(o_dist)), f"distance bits differ: {what}"
    assert np.array_equal(D, o_D), f"distance-evaluation counts differ: {what}"
    assert np.array_equal(E, o_E), f"expansion counts differ: {what}"


# ------------------------------------------------------------------------------------------------
# 3. build and search at every width: the twin of test_quantised_row_widths_around_the_load_block_boundaries above 125 chunks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("d", WIDE)
def test_build_and_search_at_every_width(capi, oracle, monkeypatch, metric, d):
    assert f16_chunks(d) >= 128
    rng = np.random.default_rng(d)
    n, nq, k = 500, 40, 5
    base, queries = halves(rng, n, d), halves(rng, nq, d)
    rb, rq = oracle.round_f16(base), oracle.round_f16(queries)
    labels = np.arange(n, dtype=np.uint64) + LABEL0
    ora = oracle.OracleIndex(metric, d, M=8, ef_construction=32, ef=24, seed=13, sum_mode=oracle.SUM_WAVE64_F16)
    ora.add_planned(labels, rb, max_batch=128, min_ratio=4)
    gpu = capi.GpuIndex(metric, d, M=8, ef_construction=32, ef=24, seed=13, quantization="f16")
    gpu.set_add_batch(128, 4)
    gpu.add_many(labels, base)
    gpu.flush()
    gg = gpu.export_graph(with_vectors=True)
    assert_same_graph(gg, ora.export_graph())
    assert np.array_equal(gg["vectors"].view(np.uint16), base.astype(np.float16).view(np.uint16))
    want = ora.search_batch(rq, k)
    dev = Answers(gpu, queries, k)
    for waves in (0, 4):  # the automatic shape (40 queries: the latency-bound walk) and the classic kernel
        gpu.set_search_shape(waves)
        assert_answers(dev.search(nq), want, nq, f"waves={waves}")
    gpu.set_search_shape(0)
    l1, d1 = gpu.search(queries[0], k)
    assert np.array_equal(l1, want[0][0][: len(l1)]) and np.array_equal(bits(d1), bits(want[1][0][: len(d1)])) and len(l1) == k
    picks = rng.integers(0, n, 64).astype(np.uint32)
    gref = np.array([oracle.distance(rq[1], rb[s], metric, oracle.SUM_WAVE64_F16) for s in picks], dtype=np.float32)
    for kernel, g in zip(("plain", "walkshape"), gathers(gpu, queries[1], picks, monkeypatch)):
        assert np.array_equal(bits(g), bits(gref)), ("distance_gather", kernel, int(np.sum(bits(g) != bits(gref))))
    assert gpu.counters()["add_reprunes"] > 0, "no full list was re-pruned: the reverse-link kernel under test did not run"
    assert has_no_screen(gpu), "an f16 index has an int8 screen"
    gpu.close()


# ------------------------------------------------------------------------------------------------
# 4. every reverse-link class (kernels.hip launch_revlink)
# ------------------------------------------------------------------------------------------------
def staged_lds_bytes(chunks, cap):  # kernels.hip
    up16 = lambda x: (x + 15) & ~15
    n = cap + 1
    return (cap + 2) * chunks * 16 + 4 * up16(n * 4) + up16(n * 2) + up16(n * n * 4) + S_SCALARS * 4 + up16((n + 1) * 4) + 2 * up16(n + 1)


def revlink_class(chunks, M0):
    """which kernel launch_revlink sends an f16 index's full lists to"""
    if 128 <= chunks <= 512 and M0 <= 32:
        return "pairs3" if chunks <= 192 else "pairs4" if chunks <= 256 else "pairs6+"
    if staged_lds_bytes(chunks, M0) <= 150 * 1024 and M0 <= 256:
        return "staged"
    return "generic"


REVLINK_CASES = [  # metric, n, d, M, efc, the kernel reached
    ("l2sq", 1200, 1536, 4, 32, "pairs3"),   # small M on high-dimensional Gaussian rows: hub lists collect chains of re-prunes per batch
    ("cos", 900, 2000, 8, 40, "pairs4"),
    ("l2sq", 500, 1024, 20, 48, "staged"),   # M0 = 40 > 32: no all-pairs table; 42 rows of 128 chunks are ~ 92 KB of LDS
    ("cos", 400, 2000, 20, 48, "generic"),   # M0 = 40 at 250 chunks: 168 KB of rows > the 150 KB the staged kernel may take
]


def test_the_reverse_link_cases_land_in_their_classes():
    for metric, n, d, M, efc, kernel in REVLINK_CASES:
        assert revlink_class(f16_chunks(d), 2 * M) == kernel, (d, M)
    assert 90 * 1024 < staged_lds_bytes(128, 40) < 96 * 1024 and staged_lds_bytes(250, 40) > 168000


def build_pair(capi, oracle, metric, n, d, M, efc, plan, seed=21):
    rng = np.random.default_rng(n * 7 + d)
    base = halves(rng, n, d)
    labels = np.arange(n, dtype=np.uint64) + LABEL0
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=32, seed=seed, sum_mode=oracle.SUM_WAVE64_F16)
    ora.add_planned(labels, oracle.round_f16(base), max_batch=plan[0], min_ratio=plan[1])
    gpu = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=32, seed=seed, quantization="f16")
    gpu.set_add_batch(*plan)
    gpu.add_many(labels, base)
    gpu.flush()
    assert len(gpu) == n
    return base, ora, gpu


@pytest.mark.parametrize("plan", [(1, 1), (64, 4), (512, 16)])  # (1, 1): every row alone, through k_insert_spec on wide halves
@pytest.mark.parametrize("metric,n,d,M,efc,kernel", REVLINK_CASES, ids=[f"{c[0]}-{c[2]}-M{c[3]}-{c[5]}" for c in REVLINK_CASES])
def test_build_matches_the_oracle_edge_for_edge_in_every_reverse_link_class(capi, oracle, metric, n, d, M, efc, kernel, plan):
    base, ora, gpu = build_pair(capi, oracle, metric, n, d, M, efc, plan)
    gg = gpu.export_graph(with_vectors=True)
    assert_same_graph(gg, ora.export_graph())
    assert np.array_equal(gg["vectors"].view(np.uint16), base.astype(np.float16).view(np.uint16))
    c = gpu.counters()
    assert c["add_revlink_evals"] > 0, "no full list was re-pruned"
    # (k_revlink_pairs and k_revlink_staged count their re-prunes; the generic k_revlink counts its distance evaluations alone -- so the
    # counter also tells that the last case was not staged after all)
    assert (c["add_reprunes"] == 0) == (kernel == "generic"), c
    gpu.close()


def test_build_without_the_reprune_state_is_the_same_graph(capi, oracle, monkeypatch):
    """LANTERN_GPU_REPRUNE_STATE=0 sends every request to a full list through k_revlink_pairs<F16, 3>'s all-pairs table"""
    metric, n, d, M, efc, _ = REVLINK_CASES[0]
    monkeypatch.setenv("LANTERN_GPU_REPRUNE_STATE", "0")
    base, ora, gpu = build_pair(capi, oracle, metric, n, d, M, efc, (64, 4))
    without = gpu.counters()["add_reprunes"]
    assert_same_graph(gpu.export_graph(), ora.export_graph())
    monkeypatch.delenv("LANTERN_GPU_REPRUNE_STATE")
    _, _, default = build_pair(capi, oracle, metric, n, d, M, efc, (64, 4))
    assert default.checksum() == gpu.checksum()
    assert without >= default.counters()["add_reprunes"] > 0  # (the recorded radii only ever spare a re-prune)
    gpu.close()
    default.close()


# ------------------------------------------------------------------------------------------------
# 5. every search launch shape on one graph
# ------------------------------------------------------------------------------------------------
SHAPE_INDEXES = {"l2sq": 1536, "cos": 2000}
SHAPE_N, SHAPE_M, SHAPE_EFC, SHAPE_EF, SHAPE_K, SHAPE_NQ = 1500, 16, 64, 64, 10, 1100
_shape_cache = {}


def shape_index(capi, oracle, metric):
    """a device-built 1500-row index with 50 exact duplicate rows (equal distances: the slot decides), the oracle over its exported graph"""
    if metric not in _shape_cache:
        d = SHAPE_INDEXES[metric]
        rng = np.random.default_rng(SHAPE_N + d)
        base, queries = halves(rng, SHAPE_N, d), halves(rng, SHAPE_NQ, d)
        base[SHAPE_N // 2: SHAPE_N // 2 + 50] = base[:50]
        gpu = capi.GpuIndex(metric, d, M=SHAPE_M, ef_construction=SHAPE_EFC, ef=SHAPE_EF, seed=9, quantization="f16")
        gpu.set_add_batch(256, 8)
        gpu.add_many(np.arange(SHAPE_N, dtype=np.uint64) + LABEL0, base)
        gpu.flush()
        g = gpu.export_graph()
        ora = oracle.OracleIndex.from_graph(metric, oracle.round_f16(base), g, SHAPE_M, SHAPE_EFC, SHAPE_EF, 9, oracle.SUM_WAVE64_F16)
        gpu.set_search_shape(0)
        _shape_cache[metric] = {"gpu": gpu, "ora": ora, "queries": queries, "oq": oracle.round_f16(queries), "dev": Answers(gpu, queries, SHAPE_K), "d": d}
    return _shape_cache[metric]


def shape_meant(nq, ef, spec):
    """(path, four rows per group) of a launch of nq queries at expansion ef under LANTERN_GPU_SPEC = spec (None: unset) on 256 CUs"""
    if ef <= 128 and spec in ("1", "2"):
        return (PATH_SPEC1 if spec == "1" else PATH_SPEC2), 0
    if ef <= 128 and spec is None and nq <= 2 * NUM_CUS:
        return PATH_SPEC2, 0
    return PATH_CLASSIC, int(64 <= nq <= 4 * NUM_CUS)


def planned(capi, chunks, mcode, M, n, ef_default, nq, k, ef, spec, **over):
    f = dict.fromkeys(capi.PLAN_SEARCH_IN, 0)
    f.update(chunks=chunks, M=M, M0=2 * M, mcode=mcode, n=n, ef_default=ef_default, num_cus=NUM_CUS, search_vis_slots=-1, nq=nq, k=k, ef=ef,
             env_spec_set=int(spec is not None), env_spec=int(spec or 0), env_wide_rows=-1)
    f.update(over)
    out, why = capi.plan_search(f)
    assert why is None, why
    return out


@pytest.mark.parametrize("ef", [64, 128, 200])  # one list key per lane, two per lane, the LDS list
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_every_search_launch_shape_on_one_graph(capi, oracle, cores, monkeypatch, metric, ef):
    c = shape_index(capi, oracle, metric)
    gpu, dev, k = c["gpu"], c["dev"], SHAPE_K
    want = c["ora"].search_batch(c["oq"], k, ef, min(cores, 8))
    assert len({tuple(r) for r in want[1][:64].tolist()}) == 64  # (64 different answers: a launch that mixed its queries up shows)
    reached = set()
    for spec in (None, "0", "1", "2"):
        if spec in ("1", "2") and ef > 128:
            continue  # the latency-bound walk keeps its list in registers: at most 128 entries
        if spec is None:
            monkeypatch.delenv("LANTERN_GPU_SPEC", raising=False)
        else:
            monkeypatch.setenv("LANTERN_GPU_SPEC", spec)
        for nq in (1, 37, 64, 700, 1100):
            what = f"{metric} ef={ef} nq={nq} LANTERN_GPU_SPEC={spec}"
            p = planned(capi, f16_chunks(c["d"]), mcode_of(metric), SHAPE_M, SHAPE_N, SHAPE_EF, nq, k, ef, spec)
            assert (p["path"], p["wide_rows"]) == shape_meant(nq, ef, spec), (what, p)
            assert p["expansion"] == ef and p["lds_list"] == 0
            got = dev.search(nq, ef)
            assert gpu.last_search_grid() == p["grid"], (what, "the launch is not the one planned", gpu.last_search_grid(), p["grid"])
            assert_answers(got, want, nq, what)
            reached.add((p["path"], p["wide_rows"], nq, spec))
    monkeypatch.delenv("LANTERN_GPU_SPEC", raising=False)
    # four rows per group at 64 .. 1024 queries (on request below 2 x CUs, by itself above), two rows at 1100, the latency-bound shapes
    assert {(PATH_CLASSIC, 1, 64, "0"), (PATH_CLASSIC, 1, 700, "0"), (PATH_CLASSIC, 1, 700, None), (PATH_CLASSIC, 0, 1100, None), (PATH_CLASSIC, 0, 1, "0"),
            (PATH_CLASSIC, 0, 37, "0")} <= reached
    if ef <= 128:
        assert {(PATH_SPEC2, 0, 1, None), (PATH_SPEC2, 0, 37, None), (PATH_SPEC2, 0, 64, None), (PATH_SPEC2, 0, 1100, "2"), (PATH_SPEC1, 0, 700, "1")} <= reached
    # the host-buffer batch and the lane form
    h_lab, h_dist, h_cnt = gpu.search_batch(c["queries"][:33], k, ef)
    l_lab, l_dist, l_cnt = gpu.search_batch_lane(2, c["queries"][:33], k, ef)
    for lab, dist, cnt in ((h_lab, h_dist, h_cnt), (l_lab, l_dist, l_cnt)):
        assert np.array_equal(lab, want[0][:33]) and np.array_equal(bits(dist), bits(want[1][:33])) and np.all(cnt == k)


# ------------------------------------------------------------------------------------------------
# 6. per-query parameters
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [40, 700])
@pytest.mark.parametrize("metric,d", [("l2sq", 1536), ("cos", 2000)])
def test_per_query_parameters_on_wide_halves(capi, oracle, monkeypatch, metric, d, nq):
    monkeypatch.delenv("LANTERN_GPU_SPEC", raising=False)
    case = Case(capi, oracle, metric, 1500, d, 16, 64, nq, quant="f16")
    params = small_mix(nq)
    want = case.want(params)
    got = case.params(params)
    regime = case.gpu.last_params_launch()
    # three classes of about nq / 4, nq / 2 and nq / 4 queries, each at most two per CU: the register-list classes walk latency-bound, the
    # LDS-list class takes the classic shape -- two rows per group at 10 queries, four at 175
    assert regime == {"launches": 3, "classes": classes(params, 64)[0], "largest_expansion": 136, "spec": True}, regime
    assert min(regime["classes"]) == (10 if nq == 40 else 175) and max(regime["classes"]) <= 2 * NUM_CUS
    chunks, mcode = f16_chunks(d), mcode_of(metric)
    for count, top, path in zip(regime["classes"], (64, 128, 136), (PATH_SPEC2, PATH_SPEC2, PATH_CLASSIC)):
        p = planned(capi, chunks, mcode, 16, 1500, 64, count, 129, 0, None, each=1, max_expansion=top)
        assert p["path"] == path and p["wide_rows"] == int(path == PATH_CLASSIC and count >= 64), (count, top, p)
    check(got, want, f"{metric} f16 nq={nq}")
    check_uniform(case, params, got)
    # the same batch in the bandwidth-bound shape: every class classic, four rows per group from 64 queries on
    monkeypatch.setenv("LANTERN_GPU_SPEC", "0")
    got = case.params(params)
    regime = case.gpu.last_params_launch()
    assert regime["launches"] == 3 and not regime["spec"], regime
    for count, top in zip(regime["classes"], (64, 128, 136)):
        p = planned(capi, chunks, mcode, 16, 1500, 64, count, 129, 0, "0", each=1, max_expansion=top)
        assert p["path"] == PATH_CLASSIC and p["wide_rows"] == int(count >= 64), (count, top, p)
    check(got, want, f"{metric} f16 nq={nq} LANTERN_GPU_SPEC=0")


# ------------------------------------------------------------------------------------------------
# 7. filtered search: the walk, the exact path, one filter and a filter per query
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d", [("l2sq", 1536), ("cos", 2000)])
def test_filtered_search_on_wide_halves(capi, oracle, metric, d):
    from tests.test_gpu_filtered_each import EachDev, regime_is, want_each
    from tests.test_gpu_filtered_regimes import check as check_filtered
    from tests.test_gpu_filtered_regimes import instance, shape_is

    n, nq, M, ef, k = 1000, 32, 16, 64, 10
    gpu, g, dist, queries = instance(capi, oracle, "f16", metric, d, M, None, n, nq, ef)
    dev = EachDev(gpu, queries, k)
    u = np.random.default_rng(7).random(n)
    # the rule (filter.hip): exact iff allowed^2 <= 5.6 ef n, i.e. up to 598 allowed rows here
    sets = [u < 0.8, u < 0.1, None]
    assert sets[0].sum() ** 2 > 5.6 * ef * n >= sets[1].sum() ** 2 and sets[1].sum() > k
    filt = [None if a is None else gpu.filter_from_bitmap(a) for a in sets]
    try:
        gpu.set_filter_policy("auto")
        for skip in (0, 3):
            got = dev.filtered(filt[0], skip=skip)
            shape_is(gpu, "walk", expansion=ef, grid=nq)
            check_filtered(got, ref.search(g, dist, sets[0], M, k, ef, skip=skip), g["labels"])
            got = dev.filtered(filt[1], skip=skip)
            shape_is(gpu, "exact", expansion=k + skip, grid=nq)
            check_filtered(got, ref.search(None, dist, sets[1], M, k, ef, skip=skip, path="exact"), g["labels"])
        # a filter per query: the wide one (walk), the narrow one (exact) and none (walk), by turns, in one call
        which = [q % 3 for q in range(nq)]
        want, tally = want_each(g, dist, sets, which, n, M, k, ef)
        got = dev.each([filt[w] for w in which])
        regime_is(gpu, tally, distinct=2)
        assert tally["walk"] >= 20 and tally["exact"] >= 10 and tally["unfiltered"] >= 10
        check_filtered(got, want, g["labels"])
        # the walk under the selective filter, alone and per query
        gpu.set_filter_policy("walk")
        got = dev.filtered(filt[1])
        shape_is(gpu, "walk", expansion=ef, grid=nq)
        check_filtered(got, ref.search(g, dist, sets[1], M, k, ef), g["labels"])
        want, tally = want_each(g, dist, sets, which, n, M, k, ef, forced="walk")
        got = dev.each([filt[w] for w in which])
        regime_is(gpu, tally, distinct=2)
        assert tally["exact"] == 0
        check_filtered(got, want, g["labels"])
    finally:
        gpu.set_filter_policy("auto")
    gpu.close()


# ------------------------------------------------------------------------------------------------
# 8. the exact k-NN: k_dequant_f16 in front of the MFMA contraction, k_rerank on 64 lanes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("metric,n,d,nq,k", [("l2sq", 4097, 1536, 33, 10), ("cos", 4097, 2000, 33, 10)])
def test_exact_search_on_wide_halves_is_the_brute_force(capi, oracle, cores, monkeypatch, metric, n, d, nq, k, fused):
    from tests.test_gpu_exact_knn import index_of, referee

    rng = np.random.default_rng([n, d, nq, k])
    rows, queries = halves(rng, n, d), halves(rng, nq, d)
    ids, dists, stored = referee(oracle, cores, metric, "f16", rows, queries, k)  # (held to float64 in there)
    ix = index_of(capi, metric, "f16", rows, stored)
    monkeypatch.setenv("LANTERN_GPU_DENSE_FUSED", "1" if fused else "0")
    before = capi.exact_knn_stats()
    slots, got = ix.exact_search(queries, k)
    after = capi.exact_knn_stats()
    bad = np.nonzero(np.any(slots != ids, axis=1) | np.any(bits(got) != bits(dists), axis=1))[0]
    assert bad.size == 0, (f"{bad.size} of {nq} queries differ from the brute force", bad[:8].tolist(), slots[bad[0]].tolist(), ids[bad[0]].tolist())
    st = {key: after[key] - before[key] for key in after}
    assert st["queries"] == nq and st["certified"] + st["fallback"] == nq, st
    ix.close()


# ------------------------------------------------------------------------------------------------
# 9. denormal and top-of-range halves through 64 lanes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_gathers_have_the_oracles_bits_on_denormal_wide_halves(capi, oracle, monkeypatch, metric):
    from tests.test_gpu_value_range import empty_graph

    d, NA, NB = 1536, 7, 33
    rows, queries = vr.strict_data("f16_denorm", NB, d, NA)
    sr, sq = oracle.round_f16(rows), oracle.round_f16(queries)
    assert np.any((np.abs(sr) > 0) & (np.abs(sr) < 2.0 ** -14)) and np.any(np.abs(sr) > 4.9e4)
    want = np.array([[oracle.distance(q, r, metric, oracle.SUM_WAVE64_F16) for r in sr] for q in sq], dtype=np.float32)
    assert np.all(vr.within_rounding(metric, want, vr.exact64(metric, sr, sq, direct=True), d)), "the oracle is off float64"
    ix = capi.GpuIndex(metric, d, M=4, ef_construction=8, seed=1, quantization="f16")
    ix.import_graph(rows, empty_graph(NB))
    slots = np.random.default_rng(d).integers(0, NB, 3 * NB).astype(np.uint32)
    for i, q in enumerate(queries):
        for kernel, g in zip(("plain", "walkshape"), gathers(ix, q, slots, monkeypatch)):
            assert np.array_equal(bits(g), bits(want[i, slots])), ("distance_gather", kernel, i, int(np.sum(bits(g) != bits(want[i, slots]))))
    ix.close()


@pytest.mark.parametrize("plan", [(1, 1), (512, 16)])
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_build_on_denormal_wide_halves_is_edge_for_edge(capi, oracle, cores, metric, plan):
    n, d, M, efc = 400, 1536, 16, 64
    base, _ = vr.strict_data("f16_denorm", n, d, 1)
    labels = np.arange(n, dtype=np.uint64) + LABEL0
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=32, seed=21, sum_mode=oracle.SUM_WAVE64_F16)
    ora.set_build_threads(min(cores, 8))
    ora.add_planned(labels, oracle.round_f16(base), max_batch=plan[0], min_ratio=plan[1])
    gpu = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=32, seed=21, quantization="f16")
    gpu.set_add_batch(*plan)
    gpu.add_many(labels, base)
    gpu.flush()
    gg = gpu.export_graph(with_vectors=True)
    assert_same_graph(gg, ora.export_graph())
    assert np.array_equal(gg["vectors"].view(np.uint16), base.astype(np.float16).view(np.uint16))
    gpu.close()


# ------------------------------------------------------------------------------------------------
# 10. the file: 2 d vector bytes per node, and back
# ------------------------------------------------------------------------------------------------
def test_file_round_trip_at_the_cap(capi, oracle):
    metric, n, d, M, efc, _ = REVLINK_CASES[1]
    base, ora, gpu = build_pair(capi, oracle, metric, n, d, M, efc, (64, 4))
    queries = halves(np.random.default_rng(5), 40, d)
    lab, dist, cnt = gpu.search_batch(queries, 10)
    o_lab, o_dist, _, _, _ = ora.search_batch(oracle.round_f16(queries), 10)
    assert np.array_equal(lab, o_lab) and np.array_equal(bits(dist), bits(o_dist))
    levels = gpu.export_graph()["levels"]
    blob = gpu.save_buffer()
    assert len(blob) == 136 + sum(10 + (4 + 2 * M * 6) + int(l) * (4 + M * 6) + 2 * d for l in levels)
    again = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=32, seed=21, quantization="f16")
    again.load_buffer(blob)
    assert len(again) == n and again.checksum() == gpu.checksum()
    lab2, dist2, cnt2 = again.search_batch(queries, 10)
    assert np.array_equal(lab2, lab) and np.array_equal(bits(dist2), bits(dist)) and np.array_equal(cnt2, cnt)
    gpu.close()
    again.close()


# ------------------------------------------------------------------------------------------------
# 11. a small relative: wide Hamming rows in the four-row shape (the other hand-listed four-row instantiation, search_launch.hpp)
# ------------------------------------------------------------------------------------------------
def test_wide_hamming_rows_in_the_four_row_shape(capi, oracle, cores, monkeypatch):
    metric, n, words, M, efc, ef, k = "hamming", 600, 512, 8, 32, 32, 5
    rng = np.random.default_rng(n + words)
    base = rng.integers(0, 2 ** 32, size=(n, words), dtype=np.uint32)
    queries = rng.integers(0, 2 ** 32, size=(1024, words), dtype=np.uint32)
    gpu = capi.GpuIndex(metric, words, M=M, ef_construction=efc, ef=ef, seed=13)
    gpu.set_add_batch(128, 4)
    gpu.add_many(np.arange(n, dtype=np.uint64) + LABEL0, base)
    gpu.flush()
    ora = oracle.OracleIndex.from_graph(metric, base, gpu.export_graph(), M, efc, ef, 13, oracle.SUM_WAVE64)
    want = ora.search_batch(queries, k, ef, min(cores, 8))
    dev = Answers(gpu, queries, k)
    gpu.set_search_shape(0)
    monkeypatch.setenv("LANTERN_GPU_SPEC", "0")
    for nq in (64, 200, 1024):
        p = planned(capi, words // 4, M_HAMMING, M, n, ef, nq, k, 0, "0")
        assert p["path"] == PATH_CLASSIC and p["wide_rows"] == 1 and p["waves"] == 4, p
        got = dev.search(nq)
        assert gpu.last_search_grid() == p["grid"]
        assert_answers(got, want, nq, f"hamming nq={nq}")
    gpu.close()
