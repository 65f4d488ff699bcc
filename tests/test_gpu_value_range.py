"""The float kernels at the edges of the f32 range (tests/value_range.py): denormal squares, sums that overflow to +inf, scales 2^-45 ..
2^55 in one index, denormal halves in f16 storage.  The pair kernel, both gathers, every walk, the build: bit for bit the oracle's
device-order arithmetic (which tests/test_value_range_ref.py holds to float64) -- one flushed denormal or one +inf tie out of slot
order changes distance bits, slots or the D / E counts and fails here.  Non-finite rows and queries: the class of every distance, and
that a search over them comes back with a well-formed answer.  Needs an MI355X."""
import numpy as np
import pytest

from tests import value_range as vr

pytestmark = pytest.mark.gpu

F32 = np.float32
PAIR_DIMS = [1, 3, 33, 128, 520, 768, 2000]
NA, NB = 7, 33


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def empty_graph(n):
    return {"levels": np.zeros(n, np.uint8), "nbr0": np.full((n, 8), 0xFFFFFFFF, np.uint32), "upper_off": np.full(n, 0xFFFFFFFF, np.uint32),
            "upper_nbr": np.zeros((0, 4), np.uint32), "labels": None, "entry_slot": 0, "max_level": 0}


def stored(oracle, storage, rows, queries):
    """what the index holds and computes on, and the oracle's matching sum mode"""
    if storage == "f16":
        return oracle.round_f16(rows), oracle.round_f16(queries), oracle.SUM_WAVE64_F16
    return rows, queries, oracle.SUM_WAVE64


def oracle_matrix(oracle, metric, rows, queries, mode):
    return np.array([[oracle.distance(q, r, metric, mode) for r in rows] for q in queries], dtype=F32)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=F32).view(np.uint32), np.ascontiguousarray(b, dtype=F32).view(np.uint32))


def gathers(ix, queries, slots, monkeypatch):
    """distance_gather of every query through the plain kernel and through the walk's launch shape"""
    out = []
    for walkshape in ("0", "1"):
        monkeypatch.setenv("LANTERN_GPU_GATHER_WALKSHAPE", walkshape)
        out.append(np.stack([ix.distance_gather(q, slots) for q in queries]))
    monkeypatch.delenv("LANTERN_GPU_GATHER_WALKSHAPE")
    return out


# ---- a. the pair kernels --------------------------------------------------------------------------------------------------------
def assert_oracles_bits(got, want, what):
    """bit for bit wherever the oracle's value is a number (+inf included); the same class where it is a NaN"""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    num = ~np.isnan(want)
    differ = num & (got.view(np.uint32) != want.view(np.uint32))
    assert not differ.any(), (what, int(differ.sum()), np.argwhere(differ)[:4].tolist())
    assert np.all(np.isnan(got[~num])), (what, "a number where the oracle has a NaN")


@pytest.mark.parametrize("d", PAIR_DIMS)
@pytest.mark.parametrize("family,metric", vr.F32_PAIRS, ids=[f"{f}-{m}" for f, m in vr.F32_PAIRS])
def test_pair_kernels_have_the_oracles_bits(capi, oracle, monkeypatch, family, metric, d):
    rows, queries = vr.strict_data(family, NB, d, NA)
    want = oracle_matrix(oracle, metric, rows, queries, oracle.SUM_WAVE64)
    strict = vr.in_domain(family, metric)  # (an l2sq family under cosine: bits where the oracle has a number, no float64 check)
    ref = vr.exact64(metric, rows, queries, direct=True)
    if strict:
        assert not np.any(np.isnan(want)) and np.all(vr.within_rounding(metric, want, ref, d)), "the oracle is off float64"
    got = capi.distance_matrix(queries, rows, metric, exact_order=True)
    print(family, metric, d, "distance_matrix bits differing:", int(np.sum(got.view(np.uint32) != want.view(np.uint32))), "oracle NaNs:", int(np.isnan(want).sum()))
    assert_oracles_bits(got, want, "distance_matrix")
    if strict:
        assert np.all(vr.within_rounding(metric, got, ref, d))
    one = np.array([capi.distance(queries[i], rows[(5 * i) % NB], metric) for i in range(NA)], dtype=F32)
    assert_oracles_bits(one, want[np.arange(NA), (5 * np.arange(NA)) % NB], "usearch_distance")
    ix = capi.GpuIndex(metric, d, M=4, ef_construction=8, seed=1)
    ix.import_graph(rows, empty_graph(NB))
    slots = np.random.default_rng(d).integers(0, NB, 3 * NB).astype(np.uint32)
    for kernel, g in zip(("plain", "walkshape"), gathers(ix, queries, slots, monkeypatch)):
        assert_oracles_bits(g, want[:, slots], "distance_gather " + kernel)
    ix.close()


@pytest.mark.parametrize("d", [33, 200, 768])
@pytest.mark.parametrize("family,metric", vr.F16_STRICT, ids=[f"{f}-{m}" for f, m in vr.F16_STRICT])
def test_f16_gathers_have_the_oracles_bits_on_denormal_halves(capi, oracle, monkeypatch, family, metric, d):
    rows, queries = vr.strict_data(family, NB, d, NA)
    sr, sq, mode = stored(oracle, "f16", rows, queries)
    assert np.any((np.abs(sr) > 0) & (np.abs(sr) < 2.0 ** -14)), "no denormal half among the stored operands"
    want = oracle_matrix(oracle, metric, sr, sq, mode)
    assert np.all(vr.within_rounding(metric, want, vr.exact64(metric, sr, sq, direct=True), d)), "the oracle is off float64"
    ix = capi.GpuIndex(metric, d, M=4, ef_construction=8, seed=1, quantization="f16")
    ix.import_graph(rows, empty_graph(NB))
    slots = np.random.default_rng(d).integers(0, NB, 3 * NB).astype(np.uint32)
    for kernel, g in zip(("plain", "walkshape"), gathers(ix, queries, slots, monkeypatch)):
        assert same_bits(g, want[:, slots]), ("distance_gather", kernel, int(np.sum(g.view(np.uint32) != want[:, slots].view(np.uint32))))
    ix.close()


# ---- b. search on the oracle's graph ----------------------------------------------------------------------------------------------
ALL_STRICT = vr.F32_STRICT + vr.F16_STRICT


@pytest.mark.parametrize("d", [33, 768])
@pytest.mark.parametrize("family,metric", ALL_STRICT, ids=[f"{f}-{m}" for f, m in ALL_STRICT])
def test_walks_on_the_oracles_graph_are_the_oracles_walks(capi, oracle, cores, monkeypatch, family, metric, d):
    from lantern_amd import hip

    n, nq, M, efc, k = 1500, 64, 16, 64, 10
    storage = vr.STRICT[family][1]
    base, queries = vr.strict_data(family, n, d, nq)
    obase, oq, mode = stored(oracle, storage, base, queries)
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=64, seed=9, sum_mode=mode)
    ora.set_build_threads(min(cores, 8))  # (x86 takes microcode assists on denormals: the sequential build of l2_denorm is ten times slower)
    ora.add_planned(np.arange(n, dtype=np.uint64) + 1, obase, max_batch=256, min_ratio=8)
    g = ora.export_graph()
    monkeypatch.delenv("LANTERN_GPU_SPEC", raising=False)
    gpu = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=64, seed=9, quantization=storage)
    gpu.import_graph(base, g)
    rows = gpu.device_query_rows(queries)
    dq = hip.Buffer.from_numpy(rows)
    lab, dist, slot = hip.Buffer(nq * k * 8), hip.Buffer(nq * k * 4), hip.Buffer(nq * k * 4)
    D, E = hip.Buffer(nq * 8), hip.Buffer(nq * 8)
    # (waves, LANTERN_GPU_SPEC): the classic walk at 4 and 8 waves, the default shape, the two latency-bound shapes
    shapes = [(4, None), (8, None), (0, None), (0, "1"), (0, "2")]
    for ef in (10, 64, 200):
        o_lab, o_dist, o_slot, o_D, o_E = ora.search_batch(oq, k, ef, min(cores, 8))
        assert not np.any(np.isnan(o_dist)), "a strict family gave the oracle a NaN"
        for waves, spec in shapes:
            if spec is None:
                monkeypatch.delenv("LANTERN_GPU_SPEC", raising=False)
            else:
                monkeypatch.setenv("LANTERN_GPU_SPEC", spec)
            gpu.set_search_shape(waves)
            gpu.search_batch_device(dq.ptr, nq, k, ef, 0, lab.ptr, dist.ptr, slot.ptr, None, D.ptr, E.ptr, query_stride=rows.strides[0])
            hip.synchronize()
            what = f"ef={ef} waves={waves} spec={spec}"
            assert np.array_equal(slot.download((nq, k), np.uint32), o_slot), "slots differ: " + what
            assert np.array_equal(lab.download((nq, k), np.uint64), o_lab), "labels differ: " + what
            assert same_bits(dist.download((nq, k), np.float32), o_dist), "distance bits differ: " + what
            assert np.array_equal(D.download(nq, np.uint64), o_D), "distance-evaluation counts differ: " + what
            assert np.array_equal(E.download(nq, np.uint64), o_E), "expansion counts differ: " + what
        monkeypatch.delenv("LANTERN_GPU_SPEC", raising=False)
        gpu.set_search_shape(0)
        h_lab, h_dist, h_cnt = gpu.search_batch(queries, k, ef)
        assert np.array_equal(h_lab, o_lab) and same_bits(h_dist, o_dist), f"host-buffer batch differs: ef={ef}"
    if metric == "l2sq" and storage == "f32" and d == 768:  # rows of >= 128 chunks: the classic walks above went through the int8 screen
        logical, exact = gpu.screen_stats()
        print(family, "screen: logical", logical, "exact", exact)
        assert logical > 0
    gpu.close()


# ---- c. the build ------------------------------------------------------------------------------------------------------------------
BUILD_FAMILIES = [("l2_denorm", "l2sq"), ("l2_edge", "l2sq"), ("cos_mixed", "cos"), ("f16_denorm", "l2sq"), ("f16_denorm", "cos")]


@pytest.mark.parametrize("plan", [(1, 1), (512, 16)])
@pytest.mark.parametrize("d", [33, 520])
@pytest.mark.parametrize("family,metric", BUILD_FAMILIES, ids=[f"{f}-{m}" for f, m in BUILD_FAMILIES])
def test_build_matches_the_oracle_edge_for_edge(capi, oracle, cores, family, metric, d, plan):
    n, M, efc = 900, 16, 64
    storage = vr.STRICT[family][1]
    base, _ = vr.strict_data(family, n, d, 1)
    obase, _, mode = stored(oracle, storage, base, base[:1])
    labels = np.arange(n, dtype=np.uint64) + 1
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=32, seed=21, sum_mode=mode)
    ora.set_build_threads(min(cores, 8))
    ora.add_planned(labels, obase, max_batch=plan[0], min_ratio=plan[1])
    gpu = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=32, seed=21, quantization=storage)
    gpu.set_add_batch(*plan)
    gpu.add_many(labels, base)
    gpu.flush()
    assert len(gpu) == n
    go, gg = ora.export_graph(), gpu.export_graph(with_vectors=True)
    assert gg["entry_slot"] == go["entry_slot"] and gg["max_level"] == go["max_level"]
    assert np.array_equal(gg["levels"], go["levels"]) and np.array_equal(gg["labels"], go["labels"])
    assert np.array_equal(gg["upper_off"], go["upper_off"])
    assert np.array_equal(gg["nbr0"], go["nbr0"]), ("level-0 adjacency differs", int(np.sum(np.any(gg["nbr0"] != go["nbr0"], axis=1))))
    assert np.array_equal(gg["upper_nbr"], go["upper_nbr"]), "upper-level adjacency differs"
    assert np.array_equal(gg["vectors"], base.astype(np.float16) if storage == "f16" else base)
    gpu.close()


# ---- d. non-finite rows and queries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 33, 768])
def test_non_finite_pairs_have_the_referees_class(capi, oracle, d):
    results = []
    for name, a, b in vr.loose_pairs(np.random.default_rng(d), d):  # (nothing asserted in this loop: the log holds every NaN's bits)
        for metric in ("l2sq", "cos"):
            got = F32(capi.distance(a, b, metric))
            mat = capi.distance_matrix(a[None, :], b[None, :], metric, exact_order=True)[0, 0]
            ora = F32(oracle.distance(a, b, metric, oracle.SUM_WAVE64))
            results.append((name, metric, a, b, got, mat, ora))
            if np.isnan(got) or np.isnan(ora):
                print(f"d={d} {name} {metric}: device 0x{int(got.view(np.uint32)):08X} oracle 0x{int(ora.view(np.uint32)):08X}")
    for name, metric, a, b, got, mat, ora in results:
        assert vr.value_class(got) == vr.value_class(mat), (name, metric, "usearch_distance and distance_matrix")
        assert vr.value_class(got) == vr.value_class(ora), (name, metric, "the oracle's class", float(got), float(ora))
        if not name.startswith("finite_1e19"):  # (there the class depends on where the f32 sums overflow: the oracle's order decides)
            assert vr.value_class(got) == vr.class64(metric, a, b), (name, metric, "float64's class", float(got))
        if vr.value_class(got) == "num":
            assert got.view(np.uint32) == ora.view(np.uint32), (name, metric)


def test_search_with_non_finite_queries_returns_a_well_formed_answer(capi, oracle):
    n, d, k, M, efc = 1500, 33, 10, 16, 64
    base, q = vr.strict_data("l2_tiny", n, d, 16)
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=efc, ef=64, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    gpu = capi.GpuIndex("l2sq", d, M=M, ef_construction=efc, ef=64, seed=9)
    gpu.import_graph(base, ora.export_graph())
    sp = list(vr.loose_specials().values())
    queries = q.copy()
    for i in range(16):  # one special component, two of them, a whole row
        queries[i, i % d] = sp[i % 4]
        if i >= 8:
            queries[i, (i + 7) % d] = sp[(i // 4) % 4]
    queries[15] = sp[0]
    for waves in (0, 4):
        gpu.set_search_shape(waves)
        for ef in (10, 64, 200):
            lab, dist, cnt = gpu.search_batch(queries, k, ef)
            assert np.all(cnt <= k)
            for i in range(16):
                c = int(cnt[i])
                got = lab[i, :c]
                assert len(set(got.tolist())) == c, ("a label twice", waves, ef, i, got.tolist())
                assert np.all((got >= 1) & (got <= n)), ("a label that is not in the index", waves, ef, i, got.tolist())
                fin = np.isfinite(dist[i, :c])
                if fin.any():
                    want = gpu.distance_gather(queries[i], (got[fin] - 1).astype(np.uint32))
                    assert same_bits(dist[i, :c][fin], want), (waves, ef, i)
    gpu.set_search_shape(0)
    gpu.close()
