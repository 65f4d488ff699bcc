"""Per-query k, ef and skip in one call (include/lantern_gpu.h "PER-QUERY k, ef AND skip").  Needs an MI355X.

The contract has no tolerance: for query i the ids, distance bits, count, D and E of lantern_gpu_search_batch_params* are those of
the uniform search with (k_i, ef_i, skip_i).  The arbiter is the one the uniform tests use -- OracleIndex.search(q, k_i, ef_i, skip_i)
on the exported graph, in the storage's summation mode -- and the library's own uniform call with that triple is a second check.
Every case states its regime through GpuIndex.last_params_launch (launches, queries per list-placement class, spec shape or not).
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
KS, EFS = (1, 10, 37, 64, 65, 128, 129, 300), (0, 4, 64, 128, 200)


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def rand_rows(rng, n, d, metric):
    if metric == "hamming":
        return rng.integers(0, 2**32, size=(n, d), dtype=np.uint32)
    return rng.standard_normal((n, d), dtype=np.float32)


def full_mix(reps=1):
    """Every (k, ef, skip) of the issue's grid -- 8 x 5 x 3 = 120 triples, skip in {0, 7, k} -- `reps` times over, interleaved."""
    one = [(k, ef, s) for s_i in range(3) for ef in EFS for k in KS for s in [(0, 7, k)[s_i]]]
    return [one[i % len(one)] for i in range(len(one) * reps)]


def small_mix(nq, ks=(1, 10, 65, 129), efs=(0, 128), skips=(0, 7)):
    grid = [(k, ef, s) for s in skips for ef in efs for k in ks]
    return [grid[i % len(grid)] for i in range(nq)]


def expansion(p, index_ef):
    k, ef, skip = p
    return max(ef or index_ef, k + skip)


def classes(params, index_ef):
    e = np.array([expansion(p, index_ef) for p in params])
    return (int((e <= 64).sum()), int(((e > 64) & (e <= 128)).sum()), int((e > 128).sum())), int(e.max())


class Case:
    """One index on the device, the oracle over its exported graph, and device buffers for nq x k_stride answers."""

    def __init__(self, capi, oracle, metric, n, d, M, ef, nq, quant="f32", seed=9):
        rng = np.random.default_rng(n + d + M)
        scale = np.float32(0.4 if quant == "i8" else 1.0)
        base, queries = rand_rows(rng, n, d, metric), rand_rows(rng, nq, d, metric)
        if metric != "hamming":
            base, queries = base * scale, queries * scale
            if n >= 200:
                base[n // 2: n // 2 + 50] = base[:50]  # exact duplicates: equal distances, the slot decides
        if quant == "f16":
            obase, oq, mode = oracle.round_f16(base), oracle.round_f16(queries), oracle.SUM_WAVE64_F16
        elif quant == "i8":
            obase, oq, mode = oracle.quantize_i8(base), oracle.quantize_i8(queries), oracle.SUM_I8
        else:
            obase, oq, mode = base, queries, oracle.SUM_WAVE64
        self.capi, self.metric, self.n, self.ef, self.nq, self.queries, self.oq = capi, metric, n, ef, nq, queries, oq
        self.gpu = capi.GpuIndex(metric, d, M=M, ef_construction=48, ef=ef, seed=seed, quantization="f32" if quant == "b1" else quant)
        self.gpu.set_add_batch(256, 8)
        if n:
            self.gpu.add_many(np.arange(n, dtype=np.uint64) + 1, base)
            g = self.gpu.export_graph()
            self.ora = oracle.OracleIndex.from_graph(metric, obase, g, M, 48, ef, seed, mode)
            self.labels = g["labels"]
        else:
            self.ora, self.labels = None, np.zeros(0, dtype=np.uint64)
        self.gpu.set_search_shape(0)
        self._dev()

    def _dev(self):
        from lantern_amd import hip

        self.hip = hip
        self.rows = self.gpu.device_query_rows(self.queries)
        self.dq = hip.Buffer.from_numpy(self.rows)
        self.bufs = {}

    def _buffers(self, ks):
        if ks not in self.bufs:
            nq, h = self.nq, self.hip
            self.bufs[ks] = (h.Buffer(max(nq * ks, 1) * 8), h.Buffer(max(nq * ks, 1) * 4), h.Buffer(max(nq * ks, 1) * 4), h.Buffer(nq * 4), h.Buffer(nq * 8),
                             h.Buffer(nq * 8))
        return self.bufs[ks]

    def _out(self, ks):
        lab, dist, slot, cnt, D, E = self._buffers(ks)
        self.hip.synchronize()
        nq = self.nq
        return (slot.download((nq, ks), np.uint32), dist.download((nq, ks), np.float32), cnt.download(nq, np.uint32), D.download(nq, np.uint64),
                E.download(nq, np.uint64), lab.download((nq, ks), np.uint64))

    def params(self, params, k_stride=None):
        ks = max(p[0] for p in params) if k_stride is None else k_stride
        lab, dist, slot, cnt, D, E = self._buffers(ks)
        for b in (lab, dist, slot, cnt, D, E):  # whatever the call leaves unwritten shows
            b.upload(np.full(b.nbytes, 0xA5, dtype=np.uint8))
        self.gpu.search_batch_params_device(self.dq.ptr, self.rows.strides[0], self.nq, params, ks, lab.ptr, dist.ptr, slot.ptr, cnt.ptr, D.ptr, E.ptr)
        return self._out(ks)

    def uniform(self, k, ef, skip):
        lab, dist, slot, cnt, D, E = self._buffers(k)
        self.gpu.search_batch_device(self.dq.ptr, self.nq, k, ef, skip, lab.ptr, dist.ptr, slot.ptr, cnt.ptr, D.ptr, E.ptr, query_stride=self.rows.strides[0])
        return self._out(k)

    def want(self, params, ks=None):
        """The oracle's answer per query with that query's own triple, laid out as the call lays it out."""
        ks = max(p[0] for p in params) if ks is None else ks
        nq = self.nq
        slots, dists = np.full((nq, ks), EMPTY, dtype=np.uint32), np.full((nq, ks), np.inf, dtype=np.float32)
        labels = np.zeros((nq, ks), dtype=np.uint64)
        counts, D, E = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint64), np.zeros(nq, dtype=np.uint64)
        for q, (k, ef, skip) in enumerate(params):
            if k == 0 or self.ora is None:
                continue
            lab, dst, slt = self.ora.search(self.oq[q], k, ef, skip)
            c = len(lab)
            labels[q, :c], dists[q, :c], slots[q, :c], counts[q] = lab, dst, slt, c
            D[q], E[q] = self.ora.last_counters()
        return slots, dists, counts, D, E, labels


def check(got, want, what=""):
    names = ("slots", "distance bits", "counts", "D", "E", "labels")
    for name, a, b in zip(names, got, want):
        if name == "distance bits":
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not np.array_equal(a, b):
            bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
            raise AssertionError(f"{what}: {name} differ for {len(bad)} queries, first {bad[:8]}")


def check_uniform(case, params, got):
    """the library's own uniform call with each distinct triple answers that triple's queries identically"""
    for t in sorted(set(params)):
        if t[0] == 0:
            continue
        qs = [q for q, p in enumerate(params) if p == t]
        uni = case.uniform(*t)
        k = t[0]
        for name, a, b in zip(("slots", "dists", "counts", "D", "E", "labels"), got, uni):
            a = a[qs, :k] if a.ndim == 2 else a[qs]
            b = b[qs]
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), (t, name)


# ------------------------------------------------------------------------------------------------
# 1. the mixed batch of the issue, in both regimes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reps,spec", [(1, True), (20, False)])
def test_mixed_batch_is_the_uniform_search_per_query(capi, oracle, reps, spec):
    """120 queries: every class is small enough for the 3 + 8 wave shape (the two register-list classes take it, the LDS-list class
    cannot).  2400 queries: every class has more than two queries per CU -- the classic shape throughout."""
    params = full_mix(reps)
    case = Case(capi, oracle, "l2sq", 3000, 128, 16, 64, len(params))
    got = case.params(params)
    cls, top = classes(params, 64)
    regime = case.gpu.last_params_launch()
    assert regime == {"launches": 3, "classes": cls, "largest_expansion": top, "spec": spec}, regime
    assert cls == (27 * reps, 33 * reps, 60 * reps) and top == 600
    if not spec:
        assert min(cls) > 2 * 256  # more than two queries per CU in every launch
    check(got, case.want(params), "mixed")
    if reps == 1:
        check_uniform(case, params, got)


# ------------------------------------------------------------------------------------------------
# 2. single-class batches, uniform parameters
# ------------------------------------------------------------------------------------------------
def test_single_class_batches_make_one_launch(capi, oracle):
    case = Case(capi, oracle, "l2sq", 2500, 96, 16, 64, 160)
    for c, params in enumerate((small_mix(160, (1, 10, 37), (0, 4, 64), (0, 7)), small_mix(160, (65, 100), (0, 128), (0, 7)),
                                small_mix(160, (129, 200), (0, 300), (0, 7)))):
        got = case.params(params)
        regime = case.gpu.last_params_launch()
        assert regime["launches"] == 1 and regime["classes"][c] == 160 and sum(regime["classes"]) == 160, regime
        check(got, case.want(params), f"class {c}")


@pytest.mark.parametrize("nq", [40, 700])
def test_uniform_parameters_equal_search_batch_bit_for_bit(capi, oracle, nq):
    case = Case(capi, oracle, "cos", 2000, 200, 16, 64, nq)
    for k, ef in ((10, 0), (10, 100), (70, 0)):
        lab, dist, cnt = case.gpu.search_batch_params(case.queries, [(k, ef)] * nq)
        ulab, udist, ucnt = case.gpu.search_batch(case.queries, k, ef)
        assert np.array_equal(lab, ulab) and np.array_equal(dist.view(np.uint32), udist.view(np.uint32)) and np.array_equal(cnt, ucnt)
        assert case.gpu.last_params_launch()["launches"] == 1


# ------------------------------------------------------------------------------------------------
# 3. metrics and storage kinds; both batch sizes (the latency-bound shape, the bandwidth-bound ones)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,n,d,M,quant", [("cos", 2000, 768, 16, "f32"), ("hamming", 3000, 24, 16, "b1"), ("l2sq", 1500, 768, 8, "f16"),
                                                ("cos", 1500, 256, 16, "i8"), ("l2sq", 1200, 40, 5, "f32")])
def test_metrics_and_storage_kinds(capi, oracle, metric, n, d, M, quant):
    for nq in (96, 2100):  # (2100: more than two queries per CU in every class)
        case = Case(capi, oracle, metric, n, d, M, 64, nq, quant)
        params = small_mix(nq)
        got = case.params(params)
        regime = case.gpu.last_params_launch()
        assert regime["launches"] == 3 and regime["spec"] == (nq == 96), regime
        check(got, case.want(params), f"{metric} {quant} nq={nq}")
        if nq == 96:
            check_uniform(case, params, got)


def test_four_row_small_batch_shape(capi, oracle):
    """600 queries of 768-d rows in ONE class: too many for the 3 + 8 wave shape, few enough for four rows in flight per group."""
    nq = 600
    case = Case(capi, oracle, "cos", 1500, 768, 16, 64, nq)
    params = small_mix(nq, (1, 10, 30), (0, 20, 64), (0, 7))
    got = case.params(params)
    assert case.gpu.last_params_launch() == {"launches": 1, "classes": (nq, 0, 0), "largest_expansion": 64, "spec": False}
    check(got, case.want(params), "four-row")


def _pq_case(capi, oracle, metric, n, d, S, C, M, ef, nq):
    from tests.test_gpu_quantized_indexes import make_codebook

    rng = np.random.default_rng(n + d + S)
    base = rng.standard_normal((n, d), dtype=np.float32)
    queries = rng.standard_normal((nq, d), dtype=np.float32)
    cb = make_codebook(rng, base, S, C)
    ix = capi.GpuIndex(metric, d, M=M, ef_construction=48, ef=ef, seed=5, pq_codebook=cb, num_subvectors=S)
    ix.set_add_batch(256, 16)
    ix.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    codes = ix.export_codes()
    g = ix.export_graph(with_vectors=True)
    ora = oracle.OracleIndex.from_graph(metric, g["vectors"], g, M, 48, ef, 5, oracle.SUM_WAVE64)
    ix.pq_compact()
    case = Case.__new__(Case)
    case.capi, case.metric, case.n, case.ef, case.nq, case.queries, case.oq = capi, metric, n, ef, nq, queries, queries
    case.gpu, case.ora, case.labels = ix, ora, g["labels"]
    case._dev()
    return case, cb, codes


@pytest.mark.parametrize("metric,n,d,S,C,M", [("l2sq", 3000, 128, 32, 256, 8), ("cos", 2000, 768, 96, 64, 16)])
def test_compact_pq_index_decoding_on_the_fly(capi, oracle, metric, n, d, S, C, M, monkeypatch):
    monkeypatch.delenv("LANTERN_GPU_PQ_ADC", raising=False)
    for nq in (80, 2100):
        case, _, _ = _pq_case(capi, oracle, metric, n, d, S, C, M, 40, nq)
        params = small_mix(nq)
        got = case.params(params)
        assert case.gpu.last_params_launch()["spec"] == (nq == 80)
        check(got, case.want(params), f"pqd {metric} nq={nq}")


@pytest.mark.parametrize("metric,n,d,S,C,M", [("l2sq", 3000, 128, 32, 256, 8), ("cos", 2000, 768, 96, 64, 16)])
def test_compact_pq_index_by_adc(capi, oracle, metric, n, d, S, C, M, monkeypatch):
    monkeypatch.setenv("LANTERN_GPU_PQ_ADC", "1")
    nq = 150
    case, cb, codes = _pq_case(capi, oracle, metric, n, d, S, C, M, 40, nq)
    case.ora.set_pq_view(cb, codes)
    params = small_mix(nq)
    for forced in (None, "0", "1"):  # the automatic ADC shape, the classic 8-wave walk, the 3 + 8 wave one
        if forced is None:
            monkeypatch.delenv("LANTERN_GPU_ADC_SPEC", raising=False)
        else:
            monkeypatch.setenv("LANTERN_GPU_ADC_SPEC", forced)
        got = case.params(params)
        assert case.gpu.last_params_launch()["launches"] == 3
        check(got, case.want(params), f"adc {metric} ADC_SPEC={forced}")
    monkeypatch.delenv("LANTERN_GPU_ADC_SPEC", raising=False)
    check_uniform(case, params, got)


# ------------------------------------------------------------------------------------------------
# 4. the int8 screen
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("screen", ["1", "0"])
def test_screened_index(capi, oracle, screen, monkeypatch):
    monkeypatch.setenv("LANTERN_GPU_SCREEN", screen)
    nq = 1400  # (the screen is part of the bandwidth-bound walk: more than two queries per CU in both classes)
    case = Case(capi, oracle, "l2sq", 2500, 512, 16, 64, nq)
    params = small_mix(nq, (1, 10, 40, 65, 100), (0, 64, 128), (0, 7))
    before = case.gpu.screen_stats()
    got = case.params(params)
    regime = case.gpu.last_params_launch()
    assert regime["launches"] == 2 and not regime["spec"], regime
    check(got, case.want(params), f"screen={screen}")
    after = case.gpu.screen_stats()
    if screen == "1":
        assert after[0] > before[0] and after[1] - before[1] < after[0] - before[0]  # rows were rejected on the screen copy
    else:
        assert after == before == (0, 0)


# ------------------------------------------------------------------------------------------------
# 5. edge cases
# ------------------------------------------------------------------------------------------------
def test_k_zero_rows_take_no_walk(capi, oracle):
    nq = 64
    case = Case(capi, oracle, "l2sq", 1500, 64, 8, 32, nq)
    params = [(0, 0, 0) if q % 3 == 0 else (0, 200, 5) if q % 3 == 1 else (10, 0, 0) for q in range(nq)]
    got = case.params(params, k_stride=12)
    check(got, case.want(params, 12), "k = 0")
    zero = [q for q in range(nq) if q % 3 != 2]
    assert not got[2][zero].any() and not got[3][zero].any() and not got[4][zero].any()
    assert np.all(got[0][zero] == EMPTY) and np.all(np.isinf(got[1][zero])) and not got[5][zero].any()
    assert np.all(got[0][:, 10:] == EMPTY) and np.all(np.isinf(got[1][:, 10:])) and not got[5][:, 10:].any()  # the tail of a row beyond its k
    # all of them: still answered (and handed on, by the notify form)
    lab, dist, cnt, calls, _ = case.gpu.search_batch_params_lane_notify(0, case.queries, [(0, 0, 0)] * nq, k_stride=4)
    assert sorted(j for c in calls for j in c) == list(range(nq)) and not cnt.any() and not lab.any() and np.all(np.isinf(dist))


def test_more_rows_wanted_than_the_index_has(capi, oracle):
    nq, n = 48, 90
    case = Case(capi, oracle, "l2sq", n, 32, 4, 16, nq)
    params = small_mix(nq, (5, 60, 90, 200), (0, 300), (0, 50, 95))
    got = case.params(params)
    check(got, case.want(params), "k + skip > n")
    assert got[2].max() <= n and (got[2] == 0).any()


def test_empty_index(capi, oracle):
    nq = 20
    case = Case(capi, oracle, "cos", 0, 48, 8, 64, nq)
    params = small_mix(nq)
    got = case.params(params)
    check(got, case.want(params), "empty index")
    assert case.gpu.last_params_launch()["launches"] == 3


def test_more_queries_than_workgroups(capi, oracle):
    """Four workgroups serve 900 queries: every one of them draws its next list position from the ticket, a few hundred times."""
    nq = 900
    case = Case(capi, oracle, "l2sq", 2000, 100, 8, 48, nq)
    case.gpu.set_search_shape(0, 4)
    params = small_mix(nq, (1, 10, 50, 65, 129), (0, 30, 128), (0, 7))
    got = case.params(params)
    check(got, case.want(params), "tickets")


def test_an_expansion_past_the_lds_budget_is_refused_whole_and_named(capi, oracle):
    nq = 40
    case = Case(capi, oracle, "l2sq", 500, 64, 8, 32, nq)
    params = small_mix(nq)
    params[17] = (10, 40000, 0)
    params[29] = (30000, 0, 0)
    lab, dist, slot, cnt, D, E = case._buffers(30000)
    marker = np.full(nq, 0x5A5A5A5A, dtype=np.uint32)
    cnt.upload(marker)
    regime = case.gpu.last_params_launch()
    with pytest.raises(capi.LanternGpuError, match=r"exceed the 160 KiB LDS budget of the search kernel \(params\[17\]\)"):
        case.gpu.search_batch_params_device(case.dq.ptr, case.rows.strides[0], nq, params, 30000, lab.ptr, dist.ptr, slot.ptr, cnt.ptr, D.ptr, E.ptr)
    case.hip.synchronize()
    assert case.gpu.last_params_launch() == regime  # nothing was launched ...
    assert np.array_equal(cnt.download(nq, np.uint32), marker)  # ... or written
    with pytest.raises(capi.LanternGpuError, match=r"reserved parameter word must be 0 \(params\[3\]\)"):
        P = capi.query_params(small_mix(nq))
        P["reserved"][3] = 1
        case.gpu.search_batch_params(case.queries, P)
    with pytest.raises(capi.LanternGpuError, match=r"k_stride is smaller than a query's k \(params\[1\]\)"):
        case.gpu.search_batch_params(case.queries, small_mix(nq), k_stride=9)
    # the index still answers
    check(case.params(small_mix(nq)), case.want(small_mix(nq)), "after the refusals")


# ------------------------------------------------------------------------------------------------
# 6. the other forms
# ------------------------------------------------------------------------------------------------
def test_host_lane_and_notify_forms(capi, oracle):
    nq = 200
    case = Case(capi, oracle, "l2sq", 3000, 128, 16, 64, nq)
    params = small_mix(nq, (1, 10, 65, 129), (0, 128), (0, 7, 10))
    want = case.want(params)
    for form in ("host", "lane", "notify"):
        if form == "host":
            lab, dist, cnt = case.gpu.search_batch_params(case.queries, params)
        elif form == "lane":
            lab, dist, cnt = case.gpu.search_batch_params_lane(3, case.queries, params)
        else:
            lab, dist, cnt, calls, snaps = case.gpu.search_batch_params_lane_notify(5, case.queries, params)
            handed = [j for c in calls for j in c]
            assert sorted(handed) == list(range(nq)), "every query is handed on exactly once"
            for j in range(nq):  # ... with its final rows in place when its callback runs
                assert np.array_equal(snaps[j][0], want[5][j]) and np.array_equal(snaps[j][1].view(np.uint32), want[1][j].view(np.uint32)) and snaps[j][2] == want[2][j]
        assert np.array_equal(lab, want[5]) and np.array_equal(dist.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(cnt, want[2]), form
        assert case.gpu.last_params_launch()["launches"] == 3


def test_two_lanes_concurrently(capi, oracle):
    nq = 300
    case = Case(capi, oracle, "l2sq", 3000, 128, 16, 64, nq)
    mixes = [small_mix(nq, (1, 10, 65, 129), (0, 128), (0, 7)), small_mix(nq, (129, 3, 70, 20), (200, 0), (7, 0))]
    wants = [case.want(m) for m in mixes]
    out, errors = [None, None], []

    def run(lane):
        try:
            for _ in range(4):
                out[lane] = case.gpu.search_batch_params_lane(lane, case.queries, mixes[lane])
                lab, dist, cnt = out[lane]
                assert np.array_equal(lab, wants[lane][5]) and np.array_equal(dist.view(np.uint32), wants[lane][1].view(np.uint32))
                assert np.array_equal(cnt, wants[lane][2])
        except BaseException as ex:  # noqa: BLE001
            errors.append((lane, ex))

    threads = [threading.Thread(target=run, args=(lane,)) for lane in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ------------------------------------------------------------------------------------------------
# 7. the switches, each once against the default
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,value", [("LANTERN_GPU_SPEC", "0"), ("LANTERN_GPU_SPEC", "1"), ("LANTERN_GPU_LDS_LIST", "1"), ("LANTERN_GPU_VIS_SLOTS", "0")])
def test_switches_do_not_change_an_answer(capi, oracle, name, value, monkeypatch):
    nq = 120
    params = full_mix()
    monkeypatch.delenv(name, raising=False)
    case = Case(capi, oracle, "l2sq", 3000, 128, 16, 64, nq)
    default = case.params(params)
    assert case.gpu.last_params_launch()["spec"]
    monkeypatch.setenv(name, value)
    other = Case(capi, oracle, "l2sq", 3000, 128, 16, 64, nq)  # (LANTERN_GPU_VIS_SLOTS is read when an index is made)
    got = other.params(params)
    if name != "LANTERN_GPU_VIS_SLOTS":
        assert not other.gpu.last_params_launch()["spec"]  # spec 1 has no per-query form: the classic shape, as for spec 0 and the LDS list
    check(got, default, f"{name}={value}")
    check(got, case.want(params), f"{name}={value} against the oracle")
