"""The screened descent on the device (walk.hpp greedy_descent<.., SCREEN>: a step's listed upper-level rows go through the int8 screen
at radius = the best distance when the step starts; SearchArgs::screen_descent, LANTERN_GPU_SCREEN_DESCENT is its switch, read on every
call).  Every answer is compared with the oracle on the exported graph -- ids, distance bits, D and E -- and with the same index
searched with the switch off, byte for byte; lantern_gpu_search_screen_stats must show fewer f32 row reads with the switch on.

  shapes   d = 512 (128 chunks: the smallest row that screens), 516 (a partial last screen chunk), 768 (the headline's row), 2000 (a
           partial block); 6000 rows at M = 16 (levels to 3), 2000 rows at M = 4 (a descent of five levels with short lists), 6000 rows at
           M = 64 (upper lists of more than 32 rows: a second round of screen groups); l2sq and cosine; 64 queries (four rows in flight
           per group at four waves) and 63 (two: the headline's instantiation); workgroups of 256 and 512 threads; once with two
           workgroups for the whole batch, so that a workgroup's LDS scalars cross 32 walks.
  edges    duplicated rows and queries that are rows (distances equal to the best, and 0); a non-finite and a zero row at upper-level
           slots; queries that cannot be quantised (a NaN component, all zero): they reject nothing; an index with max_level 0.
  scope    an insertion, a filtered search and a 64-query latency-bound search answer as they do with the switch off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
NQ, K, EFC, SEED = 64, 10, 64, 1
SWITCH = "LANTERN_GPU_SCREEN_DESCENT"
SHAPES = [(512, 6000, 16), (516, 6000, 16), (768, 6000, 16), (2000, 6000, 16), (516, 2000, 4), (768, 2000, 4), (768, 6000, 64)]
NAMES = ("labels", "distance bits", "slots", "counts", "D", "E")


@pytest.fixture(scope="module")
def libs():
    from lantern_amd import capi, hip
    from oracle import binding as oracle

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi, oracle, hip


class Searcher:
    """one index's device-side search: every output array of lantern_gpu_search_batch_device, downloaded"""

    def __init__(self, hip, ix, queries):
        self.hip, self.ix = hip, ix
        self.rows = ix.device_query_rows(queries)
        self.dq = hip.Buffer.from_numpy(self.rows)
        self.nq = len(queries)
        self.out = [hip.Buffer(self.nq * K * 8), hip.Buffer(self.nq * K * 4), hip.Buffer(self.nq * K * 4), hip.Buffer(self.nq * 4), hip.Buffer(self.nq * 8),
                    hip.Buffer(self.nq * 8)]

    def search(self, nq, ef=64):
        """(labels, distance bits, slots, counts, D, E) of the first nq queries, and the launch's (row evaluations, f32 row reads)"""
        for b in self.out:
            b.zero()
        st0 = self.ix.screen_stats()
        self.ix.search_batch_device(self.dq.ptr, nq, K, ef, 0, *[b.ptr for b in self.out], query_stride=self.rows.strides[0])
        self.hip.synchronize()
        st1 = self.ix.screen_stats()
        lab, dist, slot, cnt, D, E = self.out
        got = (lab.download((self.nq, K), np.uint64)[:nq], dist.download((self.nq, K), np.uint32)[:nq], slot.download((self.nq, K), np.uint32)[:nq],
               cnt.download(self.nq, np.uint32)[:nq], D.download(self.nq, np.uint64)[:nq], E.download(self.nq, np.uint64)[:nq])
        return got, (st1[0] - st0[0], st1[1] - st0[1])


def same(a, b, tag):
    for name, x, y in zip(NAMES, a, b):
        assert np.array_equal(x, y), (tag, name)


def built(capi, metric, base, M, seed=SEED):
    ix = capi.GpuIndex(metric, base.shape[1], M=M, ef_construction=EFC, ef=64, seed=seed)
    ix.set_add_batch(512, 16)
    with np.errstate(all="ignore"):
        ix.add_many(np.arange(len(base), dtype=np.uint64) + 1, base)
    ix.flush()
    assert ix.export_screen(0, 1)["row_bytes"] != 0  # the index has a screen table
    return ix


def on_and_off(monkeypatch, s, nq, tag, ef=64):
    """the launch with the switch on and off: byte-identical answers, never more f32 rows with it on.  Returns the `on` answers and
    both f32-row counts."""
    monkeypatch.setenv(SWITCH, "1")
    on, (logical_on, exact_on) = s.search(nq, ef)
    monkeypatch.setenv(SWITCH, "0")
    off, (logical_off, exact_off) = s.search(nq, ef)
    monkeypatch.delenv(SWITCH)
    same(on, off, tag)
    assert logical_on == logical_off == int(on[4].sum()), tag
    assert exact_on <= exact_off <= logical_off, (tag, exact_on, exact_off)
    return on, exact_on, exact_off


def against_oracle(got, want, nq, tag):
    o_lab, o_dist, o_slot, o_D, o_E = want
    assert np.array_equal(got[4], o_D[:nq]) and np.array_equal(got[5], o_E[:nq]), (tag, "D, E")
    assert np.array_equal(got[0], o_lab[:nq]) and np.array_equal(got[1], o_dist[:nq].view(np.uint32)) and np.array_equal(got[2], o_slot[:nq]), (tag, "ids, bits")


def run_shapes(libs, monkeypatch, ix, metric, base, M, queries, tag, reject=True):
    capi, oracle, hip = libs
    g = ix.export_graph()
    ora = oracle.OracleIndex.from_graph(metric, base, g, M, EFC, 64, SEED, oracle.SUM_WAVE64)
    with np.errstate(all="ignore"):
        want = ora.search_batch(queries, K, 64)  # once, shared by every shape below
    s = Searcher(hip, ix, queries)
    for waves, max_wg, nq in ((4, 0, NQ), (4, 0, NQ - 1), (8, 0, NQ), (4, 2, NQ)):
        ix.set_search_shape(waves, max_wg)
        t = tag + (waves, max_wg, nq)
        capi.last_search_cells()
        got, exact_on, exact_off = on_and_off(monkeypatch, s, nq, t)
        made, cells = capi.last_search_cells()
        assert made == 2 and all(c[8] == 1 and c[6] == 0 for c in cells), (t, cells)  # both launches screen, in the classic shape
        against_oracle(got, want, nq, t)
        if max_wg:
            assert ix.last_search_grid() == max_wg, t
        if reject and g["max_level"] > 0:
            assert exact_on < exact_off, (t, exact_on, exact_off)  # strictly fewer f32 rows
        print(f"{t}: f32 rows {exact_off} -> {exact_on} of {int(got[4].sum())} evaluations")
    ix.set_search_shape(0, 0)
    return g


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("d,n,M", SHAPES)
def test_the_screened_descent_answers_as_the_oracle_and_as_the_unscreened_one(libs, monkeypatch, d, n, M, metric):
    rng = np.random.default_rng(7000 + d + M)
    base = rng.standard_normal((n, d), dtype=F32)
    queries = rng.standard_normal((NQ, d), dtype=F32)
    ix = built(libs[0], metric, base, M)
    g = run_shapes(libs, monkeypatch, ix, metric, base, M, queries, (metric, d, n, M))
    assert g["max_level"] >= (3 if M == 4 else 1 if M == 64 else 2)
    if M == 64:  # an upper list of more than 32 rows: a second round of screen groups
        assert max(int((lst != 0xFFFFFFFF).sum()) for lst in g["upper_nbr"]) > 32


def upper_slots(oracle, n, M):
    lv = oracle.levels_for(SEED, 0, n, M)
    order = np.argsort(-lv, kind="stable")
    assert lv[order[2]] >= 1
    return int(order[1]), int(order[2])


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("kind", ["duplicates", "special"])
def test_ties_and_special_rows(libs, monkeypatch, kind, metric):
    capi, oracle, hip = libs
    d, n, M = 512, 2000, 4
    rng = np.random.default_rng(7100)
    base = rng.standard_normal((n, d), dtype=F32)
    queries = rng.standard_normal((NQ, d), dtype=F32)
    if kind == "duplicates":  # every row four times; half of the queries are rows
        base = np.ascontiguousarray(np.tile(base[: n // 4], (4, 1)))
        queries[: NQ // 2] = base[rng.integers(0, n, NQ // 2)]
    else:  # a non-finite row and a zero row at upper-level slots
        a, b = upper_slots(oracle, n, M)
        base[a, 3] = F32(np.inf)
        base[b] = 0
    ix = built(capi, metric, base, M)
    run_shapes(libs, monkeypatch, ix, metric, base, M, queries, (kind, metric))


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_queries_that_cannot_be_quantised_reject_nothing(libs, monkeypatch, metric):
    capi, oracle, hip = libs
    d, n, M = 768, 2000, 4
    rng = np.random.default_rng(7200)
    base = rng.standard_normal((n, d), dtype=F32)
    queries = rng.standard_normal((8, d), dtype=F32)
    queries[::2] = 0          # all zero
    queries[1::2, 5] = np.nan  # a NaN component
    ix = built(capi, metric, base, M)
    s = Searcher(hip, ix, queries)
    for waves in (4, 8):
        ix.set_search_shape(waves)
        on, exact_on, exact_off = on_and_off(monkeypatch, s, 8, (metric, waves))
        assert exact_on == exact_off == int(on[4].sum())  # nothing rejected, in the descent or in the hops


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_an_index_without_upper_levels_has_no_descent(libs, monkeypatch, metric):
    capi, oracle, hip = libs
    d, n, M = 768, 40, 16
    seed = next(s for s in range(1, 400) if oracle.levels_for(s, 0, n, M).max() == 0)
    rng = np.random.default_rng(7300)
    base = rng.standard_normal((n, d), dtype=F32)
    queries = rng.standard_normal((NQ, d), dtype=F32)
    ix = built(capi, metric, base, M, seed=seed)
    g = ix.export_graph()
    assert g["max_level"] == 0
    ora = oracle.OracleIndex.from_graph(metric, base, g, M, EFC, 64, seed, oracle.SUM_WAVE64)
    want = ora.search_batch(queries, K, 64)
    s = Searcher(hip, ix, queries)
    for waves in (4, 8):
        ix.set_search_shape(waves)
        on, exact_on, exact_off = on_and_off(monkeypatch, s, NQ, (metric, waves))
        against_oracle(on, want, NQ, (metric, waves))
        assert exact_on == exact_off


def test_the_other_walks_answer_as_before(libs, monkeypatch):
    """insertion, filtered search and the latency-bound search keep the unscreened descent: the switch changes nothing in them"""
    capi, oracle, hip = libs
    d, n, M = 768, 3000, 16
    rng = np.random.default_rng(7400)
    base = rng.standard_normal((n + 200, d), dtype=F32)
    queries = rng.standard_normal((NQ, d), dtype=F32)
    allowed = np.arange(1, n + 1, 3, dtype=np.uint64)
    res = {}
    for switch in ("1", "0"):
        monkeypatch.setenv(SWITCH, switch)
        ix = built(capi, "l2sq", base[:n], M)
        ix.add_many(np.arange(n, n + 200, dtype=np.uint64) + 1, base[n:])  # insertions into the built index
        ix.flush()
        g = ix.export_graph()
        filt = ix.filter_from_labels(allowed)
        ix.set_filter_policy("walk")
        filtered = ix.search_batch_filtered(filt, queries, K, 64)
        capi.last_search_cells()
        lone = ix.search_batch(queries, K, 64)  # 64 queries, automatic shape: the latency-bound walk
        made, cells = capi.last_search_cells()
        assert made == 1 and cells[0][6] == 2 and cells[0][8] == 0, cells  # spec 2, no screen
        res[switch] = (g, filtered, lone)
        filt.close()
    monkeypatch.delenv(SWITCH)
    g1, f1, l1 = res["1"]
    g0, f0, l0 = res["0"]
    for key in ("levels", "nbr0", "upper_off", "upper_nbr"):
        assert np.array_equal(g1[key], g0[key]), key
    assert g1["entry_slot"] == g0["entry_slot"] and g1["max_level"] == g0["max_level"]
    for x, y in zip(f1 + l1, f0 + l0):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    ora = oracle.OracleIndex.from_graph("l2sq", base, g1, M, EFC, 64, SEED, oracle.SUM_WAVE64)
    o_lab, o_dist, _, _, _ = ora.search_batch(queries, K, 64)
    assert np.array_equal(l1[0], o_lab) and np.array_equal(l1[1].view(np.uint32), o_dist.view(np.uint32))
