"""The screened hop at the edges of its row blocks (walk.hpp hop_distances_screened: a lane requests LGPU_SCREEN_NB uint4 of an int8
row before it consumes the first -- blocks of 24 screen chunks per row at NB = 3, the default, and of 48 at NB = 6, the whole 768-d
row) and with the front's neighbour list requested one hop ahead (search_level_reg, SearchArgs::list_prefetch;
LANTERN_GPU_SCREEN_LIST_PREFETCH is its switch, read on every call).  Every comparison is with the oracle or with the same graph
searched without a screen, never with this library's other settings alone.

  block edges  d = 512 .. 2000: 32, 48, 48, 49, 96, 97 and 125 screen chunks -- in blocks of 48: a partial single block, the exact block
               (764: with a partial last f32 chunk), one chunk into the second block, exactly two, two plus one, and the cap; in blocks
               of 24: a partial second block, exactly two, one chunk into the third, exactly four, four plus one, five plus five.  l2sq and cosine, ef 64
               (one key per lane) and 128 (two), workgroups of 256 and 512 threads, batches of 64 (four rows in flight per group: the
               small-batch instantiation) and 63 queries (two: the headline's).
  verdicts     the probe's reject vector over hops of 1, 31, 32, 33 and 64 slots against the host restatement of the test.
  prefetch     a 600-row index (the next node is mostly NOT the front) and a 3000-row clustered one (it mostly is), batches of 1, 7
               and 40 queries, the switch on and off.

Why 2 e: the device and the restatement differ by the order of a sum and the last place of a norm -- under 259 u relative on the l2sq
bound, 2^-21 absolute on the cosine one (tests/test_gpu_screen_rows.py T7), both below e = max(2^-12, (2 chunks + 64) 2^-24): a slot
whose restated bound is at least 2 e from the radius has one verdict."""
import numpy as np
import pytest

from tests import test_gpu_screen_rows as stored
from tests import test_screen_bound_cos as cs

pytestmark = pytest.mark.gpu

F32 = np.float32
N, NQ, K, M, EFC = 3000, 64, 10, 16, 64
DIMS = (512, 764, 768, 772, 1536, 1540, 2000)
SCREEN_CHUNKS = {512: 32, 764: 48, 768: 48, 772: 49, 1536: 96, 1540: 97, 2000: 125}
SWITCH = "LANTERN_GPU_SCREEN_LIST_PREFETCH"


@pytest.fixture(scope="module")
def libs():
    from lantern_amd import capi, hip
    from oracle import binding as oracle

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi, oracle, hip


def test_the_dimensions_sit_on_the_block_edges():
    for d, sch in SCREEN_CHUNKS.items():
        assert ((d + 3) // 4 + 3) // 4 == sch
    assert sorted(SCREEN_CHUNKS) == sorted(DIMS)
    assert [-(-s // 48) for s in SCREEN_CHUNKS.values()] == [1, 1, 1, 2, 2, 3, 3] and 125 % 48 != 0 and 32 % 48 != 0
    assert [-(-s // 24) for s in SCREEN_CHUNKS.values()] == [2, 2, 2, 3, 4, 5, 6] and [s % 24 for s in SCREEN_CHUNKS.values()] == [8, 0, 0, 1, 0, 1, 5]


class Searcher:
    """one index's device-side search: every output array of lantern_gpu_search_batch_device, downloaded"""

    def __init__(self, hip, ix, queries):
        self.hip, self.ix = hip, ix
        self.rows = ix.device_query_rows(queries)
        self.dq = hip.Buffer.from_numpy(self.rows)
        self.nq = len(queries)
        self.out = [hip.Buffer(self.nq * K * 8), hip.Buffer(self.nq * K * 4), hip.Buffer(self.nq * K * 4), hip.Buffer(self.nq * 4), hip.Buffer(self.nq * 8),
                    hip.Buffer(self.nq * 8)]

    def search(self, nq, ef):
        """(labels, distance bits, slots, counts, D, E) of the first nq queries"""
        for b in self.out:
            b.zero()
        self.ix.search_batch_device(self.dq.ptr, nq, K, ef, 0, *[b.ptr for b in self.out], query_stride=self.rows.strides[0])
        self.hip.synchronize()
        lab, dist, slot, cnt, D, E = self.out
        return (lab.download((self.nq, K), np.uint64)[:nq], dist.download((self.nq, K), np.uint32)[:nq], slot.download((self.nq, K), np.uint32)[:nq],
                cnt.download(self.nq, np.uint32)[:nq], D.download(self.nq, np.uint64)[:nq], E.download(self.nq, np.uint64)[:nq])


NAMES = ("labels", "distance bits", "slots", "counts", "D", "E")


def same(a, b, tag):
    for name, x, y in zip(NAMES, a, b):
        assert np.array_equal(x, y), (tag, name)


def pair(capi, monkeypatch, metric, d, base, M_=M, efc=EFC):
    """the index built with the screen, and its graph imported into an index made without one (LANTERN_GPU_SCREEN is read when an
    index is made)"""
    monkeypatch.delenv("LANTERN_GPU_SCREEN", raising=False)
    on = capi.GpuIndex(metric, d, M=M_, ef_construction=efc, ef=64, seed=1)
    on.set_add_batch(512, 16)
    on.add_many(np.arange(len(base), dtype=np.uint64) + 1, base)
    on.flush()
    g = on.export_graph()
    monkeypatch.setenv("LANTERN_GPU_SCREEN", "0")
    off = capi.GpuIndex(metric, d, M=M_, ef_construction=efc, ef=64, seed=1)
    off.import_graph(base, g)
    monkeypatch.delenv("LANTERN_GPU_SCREEN")
    assert on.export_screen(0, 1)["row_bytes"] == ((d + 3) // 4 + 3) // 4 * 16 and off.export_screen(0, 1)["row_bytes"] == 0
    return on, off, g


# ---- block edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("d", DIMS)
def test_block_edges_screen_on_equals_screen_off_and_the_oracle(libs, monkeypatch, d, metric):
    capi, oracle, hip = libs
    monkeypatch.delenv(SWITCH, raising=False)
    rng = np.random.default_rng(5000 + d)
    base = rng.standard_normal((N, d), dtype=np.float32)
    queries = rng.standard_normal((NQ, d), dtype=np.float32)
    on, off, g = pair(capi, monkeypatch, metric, d, base)
    ora = oracle.OracleIndex.from_graph(metric, base, g, M, EFC, 64, 1, oracle.SUM_WAVE64)
    s_on, s_off = Searcher(hip, on, queries), Searcher(hip, off, queries)
    for ef in (64, 128):
        o_lab, o_dist, o_slot, o_D, o_E = ora.search_batch(queries, K, ef)  # once per ef, shared by every shape below
        for waves in (4, 8):  # workgroups of 256 and 512 threads: the classic walk, which the screen serves
            on.set_search_shape(waves)
            off.set_search_shape(waves)
            for nq in (NQ, NQ - 1):  # four and two rows in flight per group
                tag = (metric, d, ef, waves, nq)
                st0 = on.screen_stats()
                got = s_on.search(nq, ef)
                st1 = on.screen_stats()
                same(got, s_off.search(nq, ef), tag)
                assert np.array_equal(got[4], o_D[:nq]) and np.array_equal(got[5], o_E[:nq]), tag
                assert np.array_equal(got[0], o_lab[:nq]) and np.array_equal(got[1], o_dist[:nq].view(np.uint32)) and np.array_equal(got[2], o_slot[:nq]), tag
                logical, exact = st1[0] - st0[0], st1[1] - st0[1]
                assert logical == int(o_D[:nq].sum()), tag
                assert 0 < exact < logical, (tag, logical, exact)  # the screen ran, and rejected rows
                assert off.screen_stats() == (0, 0)


# ---- verdicts -----------------------------------------------------------------------------------------------------------------------
def edge_band(c, x, i, ra, radius):
    """the restated bound of row i is within 2 e of the radius (module docstring)"""
    b = c.host_bound(x, i, ra)[0]
    e = float(c.e)
    return b * (1 - 2 * e) <= radius <= b * (1 + 2 * e) if c.metric == "l2sq" else abs(radius - b) <= 2 * e


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("d", [768, 772, 2000])
def test_verdicts_at_the_block_edges_are_the_restatement_s(libs, d, metric):
    c = stored.case(libs[0], metric, d)
    gs = c.family("gaussian")
    assert len(gs) == 64
    x = stored.gaussian_queries(d, 1)[0]  # (a fixed seed: 7 d)
    ra = cs.rooted_norm(x) if metric == "cos" else None
    radius = F32(np.median([c.host_bound(x, i, ra)[0] for i in gs]))
    close = {i for i in gs if edge_band(c, x, i, ra, float(radius))}
    assert len(close) <= 4, (len(close), "the restatement alone leaves out more than 4 of 64 slots at this seed")  # (host arithmetic)
    want = {i: bool(c.host_rejects(x, i, radius, ra)) for i in gs}
    assert 16 <= sum(want.values()) <= 48, sum(want.values())
    rng = np.random.default_rng(d)
    for n in (1, 31, 32, 33, 64):
        for wg in (256, 512):
            perm = [gs[j] for j in rng.permutation(64)]
            rows = perm[: n - 1] + [perm[0]] if n > 1 else perm[:1]  # (n > 1: the first slot is there twice)
            got = c.probe(x, rows, radius, wg)
            assert len(got) == n
            for pos, (i, g_) in enumerate(zip(rows, got)):
                if i not in close:
                    assert bool(g_) == want[i], (n, wg, pos, i, "rejects" if g_ else "keeps", c.host_bound(x, i, ra)[0], float(radius))
            if n > 1:
                assert got[0] == got[n - 1], (n, wg, "one slot, two verdicts")


# ---- prefetch -----------------------------------------------------------------------------------------------------------------------
def prefetch_data(kind, d):
    rng = np.random.default_rng(77)
    if kind == "small":  # 600 Gaussian rows: the next node is the front in about half of the hops
        return rng.standard_normal((600, d), dtype=np.float32), rng.standard_normal((40, d), dtype=np.float32)
    centres = rng.standard_normal((16, d), dtype=np.float32) * 4  # 3000 clustered rows: it mostly is
    base = (centres[rng.integers(0, 16, N)] + rng.standard_normal((N, d), dtype=np.float32) * 0.5).astype(np.float32)
    queries = (centres[rng.integers(0, 16, 40)] + rng.standard_normal((40, d), dtype=np.float32) * 0.5).astype(np.float32)
    return base, queries


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("kind", ["small", "clustered"])
def test_list_prefetch_on_and_off_equal_each_other_and_the_oracle(libs, monkeypatch, kind, metric):
    capi, oracle, hip = libs
    d = 768
    base, queries = prefetch_data(kind, d)
    on, off, g = pair(capi, monkeypatch, metric, d, base)
    ora = oracle.OracleIndex.from_graph(metric, base, g, M, EFC, 64, 1, oracle.SUM_WAVE64)
    s_on, s_off = Searcher(hip, on, queries), Searcher(hip, off, queries)
    in_ = dict.fromkeys(capi.PLAN_SEARCH_IN, 0)
    in_.update(chunks=d // 4, M=M, M0=2 * M, mcode=3 if metric == "l2sq" else 1, n=len(base), ef_default=64, num_cus=256, search_vis_slots=-1, k=K,
               env_wide_rows=-1, waves=4, screen=1)
    for ef in (64, 128):
        o_lab, o_dist, o_slot, o_D, o_E = ora.search_batch(queries, K, ef)
        for waves in (4, 8):
            on.set_search_shape(waves)
            off.set_search_shape(waves)
            for nq in (1, 7, 40):
                want = (o_lab[:nq], o_dist[:nq].view(np.uint32), o_slot[:nq], None, o_D[:nq], o_E[:nq])
                unscreened = s_off.search(nq, ef)
                for switch in ("1", "0"):
                    monkeypatch.setenv(SWITCH, switch)
                    # (what the launch below is planned as: it screens, and fetches ahead iff the switch says so)
                    p = capi.plan_search(dict(in_, nq=nq, ef=ef, waves=waves, screen_list_prefetch=int(switch)))[0]
                    assert p["screen_lds"] != 0 and p["list_prefetch"] == int(switch)
                    tag = (kind, metric, ef, waves, nq, "prefetch " + switch)
                    st0 = on.screen_stats()
                    got = s_on.search(nq, ef)
                    st1 = on.screen_stats()
                    same(got, unscreened, tag)
                    for name, x, y in zip(NAMES, got, want):
                        assert y is None or np.array_equal(x, y), (tag, name, "oracle")
                    assert st1[0] - st0[0] == int(o_D[:nq].sum()) and 0 < st1[1] - st0[1] <= st1[0] - st0[0], tag
                monkeypatch.delenv(SWITCH)
