"""Filtered search on the device (include/lantern_gpu.h "Filtered search").  Needs an MI355X.

Graphs are built by the oracle and imported (as test_gpu_parity.py does), so the CPU restatement of tests/filtered_walk_ref.py
walks the very graph the kernel walks; distances are compared bit for bit.
"""
import numpy as np
import pytest

from lantern_amd import synth
from tests import filtered_walk_ref as ref

pytestmark = pytest.mark.gpu

CASES = [  # test_gpu_parity.py::CASES -- metric, n, d, M, efc, ef, k
    ("l2sq", 3000, 128, 16, 64, 64, 10),
    ("cos", 2000, 768, 16, 64, 64, 10),
    ("l2sq", 1500, 100, 8, 40, 32, 5),
    ("l2sq", 800, 3, 2, 10, 4, 1),
    ("hamming", 3000, 24, 16, 64, 64, 10),
    ("cos", 600, 1536, 16, 32, 128, 10),
]
NQ = 64


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def rows(rng, n, d, metric):
    if metric == "hamming":
        return rng.integers(0, 2**32, size=(n, d), dtype=np.uint32)
    return rng.standard_normal((n, d), dtype=np.float32)


class Dev:
    """device buffers for nq x k answers of one index"""

    def __init__(self, gpu, queries, k):
        from lantern_amd import hip

        self.hip, self.gpu, self.k = hip, gpu, k
        self.rows = gpu.device_query_rows(queries)
        self.nq = self.rows.shape[0]
        self.dq = hip.Buffer.from_numpy(self.rows)
        nq = self.nq
        self.lab, self.dist, self.slot = hip.Buffer(nq * k * 8), hip.Buffer(nq * k * 4), hip.Buffer(nq * k * 4)
        self.cnt, self.D, self.E = hip.Buffer(nq * 4), hip.Buffer(nq * 8), hip.Buffer(nq * 8)

    def _out(self):
        self.hip.synchronize()
        nq, k = self.nq, self.k
        return (self.slot.download((nq, k), np.uint32), self.dist.download((nq, k), np.float32), self.cnt.download(nq, np.uint32),
                self.D.download(nq, np.uint64), self.E.download(nq, np.uint64), self.lab.download((nq, k), np.uint64))

    def plain(self, ef=0):
        self.gpu.search_batch_device(self.dq.ptr, self.nq, self.k, ef, 0, self.lab.ptr, self.dist.ptr, self.slot.ptr, self.cnt.ptr, self.D.ptr,
                                     self.E.ptr, query_stride=self.rows.strides[0])
        return self._out()

    def filtered(self, filt, ef=0, skip=0):
        self.gpu.search_batch_filtered_device(filt, self.dq.ptr, self.rows.strides[0], self.nq, self.k, ef, skip, self.lab.ptr, self.dist.ptr,
                                              self.slot.ptr, self.cnt.ptr, self.D.ptr, self.E.ptr)
        return self._out()


def same(a, b):
    sa, da, ca, Da, Ea = a[:5]
    sb, db, cb, Db, Eb = b[:5]
    assert np.array_equal(sa, sb), "slots differ"
    assert np.array_equal(da.view(np.uint32), db.view(np.uint32)), "distance bits differ"
    assert np.array_equal(ca, cb), "counts differ"
    assert np.array_equal(Da, Db), "D differs"
    assert np.array_equal(Ea, Eb), "E differs"


def oracle_index(capi, oracle, metric, n, d, M, efc, ef, seed):
    rng = np.random.default_rng(n + d)
    base, queries = rows(rng, n, d, metric), rows(rng, NQ, d, metric)
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=ef, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    gpu = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=ef, seed=9)
    gpu.import_graph(base, g)
    return base, queries, g, gpu


def all_allowed(gpu, n):
    return gpu.filter_from_bitmap(np.ones(n, dtype=bool))


# ------------------------------------------------------------------------------------------------
# all-allowed: the walk path IS the unfiltered search
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,n,d,M,efc,ef,k", CASES)
def test_all_allowed_walk_equals_unfiltered_search(capi, oracle, metric, n, d, M, efc, ef, k):
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    f = all_allowed(gpu, n)
    assert f.count == n
    gpu.set_filter_policy("walk")
    dev = Dev(gpu, queries, k)
    same(dev.filtered(f), dev.plain())
    gpu.set_filter_policy("walk", cand_cap=max(ef, k))  # C = expansion
    same(dev.filtered(f), dev.plain())


def test_all_allowed_walk_over_ef(capi, oracle):
    base, queries, g, gpu = oracle_index(capi, oracle, "l2sq", 3000, 128, 16, 64, 64, 9)
    f = all_allowed(gpu, 3000)
    gpu.set_filter_policy("walk")
    dev = Dev(gpu, queries, 10)
    for ef in (10, 64, 128, 400):
        same(dev.filtered(f, ef=ef), dev.plain(ef=ef))


@pytest.mark.parametrize("storage", ["f16", "i8", "b1"])
def test_all_allowed_walk_storage_kinds(capi, storage):
    rng = np.random.default_rng(21)
    n, d, k = 2500, 96, 10
    base = rng.standard_normal((n, d), dtype=np.float32)
    queries = rng.standard_normal((NQ, d), dtype=np.float32)
    if storage == "i8":
        base, queries = base * np.float32(0.4), queries * np.float32(0.4)
    gpu = capi.GpuIndex("l2sq", d, M=16, ef_construction=64, ef=64, seed=4, quantization=storage)
    gpu.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    gpu.flush()
    f = all_allowed(gpu, n)
    gpu.set_filter_policy("walk")
    dev = Dev(gpu, queries, k)
    same(dev.filtered(f), dev.plain())


# ------------------------------------------------------------------------------------------------
# selective filters: the walk path against the CPU restatement, the exact path against brute force
# ------------------------------------------------------------------------------------------------
def test_selective_walk_matches_restatement(capi, oracle):
    n, d, M, efc, ef, k = 3000, 128, 16, 64, 64, 10
    base, queries, g, gpu = oracle_index(capi, oracle, "l2sq", n, d, M, efc, ef, 9)
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64)
    rng = np.random.default_rng(1)
    dev = Dev(gpu, queries, k)
    for sel in (0.5, 0.1, 0.01):
        allowed = rng.random(n) < sel
        f = gpu.filter_from_labels(np.flatnonzero(allowed).astype(np.uint64) + 1)
        assert f.count == allowed.sum()
        for cap in (0, ef):  # the default cap, and C = expansion (drops happen)
            gpu.set_filter_policy("walk", cand_cap=cap)
            got = dev.filtered(f)
            want = ref.search(g, dist, allowed, M, k, ef, cand_cap=cap or None)
            same(got, want)
            s, _, c = got[0], got[1], got[2]
            for q in range(dev.nq):
                assert allowed[s[q, : c[q]]].all()
                assert np.all(got[5][q, c[q]:] == 0)


def test_cluster_correlated_walk_matches_restatement(capi, oracle):
    n, d, M, efc, ef, k = 4000, 64, 16, 64, 64, 10
    base = synth.base_rows("clustered", n, d)
    cluster = np.random.default_rng(synth.BASE_SEED).integers(0, synth.CLUSTERS, n)  # the draw base_rows makes first
    qrng_seed = 99
    qall = synth.query_maker("clustered", d)(np.random.default_rng(qrng_seed), 4 * NQ)
    qcl = np.random.default_rng(qrng_seed).integers(0, synth.CLUSTERS, 4 * NQ)
    queries = qall[qcl != 0][:NQ]  # queries from the other clusters
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=efc, ef=ef, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    gpu = capi.GpuIndex("l2sq", d, M=M, ef_construction=efc, ef=ef, seed=9)
    gpu.import_graph(base, g)
    allowed = cluster == 0
    f = gpu.filter_from_bitmap(allowed)
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64)
    dev = Dev(gpu, queries, k)
    for cap in (0, ef):
        gpu.set_filter_policy("walk", cand_cap=cap)
        same(dev.filtered(f), ref.search(g, dist, allowed, M, k, ef, cand_cap=cap or None))


@pytest.mark.parametrize("metric", ["l2sq", "cos", "hamming"])
def test_exact_path_is_bruteforce_over_allowed_rows(capi, oracle, metric):
    n, d, M, efc, ef, k = 2000, 48, 16, 64, 64, 10
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    gpu.set_filter_policy("exact")
    rng = np.random.default_rng(2)
    dev = Dev(gpu, queries, k)
    for sel in (0.3, 0.02, 0.003):
        allowed = rng.random(n) < sel
        idx = np.flatnonzero(allowed)
        f = gpu.filter_from_bitmap(allowed)
        for skip in (0, 3):
            s, dd, c, D, E, lab = dev.filtered(f, skip=skip)
            kk = max(0, min(k, idx.size - skip))
            if kk:
                t_ids, t_d = oracle.bruteforce(base[idx], queries, kk + skip, metric, sum_mode=oracle.SUM_WAVE64)
                assert np.array_equal(s[:, :kk], idx[t_ids[:, skip:]].astype(np.uint32))
                assert np.array_equal(dd[:, :kk].view(np.uint32), t_d[:, skip:].view(np.uint32))
            assert np.all(c == kk) and np.all(D == idx.size) and np.all(E == 0)
            assert np.all(s[:, kk:] == ref.EMPTY) and np.all(np.isinf(dd[:, kk:])) and np.all(lab[:, kk:] == 0)


def test_auto_path_follows_the_rule(capi, oracle):
    n, ef = 3000, 64
    base, queries, g, gpu = oracle_index(capi, oracle, "l2sq", n, 128, 16, 64, ef, 9)
    factor = 0.5
    gpu.set_filter_policy("auto", exact_factor=factor)
    rng = np.random.default_rng(3)
    for sel in (0.5, 0.1, 0.01, 0.002):
        f = gpu.filter_from_bitmap(rng.random(n) < sel)
        before = gpu.filter_stats()
        gpu.search_batch_filtered(f, queries[:8], 10)
        after = gpu.filter_stats()
        exact = f.count ** 2 <= factor * ef * n
        assert after["exact"] - before["exact"] == (1 if exact else 0), (f.count, before, after)
        assert after["walk"] - before["walk"] == (0 if exact else 1)
    empty = gpu.filter_from_bitmap(np.zeros(n, dtype=bool))
    before = gpu.filter_stats()
    lab, dist, cnt = gpu.search_batch_filtered(empty, queries[:4], 10)
    assert gpu.filter_stats() == before  # no launch
    assert np.all(lab == 0) and np.all(np.isinf(dist)) and np.all(cnt == 0)


# ------------------------------------------------------------------------------------------------
# labels, deleted rows, streaming, the scan
# ------------------------------------------------------------------------------------------------
def test_skip_deleted(capi, oracle):
    n, d, M, efc, ef, k = 2000, 32, 16, 64, 64, 10
    rng = np.random.default_rng(4)
    base, queries = rows(rng, n, d, "l2sq"), rows(rng, 16, d, "l2sq")
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=efc, ef=ef, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    g = ora.export_graph()
    dead = rng.random(n) < 0.6
    g["labels"] = np.where(dead, 0, g["labels"]).astype(np.uint64)
    gpu = capi.GpuIndex("l2sq", d, M=M, ef_construction=efc, ef=ef, seed=9)
    gpu.import_graph(base, g)
    for path in ("walk", "exact"):
        gpu.set_filter_policy(path)
        f = gpu.filter_from_bitmap(np.ones(n, dtype=bool), skip_deleted=True)
        assert f.count == (~dead).sum()
        lab, dist, cnt = gpu.search_batch_filtered(f, queries, k)
        assert np.all(lab != 0) and np.all(cnt == k)
        f2 = gpu.filter_from_labels(g["labels"], skip_deleted=True)  # label 0 in the set, and still refused
        lab2, _, _ = gpu.search_batch_filtered(f2, queries, k)
        assert np.array_equal(lab, lab2)


def test_cursor_pages_join_to_one_search(capi, oracle):
    n, ef, k = 3000, 64, 10
    base, queries, g, gpu = oracle_index(capi, oracle, "l2sq", n, 128, 16, 64, ef, 9)
    rng = np.random.default_rng(5)
    allowed = rng.random(n) < 0.2
    f = gpu.filter_from_bitmap(allowed)
    for path in ("walk", "exact"):
        gpu.set_filter_policy(path)
        cur = gpu.cursor()
        for q in queries[:4]:
            pages = [cur.search_filtered(f, q, k, ef=ef, streaming=i > 0) for i in range(5)]
            labels = np.concatenate([p[0] for p in pages])
            dists = np.concatenate([p[1] for p in pages])
            assert len(set(labels.tolist())) == labels.size == 5 * k
            one_l, one_d, _ = gpu.search_batch_filtered(f, q[None, :], 5 * k, ef=ef)
            assert np.array_equal(labels, one_l[0]) and np.array_equal(dists.view(np.uint32), one_d[0].view(np.uint32))
            assert allowed[labels.astype(np.int64) - 1].all()
        cur.close()


def test_filtered_scan_returns_limit_rows_where_post_filtering_cannot(capi):
    n, d = 20000, 32
    base = synth.base_rows("clustered", n, d)
    cluster = np.random.default_rng(synth.BASE_SEED).integers(0, synth.CLUSTERS, n)
    members = np.flatnonzero(cluster == 0)
    allowed_slots = np.sort(np.random.default_rng(6).choice(members, n // 50, replace=False))  # 2 %
    qrng = np.random.default_rng(7)
    qall = synth.query_maker("clustered", d)(qrng, 32)
    qcl = np.random.default_rng(7).integers(0, synth.CLUSTERS, 32)
    query = qall[np.flatnonzero(qcl != 0)[0]]
    gpu = capi.GpuIndex("l2sq", d, M=16, ef_construction=64, ef=64, seed=1)
    gpu.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    gpu.flush()
    allowed_labels = set((allowed_slots + 1).tolist())
    plain = capi.Scan(gpu, init_k=10)
    plain.rescan(query)
    got = [l for l in plain.fetch(5000) if l in allowed_labels]
    plain.end()
    assert len(got) < 50
    f = gpu.filter_from_labels(np.array(sorted(allowed_labels), dtype=np.uint64)[::-1])  # any order
    assert f.count == allowed_slots.size
    scan = capi.Scan(gpu, init_k=10)
    scan.set_filter(f)
    scan.rescan(query)
    rows_ = scan.fetch(50)
    scan.end()
    assert len(rows_) == 50 and all(l in allowed_labels for l in rows_)
    d_ = gpu.distance_gather(query, np.array(rows_, dtype=np.uint32) - 1)
    assert np.all(np.diff(d_) >= 0)


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_refusals(capi, oracle):
    n = 1500
    base, queries, g, gpu = oracle_index(capi, oracle, "l2sq", n, 100, 8, 40, 32, 9)
    f = all_allowed(gpu, n)
    with pytest.raises(capi.LanternGpuError, match="slot bitmap has 3 words"):
        gpu.filter_from_bitmap(np.ones(3, dtype=np.uint32))
    with pytest.raises(capi.LanternGpuError, match="filter path must be"):
        gpu.set_filter_policy(5)
    other = capi.GpuIndex("l2sq", 100, M=8, ef_construction=40, ef=32, seed=9)
    other.import_graph(base, g)
    with pytest.raises(capi.LanternGpuError, match="another index"):
        other.search_batch_filtered(f, queries[:2], 10)
    gpu.set_filter_policy("walk")
    with pytest.raises(capi.LanternGpuError, match="LDS budget"):
        gpu.search_batch_filtered(f, queries[:2], 10, ef=20000)
    gpu.set_filter_policy("exact")
    with pytest.raises(capi.LanternGpuError, match="LDS budget"):
        gpu.search_batch_filtered(f, queries[:2], 12000)
    gpu.set_filter_policy("auto")
    gpu.add(10**6, base[0] * np.float32(0.5))
    with pytest.raises(capi.LanternGpuError, match="stale filter: built when the index held 1500 rows, it now holds 1501"):
        gpu.search_batch_filtered(f, queries[:2], 10)
    # a compact pq index
    rng = np.random.default_rng(8)
    pn, pd, S, C = 1000, 64, 8, 32
    pbase = rng.standard_normal((pn, pd), dtype=np.float32)
    cb = np.zeros((C, pd), dtype=np.float32)
    for s in range(S):
        cb[:, s * 8:(s + 1) * 8] = pbase[rng.choice(pn, size=C, replace=False), s * 8:(s + 1) * 8]
    pq = capi.GpuIndex("l2sq", pd, M=8, ef_construction=48, ef=40, seed=3, pq_codebook=cb, num_subvectors=S)
    pq.add_many(np.arange(pn, dtype=np.uint64) + 1, pbase)
    pq.flush()
    pf = all_allowed(pq, pn)
    lab, _, cnt = pq.search_batch_filtered(pf, pbase[:4], 10)  # expanded: served
    assert np.all(cnt == 10)
    pq.pq_compact()
    with pytest.raises(capi.LanternGpuError, match="expand it first"):
        pq.search_batch_filtered(pf, pbase[:4], 10)
