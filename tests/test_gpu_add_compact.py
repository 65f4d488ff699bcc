"""Adds to a COMPACT pq index under lantern_gpu_set_add_compact (include/lantern_gpu.h; DESIGN.md 4.7 "Compact pq indexes: adding"): the batch is
quantised from a staging block, the insertion kernels run over the code rows (k_insert, k_connect, k_revlink_* for M_*_PQD), the index
stays compact.  Needs an MI355X.

Arbiters: for the codes of the new rows, the float64 nearest centroid per subvector of the caller's rows where best and second best are
more than 2e-5 max(1, best) apart (at most 0.1 % of the pairs may be closer: asserted); for the graph, the oracle's index over the decoded
rows cb[codes] with the same batches and levels, edge for edge; for search distances, float64 over the decoded rows at 1e-5 max(1, |ref|)
(SURVEY 8c).  The expanded twin, continued from the same saved state, is a second equality, never the arbiter.
"""
import numpy as np
import pytest

from tests.filtered_adc_ref import make_codebook

pytestmark = pytest.mark.gpu

N0, N = 500, 760
SHAPES = {"cps1": ("l2sq", 64, 16, 64), "cps5_straddle": ("l2sq", 120, 6, 16), "cps6": ("l2sq", 96, 4, 200), "cos768": ("cos", 768, 96, 64)}
LABELS = np.arange(N, dtype=np.uint64) + 1
# way (c): assigned levels for the new rows; RAISE is one above the saved index's max_level
LEVELS = [(i % 7 == 0) + (i % 31 == 0) for i in range(N - N0)]
RAISE = 100
_SAVED = {}


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def code_row_bytes(S):
    s16 = (S + 15) // 16 * 16
    return 128 if 64 < s16 < 128 else s16


def metric64(metric, x, c):
    """float64 distances of rows x to rows c under the index metric, the cosine with its zero-norm rules"""
    xn, cn, dot = (x * x).sum(1)[:, None], (c * c).sum(1)[None, :], x @ c.T
    if metric == "l2sq":
        return np.maximum(xn + cn - 2 * dot, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((xn == 0) & (cn == 0), 0.0, np.where((xn == 0) | (cn == 0), 1.0, 1 - dot / np.sqrt(xn * cn)))


def saved(capi, name, efc):
    """the data of a shape and the buffer of its first N0 rows built expanded; make() gives an empty index of the shape"""
    if (name, efc) not in _SAVED:
        metric, d, S, C = SHAPES[name]
        rng = np.random.default_rng(N + d + S)
        base = rng.standard_normal((N, d), dtype=np.float32)
        queries = rng.standard_normal((64, d), dtype=np.float32)
        cb = make_codebook(rng, base, S, C)
        if metric == "cos":  # three all-zero rows (two of them added compact) and an all-zero centroid; zeroed after the codebook is drawn, so no second zero centroid makes a zero row's code a tie
            base[[5, N0 + 3, N - 1]] = 0
            cb[0] = 0

        def make():
            ix = capi.GpuIndex(metric, d, M=4, ef_construction=efc, ef=16, seed=5, pq_codebook=cb, num_subvectors=S)
            ix.set_add_batch(256, 16)
            return ix

        first = make()
        first.add_many(LABELS[:N0], base[:N0])
        first.flush()
        _SAVED[name, efc] = {"base": base, "queries": queries, "cb": cb, "make": make, "blob": first.save_buffer(), "top": int(first.export_graph()["levels"].max())}
    return _SAVED[name, efc]


def add_rows(ix, way, base, top, after_each=lambda: None):
    if way in ("many", "empty"):  # one call beyond the capacity: the code rows grow
        ix.add_many(LABELS[len(ix):], base[len(ix):])
        ix.flush()
        after_each()
        return
    ix.reserve(N)
    after_each()
    for i in range(N0, N):  # one row per batch; way "levels": with assigned levels
        ix.add(LABELS[i], base[i], level=None if way == "lone" else top + 1 if i - N0 == RAISE else LEVELS[i - N0])
        ix.flush()
        after_each()


@pytest.mark.parametrize("name,efc,way", [(s, 16, w) for s in SHAPES for w in ("many", "lone", "levels")] + [("cps1", 160, "many"), ("cps5_straddle", 16, "empty")])
def test_adds_from_the_code_rows_match_float64_the_oracle_and_the_expanded_twin(capi, oracle, name, efc, way):
    metric, d, S, C = SHAPES[name]
    sv = saved(capi, name, efc)
    base, queries, cb, sub = sv["base"], sv["queries"], sv["cb"], d // S
    twin, ix = sv["make"](), sv["make"]()
    if way != "empty":
        twin.load_buffer(sv["blob"])
        ix.load_buffer(sv["blob"])
    ix.pq_compact()
    ix.set_add_compact(1)

    def still_compact():
        assert ix.memory_usage()[0] == max(len(ix), 1) * code_row_bytes(S) and ix.add_compact() == 2

    still_compact()
    add_rows(twin, way, base, sv["top"])
    add_rows(ix, way, base, sv["top"], still_compact)
    assert len(ix) == N
    # ---- the codes of the rows added compact: float64 nearest centroid, where it is unambiguous
    codes, first_new = ix.export_codes(), 0 if way == "empty" else N0
    left_out = 0
    for s in range(S):
        dist = metric64(metric, base[first_new:, s * sub:(s + 1) * sub].astype(np.float64), cb[:, s * sub:(s + 1) * sub].astype(np.float64))
        order = np.argsort(dist, axis=1, kind="stable")
        best, second = np.take_along_axis(dist, order[:, :1], 1)[:, 0], np.take_along_axis(dist, order[:, 1:2], 1)[:, 0]
        clear = second - best > 2e-5 * np.maximum(1, best)
        left_out += int((~clear).sum())
        assert np.array_equal(codes[first_new:, s][clear], order[:, 0][clear]), s
    print(f"{name}: {left_out} of {(N - first_new) * S} (row, subvector) pairs closer than the gap")
    assert left_out <= 0.001 * (N - first_new) * S
    # ---- the graph: the oracle's index over the decoded rows, the same batches and levels
    dec = np.concatenate([cb[codes[:, s], s * sub:(s + 1) * sub] for s in range(S)], axis=1)
    ora = oracle.OracleIndex(metric, d, M=4, ef_construction=efc, ef=16, seed=5, sum_mode=oracle.SUM_WAVE64)
    if way in ("many", "empty"):
        for lo, hi in ([(0, N)] if way == "empty" else [(0, N0), (N0, N)]):
            ora.add_planned(LABELS[lo:hi], dec[lo:hi], 256, 16)
    else:
        ora.add_planned(LABELS[:N0], dec[:N0], 256, 16)
        for i in range(N0, N):
            ora.add(LABELS[i], dec[i], level=None if way == "lone" else sv["top"] + 1 if i - N0 == RAISE else LEVELS[i - N0])
    g, o = ix.export_graph(), ora.export_graph()
    for key in ("levels", "nbr0", "upper_off", "upper_nbr"):
        assert np.array_equal(g[key], o[key]), key
    # ---- searches on the compact index: float64 over the decoded rows
    lab, dist, cnt = ix.search_batch(queries, 10)
    ref = np.take_along_axis(metric64(metric, queries.astype(np.float64), dec.astype(np.float64)), lab.astype(np.int64) - 1, axis=1)
    assert (cnt == 10).all() and (np.abs(dist - ref) <= 1e-5 * np.maximum(1, np.abs(ref))).all()
    # ---- second equalities: the expanded twin
    tg = twin.export_graph(with_vectors=True)
    assert np.array_equal(codes, twin.export_codes()) and ix.checksum() == twin.checksum()
    for key in ("levels", "nbr0", "upper_off", "upper_nbr"):
        assert np.array_equal(g[key], tg[key]), key
    for stage in ("compact", "expanded"):  # (the cosine shape: the second round reads the norm words written while compact)
        tlab, tdist, _ = twin.search_batch(queries, 10)
        lab, dist, _ = ix.search_batch(queries, 10)
        assert np.array_equal(lab, tlab) and np.array_equal(dist.view(np.uint32), tdist.view(np.uint32)), stage
        still_compact() if stage == "compact" else None
        ix.pq_expand()
    assert ix.export_graph(with_vectors=True)["vectors"].tobytes() == tg["vectors"].tobytes()


def test_rows_that_cannot_be_decoded_on_the_fly_expand_as_before(capi):
    rng = np.random.default_rng(3)
    base = rng.standard_normal((400, 96), dtype=np.float32)
    cb = make_codebook(rng, base, 16, 32)  # subvectors of 6 dimensions are not whole 16-byte chunks: pqd_inv = 0
    make = lambda: capi.GpuIndex("l2sq", 96, M=4, ef_construction=16, ef=16, seed=5, pq_codebook=cb, num_subvectors=16)
    twin, ix = make(), make()
    twin.add_many(LABELS[:300], base[:300])
    twin.flush()
    ix.load_buffer(twin.save_buffer())
    ix.pq_compact()
    ix.set_add_compact(1)
    assert ix.add_compact() == 1 and ix.memory_usage()[0] == 300 * 16 and twin.add_compact() == 0
    for t in (twin, ix):
        t.add_many(LABELS[300:400], base[300:])
        t.flush()
    assert ix.memory_usage()[0] >= 400 * 96 * 4 and ix.add_compact() == 1  # the add expanded it
    assert np.array_equal(ix.export_codes(), twin.export_codes()) and ix.checksum() == twin.checksum()
    got, want = ix.search_batch(base[:20], 5), twin.search_batch(base[:20], 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
