"""k_pq_encode (lantern_amd/csrc/pq_encode.hip; DESIGN.md 4.7 "Encoding in one launch"): all code bytes of a block of rows in one launch.
Needs an MI355X.

Arbiters: the float64 nearest centroid per (row, subvector), first minimum, where best and second best are more than the distance
tolerance 1e-5 max(1, |best|) apart (at most 1 % of the pairs may be closer: asserted on the reference alone), and float64 distances at
that tolerance.  Second equality, bit for bit: today's path, lantern_gpu_assign_to_clusters per subvector.  Under cosine the two
subnormal-scale rows are compared with today's path only: their squared norms underflow in f32, so the device applies the zero-norm
rules where float64 still sees a direction.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (dims, S, C): the smallest; subdim 3, unaligned and padded; SC 2, strips of whole lines; subdim 20, SC 5; SC 8, the top; subdim 36, not
# served: the passes; S = 128, the compact form's limit; S = 5 at strips of 4: a last strip of one subvector
SHAPES = [(4, 1, 1), (12, 4, 10), (64, 8, 256), (100, 5, 255), (128, 4, 256), (144, 4, 16), (1024, 128, 256), (40, 5, 16)]
ROWS = 257  # two blocks of 256 rows
ZERO, TINY, DUP = 2, (5, 6), 7  # an all-zero row; rows at subnormal scale; a row that IS centroid 1 == centroid 3
_REF = {}


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def metric64(metric, x, c):
    """float64 distances of rows x to rows c, the cosine with its zero-norm rules"""
    xn, cn, dot = (x * x).sum(1)[:, None], (c * c).sum(1)[None, :], x @ c.T
    if metric == "l2sq":
        return ((x[:, None, :] - c[None, :, :]) ** 2).sum(2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((xn == 0) & (cn == 0), 0.0, np.where((xn == 0) | (cn == 0), 1.0, 1 - dot / np.sqrt(xn * cn)))


def reference(metric, shape, rows=ROWS):
    """data of a shape and its float64 answer: rows, codebook, codes64[n][S], dist64[n][S], clear[n][S] -- computed once"""
    if (metric, shape, rows) not in _REF:
        d, S, C = shape
        sub = d // S
        rng = np.random.default_rng(7 + d + S + C)
        X, cb = rng.standard_normal((rows, d), dtype=np.float32), rng.standard_normal((C, d), dtype=np.float32)
        if C >= 4:
            cb[2] = 0        # an all-zero centroid
            cb[3] = cb[1]    # exact ties: the lower index wins
            X[DUP] = cb[1]
        X[ZERO] = 0
        X[TINY[0]] *= np.float32(1e-41)
        X[TINY[1]] *= np.float32(1e-20)
        codes, dist, clear = np.zeros((rows, S), np.int64), np.zeros((rows, S)), np.ones((rows, S), bool)
        for s in range(S):
            dd = metric64(metric, X[:, s * sub:(s + 1) * sub].astype(np.float64), cb[:, s * sub:(s + 1) * sub].astype(np.float64))
            order = np.argsort(dd, axis=1, kind="stable")
            codes[:, s], dist[:, s] = order[:, 0], np.take_along_axis(dd, order[:, :1], 1)[:, 0]
            if C > 1:  # the gap to the next DISTINCT centroid: the copy gets the original's bits from any arithmetic, so that tie is not a doubt
                rest = np.sort(np.delete(dd, 3, axis=1) if C >= 4 else dd, axis=1)
                clear[:, s] = rest[:, 1] - dist[:, s] > 1e-5 * np.maximum(1, np.abs(dist[:, s]))
        assert (~clear).sum() <= 0.01 * clear.size, (metric, shape, int((~clear).sum()))
        _REF[metric, shape, rows] = (X, cb, codes, dist, clear)
    return _REF[metric, shape, rows]


def todays_path(capi, metric, shape, X, cb):
    d, S, _ = shape
    sub = d // S
    got = [capi.assign_to_clusters(X, cb[:, s * sub:(s + 1) * sub], metric, s * sub, sub) for s in range(S)]
    return np.stack([g[0] for g in got], 1), np.stack([g[1] for g in got], 1)


def check(capi, metric, shape, n, X, cb, codes64, dist64, clear, old):
    d, S, C = shape
    codes, dist = capi.pq_encode(X[:n], cb, S, metric)
    rec, served, pieces = capi.last_pq_encode(), capi.plan_pq_encode(metric, d, S, C)["served"], (n + 65535) // 65536
    assert served == (d // S <= 32)
    assert rec == {"pieces": pieces, "fused": pieces if served else 0, "passes": 0 if served else S * pieces, "rows": n}
    f64 = np.ones(n, bool)
    if metric == "cos":
        f64[[r for r in TINY if r < n]] = False
    err = np.abs(dist[f64] - dist64[:n][f64])
    print(f"{metric} {shape} n={n}: largest distance error {err.max():.3g}, {int((~clear[:n]).sum())} pairs inside the gap")
    assert (err <= 1e-5 * np.maximum(1, np.abs(dist64[:n][f64]))).all()
    use = clear[:n] & f64[:, None]
    assert np.array_equal(codes[use], codes64[:n][use])
    assert np.array_equal(codes, old[0][:n]) and np.array_equal(dist.view(np.uint32), old[1][:n].view(np.uint32))
    if C >= 4 and n > DUP:
        assert (codes[DUP] == 1).all() and (codes[ZERO] == 2).all() and (dist[ZERO] == 0).all()
    elif n > ZERO and metric == "cos":
        assert (codes[ZERO] == 0).all() and (dist[ZERO] == 1).all()  # a zero row against nonzero centroids: 1 everywhere, the first wins


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_codes_match_float64_and_todays_path(capi, metric, shape):
    X, cb, codes64, dist64, clear = reference(metric, shape)
    old = todays_path(capi, metric, shape, X, cb)
    for n in (1, 255, 257):
        check(capi, metric, shape, n, X, cb, codes64, dist64, clear, old)


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_a_second_staging_piece(capi, metric):
    shape = (12, 4, 10)
    X, cb, codes64, dist64, clear = reference(metric, shape, 65537)
    check(capi, metric, shape, 65537, X, cb, codes64, dist64, clear, todays_path(capi, metric, shape, X, cb))


N0, N = 400, 700
LABELS = np.arange(N, dtype=np.uint64) + 1


def index_pair(capi, metric, shape):
    """(data, queries, make): make(on) gives an empty pq index of the shape with the switch set"""
    d, S, C = shape
    X, cb = reference(metric, shape, N)[:2]

    def make(on):
        ix = capi.GpuIndex(metric, d, M=4, ef_construction=16, ef=16, seed=5, pq_codebook=cb, num_subvectors=S)
        ix.set_add_batch(256, 16)
        ix.set_pq_encode_fused(on)
        assert ix.pq_encode_fused() == (2 if on else 0)
        return ix

    return X, X[:32] + np.float32(0.01), make


def same_index(a, b, queries):
    assert np.array_equal(a.export_codes(), b.export_codes()) and a.checksum() == b.checksum()
    (la, da, _), (lb, db, _) = a.search_batch(queries, 10), b.search_batch(queries, 10)
    assert np.array_equal(la, lb) and np.array_equal(da.view(np.uint32), db.view(np.uint32))


@pytest.mark.parametrize("metric,shape", [("l2sq", (64, 8, 256)), ("cos", (100, 5, 255))])
def test_an_index_built_fused_is_its_twin(capi, metric, shape):
    X, queries, make = index_pair(capi, metric, shape)
    built = []
    for on in (1, 0):
        ix = make(on)
        ix.add_many(LABELS, X)
        ix.flush()
        assert capi.last_pq_encode() == {"pieces": 1, "fused": on, "passes": 0 if on else shape[1], "rows": N}
        built.append(ix)
    same_index(built[0], built[1], queries)
    assert built[0].export_graph(with_vectors=True)["vectors"].tobytes() == built[1].export_graph(with_vectors=True)["vectors"].tobytes()


@pytest.mark.parametrize("way", ["bulk", "lone"])
@pytest.mark.parametrize("metric,shape", [("l2sq", (64, 8, 256)), ("cos", (40, 5, 16))])
def test_a_compact_index_grown_fused_is_its_twin(capi, metric, shape, way):
    X, queries, make = index_pair(capi, metric, shape)
    S = shape[1]
    first = make(0)
    first.add_many(LABELS[:N0], X[:N0])
    first.flush()
    blob, grown = first.save_buffer(), []
    last = N if way == "bulk" else N0 + 24
    for on in (1, 0):
        ix = make(on)
        ix.load_buffer(blob)
        ix.pq_compact()
        ix.set_add_compact(1)
        if way == "bulk":
            ix.add_many(LABELS[N0:], X[N0:])
            ix.flush()
            want = {"pieces": 1, "fused": on, "passes": 0 if on else S, "rows": N - N0}
        else:
            ix.reserve(last)
            for i in range(N0, last):
                ix.add(LABELS[i], X[i])
                ix.flush()
                assert capi.last_pq_encode() == {"pieces": 1, "fused": on, "passes": 0 if on else S, "rows": 1}
            want = capi.last_pq_encode()
        assert capi.last_pq_encode() == want and ix.add_compact() == 2 and len(ix) == last
        assert ix.memory_usage()[0] == last * ((S + 15) // 16 * 16)  # still compact: the code rows are all the rows it holds
        grown.append(ix)
    same_index(grown[0], grown[1], queries)
    for ix in grown:
        ix.pq_expand()
    same_index(grown[0], grown[1], queries)
