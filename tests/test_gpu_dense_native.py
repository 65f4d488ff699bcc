"""The native f16 / i8 contraction (dense_native.hip) on the device: the exact k-NN over quantised indexes against
the brute force in the pair kernel's order, with the counters that show WHICH contraction ran; native on against off; the i8
extremes bit for bit; the f16 certificate's bound measured on the hardware (with subnormal halves and halves at the top of the
range); the matrix forms of lantern_gpu_distance_matrix / usearch_distance for both kinds; the launch sequence of a certified call."""
import numpy as np
import pytest

from tests.exact_knn_bound import mfma_error_cos, mfma_error_l2
from tests.test_gpu_exact_knn import FAMILIES, index_of, run_case
from tests.value_range import exact64

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
KIND = {"f16": 1, "i8": 2}


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0
    return capi


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def kind_delta(capi, before):
    return [a - b for a, b in zip(capi.dense_kind_stats(), before)]


# ---- the exact k-NN is the brute force, and the native kernel is what ran ---------------------------------------------------------
# (storage, family, metric, n, d, nq, k): a list over the edges, not a product.  (n, nq): one row, fewer rows than k, the fused path's
# start (4096 seed columns) and one past it with a ragged query tile, the 64k chunk edge with the 1024-query block edge; d: around the
# 128-byte K slab (f16: 64 halves, i8: 128 bytes) and the widest group; k: 1, 10, 240.  The f16 rows of 1 and 31 dimensions come
# with fewer rows than k + 16, where every row survives: rounded to halves, thousands of Gaussian rows of so few dimensions tie
# exactly, and ties beyond the survivors are refused whatever the contraction does.
CASES = [
    ("f16", "gauss", "l2sq", 1, 1, 1, 1),
    ("f16", "gauss", "cos", 9, 31, 127, 10),
    ("f16", "gauss", "l2sq", 4096, 33, 128, 240),
    ("f16", "gauss", "cos", 4097, 64, 129, 10),
    ("f16", "gauss", "l2sq", 4097, 65, 129, 10),
    ("f16", "gauss", "cos", 4097, 1017, 129, 1),
    ("f16", "gauss", "l2sq", 65537, 128, 1025, 10),
    ("f16", "offset10", "l2sq", 4097, 128, 129, 10),
    ("f16", "offset100", "cos", 4096, 31, 128, 10),
    ("f16", "lattice", "l2sq", 4097, 33, 129, 10),
    ("f16", "scaled", "cos", 4097, 64, 129, 10),
    ("i8", "i8gauss", "l2sq", 1, 1, 1, 1),
    ("i8", "i8gauss", "cos", 9, 33, 127, 10),
    ("i8", "i8gauss", "l2sq", 4096, 128, 128, 240),
    ("i8", "i8offset", "cos", 4097, 129, 129, 10),
    ("i8", "i8gauss", "cos", 4097, 768, 129, 10),
    ("i8", "i8offset", "l2sq", 4097, 2000, 129, 1),
    ("i8", "i8gauss", "l2sq", 65537, 128, 1025, 10),
]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("storage,family,metric,n,d,nq,k", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-n{c[3]}-d{c[4]}-q{c[5]}-k{c[6]}" for c in CASES])
def test_native_exact_search_is_the_brute_force(capi, oracle, cores, monkeypatch, storage, family, metric, n, d, nq, k, fused):
    monkeypatch.setenv("LANTERN_GPU_DENSE_NATIVE", "1")
    before = capi.dense_kind_stats()
    st = run_case(capi, oracle, cores, monkeypatch, family, metric, n, d, nq, k, storage=storage, fused=fused)
    moved = kind_delta(capi, before)
    assert moved[KIND[storage]] >= 1 and moved[0] == 0 and moved[3 - KIND[storage]] == 0, moved  # the native kernel of this kind, and no other
    assert st["queries"] == nq and st["certified"] + st["fallback"] == nq, st
    if storage == "i8":
        assert st["fallback"] == 0, st  # the keys are the exact-order distances: certified by construction
    elif family == "gauss":
        assert st["fallback"] == 0, st
    elif (family, metric) == ("offset10", "l2sq"):
        assert st["fallback"] >= 1, st


# ---- native on against off ------------------------------------------------------------------------------------------------------------
def search_on_off(capi, monkeypatch, ix, queries, k, kind):
    out = []
    for native in ("1", "0"):
        monkeypatch.setenv("LANTERN_GPU_DENSE_NATIVE", native)
        before = capi.dense_kind_stats()
        out.append(ix.exact_search(queries, k))
        moved = kind_delta(capi, before)
        want = kind if native == "1" else 0
        assert moved[want] >= 1 and sum(moved) == moved[want], (native, moved)  # the launches move from [0] to [1] / [2]
    return out


ON_OFF = [("f16", f, m) for f in ("gauss", "offset10", "offset100", "lattice", "scaled") for m in ("l2sq", "cos")] + \
         [("i8", f, m) for f in ("i8gauss", "i8offset") for m in ("l2sq", "cos")]


@pytest.mark.parametrize("storage,family,metric", ON_OFF, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in ON_OFF])
def test_native_on_and_off_agree(capi, oracle, monkeypatch, storage, family, metric):
    n, d, nq, k = 9000, 65, 130, 10
    rows, queries = FAMILIES[family](np.random.default_rng([5, len(family), len(metric)]), n, d, nq)
    ix = index_of(capi, metric, storage, rows, oracle.quantize_i8(rows))
    (s1, d1), (s0, d0) = search_on_off(capi, monkeypatch, ix, queries, k, KIND[storage])
    ix.close()
    assert np.array_equal(s1, s0) and np.array_equal(bits(d1), bits(d0)), int(np.sum(np.any(s1 != s0, axis=1)))


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_native_on_and_off_agree_on_non_finite_halves(capi, oracle, monkeypatch, metric):
    n, d, nq, k = 5000, 40, 64, 10
    rng = np.random.default_rng(17)
    rows, queries = rng.standard_normal((n, d), dtype=F32), rng.standard_normal((nq, d), dtype=F32)
    rows[7, 3], rows[900, 0], rows[901, 39], rows[4999, 8] = np.inf, -np.inf, np.nan, -np.inf
    rows[13, :] = np.inf
    queries[5, 2], queries[6, 7], queries[7, 1] = np.inf, np.nan, -np.inf
    ix = index_of(capi, metric, "f16", rows, rows)
    (s1, d1), (s0, d0) = search_on_off(capi, monkeypatch, ix, queries, k, 1)
    ix.close()
    for s in (s1, s0):  # well formed: at most k distinct valid slots per query
        for q in range(nq):
            valid = s[q][s[q] != 0xFFFFFFFF]
            assert np.all(valid < n) and len(set(valid.tolist())) == len(valid)
    both = ~np.isnan(d1) & ~np.isnan(d0)
    assert both.any()
    assert np.array_equal(s1[both], s0[both]) and np.array_equal(bits(d1)[both], bits(d0)[both])


# ---- i8 extremes: the zero-norm rules and the largest int32 sums ---------------------------------------------------------------------
def test_i8_extremes_are_the_pair_kernel_bit_for_bit(capi, oracle):
    d = 2000
    alt = np.where(np.arange(d) % 2 == 0, 100, -100)
    rows = np.stack([np.full(d, 100), np.full(d, -100), alt, np.zeros(d, int), -alt]).astype(np.int8)
    for metric in ("l2sq", "cos"):
        want = np.array([[oracle.distance(a.astype(F32), b.astype(F32), metric, oracle.SUM_I8) for b in rows] for a in rows], dtype=F32)
        for exact in (True, False):
            got = capi.distance_matrix(rows, rows, metric, exact_order=exact, kind="i8")
            assert np.array_equal(bits(got), bits(want)), (metric, exact, got.tolist(), want.tolist())
    assert want[3, 3] == 0.0 and want[3, 0] == 1.0 and want[0, 1] == 2.0  # (cos: both zero, one zero, opposite)


# ---- the f16 bound on the hardware --------------------------------------------------------------------------------------------------
def halves_padded(d):
    return (d + 7) // 8 * 8


def fam_subnormal(rng, n, d, nq):  # every half subnormal (below 2^-14 = 6.1e-5): values ~1e-6, multiples of 2^-24
    return (F32(1e-6) * rng.standard_normal((n, d), dtype=F32)).astype(F32), (F32(1e-6) * rng.standard_normal((nq, d), dtype=F32)).astype(F32)


def fam_top(rng, n, d, nq):  # the top of the half range (largest half: 65504)
    return tuple(np.clip(F32(3e4) * rng.standard_normal((m, d), dtype=F32), -65000, 65000).astype(F32) for m in (n, nq))


BOUND_FAMILIES = [(f, FAMILIES[f]) for f in ("gauss", "offset10", "offset100", "dupgroups", "repeated", "lattice", "scaled")] + \
                 [("subnormal", fam_subnormal), ("top", fam_top)]


@pytest.mark.parametrize("na,nb", [(1, 1), (127, 257), (129, 127), (257, 129)])
@pytest.mark.parametrize("d", [1, 3, 31, 33, 64, 65, 128, 768])
def test_f16_contraction_is_within_the_bound(capi, na, nb, d):
    dims = 2 * halves_padded(d)  # the certificate's dims for halves: twice the halves contracted, padding included
    worst = {}
    for fi, (family, make) in enumerate(BOUND_FAMILIES):
        rng = np.random.default_rng([fi, na, nb, d])
        rows, a = (x.astype(F16) for x in make(rng, nb, d, na))
        if family == "subnormal":
            assert np.all(np.abs(rows.astype(F32)) < 2.0 ** -14) and np.any(rows != 0)
        for metric in ("l2sq", "cos"):
            got = capi.distance_matrix(a, rows, metric, exact_order=False, kind="f16").astype(np.float64)
            ref = exact64(metric, rows.astype(F32), a.astype(F32))
            if metric == "l2sq":
                qn, bn = np.sqrt((a.astype(np.float64) ** 2).sum(1)), np.sqrt((rows.astype(np.float64) ** 2).sum(1))
                E = mfma_error_l2(qn[:, None], bn[None, :], dims)
            else:
                E = np.full(ref.shape, mfma_error_cos(dims))
            worst[(family, metric)] = float(np.max(np.abs(got - ref) / E))
    print(f"f16 bound na={na} nb={nb} d={d}: largest error / bound = {max(worst.values()):.4f} at {max(worst, key=worst.get)};"
          f" subnormal {max(worst[('subnormal', m)] for m in ('l2sq', 'cos')):.4f}, top {max(worst[('top', m)] for m in ('l2sq', 'cos')):.4f}")
    over = {key: v for key, v in worst.items() if not v <= 1.0}
    assert not over, over


# ---- the matrix forms ---------------------------------------------------------------------------------------------------------------
def oracle_matrix(oracle, cores, a, rows, metric, mode):
    """[na][nb] distances in the oracle's order `mode`: the brute force with k = every row, put back in column order"""
    ids, dists = oracle.bruteforce(rows, a, rows.shape[0], metric, mode, cores)
    out = np.empty(ids.shape, F32)
    np.put_along_axis(out, ids.astype(np.int64), dists, axis=1)
    return out


def stored(oracle, storage, rng, n, d):
    """n rows of storage `storage`: (the array the C entry takes, the same values as f32 for the oracle)"""
    if storage == "f16":
        h = rng.standard_normal((n, d), dtype=F32).astype(F16)
        return h, h.astype(F32)
    q = oracle.quantize_i8(F32(0.4) * rng.standard_normal((n, d), dtype=F32))
    return q.astype(np.int8), q


@pytest.mark.parametrize("na,nb", [(1, 1), (127, 257), (129, 127), (257, 129)])
@pytest.mark.parametrize("d", [1, 33, 128, 129, 768])
def test_i8_contraction_equals_the_exact_order(capi, oracle, na, nb, d):
    rng = np.random.default_rng([na, nb, d])
    (a, _), (rows, _) = stored(oracle, "i8", rng, na, d), stored(oracle, "i8", rng, nb, d)
    rows[0] = 0  # a zero norm
    for metric in ("l2sq", "cos"):
        dense = capi.distance_matrix(a, rows, metric, exact_order=False, kind="i8")
        exact = capi.distance_matrix(a, rows, metric, exact_order=True, kind="i8")
        assert np.array_equal(bits(dense), bits(exact)), (metric, int(np.sum(bits(dense) != bits(exact))))


# d at the group-width edges of the pair kernel: 8 / 16 / 32 / 64 lanes from 32 / 64 / 128 chunks on (f16: 8 halves per chunk, so rows of
# 1017 - 2000 dimensions take the 64-lane form; i8: 16 per chunk)
@pytest.mark.parametrize("storage,d", [("f16", d) for d in (1, 248, 249, 504, 505, 1016, 1017, 2000)] + [("i8", d) for d in (1, 496, 497, 1008, 1009, 2000)])
def test_exact_order_matrix_is_the_oracle(capi, oracle, cores, storage, d):
    rng = np.random.default_rng([d, len(storage)])
    (a, af), (rows, rf) = stored(oracle, storage, rng, 5, d), stored(oracle, storage, rng, 37, d)
    mode = oracle.SUM_WAVE64_F16 if storage == "f16" else oracle.SUM_I8
    for metric in ("l2sq", "cos"):
        got = capi.distance_matrix(a, rows, metric, exact_order=True, kind=storage)
        want = oracle_matrix(oracle, cores, af, rf, metric, mode)
        assert np.array_equal(bits(got), bits(want)), (metric, int(np.sum(bits(got) != bits(want))))
        one = capi.distance(a[1], rows[2], metric, kind=storage)  # usearch_distance: the 1 x 1 case
        assert bits(F32(one)) == bits(F32(oracle.distance(af[1], rf[2], metric, mode))) == bits(got[1, 2])


# ---- the launch sequence -------------------------------------------------------------------------------------------------------------
def test_certified_f16_call_issues_the_launches_the_shape_predicts(capi, monkeypatch):
    monkeypatch.setenv("LANTERN_GPU_DENSE_NATIVE", "1")
    monkeypatch.setenv("LANTERN_GPU_DENSE_FUSED", "1")
    n, d, nq, k = 140000, 64, 1100, 10
    want = []
    for c0 in range(0, n, 65536):
        nc = min(65536, n - c0)
        for q0 in range(0, nq, 1024):
            nqt = min(1024, nq - q0)
            plain = min(nc, 4096) if c0 == 0 else 0
            if plain:
                want.append((nqt, plain, False))
            if plain < nc:
                want.append((nqt, nc - plain, True))
    rows, queries = FAMILIES["gauss"](np.random.default_rng(1), n, d, nq)
    ix = index_of(capi, "l2sq", "f16", rows, rows)
    before, kinds = capi.exact_knn_stats(), capi.dense_kind_stats()
    capi.dense_profile(True)
    ix.exact_search(queries, k)
    got = [(r["rows"], r["cols"], r["fused"]) for r in capi.dense_profile(False)]
    after = capi.exact_knn_stats()
    ix.close()
    assert got == want
    assert after["fallback"] == before["fallback"] and after["certified"] - before["certified"] == nq
    assert kind_delta(capi, kinds) == [0, len(want), 0]
