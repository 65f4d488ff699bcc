"""The exact k-NN's certificate (bruteforce.hip k_certify; restated in tests/exact_knn_bound.py) against a numpy
model of the fp32-MFMA contraction: |q|^2 and |b|^2 as f32 fma chains, q.b as one f32 fma chain in k order, the epilogue, the
top-(k + 16) pre-selection.  Whenever the certificate says "certified", the pre-selection must hold the exact top-k of the brute
force in the pair kernel's order (the oracle's SUM_WAVE64); on Gaussian rows it must say "certified" (an implementation that always
fell back would pass the first check alone); on offset rows the pre-selection really misses, and those queries are refused.
CPU only.  The fma is modelled as a float64 multiply-add rounded to f32 (the product is exact in float64; the sum rounds twice,
which stays inside the same bound)."""
import numpy as np
import pytest

from oracle import binding as oracle
from tests.exact_knn_bound import certify, gamma, mfma_error_cos, mfma_error_l2, padded_dims

F32 = np.float32


def fma_chain(a, b):
    """sum_k a[..., k] * b[..., k] as an f32 fma chain in k order (broadcasting over the leading axes)"""
    s = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), dtype=F32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for i in range(a.shape[-1]):
        s = (a64[..., i] * b64[..., i] + s.astype(np.float64)).astype(F32)
    return s


def contraction(metric, rows, queries):
    """k_dense_f32's distance matrix [nq][n] and the query norms^2 it used"""
    qn2, bn2 = fma_chain(queries, queries), fma_chain(rows, rows)
    dot = fma_chain(queries[:, None, :], rows[None, :, :])
    if metric == "l2sq":
        d = (F32(qn2[:, None] + bn2[None, :]) - F32(2) * dot).astype(F32)
        return np.maximum(d, F32(0)), qn2
    with np.errstate(divide="ignore"):
        rq = np.where(qn2 == 0, F32(0), (F32(1) / np.sqrt(qn2)).astype(F32)).astype(F32)
        rb = np.where(bn2 == 0, F32(0), (F32(1) / np.sqrt(bn2)).astype(F32)).astype(F32)
    d = (F32(1) - dot * (rq[:, None] * rb[None, :]).astype(F32)).astype(F32)
    zq, zb = (qn2 == 0)[:, None], (bn2 == 0)[None, :]
    d = np.where(zq & zb, F32(0), np.where(zq | zb, F32(1), d))
    return d, qn2


def exact64(metric, rows, queries):
    R, Q = rows.astype(np.float64), queries.astype(np.float64)
    if metric == "l2sq":
        return ((Q[:, None, :] - R[None, :, :]) ** 2).sum(2)
    qn, rn = np.sqrt((Q * Q).sum(1)), np.sqrt((R * R).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = 1.0 - (Q @ R.T) / (qn[:, None] * rn[None, :])
    zq, zb = (qn == 0)[:, None], (rn == 0)[None, :]
    return np.where(zq & zb, 0.0, np.where(zq | zb, 1.0, out))


def check(metric, rows, queries, k):
    """(refused, missed) per query; asserts that no certified query's pre-selection misses an exact top-k row"""
    n, d = rows.shape
    kk, dims = k + 16, padded_dims(d)
    dt, qn2 = contraction(metric, rows, queries)
    # the model is itself within the bound (else the test would prove nothing about the kernel)
    ref = exact64(metric, rows, queries)
    if metric == "l2sq":
        E = mfma_error_l2(np.sqrt((queries.astype(np.float64) ** 2).sum(1))[:, None], np.sqrt((rows.astype(np.float64) ** 2).sum(1))[None, :], dims)
    else:
        E = mfma_error_cos(dims)
    assert np.all(np.abs(dt.astype(np.float64) - ref) <= E)
    ids, dists = oracle.bruteforce(rows, queries, k, metric, oracle.SUM_WAVE64, 4)
    refused, missed = [], []
    for q in range(queries.shape[0]):
        order = np.lexsort((np.arange(n), dt[q]))  # keys (distance, slot), as k_select orders them
        pre = set(order[:kk].tolist())
        tau = None if n <= kk else dt[q, order[kk - 1]]
        ok = certify(metric, tau, dists[q, k - 1], qn2[q], dims)
        miss = not set(ids[q].tolist()) <= pre
        assert not (ok and miss), ("certified, yet the pre-selection misses the exact top-k", q)
        refused.append(not ok)
        missed.append(miss)
    return np.array(refused), np.array(missed)


def offset(rng, n, d, nq, o, s):
    return (F32(o) + F32(s) * rng.standard_normal((n, d), dtype=F32)).astype(F32), (F32(o) + F32(s) * rng.standard_normal((nq, d), dtype=F32)).astype(F32)


@pytest.mark.parametrize("o,s", [(10, 0.01), (100, 0.1)])
def test_offset_rows_are_refused_where_the_preselection_misses(o, s):
    rng = np.random.default_rng(o)
    rows, queries = offset(rng, 4000, 128, 16, o, s)
    refused, missed = check("l2sq", rows, queries, 10)
    assert missed.any() and refused[missed].all()


def test_near_duplicate_groups_larger_than_the_margin():
    rng = np.random.default_rng(2)
    centres = rng.standard_normal((100, 128), dtype=F32)
    rows = (np.repeat(centres, 40, axis=0) + F32(1e-3) * rng.standard_normal((4000, 128), dtype=F32)).astype(F32)
    queries = (centres[rng.integers(0, 100, 16)] + F32(1e-3) * rng.standard_normal((16, 128), dtype=F32)).astype(F32)
    refused, missed = check("l2sq", rows, queries, 10)
    assert refused.any()


def test_assign_to_clusters_offset_subvectors():
    # k = 1 over 256 centroids drawn from the data: subvectors 30 + 0.01 N(0, 1) of width 12
    rng = np.random.default_rng(3)
    data = (F32(30) + F32(0.01) * rng.standard_normal((200, 12), dtype=F32)).astype(F32)
    centres = data[rng.choice(200, 256, replace=True)]
    refused, missed = check("l2sq", centres, data, 1)
    assert missed.any() and refused[missed].all()


@pytest.mark.parametrize("family", ["lattice", "repeated", "cos_scaled"])
def test_tie_heavy_rows_are_never_certified_wrongly(family):
    rng = np.random.default_rng(4)
    if family == "lattice":
        rows, queries, metric = rng.integers(-2, 3, (3000, 31)).astype(F32), rng.integers(-2, 3, (16, 31)).astype(F32), "l2sq"
    elif family == "repeated":
        rows = rng.standard_normal((3000, 33), dtype=F32)
        rows[rng.choice(3000, 300, replace=False)] = rows[0]
        queries, metric = np.repeat(rows[:1], 4, axis=0), "l2sq"
    else:
        rows = rng.standard_normal((3000, 24), dtype=F32)
        c = rng.standard_normal(24, dtype=F32)
        rows[rng.choice(3000, 300, replace=False)] = c[None, :] * rng.uniform(0.01, 100, 300).astype(F32)[:, None]
        rows[:5] = 0
        queries, metric = np.stack([c, c * F32(3), np.zeros(24, F32), rng.standard_normal(24, dtype=F32)]), "cos"
    check(metric, rows, queries, 10)


@pytest.mark.parametrize("metric,d", [("l2sq", 128), ("l2sq", 33), ("cos", 128), ("cos", 3)])
def test_gaussian_rows_are_certified(metric, d):
    rng = np.random.default_rng(d)
    rows, queries = rng.standard_normal((4000, d), dtype=F32), rng.standard_normal((16, d), dtype=F32)
    refused, _ = check(metric, rows, queries, 10)
    assert not refused.any()


def test_the_decision_is_strict():
    # tau exactly at the bound is refused; one ulp above it passes
    g = gamma(136)
    qn2, dk = 100.0, 50.0
    qa, dup = np.sqrt(qn2 / (1 - g)), dk / (1 - g)
    s = 2 * qa + np.sqrt(dup)
    bound = (dup + g * s * s + 4 * 136 * 2.0 ** -126) * (1 + 2.0 ** -40)
    assert not certify("l2sq", bound, dk, qn2, 128)
    assert certify("l2sq", np.nextafter(bound, np.inf), dk, qn2, 128)
    assert certify("l2sq", None, dk, qn2, 128)  # fewer than kk rows: all of them survived
    assert not certify("l2sq", 1e30, np.inf, qn2, 128) and not certify("l2sq", np.nan, dk, qn2, 128)
    assert not certify("cos", 0.5, 0.4, 2.0 ** -70, 128)  # a query norm outside the bound's range
