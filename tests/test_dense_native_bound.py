"""The certificate's bound for the native f16 contraction, pinned against a numpy model, CPU only.

Products of two halves are exact in f32, so the contraction's only errors are its additions.  What the matrix core does inside one
instruction is not specified; the derivation allows every addend to cost one f32 ulp of the running sum (2u relative: truncation
as well as rounding, in any order), which gives |dot~ - dot| <= 2 d u sum|q_i b_i| and, with the norms' roundings, the f32
kernel's bound at dims = 2 x (halves contracted, padding included).  The model here is a harsh member of that class: exact
products summed in blocks of 16 (one MFMA's K), the running sum TRUNCATED to 24 bits after every block.  It must stay inside
mfma_error_l2(., ., 2 dims) / mfma_error_cos(2 dims) against float64.  This pins the derivation, not the device
(tests/test_gpu_dense_native.py does that)."""
import numpy as np
import pytest

from tests.exact_knn_bound import mfma_error_cos, mfma_error_l2

F32, F16 = np.float32, np.float16


def halves_padded(d):
    return (d + 7) // 8 * 8  # a stored f16 row is whole 16-byte chunks


def trunc24(x):
    """float64 -> the nearest value toward zero with 24 significant bits"""
    m, e = np.frexp(x)
    return np.ldexp(np.trunc(m * 2.0 ** 24) / 2.0 ** 24, e)


def f32_chain_norm(x):
    s = np.zeros(x.shape[0], F32)
    x64 = x.astype(np.float64)
    for i in range(x.shape[1]):
        s = (x64[:, i] * x64[:, i] + s.astype(np.float64)).astype(F32)
    return s


def model(metric, rows, queries):
    """the native f16 contraction's distance matrix [nq][n]: norms as f32 fma chains, the dot product in truncated blocks of 16"""
    R, Q = rows.astype(np.float64), queries.astype(np.float64)
    dot = np.zeros((Q.shape[0], R.shape[0]))
    for k0 in range(0, R.shape[1], 16):
        dot = trunc24(dot + Q[:, k0:k0 + 16] @ R[:, k0:k0 + 16].T)  # (a block's 16 exact products summed in float64: 22-bit products)
    dot = dot.astype(F32)
    qn2, bn2 = f32_chain_norm(queries), f32_chain_norm(rows)
    if metric == "l2sq":
        d = (F32(qn2[:, None] + bn2[None, :]) - F32(2) * dot).astype(F32)
        return np.maximum(d, F32(0))
    with np.errstate(divide="ignore"):
        rq = np.where(qn2 == 0, F32(0), (F32(1) / np.sqrt(qn2)).astype(F32)).astype(F32)
        rb = np.where(bn2 == 0, F32(0), (F32(1) / np.sqrt(bn2)).astype(F32)).astype(F32)
    d = (F32(1) - dot * (rq[:, None] * rb[None, :]).astype(F32)).astype(F32)
    zq, zb = (qn2 == 0)[:, None], (bn2 == 0)[None, :]
    return np.where(zq & zb, F32(0), np.where(zq | zb, F32(1), d))


def exact64(metric, rows, queries):
    R, Q = rows.astype(np.float64), queries.astype(np.float64)
    if metric == "l2sq":
        return ((Q[:, None, :] - R[None, :, :]) ** 2).sum(2)
    qn, rn = np.sqrt((Q * Q).sum(1)), np.sqrt((R * R).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = 1.0 - (Q @ R.T) / (qn[:, None] * rn[None, :])
    zq, zb = (qn == 0)[:, None], (rn == 0)[None, :]
    return np.where(zq & zb, 0.0, np.where(zq | zb, 1.0, out))


def family(name, rng, n, d, nq):
    if name == "gauss":
        return rng.standard_normal((n, d)), rng.standard_normal((nq, d))
    if name in ("offset10", "offset100"):
        o, s = (10, 0.01) if name == "offset10" else (100, 0.1)
        return o + s * rng.standard_normal((n, d)), o + s * rng.standard_normal((nq, d))
    if name == "lattice":
        return rng.integers(-2, 3, (n, d)).astype(np.float64), rng.integers(-2, 3, (nq, d)).astype(np.float64)
    assert name == "scaled"  # scaled copies of one vector, zero rows, Gaussian rows (the cosine family of the device tests)
    rows, c = rng.standard_normal((n, d)), rng.standard_normal(d)
    m = n // 2
    rows[:m] = c[None, :] * rng.uniform(0.01, 100.0, m)[:, None]
    rows[m:m + 3] = 0
    q = rng.standard_normal((nq, d))
    q[: nq // 2] = c[None, :] * rng.uniform(0.5, 2.0, nq // 2)[:, None]
    q[-1] = 0
    return rows, q


@pytest.mark.parametrize("d", [1, 33, 64, 65, 768, 2000])
@pytest.mark.parametrize("name", ["gauss", "offset10", "offset100", "lattice", "scaled"])
def test_truncating_block_model_is_within_the_bound(name, d):
    rng = np.random.default_rng([d, len(name)])
    rows, queries = (x.astype(F16) for x in family(name, rng, 48, d, 12))
    pad = halves_padded(d) - d
    rows, queries = np.pad(rows, ((0, 0), (0, pad))), np.pad(queries, ((0, 0), (0, pad)))  # the stored rows: zero padded
    dims = 2 * halves_padded(d)
    for metric in ("l2sq", "cos"):
        got, ref = model(metric, rows, queries).astype(np.float64), exact64(metric, rows, queries)
        if metric == "l2sq":
            qn, bn = np.sqrt((queries.astype(np.float64) ** 2).sum(1)), np.sqrt((rows.astype(np.float64) ** 2).sum(1))
            E = mfma_error_l2(qn[:, None], bn[None, :], dims)
        else:
            E = np.full(ref.shape, mfma_error_cos(dims))
        over = np.abs(got - ref) - E
        assert np.all(over <= 0), (name, metric, d, float(np.max(over)), float(np.max(np.abs(got - ref) / E)))


def test_the_model_does_truncate():
    # (else the test above would be the rounding model under another name)
    assert trunc24(np.float64(1 + 2.0 ** -24 + 2.0 ** -25)) == 1.0 and trunc24(np.float64(-(1 + 2.0 ** -24 + 2.0 ** -25))) == -1.0
    assert trunc24(np.float64(0.0)) == 0.0 and trunc24(np.float64(3.0)) == 3.0
