"""The exact k-NN's certificate (bruteforce.hip k_certify) restated in Python: the error bound E of the fp32-MFMA
contraction and the per-query decision.  Shared by tests/test_exact_knn_bound.py (CPU) and tests/test_gpu_exact_knn.py (device).

  u = 2^-24, g(n) = n u / (1 - n u), d = f32 scalars contracted (the row padded to whole 16-byte chunks)
  l2sq: |d~ - delta| <= g(d + 8) (|q| + |b|)^2 + 4 (d + 8) 2^-126
  cos:  |d~ - delta| <= g(2 d + 16) + 2^-100          (every nonzero norm^2 in [2^-60, 2^60])
delta = the distance in real arithmetic over the stored values.  The pair kernel's exact-order distance D obeys the same bounds
(l2sq: |D - delta| <= g(d + 8) delta)."""
import math

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def padded_dims(d):
    return (d + 3) // 4 * 4


def mfma_error_l2(qnorm, bnorm, dims):
    """E(q, b) for l2sq: qnorm, bnorm = |q|, |b| (float64 or arrays of them), dims = f32 scalars contracted"""
    return gamma(dims + 8) * (qnorm + bnorm) ** 2 + 4.0 * (dims + 8) * 2.0 ** -126


def mfma_error_cos(dims):
    return gamma(2 * dims + 16) + 2.0 ** -100


def norm_in_range(v):
    return v == 0.0 or 2.0 ** -60 <= v <= 2.0 ** 60


def certify(metric, tau, dk, qn2, dims, row_norms_ok=True):
    """k_certify's decision for one query: tau = the kk-th contraction distance (None: fewer than kk rows, every row survived),
    dk = the re-ranked k-th exact-order distance, qn2 = the query's f32 |q|^2 as the contraction computed it."""
    if tau is None:
        return True
    tau, dk, qn2 = float(tau), float(dk), float(qn2)
    if not (0.0 <= qn2 < 2.0 ** 120) or math.isnan(tau) or 2.0 * dims + 16 >= 2.0 ** 20:
        return False
    if metric == "cos":
        if not (row_norms_ok and norm_in_range(qn2) and -1.0 <= dk <= 3.0):
            return False
        bound = dk + 2.0 * gamma(2 * dims + 16) + 2.0 ** -100
    else:
        if not (0.0 <= dk < 2.0 ** 120):
            return False
        g = gamma(dims + 8)
        qa = math.sqrt(qn2 / (1.0 - g))
        dup = dk / (1.0 - g)
        s = 2.0 * qa + math.sqrt(dup)  # |q| + |b| for every row that could be in the exact top-k
        if s * s >= 2.0 ** 120:
            return False
        bound = dup + g * s * s + 4.0 * (dims + 8) * 2.0 ** -126
    return tau > bound * (1.0 + 2.0 ** -40)
