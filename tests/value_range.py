"""Rows at the edges of the f32 range -- denormal squares, sums that overflow to +inf, scales 2^-45 .. 2^55 mixed in one index,
denormal halves in f16 storage, non-finite components -- and the float64 referee with the project's own tolerance (DESIGN.md 4.1
and 4.5).  Imports without a GPU: tests/test_value_range_ref.py holds the oracle to the tolerance here, tests/test_gpu_value_range.py
and tests/test_gpu_exact_knn.py hold the device to the oracle's bits.

STRICT families: every distance is a number (+inf allowed); the device must equal the oracle bit for bit and both must be within
`pair_rounding` of float64.  LOOSE pairs: a NaN or an infinity in a row, or finite cosine rows whose norms overflow; only the class
of the result (NaN / +inf / -inf / a number) is compared."""
import numpy as np

from tests.exact_knn_bound import gamma

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
NAN_SET, NAN_CLEAR = 0xFFC00000, 0x7FC00000  # the quiet NaN with and without its sign bit (x86's default NaN is the first)


# ---- float64 distances over the stored values, and how far an exact-order f32 distance may be from them ---------------------------
def exact64(metric, rows, queries, direct=False):
    """[nq][n] float64 distances.  l2sq: the norm expansion in float64 -- far inside the f32 bounds checked with it; direct=True sums
    the squared differences themselves (small shapes: rows whose scales differ by 2^100 share a matrix there)."""
    if metric == "hamming":
        return np.stack([np.unpackbits(np.bitwise_xor(q[None, :], rows).view(np.uint8), axis=1).sum(1) for q in queries]).astype(np.float64)
    R, Q = rows.astype(np.float64), queries.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        qn, rn = (Q * Q).sum(1), (R * R).sum(1)
        if metric == "l2sq":
            if direct:
                return np.stack([((q[None, :] - R) ** 2).sum(1) for q in Q])
            return np.maximum(qn[:, None] + rn[None, :] - 2.0 * (Q @ R.T), 0.0)
        dot = np.stack([(q[None, :] * R).sum(1) for q in Q]) if direct else Q @ R.T
        den = np.sqrt(qn)[:, None] * np.sqrt(rn)[None, :]
        out = 1.0 - dot / den
    out[(qn[:, None] == 0) & (rn[None, :] == 0)] = 0.0
    out[(qn[:, None] == 0) ^ (rn[None, :] == 0)] = 1.0
    return out


def pair_rounding(metric, delta, dims):
    """how far the pair kernel's exact-order distance may be from the real one"""
    if metric == "hamming":
        return np.zeros_like(delta)
    if metric == "cos":
        return np.full_like(delta, gamma(2 * dims + 16) + 2.0 ** -100)
    return gamma(dims + 8) * np.abs(delta) + 4.0 * (dims + 8) * 2.0 ** -126


def within_rounding(metric, got, delta, dims):
    """elementwise: is the f32 distance `got` a correct rounding of the float64 `delta`?  |got - delta| <= pair_rounding, and at the top of
    the range: delta > FLT_MAX (1 + gamma(d + 8)) -> got must be +inf; FLT_MAX < delta <= that -> +inf or within the tolerance."""
    got, delta = np.asarray(got, dtype=np.float64), np.asarray(delta, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        close = np.abs(got - delta) <= pair_rounding(metric, delta, dims)
    is_inf = np.isposinf(got)
    must_inf = delta > FLT_MAX * (1.0 + gamma(dims + 8))
    may_inf = delta > FLT_MAX
    return np.where(must_inf, is_inf, np.where(may_inf, is_inf | close, close & np.isfinite(got)))


# ---- strict families: (rng, n, d, nq) -> rows, queries (f32) --------------------------------------------------------------------
def _gauss(rng, n, d):
    return rng.standard_normal((n, d), dtype=F32)


def _scaled(s):
    def make(rng, n, d, nq):
        return (_gauss(rng, n, d) * F32(s)).astype(F32), (_gauss(rng, nq, d) * F32(s)).astype(F32)
    return make


def fam_l2_edge(rng, n, d, nq):
    """half the rows (and queries) x 1e18, half x 1e19: squares of 1e36 .. 1e38 -- finite distances next to +inf"""
    def make(m):
        x = _gauss(rng, m, d)
        x[0::2] *= F32(1e18)
        x[1::2] *= F32(1e19)
        return x
    return make(n), make(nq)


def fam_l2_mixed(rng, n, d, nq):
    """tests/screen_probe.py's mixed_scale: a quarter of the rows x 1e30 in their first half, a quarter x 1e-30, then zero rows;
    queries: half of them rows of the set, half Gaussian"""
    g = _gauss(rng, n, d)
    mix = g.copy()
    mix[: n // 4, : d // 2] *= F32(1e30)
    mix[n // 4: n // 2] *= F32(1e-30)
    mix[n // 2: n // 2 + min(50, max(1, n // 16))] = 0
    q = np.concatenate([mix[rng.integers(0, n, nq // 2)], _gauss(rng, nq - nq // 2, d)])
    return mix, q.astype(F32)


def fam_cos_mixed(rng, n, d, nq):
    """rows at 2^-45, 1 and 2^55 by turns, 20 zero rows; queries at the three scales, one of them zero"""
    def make(m):
        x = _gauss(rng, m, d)
        x[0::3] *= F32(2.0 ** -45)
        x[2::3] *= F32(2.0 ** 55)
        return x
    rows, q = make(n), make(nq)
    rows[rng.choice(n, size=min(20, max(1, n // 8)), replace=False)] = 0
    q[-1] = 0
    return rows, q


def fam_f16_denorm(rng, n, d, nq):
    """f16 storage: magnitudes 1e-6 .. 6e-5 (denormal halves: below 2^-14) and magnitudes near 6e4 (the top of the half range) -- a
    third of the rows all small, a third all large, a third mixed element by element"""
    def make(m):
        sign = rng.choice(np.array([-1.0, 1.0]), size=(m, d))
        small = sign * 10.0 ** rng.uniform(np.log10(1e-6), np.log10(6e-5), (m, d))
        large = sign * rng.uniform(5.0e4, 6.0e4, (m, d))
        pick = rng.random((m, d)) < 0.5
        pick[0::3] = True
        pick[1::3] = False
        return np.where(pick, small, large).astype(F32)
    return make(n), make(nq)


# name -> (metrics, storage, maker)
STRICT = {
    "l2_denorm": (("l2sq",), "f32", _scaled(1e-20)),       # squares of 1e-40: denormal
    "l2_tiny": (("l2sq",), "f32", _scaled(2.0 ** -45)),
    "l2_huge": (("l2sq",), "f32", _scaled(2.0 ** 55)),
    "l2_edge": (("l2sq",), "f32", fam_l2_edge),
    "l2_mixed": (("l2sq",), "f32", fam_l2_mixed),
    "cos_tiny": (("cos",), "f32", _scaled(2.0 ** -45)),
    "cos_huge": (("cos",), "f32", _scaled(2.0 ** 55)),
    "cos_mixed": (("cos",), "f32", fam_cos_mixed),
    "f16_denorm": (("l2sq", "cos"), "f16", fam_f16_denorm),
}
F32_STRICT = [(name, m) for name, (metrics, storage, _) in STRICT.items() if storage == "f32" for m in metrics]
# the pair level also runs every f32 family under the other metric.  l2sq is strict for all finite inputs, so a cosine family is in its
# domain; an l2sq family under cosine is not (its norms under- or overflow): there the device must still have the oracle's bits wherever
# the oracle's result is a number (denormal operands of sqrt and divide), and its class elsewhere -- no float64 check.
F32_PAIRS = [(name, m) for name, (_, storage, _) in STRICT.items() if storage == "f32" for m in ("l2sq", "cos")]


def in_domain(name, metric):
    return metric == "l2sq" or metric in STRICT[name][0]


F16_STRICT = [(name, m) for name, (metrics, storage, _) in STRICT.items() if storage == "f16" for m in metrics]


def strict_data(name, n, d, nq, seed=0):
    """the family's rows and queries at a shape, seeded by the family and the shape"""
    rng = np.random.default_rng([seed, sorted(STRICT).index(name), n, d, nq])
    return STRICT[name][2](rng, n, d, nq)


# ---- loose pairs ----------------------------------------------------------------------------------------------------------------
def bits_to_f32(u):
    return np.array([u], dtype=np.uint32).view(F32)[0]


def loose_specials():
    return {"nan_set": bits_to_f32(NAN_SET), "nan_clear": bits_to_f32(NAN_CLEAR), "pinf": F32(np.inf), "ninf": F32(-np.inf)}


def loose_pairs(rng, d):
    """[(name, a, b)]: Gaussian pairs with one special component in a, in b, in both at the same place (inf - inf, inf * inf), against
    a zero vector (0 * inf), and finite rows of magnitude 1e19 (cosine: the norms overflow)"""
    out = []
    sp = loose_specials()
    for name, v in sp.items():
        at = int(rng.integers(0, d))
        a, b = _gauss(rng, 1, d)[0], _gauss(rng, 1, d)[0]
        a1 = a.copy(); a1[at] = v
        b1 = b.copy(); b1[at] = v
        out += [(f"{name}_in_a", a1, b), (f"{name}_in_b", a, b1), (f"{name}_in_both", a1, b1), (f"{name}_vs_zero", a1, np.zeros(d, F32))]
    a, b = _gauss(rng, 1, d)[0], _gauss(rng, 1, d)[0]
    a1 = a.copy(); a1[0] = sp["pinf"]
    b1 = b.copy(); b1[0] = sp["ninf"]
    out.append(("pinf_vs_ninf", a1, b1))
    for i in range(4):
        out.append((f"finite_1e19_{i}", (_gauss(rng, 1, d)[0] * F32(1e19)).astype(F32), (_gauss(rng, 1, d)[0] * F32(1e19)).astype(F32)))
    return out


def value_class(x):
    """'nan', '+inf', '-inf' or 'num'"""
    x = float(x)
    return "nan" if x != x else "+inf" if x == np.inf else "-inf" if x == -np.inf else "num"


def class64(metric, a, b):
    """the class of the distance in float64 arithmetic with the metric's own rules (cosine: the zero-norm rules first).  Defined for
    pairs whose class does not depend on the summation order: non-finite components among N(0,1) ones."""
    A, B = a.astype(np.float64), b.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if metric == "l2sq":
            return value_class(((A - B) ** 2).sum())
        ab, a2, b2 = (A * B).sum(), (A * A).sum(), (B * B).sum()
        if a2 == 0 and b2 == 0:
            return "num"
        if a2 == 0 or b2 == 0:
            return "num"
        return value_class(1.0 - ab / (np.sqrt(a2) * np.sqrt(b2)))
