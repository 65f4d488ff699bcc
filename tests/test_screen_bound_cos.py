"""The cosine form of the int8 screen's bound (walk.hpp hop_distances_screened<M_COS>, kernels.hip k_fill_screen<true>) restated in
numpy: on adversarial rows and queries, 1 - u - e never exceeds the f32 distance the walk computes (the oracle's SUM_WAVE64 order), so
a row the screen rejects at a radius would also have been rejected by its exact evaluation.  The twin of tests/test_screen_bound.py.
CPU only.

    sim8 = <x, c> (s / rb) / ra          (f32: the eight-lane chain of the kernel, then one multiply and one divide)
    u    = sim8 + rho + e,   rho >= ||y - s c|| / ||y||  (double, rounded up),   e = max(2^-12, (2 chunks + 64) 2^-24)
    reject iff 1 - u - e > radius, and only when ra and rb lie in [2^-48, 2^48] (rb: folded into rho = +inf by the fill)

ra and rb are restated here by the 64-lane chain in float64 rounded per step; the device's values may differ from these in the last
place, which e covers: every pair is also tried with both norms moved by two ulps either way."""
import numpy as np
import pytest

from oracle import binding as oracle
from tests import value_range as vr
from tests.test_screen_bound import adversarial

F32 = np.float32
LO, HI = F32(2.0 ** -48), F32(2.0 ** 48)  # the norms inside which no square and no product of the evaluation leaves the normal range
DIMS = [1, 3, 16, 17, 63, 64, 65, 127, 128, 129, 767, 768, 769, 1536, 2000]


def rooted_norm(v):
    """group_norm<M_COS, 64>: per lane an fma chain over its chunks (four values each), the 64-lane tree, the square root"""
    v = np.asarray(v, dtype=F32)
    chunks = (v.size + 3) // 4
    z = np.zeros(((chunks + 63) // 64) * 64 * 4, np.float64)
    z[: v.size] = v
    z = z.reshape(-1, 64, 4)  # [step][lane][value]
    s = np.zeros(64, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for step in z:
            for b in range(4):
                s = (step[:, b] * step[:, b] + s.astype(np.float64)).astype(F32)
        while s.size > 1:
            s = (s[0::2] + s[1::2]).astype(F32)
        return F32(np.sqrt(s[0]))


def screen_of(y, rb):
    """k_fill_screen<true>: (c, s / rb, rho) of one f32 row whose cached rooted norm is rb -- rho in double over the f32 values s * c,
    rounded up into f32; +inf for a row the screen must never reject"""
    y = np.asarray(y, dtype=F32)
    never = np.zeros(y.size, np.int8), F32(0), F32(np.inf)
    if not np.all(np.isfinite(y)):
        return never
    s = F32(np.max(np.abs(y))) / F32(127)
    if not np.isfinite(s) or s < F32(2.0 ** -126) or not (LO <= rb <= HI):  # (a NaN or zero rb fails the range test)
        return never
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        c = np.clip(np.rint(y / s), -127, 127).astype(np.int8)
        yp = (s * c.astype(F32)).astype(F32)
    dd = y.astype(np.float64) - yp.astype(np.float64)
    y64 = y.astype(np.float64)
    rr = np.sqrt(np.sum(dd * dd) / np.sum(y64 * y64) * (1.0 + 2.0 ** -40))
    rho = F32(rr)
    if float(rho) < rr:
        rho = np.nextafter(rho, F32(np.inf))
    return c, F32(s / rb), (rho if np.isfinite(rho) else F32(np.inf))


def screen_dot(x, c):
    """<x, c> in f32 as the kernel sums it: eight lanes, lane l takes screen chunks l, l + 8, ... (16 values each) in one fma chain,
    then the eight-lane tree"""
    x = np.asarray(x, dtype=F32)
    sch = ((x.size + 3) // 4 + 3) // 4
    steps = (sch + 7) // 8
    xs = np.zeros(steps * 8 * 16, np.float64); xs[: x.size] = x
    cs = np.zeros(steps * 8 * 16, np.float64); cs[: c.size] = c
    xs, cs = xs.reshape(steps, 8, 16), cs.reshape(steps, 8, 16)
    acc = np.zeros(8, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for st in range(steps):
            for b in range(16):
                acc = (xs[st, :, b] * cs[st, :, b] + acc.astype(np.float64)).astype(F32)
        while acc.size > 1:
            acc = (acc[0::2] + acc[1::2]).astype(F32)
    return acc[0]


def eps(chunks):
    return max(F32(2.0 ** -12), F32((2 * chunks + 64) * 2.0 ** -24))


def rejects_at(acc, t, rho, ra, e, radius):
    """the kernel's test, operation by operation in f32; a NaN anywhere fails it"""
    if not (LO <= ra <= HI):
        return False
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sim8 = F32(F32(acc * t) / ra)
        u = F32(F32(sim8 + rho) + e)
        lb = F32(F32(F32(1) - u) - e)
    return bool(lb > radius)


def nudged(v, k):
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf) if k > 0 else F32(-np.inf))
    return v


def families(rng, d):
    """(rows, queries): tests/test_screen_bound.py's rows and queries, and the cosine cases"""
    g = rng.standard_normal(d).astype(F32)
    rows = adversarial(rng, d)
    queries = [r.copy() for r in rows[:6]] + [rows[0] + F32(1e-3) * rng.standard_normal(d).astype(F32)]
    queries += [rng.standard_normal(d).astype(F32) * F32(sc) for sc in (1, 1e-3, 1e3, 1e-25, 1e25)]
    queries.append(np.zeros(d, F32))  # (a zero row is among the adversarial rows already)
    # x = +-y and x = y (1 + 1e-3 noise): distances near 0 (slightly negative after rounding) and near 2
    queries += [-g, (g * (F32(1) + F32(1e-3) * rng.standard_normal(d).astype(F32))).astype(F32)]
    h = rng.standard_normal(d).astype(F32)
    with np.errstate(over="ignore"):
        for sc in (1e18, 1e-18, 1e30, 1e-30):  # ra rb overflows and underflows
            rows.append((h * F32(sc)).astype(F32))
            queries.append((rng.standard_normal(d).astype(F32) * F32(sc)).astype(F32))
            queries.append((h * F32(sc)).astype(F32))
    rows += [(rng.standard_normal(d).astype(F32) + F32(3)) for _ in range(2)]  # a common mean: the bound is weak, not wrong
    queries.append(rng.standard_normal(d).astype(F32) + F32(3))
    mr, mq = vr.strict_data("cos_mixed", 12, d, 6)
    rows += list(mr)
    queries += list(mq)
    return rows, queries


@pytest.mark.parametrize("d", DIMS)
def test_bound_never_exceeds_the_device_distance(d):
    rng = np.random.default_rng(d)
    chunks = (d + 3) // 4
    e = eps(chunks)
    rows, queries = families(rng, d)
    qs = [(x, rooted_norm(x)) for x in queries]
    checked = rejected_far = 0
    for y in rows:
        rb = rooted_norm(y)
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            dists = [F32(oracle.distance(x, y, "cos", oracle.SUM_WAVE64)) for x, _ in qs]  # once per pair
        for kb in (0, -2, 2):
            c, t, rho = screen_of(y, nudged(rb, kb))
            if not np.isfinite(rho) and kb != 0:
                continue  # (never rejected, whatever the query: test_never_rejected_rows_and_queries)
            for (x, ra), dist in zip(qs, dists):
                if np.isnan(dist):
                    continue
                acc = screen_dot(x, c)
                # rejection is monotone in the radius: if it does not reject at radius = the row's own distance, it rejects at no
                # radius the exact evaluation would have let the row into
                for ka in (0, -2, 2):
                    assert not rejects_at(acc, t, rho, nudged(ra, ka), e, dist), (d, float(dist), float(rho), float(ra), float(rb), ka, kb)
                checked += 1
                rejected_far += rejects_at(acc, t, rho, ra, e, F32(-1))
    assert checked > 0
    if d >= 16:
        assert rejected_far > 0  # the restatement can reject at all (a radius below every distance)


def test_never_rejected_rows_and_queries():
    """rho = +inf for rows with a non-finite value, a zero or subnormal scale, or a norm of 0 or outside the range; a query whose norm
    is 0 or outside the range is never tested"""
    rng = np.random.default_rng(5)
    d = 768
    g = rng.standard_normal(d).astype(F32)
    bad = [np.zeros(d, F32), np.full(d, F32(1e-40)), g * F32(1e-30), g * F32(1e30)]
    p = g.copy(); p[3] = F32(np.inf); bad.append(p)
    n = g.copy(); n[7] = F32(np.nan); bad.append(n)
    for y in bad:
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            c, t, rho = screen_of(y, rooted_norm(y))
        assert np.isposinf(rho) and not c.any()
        assert not rejects_at(F32(0), t, rho, rooted_norm(g), eps(192), F32(-np.inf))
    c, t, rho = screen_of(g, rooted_norm(g))
    assert np.isfinite(rho)
    for x in (np.zeros(d, F32), g * F32(1e-30), g * F32(1e30)):
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            assert not rejects_at(screen_dot(x, c), t, rho, rooted_norm(x), eps(192), F32(-np.inf))


def test_bound_is_scale_invariant():
    """rows and queries scaled by powers of two inside the range: the same codes, the same rho, the same decision"""
    rng = np.random.default_rng(6)
    d = 768
    y, x = rng.standard_normal(d).astype(F32), rng.standard_normal(d).astype(F32)
    c0, t0, rho0 = screen_of(y, rooted_norm(y))
    dist = F32(oracle.distance(x, y, "cos", oracle.SUM_WAVE64))
    for ky, kx in ((-29, 0), (29, 0), (0, -29), (0, 29), (29, -29), (-29, 29)):
        ys, xs = y * F32(2.0 ** ky), x * F32(2.0 ** kx)
        c, t, rho = screen_of(ys, rooted_norm(ys))
        assert np.array_equal(c, c0) and rho == rho0
        for f in (0.5, 0.9, 0.99, 1.0):
            assert rejects_at(screen_dot(xs, c), t, rho, rooted_norm(xs), eps(192), F32(f) * dist) == \
                   rejects_at(screen_dot(x, c0), t0, rho0, rooted_norm(x), eps(192), F32(f) * dist), (ky, kx, f)


def test_bound_rejects_far_rows():
    """the bound is not vacuous: a Gaussian pair at d = 768 (rho ~ 0.0076, distance ~ 1) is rejected at 0.9 x its distance"""
    rng = np.random.default_rng(0)
    d = 768
    y = rng.standard_normal(d).astype(F32)
    x = rng.standard_normal(d).astype(F32)
    c, t, rho = screen_of(y, rooted_norm(y))
    dist = F32(oracle.distance(x, y, "cos", oracle.SUM_WAVE64))
    assert 0.004 < float(rho) < 0.012
    assert rejects_at(screen_dot(x, c), t, rho, rooted_norm(x), eps((d + 3) // 4), F32(0.9) * dist)
    assert not rejects_at(screen_dot(x, c), t, rho, rooted_norm(x), eps((d + 3) // 4), dist)
