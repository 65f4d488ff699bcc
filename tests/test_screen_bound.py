"""The int8 screen's bound (walk.hpp hop_distances_screened, kernels.hip k_fill_screen) restated in numpy: on adversarial rows,
LB (1 - e) never exceeds the f32 distance the walk computes (the oracle's SUM_WAVE64 order), so a row the screen rejects at a
radius would also have been rejected by its exact evaluation.  CPU only."""
import numpy as np
import pytest

from oracle import binding as oracle

F32 = np.float32


def screen_of(y):
    """k_fill_screen: (q, s, r) of one f32 row -- r in double over the f32 values s * q, rounded up into f32"""
    y = np.asarray(y, dtype=F32)
    if not np.all(np.isfinite(y)):
        return np.zeros(y.size, np.int8), F32(0), F32(np.inf)
    s = F32(np.max(np.abs(y))) / F32(127)
    if not np.isfinite(s) or s < F32(2.0 ** -126):
        return np.zeros(y.size, np.int8), F32(0), F32(np.inf)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.clip(np.rint(y / s), -127, 127).astype(np.int8)
        yp = (s * q.astype(F32)).astype(F32)
    dd = y.astype(np.float64) - yp.astype(np.float64)
    rr = np.sqrt(np.sum(dd * dd) * (1.0 + 2.0 ** -40))
    with np.errstate(over="ignore"):
        r = F32(rr)
    if np.isfinite(r) and float(r) < rr:
        r = np.nextafter(r, F32(np.inf))
    return q, s, (r if np.isfinite(r) else F32(np.inf))


def lower_bound(x, q, s, r, chunks):
    """the walk's LB and (1 - e): d' in f32, summed in order with one rounding per step (any order is within the bound)"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        yp = (s * q.astype(F32)).astype(F32)
        t = (x - yp).astype(F32)
        dp = F32(0)
        for v in (t * t).astype(F32):
            dp = F32(dp + v)
    ome = F32(1) - max(F32(2.0 ** -12), F32((2 * chunks + 64) * 2.0 ** -24))
    if not np.isfinite(dp):
        return F32(0), ome
    with np.errstate(over="ignore", invalid="ignore"):
        a = F32(F32(np.sqrt(dp)) * ome) - r
        lb = F32(a * a) if a > 0 else F32(0)
    return lb, ome


def rejects_at(lb, ome, radius):
    return bool(lb > F32(2.0 ** -100) and F32(lb * ome) > radius)


def adversarial(rng, d):
    g = rng.standard_normal(d).astype(F32)
    rows = [g, np.zeros(d, F32), g * F32(1e-30), g * F32(1e30), g * F32(1e-20), g * F32(3e18)]
    o = g.copy(); o[rng.integers(0, d)] = F32(1e4); rows.append(o)
    m = g.copy(); m[: d // 2] *= F32(1e30); m[d // 2:] *= F32(1e-30); rows.append(m)
    c = np.full(d, F32(0.5)); rows.append(c)  # constant: the int8 copy is (nearly) exact
    h = (rng.integers(-127, 128, d) * F32(0.01)).astype(F32); rows.append(h)  # values on the int8 grid
    p = g.copy(); p[0] = F32(np.inf); rows.append(p)
    n = g.copy(); n[-1] = F32(np.nan); rows.append(n)
    tiny = np.full(d, F32(1e-40)); rows.append(tiny)  # subnormal scale
    return rows


@pytest.mark.parametrize("d", [1, 3, 16, 17, 63, 64, 65, 127, 128, 129, 767, 768, 769, 1536, 2000])
def test_lower_bound_never_exceeds_the_device_distance(d):
    rng = np.random.default_rng(d)
    chunks = (d + 3) // 4
    rows = adversarial(rng, d)
    queries = [r.copy() for r in rows[:6]] + [rows[0] + F32(1e-3) * rng.standard_normal(d).astype(F32)]
    queries += [rng.standard_normal(d).astype(F32) * F32(sc) for sc in (1, 1e-3, 1e3, 1e-25, 1e25)]
    checked = 0
    for y in rows:
        q, s, r = screen_of(y)
        for x in queries:
            with np.errstate(over="ignore", invalid="ignore"):
                dist = F32(oracle.distance(x, y, "l2sq", oracle.SUM_WAVE64))
            lb, ome = lower_bound(x, q, s, r, chunks)
            # rejection is monotone in the radius: if it does not reject at radius = the row's own distance, it rejects at no
            # radius the exact evaluation would have let the row into
            if np.isnan(dist):
                continue
            assert not rejects_at(lb, ome, dist), (d, float(lb), float(dist), float(r))
            checked += 1
    assert checked > 0


def test_bound_rejects_far_rows():
    """the bound is not vacuous: a row far outside the radius is rejected"""
    rng = np.random.default_rng(0)
    d = 768
    y = rng.standard_normal(d).astype(F32)
    x = rng.standard_normal(d).astype(F32)
    q, s, r = screen_of(y)
    lb, ome = lower_bound(x, q, s, r, (d + 3) // 4)
    dist = F32(oracle.distance(x, y, "l2sq", oracle.SUM_WAVE64))
    assert float(r) < 0.05 * np.sqrt(float(dist))
    assert rejects_at(lb, ome, F32(0.8) * dist)
