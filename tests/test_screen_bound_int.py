"""The INTEGER form of the int8 screen's bound (walk.hpp screen_stage_query, hop_distances_screened) restated in numpy, operation by
operation: the query's 16-bit copy X = 256 h + l in two int8 planes with its scale sx, delta >= ||x - sx X|| and ||sx X||^2; the row's
three dot4 sums; the f32 steps of the l2sq and of the cosine test.  CPU only; tests/test_gpu_screen_int.py holds the device to it.

    sx = max |x| / 32639,  q = fl(x / sx),  X = rint(q),  h = (X + 128) >> 8,  l = X - 256 h
    delta = fl(sx sqrt(S)) (1 + 2^-10),  S = sum (|q - X| + 2^-9)^2   (64 lanes: chain over the lane's chunks, tree);  cosine: dq = fl(delta / ra) (1 + 2^-10)
    Ih = <h, c>, Il = <l, c>, C2 = <c, c> in int32 (eight lanes), I = 256 Ih + Il in double -> f32
    l2sq    d' = (P - 2 sx s I) + s^2 C2,  eta = 2^-20 (P + s^2 C2),  LB = max(0, sqrt(max(0, d' - eta)) (1 - e) - r - delta)^2,  reject iff LB (1 - e) > radius
    cosine  sim8 = I sx (s / rb) / ra,  u = sim8 + rho (1 + dq) + dq + e,  reject iff 1 - u - e > radius

Mutations (run on a scratch copy, not part of the suite).  delta = 0 for the queries that can be quantised: the f32 soundness test
does NOT notice for either metric (delta is about 1e-5 of the distance and e = 2^-12 hides it); test_the_planes_hold_the_query (delta
below the true error) and test_the_cosine_bound_needs_its_delta_term fail.  delta = 0 for every query: the soundness test fails at
every width (a query that cannot be quantised rejects).  eta = 0: the l2sq soundness test fails at 12 of the 15 widths, at the pairs
x = y and x ~ y, where the expansion cancels."""
import numpy as np
import pytest

from oracle import binding as oracle
from tests import test_screen_bound as l2
from tests import test_screen_bound_cos as cs

F32 = np.float32
F64 = np.float64
E12 = F32(2.0 ** -12)
UP = F32(1.0 + 2.0 ** -10)
XMAX = 32639
DIMS = [1, 3, 16, 17, 63, 64, 65, 127, 128, 129, 767, 768, 769, 1536, 2000]
NP_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")


def l2_scale_ok(s):
    """device_common.hpp screen_l2_scale_ok"""
    return bool(F32(2.0 ** -40) <= s <= F32(2.0 ** 40))


def wrap32(v):
    """an int32 accumulator: what the device holds after any number of wrapping adds"""
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def tree(v):
    v = np.asarray(v, F32)
    with np.errstate(**NP_QUIET):
        while v.size > 1:
            v = (v[0::2] + v[1::2]).astype(F32)
    return v[0]


class Staged:
    """screen_stage_query: ok, sx, X (int64, padded to whole screen chunks), h, l, delta (cosine: dq), nx2"""

    def __init__(self, x, metric, ra=None, mutate=()):
        x = np.asarray(x, F32)
        self.d = x.size
        chunks = (x.size + 3) // 4
        sch = (chunks + 3) // 4
        xp = np.zeros(sch * 16, F32); xp[: x.size] = x
        mb = int(np.max(xp.view(np.uint32) & np.uint32(0x7FFFFFFF)))
        with np.errstate(**NP_QUIET):
            sx = F32(np.array(mb, np.uint32).view(F32)) / F32(XMAX)
        ok = mb < 0x7F800000 and mb != 0
        ok = ok and (bool(F32(2.0 ** -126) <= sx <= F32(2.0 ** 100)) if metric == "cos" else l2_scale_ok(sx))
        with np.errstate(**NP_QUIET):
            q = (xp / sx).astype(F32) if ok else np.zeros_like(xp)
            Xf = np.clip(np.rint(q), -XMAX, XMAX).astype(F32)
            rho = (np.abs((q - Xf).astype(F32)) + F32(2.0 ** -9)).astype(F32)
            # lane L of 64 takes query chunks L, L + 64, ...: an fma chain over their values in order, then the 64-lane tree
            steps = (4 * sch + 63) // 64
            r3 = np.zeros(steps * 64 * 4, F64); r3[: rho.size] = rho
            r3 = r3.reshape(steps, 64, 4)
            present = np.zeros(steps * 64 * 4, bool); present[: rho.size] = True
            present = present.reshape(steps, 64, 4)
            S = np.zeros(64, F32)
            for st in range(steps):
                for b in range(4):
                    S = np.where(present[st, :, b], (r3[st, :, b] * r3[st, :, b] + S.astype(F64)).astype(F32), S)
            S = tree(S)
        self.X = Xf.astype(np.int64)
        self.h = (self.X + 128) >> 8
        self.l = self.X - 256 * self.h
        assert np.all(np.abs(self.h) <= 127) and np.all((-128 <= self.l) & (self.l <= 127))  # both planes are int8
        hh, hl, ll = wrap32((self.h * self.h).sum()), wrap32((self.h * self.l).sum()), wrap32((self.l * self.l).sum())
        self.sumX2 = 65536.0 * hh + 512.0 * hl + float(ll)  # double, exact
        self.ok, self.sx = ok, (sx if ok else F32(0))
        self.delta, self.nx2 = F32(np.inf), F32(0)
        if ok:
            with np.errstate(**NP_QUIET):
                self.delta = F32(F32(sx * F32(np.sqrt(S))) * UP)
                if metric == "cos":
                    self.delta = F32(F32(self.delta / F32(ra)) * UP)
                self.nx2 = F32(F32(sx * sx) * F32(self.sumX2))
        if "delta" in mutate:
            self.delta = F32(0)


def row_sums(st, c):
    """the three eight-lane sums: lane g takes screen chunks g, g + 8, ... (16 codes each); int32 per lane and over the group"""
    cp = np.zeros(st.X.size, np.int64); cp[: c.size] = c
    out = []
    for a in (st.h, st.l, cp):
        per = (a * cp).reshape(-1, 16).sum(axis=1)
        lanes = [wrap32(per[g::8].sum()) for g in range(8)]
        out.append(wrap32(sum(lanes)))
    return out  # Ih, Il, C2


def f_of_I(ih, il):
    return F32(256.0 * float(ih) + float(il))  # exact in double (< 2^53), one rounding


def eps(chunks):
    return max(E12, F32((2 * chunks + 64) * 2.0 ** -24))


def l2_threshold(st, c, s, r, chunks, mutate=()):
    """the value the l2sq test compares with the radius (LB (1 - e)), or None where no test is made"""
    ih, il, c2 = row_sums(st, c)
    ome = F32(1) - eps(chunks)
    if not l2_scale_ok(s):
        return None
    with np.errstate(**NP_QUIET):
        fI = f_of_I(ih, il)
        R = F32(F32(F32(2) * F32(st.sx * s)) * fI)
        Q = F32(F32(s * s) * F32(c2))
        eta = F32(0) if "eta" in mutate else F32(F32(2.0 ** -20) * F32(st.nx2 + Q))
        m = F32(F32(F32(st.nx2 - R) + Q) - eta)
        if not np.isfinite(m):
            return None
        a = F32(F32(F32(F32(np.sqrt(max(m, F32(0)))) * ome) - r) - st.delta)
        lb = F32(a * a) if a > 0 else F32(0)
        if not lb > F32(2.0 ** -100):
            return None
        return F32(lb * ome)


def cos_threshold(st, c, t, rho, ra, chunks):
    """1 - u - e, or None where no test is made"""
    if not (cs.LO <= ra <= cs.HI):
        return None
    ih, il, _ = row_sums(st, c)
    e = eps(chunks)
    with np.errstate(**NP_QUIET):
        sim8 = F32(F32(F32(f_of_I(ih, il) * st.sx) * t) / ra)
        ub = F32(F32(F32(sim8 + F32(rho * F32(F32(1) + st.delta))) + st.delta) + e)
        return F32(F32(F32(1) - ub) - e)


def rejects(thr, radius):
    return thr is not None and bool(thr > radius)  # (a NaN fails)


# ---- 1. soundness ---------------------------------------------------------------------------------------------------------------
def l2_lists(d):
    rng = np.random.default_rng(d)
    rows = l2.adversarial(rng, d)
    queries = [r.copy() for r in rows[:6]] + [rows[0] + F32(1e-3) * rng.standard_normal(d).astype(F32)]
    queries += [rng.standard_normal(d).astype(F32) * F32(sc) for sc in (1, 1e-3, 1e3, 1e-25, 1e25)]
    o = rng.standard_normal(d).astype(F32); o[rng.integers(0, d)] = F32(1e4); queries.append(o)  # (the outlier, as a query)
    queries += [r.copy() for r in rows[6:]]  # every adversarial row is a query too: x = y on the int8 grid, the non-finite ones
    return rows, queries


def check_sound(metric, d, mutate=()):
    chunks = (d + 3) // 4
    checked = far = never = 0
    if metric == "l2sq":
        rows, queries = l2_lists(d)
        staged = [Staged(x, metric, mutate=mutate) for x in queries]
        for y in rows:
            c, s, r = l2.screen_of(y)
            for x, st in zip(queries, staged):
                with np.errstate(**NP_QUIET):
                    dist = F32(oracle.distance(x, y, "l2sq", oracle.SUM_WAVE64))
                thr = l2_threshold(st, c, s, r, chunks, mutate)
                if not st.ok:
                    assert not rejects(thr, F32(-np.inf)); never += 1
                if np.isnan(dist):
                    continue
                assert not rejects(thr, dist), (d, None if thr is None else float(thr), float(dist), float(r), float(st.delta))
                checked += 1
                far += rejects(thr, F32(-1))
    else:
        with np.errstate(**NP_QUIET):
            rows, queries = cs.families(np.random.default_rng(d), d)
        qs = [(x, cs.rooted_norm(x)) for x in queries]
        staged = {(i, ka): Staged(x, metric, ra=cs.nudged(ra, ka), mutate=mutate) for i, (x, ra) in enumerate(qs) for ka in (0, -2, 2)}
        for y in rows:
            rb = cs.rooted_norm(y)
            with np.errstate(**NP_QUIET):
                c, t, rho = cs.screen_of(y, rb)
                dists = [F32(oracle.distance(x, y, "cos", oracle.SUM_WAVE64)) for x, _ in qs]
            for i, ((x, ra), dist) in enumerate(zip(qs, dists)):
                for ka in (0, -2, 2):
                    st = staged[(i, ka)]
                    thr = cos_threshold(st, c, t, rho, cs.nudged(ra, ka), chunks)
                    if not st.ok:
                        assert not rejects(thr, F32(-np.inf)); never += 1
                    if np.isnan(dist):
                        continue
                    assert not rejects(thr, dist), (d, float(thr), float(dist), float(rho), float(ra), ka)
                checked += 1
                far += rejects(cos_threshold(staged[(i, 0)], c, t, rho, ra, chunks), F32(-1))
    return checked, far, never


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_the_integer_bound_never_exceeds_the_device_distance(metric, d):
    """at radius = the pair's own f32 distance (the oracle's SUM_WAVE64 order) the test rejects nothing: rejection is monotone in the
    radius, so it rejects at no radius the exact evaluation would have let the row into"""
    checked, far, never = check_sound(metric, d)
    assert checked > 0 and never > 0  # (the lists hold queries that cannot be quantised: zero, non-finite, 1e25 for l2sq)
    if d >= 16:
        assert far > 0  # the restatement can reject at all


def test_queries_that_cannot_be_quantised_reject_nothing():
    rng = np.random.default_rng(11)
    d = 768
    g = rng.standard_normal(d).astype(F32)
    y = rng.standard_normal(d).astype(F32)
    bad = [np.zeros(d, F32)]
    for v in (np.nan, np.inf, -np.inf):
        b = g.copy(); b[5] = F32(v); bad.append(b)
    for x in bad:
        for metric in ("l2sq", "cos"):
            st = Staged(x, metric, ra=F32(1))
            assert not st.ok and np.isposinf(st.delta) and not st.X.any() and st.sx == 0
    c, s, r = l2.screen_of(y)
    for x in bad + [g * F32(1e-25), g * F32(1e25)]:  # (l2sq: a scale outside screen_l2_scale_ok)
        st = Staged(x, "l2sq")
        assert not st.ok and not rejects(l2_threshold(st, c, s, r, 192), F32(-np.inf))
    rb = cs.rooted_norm(y)
    c, t, rho = cs.screen_of(y, rb)
    for x in bad:
        assert not rejects(cos_threshold(Staged(x, "cos", ra=F32(1)), c, t, rho, F32(1), 192), F32(-np.inf))
    for sc in (1e-25, 1e25):  # (cosine: the query's norm is outside the range -- the planes are fine, the test is not made)
        x = g * F32(sc)
        ra = cs.rooted_norm(x)
        assert not rejects(cos_threshold(Staged(x, "cos", ra=ra), c, t, rho, ra, 192), F32(-np.inf))


def test_the_planes_hold_the_query():
    """X = 256 h + l in [-32639, 32639], the largest component at +-32639, and sx X within delta of x"""
    rng = np.random.default_rng(12)
    for d in (509, 768, 2000):
        x = rng.standard_normal(d).astype(F32)
        st = Staged(x, "l2sq")
        assert st.ok and np.abs(st.X).max() == XMAX and np.array_equal(256 * st.h + st.l, st.X)
        err = np.sqrt(((x.astype(F64) - float(st.sx) * st.X[:d]) ** 2).sum())
        assert err <= float(st.delta) <= 1.05 * err
        assert abs(float(st.nx2) - float(st.sx) ** 2 * float((st.X ** 2).sum())) <= 4 * 2.0 ** -24 * float(st.nx2)


# ---- 2. overflow ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1, -1])
def test_sums_at_the_edge_of_int32(sign):
    """d = 2000, every code +-127 against a query whose X are all 32639: the eight-lane sums fit int32, I = 256 Ih + Il does not; the
    restated device sums are the exact integers, and the verdicts at half and at twice the true distance are reject and keep"""
    d = 2000
    x = np.ones(d, F32)
    y = np.full(d, F32(3.0 if sign > 0 else -1.0))
    st = Staged(x, "l2sq")
    assert st.ok and np.all(st.X[:d] == XMAX)
    c, s, r = l2.screen_of(y)
    assert np.all(c == sign * 127)
    ih, il, c2 = row_sums(st, c)
    X, cc = [int(v) for v in st.X[:d]], [int(v) for v in c]
    exact_I = sum(a * b for a, b in zip(X, cc))
    assert ih == sum(((a + 128) >> 8) * b for a, b in zip(X, cc)) and c2 == sum(b * b for b in cc) == d * 127 * 127
    assert 256 * ih + il == exact_I == sign * d * XMAX * 127 and abs(exact_I) > 2 ** 32
    assert float(f_of_I(ih, il)) == float(F32(exact_I))
    assert st.sumX2 == float(sum(a * a for a in X)) and st.sumX2 > 2.0 ** 40
    dist = F32(oracle.distance(x, y, "l2sq", oracle.SUM_WAVE64))
    assert dist == F32(8000)
    thr = l2_threshold(st, c, s, r, 500)
    assert rejects(thr, F32(0.5) * dist) and not rejects(thr, F32(2) * dist)
    # cosine: distance 2 against the -127 row (reject at 1, keep at 4), 0 against the +127 row (keep at any radius >= 2 e)
    ra, rb = cs.rooted_norm(x), cs.rooted_norm(y)
    cc_, t, rho = cs.screen_of(y, rb)
    thr = cos_threshold(Staged(x, "cos", ra=ra), cc_, t, rho, ra, 500)
    if sign < 0:
        assert rejects(thr, F32(1)) and not rejects(thr, F32(4))
    else:
        assert not rejects(thr, F32(2) * eps(500)) and rejects(thr, F32(-0.01))


# ---- 3. closeness to the float form ---------------------------------------------------------------------------------------------
def float_threshold(metric, x, c, m0, m1, ra, chunks):
    """the float restatement's compared value (tests/test_screen_bound.py, test_screen_bound_cos.py)"""
    if metric == "l2sq":
        lb, ome = l2.lower_bound(x, c, m0, m1, chunks)
        return F32(lb * ome)
    e = eps(chunks)
    sim8 = F32(F32(cs.screen_dot(x, c) * m0) / ra)
    return F32(F32(F32(1) - F32(F32(sim8 + m1) + e)) - e)


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_the_integer_threshold_is_within_e_of_the_float_one(metric):
    """the 64 Gaussian rows and three Gaussian queries of tests/test_gpu_screen_rows.py at its seven widths: the device must decide as
    the FLOAT restatement 2 e either side of that restatement's threshold (its T7); the integer threshold may use half of that"""
    from tests import test_gpu_screen_rows as rows_mod

    worst = 0.0
    for d in rows_mod.DIMS:
        chunks = (d + 3) // 4
        gauss = [r for f, r in rows_mod.rows_of(d) if f == "gaussian"]
        assert len(gauss) == 64
        for x in rows_mod.gaussian_queries(d):
            ra = cs.rooted_norm(x) if metric == "cos" else None
            st = Staged(x, metric, ra=ra)
            for y in gauss:
                if metric == "l2sq":
                    c, m0, m1 = l2.screen_of(y)
                    ti = l2_threshold(st, c, m0, m1, chunks)
                else:
                    c, m0, m1 = cs.screen_of(y, cs.rooted_norm(y))
                    ti = cos_threshold(st, c, m0, m1, ra, chunks)
                tf = float_threshold(metric, x, c, m0, m1, ra, chunks)
                assert ti is not None
                gap = abs(float(ti) - float(tf)) / (float(tf) if metric == "l2sq" else 1.0)
                assert float(ti) <= float(tf) + 2.0 ** -16 * max(abs(float(tf)), 1.0)  # looser, never tighter (up to the float form's own rounding)
                worst = max(worst, gap)
                assert gap <= float(eps(chunks)), (d, float(ti), float(tf))
    print(f"{metric}: integer threshold against the float one, largest gap {worst:.3e} ({'relative' if metric == 'l2sq' else 'absolute'}); e = 2^-12 = {2.0 ** -12:.3e}")


def test_the_cosine_bound_needs_its_delta_term():
    """sigma <= sx s I / (X Y) + rho (1 + dq) + dq in float64 over the published f32 values -- and on rows that lie (nearly) on the int8
    grid, where rho ~ 1e-7, the inequality fails for some query once the dq terms are dropped: e hides that from the f32 test above"""
    rng = np.random.default_rng(13)
    d = 768
    needed = 0
    for _ in range(8):
        y = (rng.integers(-127, 128, d) * F32(0.01)).astype(F32)
        y[0] = F32(1.27)
        rb = cs.rooted_norm(y)
        c, t, rho = cs.screen_of(y, rb)
        assert float(rho) < 1e-6
        s = float(F32(np.max(np.abs(y))) / F32(127))
        for _ in range(8):
            x = rng.standard_normal(d).astype(F32)
            st = Staged(x, "cos", ra=cs.rooted_norm(x))
            X_, Y_ = np.linalg.norm(x.astype(F64)), np.linalg.norm(y.astype(F64))
            sigma = float(x.astype(F64) @ y.astype(F64)) / (X_ * Y_)
            ih, il, _ = row_sums(st, c)
            sim = float(st.sx) * s * (256 * ih + il) / (X_ * Y_)
            dq = float(st.delta)
            assert sigma <= sim + float(rho) * (1 + dq) + dq
            needed += sigma > sim + float(rho)
    assert needed > 0
