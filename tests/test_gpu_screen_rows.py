"""The int8 screen as the DEVICE stored it and as the DEVICE decides with it, against the host in float64 and exact
rationals.  tests/test_screen_bound*.py prove the bound on a numpy restatement and tests/test_gpu_screen*.py prove that answers do not
change with the screen on the data they search; here the bytes k_fill_screen wrote (GpuIndex.export_screen) and the verdicts of
hop_distances_screened itself (GpuIndex.screen_probe) are held to the restatement and to the mathematics:

  T1 l2sq rows: codes and s equal screen_of bit for bit; r^2 >= sum (y - s q)^2 and <= (1 + 2^-22)^2 times it, exactly;
     |y / s - q| <= 0.5 + 2^-16; r within one ulp of screen_of's.
  T2 cosine rows: the same codes; meta.x == f32(s / rb) for the exported norm rb; rho^2 >= sum (y - s c)^2 / sum y^2 and
     <= (1 + 2^-22)^2 times it, exactly; the exported norm within (m / 2 + 1) u + 2^-20 of the float64 norm.
  T3 rows the screen must never reject are stored as (codes 0, s 0, r +inf); every other row has a finite r.
  T4 every path that stores rows ends in the same screen bytes.
  T5 the restated test over the device's stored rows never rejects a row at the device's own distance of it.
  T6 neither does the device, at the distance, one ulp above it and at twice it; never-reject rows and queries reject nothing.
  T7 away from the knife edge the device's verdict is the restatement's.
  T8 the device's test is not vacuous.
  T9 verdicts do not depend on the number of slots in the hop, on their position or on the workgroup size.

Why the bounds are what they are: r (rho) is the double square root of the double sum times (1 + 2^-40), rounded up into f32 -- one
rounding of at most 2^-23 relative on top of 2^-40 and the double sums' own ~2^-42: (1 + 2^-22)^2 covers the square.  The code of a
value is rint of the F32 quotient y / s, |y / s| <= 127 (1 + 2^-23): the quotient rounds by at most 2^-17, 2^-16 with room."""
import threading
from fractions import Fraction

import numpy as np
import pytest

from tests import test_screen_bound as l2
from tests import test_screen_bound_cos as cs

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
DIMS = [509, 512, 513, 768, 1021, 1028, 2000]
METRICS = ["l2sq", "cos"]
ADVERSARIAL = ["gauss", "zero", "x1e-30", "x1e30", "x1e-20", "x3e18", "outlier", "mixed_scale", "constant", "int8_grid", "pos_inf", "nan", "subnormal"]
NONFINITE = ("pos_inf", "neg_inf", "nan")
NEVER = {"l2sq": {"zero", "subnormal"} | set(NONFINITE), "cos": {"zero", "subnormal", "x1e-30", "x1e30", "x1e-20", "x3e18", "mixed_scale"} | set(NONFINITE)}
M, EFC = 8, 32


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


# ---- rows, queries, and the two indexes of a (metric, d) ------------------------------------------------------------------------
def rows_of(d):
    """[(family, row)]: adversarial()'s rows, a -inf row, a row on rint ties, a row with +-max in several places, 64 Gaussian rows"""
    rng = np.random.default_rng(d)
    adv = l2.adversarial(rng, d)
    assert len(adv) == len(ADVERSARIAL)
    rows = list(zip(ADVERSARIAL, adv))
    ninf = rng.standard_normal(d).astype(F32); ninf[d // 3] = F32(-np.inf); rows.append(("neg_inf", ninf))
    # ties: max |y| = 127 * 2^-5, so s = 2^-5 exactly and y / s = k + 0.5 exactly over the first half
    s0 = F32(2.0 ** -5)
    t = np.clip(rng.standard_normal(d), -3.9, 3.9).astype(F32)
    k = rng.integers(-127, 127, d // 2)
    t[: d // 2] = (s0 * (k.astype(F32) + F32(0.5))).astype(F32)
    t[-1] = F32(127) * s0
    rows.append(("ties", t))
    m = np.clip(rng.standard_normal(d), -4.5, 4.5).astype(F32)
    for i, sign in ((0, 1), (7, -1), (d // 2, -1), (d - 2, 1), (d - 1, -1)):
        m[i] = F32(sign * 5.0)
    rows.append(("max", m))
    rows += [("gaussian", rng.standard_normal(d).astype(F32)) for _ in range(64)]
    return rows


def queries_of(metric, d, rows):
    """the list of test_lower_bound_never_exceeds_the_device_distance over these rows; cosine: and what its twin's families() adds"""
    rng = np.random.default_rng(d + 1)
    qs = [r.copy() for _, r in rows[:6]] + [rows[0][1] + F32(1e-3) * rng.standard_normal(d).astype(F32)]
    qs += [rng.standard_normal(d).astype(F32) * F32(sc) for sc in (1, 1e-3, 1e3, 1e-25, 1e25)]
    if metric == "cos":
        with np.errstate(over="ignore"):
            qs += cs.families(np.random.default_rng(d), d)[1][len(qs):]
    return qs


def ring(n):
    nbr0 = np.full((n, 2 * M), 0xFFFFFFFF, np.uint32)
    if n > 1:
        nbr0[:, 0] = (np.arange(n) + 1) % n
        nbr0[:, 1] = (np.arange(n) - 1) % n
    return {"levels": np.zeros(n, np.uint8), "nbr0": nbr0, "upper_off": np.full(n, 0xFFFFFFFF, np.uint32),
            "upper_nbr": np.zeros((0, M), np.uint32), "labels": np.arange(n, dtype=np.uint64) + 1, "entry_slot": 0, "max_level": 0}


class Case:
    """One (metric, d): the finite rows in an index built by add_many, the non-finite rows in a second one filled by import_graph
    under a hand-made ring (no walk ever runs over them); what export_screen returns for both, joined row by row."""

    def __init__(self, capi, metric, d):
        self.metric, self.d = metric, d
        self.chunks = (d + 3) // 4
        self.sch = (self.chunks + 3) // 4
        rows = rows_of(d)
        fin = [(f, r) for f, r in rows if f not in NONFINITE]
        non = [(f, r) for f, r in rows if f in NONFINITE]
        self.fam = [f for f, _ in fin] + [f for f, _ in non]
        self.rows = [r for _, r in fin] + [r for _, r in non]
        self.nfin = len(fin)
        self.built = capi.GpuIndex(metric, d, M=M, ef_construction=EFC, ef=32, seed=3)
        self.built.add_many(np.arange(len(fin), dtype=np.uint64) + 1, np.stack([r for _, r in fin]))
        self.imported = capi.GpuIndex(metric, d, M=M, ef_construction=EFC, ef=32, seed=3)
        self.imported.import_graph(np.stack([r for _, r in non]), ring(len(non)))
        a, b = self.built.export_screen(), self.imported.export_screen()
        assert a["row_bytes"] == b["row_bytes"] == self.sch * 16
        self.codes = np.concatenate([a["codes"], b["codes"]])
        self.meta = np.concatenate([a["meta"], b["meta"]])
        self.norms = np.concatenate([a["norms"], b["norms"]]) if metric == "cos" else None
        self.queries = queries_of(metric, d, rows)
        self.e = cs.eps(self.chunks)
        self._dist = {}

    def where(self, i):
        """(index, slot) of row i"""
        return (self.built, i) if i < self.nfin else (self.imported, i - self.nfin)

    def family(self, name):
        return [i for i, f in enumerate(self.fam) if f == name]

    def dists(self, qi, x):
        """the device's own distances of query x to every row (once per query)"""
        if qi not in self._dist:
            self._dist[qi] = np.concatenate([self.built.distance_gather(x, np.arange(self.nfin)),
                                             self.imported.distance_gather(x, np.arange(len(self.rows) - self.nfin))])
        return self._dist[qi]

    def probe(self, x, rows, radius, wg=256):
        """screen_probe over rows (indices into self.rows) that live in one of the two indexes"""
        ix = self.where(rows[0])[0]
        assert all(self.where(i)[0] is ix for i in rows)
        return ix.screen_probe(x, [self.where(i)[1] for i in rows], radius, wg)

    def host_rejects(self, x, i, radius, ra=None):
        """the restated test over the device's stored (codes, s, r) / (codes, s / rb, rho) of row i"""
        c = self.codes[i, : self.d]
        if self.metric == "l2sq":
            lb, ome = l2.lower_bound(x, c, self.meta[i, 0], self.meta[i, 1], self.chunks)
            return l2.rejects_at(lb, ome, radius)
        return cs.rejects_at(cs.screen_dot(x, c), self.meta[i, 0], self.meta[i, 1], cs.rooted_norm(x) if ra is None else ra, self.e, radius)

    def host_bound(self, x, i, ra):
        """float64: the value the test compares with the radius -- l2sq LB (1 - e) from the restatement's (lb, ome), cosine
        1 - (sim8 + rho + e) - e from the restatement's f32 dot product -- and, l2sq, (a, sqrt(d'))"""
        c = self.codes[i, : self.d]
        if self.metric == "l2sq":
            lb, ome = l2.lower_bound(x, c, self.meta[i, 0], self.meta[i, 1], self.chunks)
            yp = (self.meta[i, 0] * c.astype(F32)).astype(np.float64)
            return float(lb) * float(ome), float(lb), np.sqrt(((x.astype(np.float64) - yp) ** 2).sum())
        sim8 = float(cs.screen_dot(x, c)) * float(self.meta[i, 0]) / float(ra)
        return 1.0 - (sim8 + float(self.meta[i, 1]) + float(self.e)) - float(self.e), None, None


_cases = {}


def case(capi, metric, d):
    if (metric, d) not in _cases:
        _cases[(metric, d)] = Case(capi, metric, d)
    return _cases[(metric, d)]


# ---- exact arithmetic over f32 values -------------------------------------------------------------------------------------------
def scaled_ints(arrays):
    """f32 arrays -> lists of Python ints v * 2^-E and the common E (every finite f32 is an integer times a power of two)"""
    parts = [np.frexp(np.asarray(a, dtype=np.float64)) for a in arrays]
    E = min(int(e.min()) for _, e in parts) - 53
    return [[int(mi) << (int(ei) - 53 - E) for mi, ei in zip((m * 2.0 ** 53).astype(np.int64), e)] for m, e in parts], E


def exact_error(y, s, c):
    """exactly, as Fractions: sum (y - y')^2 and sum y^2 (y' the f32 products s * c: screen_val), and whether every
    |y - s c| <= (0.5 + 2^-16) s with the real product s c"""
    yp = (F32(s) * c.astype(F32)).astype(F32)
    (Y, YP, S), E = scaled_ints([y, yp, np.array([s], F32)])
    unit = Fraction(4) ** E  # (the square of the common scale)
    r2 = sum((a - b) ** 2 for a, b in zip(Y, YP)) * unit
    y2 = sum(a * a for a in Y) * unit
    codes_ok = all(abs(a - S[0] * int(q)) * 2 ** 16 <= (2 ** 15 + 1) * S[0] for a, q in zip(Y, c))
    return r2, y2, codes_ok


def ulps_apart(a, b):
    return abs(int(np.asarray(a, F32).view(np.int32)) - int(np.asarray(b, F32).view(np.int32)))  # (positive values)


UP = Fraction(2 ** 22 + 1, 2 ** 22) ** 2


# ---- T1, T2, T3: what was stored ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_T1_l2sq_rows_are_the_restatement_and_r_bounds_the_error_exactly(capi, d):
    c = case(capi, "l2sq", d)
    checked = 0
    for i, y in enumerate(c.rows):
        assert not c.codes[i, d:].any(), (c.fam[i], "padding codes")
        q, s, r = l2.screen_of(y)
        dq, ds, dr = c.codes[i, :d], c.meta[i, 0], c.meta[i, 1]
        assert np.array_equal(dq, q), (c.fam[i], np.flatnonzero(dq != q)[:8])
        assert ds.view(np.uint32) == np.asarray(s, F32).view(np.uint32), (c.fam[i], float(ds), float(s))
        if not np.isfinite(r):
            assert np.isposinf(dr), (c.fam[i], float(dr))
            continue
        assert np.isfinite(dr) and ulps_apart(dr, r) <= 1, (c.fam[i], float(dr), float(r))
        r2, _, codes_ok = exact_error(y, ds, dq)
        rr = Fraction(float(dr)) ** 2
        assert rr >= r2, (c.fam[i], "r is below the error it bounds", float(dr))
        assert rr <= UP * r2, (c.fam[i], "r is looser than one rounding up", float(dr), float(rr / r2) if r2 else None)
        assert codes_ok, (c.fam[i], "a code is more than half a step from its value")
        checked += 1
    assert checked >= 70


@pytest.mark.parametrize("d", DIMS)
def test_T2_cosine_rows_fold_the_exported_norm_and_rho_bounds_the_error_exactly(capi, d):
    c = case(capi, "cos", d)
    m = (c.chunks + 63) // 64 * 4 + 6
    checked = 0
    for i, y in enumerate(c.rows):
        assert not c.codes[i, d:].any(), (c.fam[i], "padding codes")
        rb = c.norms[i]
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            q, t, rho = cs.screen_of(y, rb)
        dq, dt, drho = c.codes[i, :d], c.meta[i, 0], c.meta[i, 1]
        assert np.array_equal(dq, q), (c.fam[i], np.flatnonzero(dq != q)[:8])
        assert dt.view(np.uint32) == np.asarray(t, F32).view(np.uint32), (c.fam[i], float(dt), float(t), float(rb))
        if not np.isfinite(rho):
            assert np.isposinf(drho), (c.fam[i], float(drho))
            continue
        assert np.isfinite(drho)
        assert np.array_equal(dq, l2.screen_of(y)[0]), (c.fam[i], "not the l2sq codes")
        s = F32(np.max(np.abs(y))) / F32(127)
        r2, y2, codes_ok = exact_error(y, s, dq)
        rr = Fraction(float(drho)) ** 2 * y2
        assert rr >= r2, (c.fam[i], "rho is below the relative error it bounds", float(drho))
        assert rr <= UP * r2, (c.fam[i], "rho is looser than one rounding up", float(drho))
        assert codes_ok, (c.fam[i], "a code is more than half a step from its value")
        n64 = np.sqrt((y.astype(np.float64) ** 2).sum())
        assert abs(float(rb) - n64) <= ((m / 2 + 1) * U + 2.0 ** -20) * n64, (c.fam[i], float(rb), n64)
        checked += 1
    assert checked >= 64


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_T3_never_rejected_rows_are_stored_as_such_and_no_other_row_is(capi, metric, d):
    c = case(capi, metric, d)
    seen = set()
    for i, f in enumerate(c.fam):
        if f in NEVER[metric]:
            assert not c.codes[i].any() and c.meta[i, 0] == 0 and np.isposinf(c.meta[i, 1]), (f, c.meta[i])
            seen.add(f)
        else:
            assert c.meta[i, 0] > 0 and np.isfinite(c.meta[i, 0]) and np.isfinite(c.meta[i, 1]) and c.meta[i, 1] >= 0, (f, c.meta[i])
            assert np.abs(c.codes[i, :d].astype(np.int32)).max() == 127, f  # the largest value sits on the last code
    assert seen == NEVER[metric]


# ---- T4: every path that stores rows ------------------------------------------------------------------------------------------------
def same_screen(a, b):
    return (a["row_bytes"] == b["row_bytes"] > 0 and np.array_equal(a["codes"], b["codes"]) and
            np.array_equal(a["meta"].view(np.uint32), b["meta"].view(np.uint32)) and
            (a["norms"] is None) == (b["norms"] is None) and (a["norms"] is None or np.array_equal(a["norms"].view(np.uint32), b["norms"].view(np.uint32))))


@pytest.mark.parametrize("metric", METRICS)
def test_T4_every_path_that_stores_rows_ends_in_the_same_screen(capi, metric):
    d = 513
    base = np.stack([r for f, r in rows_of(d) if f not in NONFINITE])
    n = len(base)
    labels = np.arange(n, dtype=np.uint64) + 1

    def fresh():
        return capi.GpuIndex(metric, d, M=M, ef_construction=EFC, ef=32, seed=3)

    twin = fresh()
    twin.add_many(labels, base)
    want = twin.export_screen()
    assert want["codes"].shape == (n, 33 * 16) and want["codes"].any()
    one = fresh()
    for lab, row in zip(labels, base):
        one.add(lab, row)
    assert same_screen(one.export_screen(), want), "one add at a time (the export flushes the buffered ones)"
    grown = fresh()
    grown.reserve(8)
    grown.add_many(labels[:8], base[:8])
    cap0 = grown.capacity
    grown.add_many(labels[8:], base[8:])
    assert cap0 < n <= grown.capacity
    assert same_screen(grown.export_screen(), want), "grown past its reserve"
    loaded = fresh()
    loaded.load_buffer(twin.save_buffer())
    assert same_screen(loaded.export_screen(), want), "load_buffer"
    imported = fresh()
    imported.import_graph(base, twin.export_graph())
    assert same_screen(imported.export_screen(), want), "import_graph"
    comms = capi.Comm.local_world(2)
    cut, out, errs = capi.shard_range(n, 2, 1)[0], [None, None], []

    def run(r):
        try:
            comms[r].set_timeout(120)
            ix = fresh()
            lo, hi = (0, cut) if r == 0 else (cut, n)
            ix.add_sharded(comms[r], labels[lo:hi], base[lo:hi])
            out[r] = ix
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            errs.append((r, repr(e)))

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for r, ix in enumerate(out):
        assert len(ix) == n and same_screen(ix.export_screen(), want), f"rank {r} of a world-2 work-sharded add"
    # a part of the range is that part of the whole; a range past the size is refused; the end of the index is an empty range
    part = twin.export_screen(5, 9)
    assert np.array_equal(part["codes"], want["codes"][5:14]) and np.array_equal(part["meta"].view(np.uint32), want["meta"][5:14].view(np.uint32))
    assert twin.export_screen(n, 0)["codes"].shape == (0, 33 * 16)
    for first, count in ((0, n + 1), (n, 1), (n + 1, 0)):
        with pytest.raises(capi.LanternGpuError, match="slot range out of the index"):
            twin.export_screen(first, count)


def test_an_index_without_a_screen_exports_none(capi, monkeypatch):
    rng = np.random.default_rng(0)
    for metric, d, quant in (("l2sq", 508, "f32"), ("cos", 508, "f32"), ("l2sq", 512, "f16"), ("cos", 512, "i8")):
        ix = capi.GpuIndex(metric, d, M=M, ef_construction=EFC, quantization=quant)
        ix.add_many([1, 2, 3], rng.standard_normal((3, d), dtype=np.float32))
        got = ix.export_screen()
        assert got["row_bytes"] == 0 and got["codes"].shape == (3, 0) and got["meta"] is None, (metric, d, quant)
        with pytest.raises(capi.LanternGpuError, match="no int8 screen"):
            ix.screen_probe(np.zeros(d, np.float32), [0], 1.0)
    monkeypatch.setenv("LANTERN_GPU_SCREEN", "0")
    ix = capi.GpuIndex("l2sq", 512, M=M, ef_construction=EFC)
    ix.add_many([1, 2, 3], rng.standard_normal((3, 512), dtype=np.float32))
    assert ix.export_screen()["row_bytes"] == 0
    monkeypatch.delenv("LANTERN_GPU_SCREEN")
    ix = capi.GpuIndex("l2sq", 512, M=M, ef_construction=EFC)
    ix.add_many([1, 2, 3], rng.standard_normal((3, 512), dtype=np.float32))
    assert ix.export_screen()["row_bytes"] == 32 * 16
    with pytest.raises(capi.LanternGpuError, match="slot out of range"):
        ix.screen_probe(np.zeros(512, np.float32), [0, 3], 1.0)


# ---- T5, T6: soundness against the device's own distance ----------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_T5_the_restated_test_over_stored_rows_never_rejects_at_the_device_distance(capi, metric, d):
    c = case(capi, metric, d)
    checked = {f: 0 for f in c.fam}
    for qi, x in enumerate(c.queries):
        dist = c.dists(qi, x)
        ra = cs.rooted_norm(x) if metric == "cos" else None
        for i in range(len(c.rows)):
            if np.isnan(dist[i]):
                continue
            assert not c.host_rejects(x, i, dist[i], ra), (c.fam[i], qi, float(dist[i]), c.meta[i])
            checked[c.fam[i]] += 1
    print(f"{metric} d={d}: {sum(checked.values())} pairs checked, per family at least {min(k for f, k in checked.items() if f not in NONFINITE)}")
    # every family met a distance that is a number; a row with a NaN (cosine: or an infinity) is NaN away from everything, and is
    # held to more than that: no radius at all rejects it
    for f, k in checked.items():
        if k == 0:
            assert f in NONFINITE, f
            for i in c.family(f):
                assert not any(c.host_rejects(x, i, F32(-np.inf)) for x in c.queries[:12])


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_T6_the_device_never_rejects_a_row_inside_the_radius(capi, metric, d):
    """at radius = a row's gathered distance, one ulp above it and twice it (twice: where the distance is not negative, so that the
    radius is above it) the probe may reject no row whose distance is at most the radius -- the row itself among them"""
    c = case(capi, metric, d)
    calls = 0
    for qi, x in enumerate(c.queries):
        dist = c.dists(qi, x)
        for lo, hi in ((0, c.nfin), (c.nfin, len(c.rows))):  # the two indexes
            ds = dist[lo:hi]
            with np.errstate(over="ignore"):
                radii = {float(r) for v in ds if not np.isnan(v) for r in (v, np.nextafter(v, F32(np.inf)), (F32(2) * v if v >= 0 else v))}
            for radius in sorted(radii):
                inside = [lo + int(j) for j in np.argsort(-ds, kind="stable") if ds[j] <= radius][:64]  # the 64 nearest the radius
                got = c.probe(x, inside, radius, 256 if calls % 2 else 512)
                calls += 1
                assert not got.any(), (qi, radius, [(c.fam[i], float(dist[i])) for i, g in zip(inside, got) if g])
    print(f"{metric} d={d}: {calls} probe launches at radii at and above a row's distance")
    assert calls > 3 * len(c.queries)
    # rows the fill marked: no query, no radius
    never = [i for i, f in enumerate(c.fam) if f in NEVER[metric]]
    for x in c.queries[:12]:
        for radius in (-np.inf, -1.0, 0.0, 1e-30, 1.0, 1e30):
            for rows in ([i for i in never if i < c.nfin], [i for i in never if i >= c.nfin]):
                assert not c.probe(x, rows, radius).any(), (radius, rows)
    if metric == "cos":  # a query whose norm is outside the range is never tested
        x = (c.rows[c.family("gaussian")[0]] * F32(1e-20)).astype(F32)
        assert not cs.LO <= cs.rooted_norm(x) <= cs.HI
        for radius in (-np.inf, -1.0, 0.0, 1e-3, 1.0, 2.0):
            assert not c.probe(x, list(range(min(64, c.nfin))), radius).any(), radius


# ---- T7, T8, T9: the device's verdict ------------------------------------------------------------------------------------------------
def gaussian_queries(d, n=3):
    rng = np.random.default_rng(7 * d)
    return [rng.standard_normal(d).astype(F32) for _ in range(n)]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_T7_away_from_the_knife_edge_the_device_decides_as_the_restatement(capi, metric, d):
    """Gaussian pairs.  The device and the restatement differ by the order of a sum and the last place of a norm: under 259 u relative
    on LB (amplified at most fourfold through a >= sqrt(d') / 2) for l2sq, 2^-21 absolute for cosine -- both below e, so 2 e either
    side of the restated bound the verdict is fixed."""
    c = case(capi, metric, d)
    e = float(c.e)
    gs = c.family("gaussian")
    for x in gaussian_queries(d):
        ra = cs.rooted_norm(x) if metric == "cos" else None
        for n_, i in enumerate(gs):
            b, lb, sqd = c.host_bound(x, i, ra)
            if metric == "l2sq":
                assert lb > 2.0 ** -90 and np.sqrt(lb) >= sqd / 2, (lb, sqd)
                below, above = F32(b * (1 - 2 * e)), F32(b * (1 + 2 * e))
            else:
                below, above = F32(b - 2 * e), F32(b + 2 * e)
            assert c.host_rejects(x, i, below, ra) and not c.host_rejects(x, i, above, ra), (i, b)
            wg = 256 if n_ % 2 else 512
            assert c.probe(x, [i], below, wg)[0], (i, "the device keeps a row the restatement rejects", b, float(below))
            assert not c.probe(x, [i], above, wg)[0], (i, "the device rejects a row the restatement keeps", b, float(above))


@pytest.mark.parametrize("metric", METRICS)
def test_T8_the_device_rejects_far_rows(capi, metric):
    c = case(capi, metric, 768)
    gs = c.family("gaussian")
    for x in gaussian_queries(768, 2):
        dist = c.built.distance_gather(x, np.arange(c.nfin))
        for i in gs:
            assert c.probe(x, [i], F32(0.8) * dist[i])[0], (i, float(dist[i]))
        assert c.probe(x, gs, F32(0.8) * dist[gs].min()).all()  # and all of them in one hop


@pytest.mark.parametrize("d", [513, 768, 2000])
@pytest.mark.parametrize("metric", METRICS)
def test_T9_verdicts_do_not_depend_on_the_shape_of_the_hop(capi, metric, d):
    c = case(capi, metric, d)
    gs = c.family("gaussian")
    x = gaussian_queries(d, 1)[0]
    ra = cs.rooted_norm(x) if metric == "cos" else None
    radius = F32(np.median([c.host_bound(x, i, ra)[0] for i in gs]))  # about half of the rows are rejected
    want = dict(zip(gs, c.probe(x, gs, radius, 256)))
    assert 16 <= sum(want.values()) <= 48, sum(want.values())
    rng = np.random.default_rng(d)
    for n in (1, 31, 32, 33, 64):
        for wg in (256, 512):
            perm = [gs[j] for j in rng.permutation(64)]
            rows = perm[: n - 1] + [perm[0]] if n > 1 else perm[:1]  # (n > 1: the first slot is there twice)
            got = c.probe(x, rows, radius, wg)
            assert len(got) == n and [bool(g) for g in got] == [bool(want[i]) for i in rows], (n, wg)
