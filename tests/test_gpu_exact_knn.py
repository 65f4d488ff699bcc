"""The exact k-NN (lantern_gpu_exact_search, _assign_to_clusters, PQ encoding: dense.cpp exact_knn_device) against a brute force
in the pair kernel's reduction order, on data where the fp32-MFMA pre-selection's distances are rounding noise: a large common
offset with a small spread, near-duplicate groups larger than k + 16, ties beyond the survivors, lattices, scaled copies under
cosine, popcount ties.  Ids and distance bits must be identical; the referee itself is checked against float64.  Also: the
contraction's error bound E on the hardware, the certificate's counters, and that a certified call issues the
contraction launches it always did."""
import numpy as np
import pytest

from tests.exact_knn_bound import certify, mfma_error_cos, mfma_error_l2, gamma, padded_dims
from tests.value_range import STRICT, exact64, pair_rounding, within_rounding
from tests.test_gpu_quantized_indexes import quantize_reference

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0
    return capi


def empty_graph(n):
    return {"levels": np.zeros(n, np.uint8), "nbr0": np.full((n, 8), 0xFFFFFFFF, np.uint32), "upper_off": np.full(n, 0xFFFFFFFF, np.uint32),
            "upper_nbr": np.zeros((0, 4), np.uint32), "labels": None, "entry_slot": 0, "max_level": 0}


# ---- data families: (rows, queries), seeded, f32 (hamming: u32 words) ------------------------------------------------------
def fam_gauss(rng, n, d, nq):
    return rng.standard_normal((n, d), dtype=F32), rng.standard_normal((nq, d), dtype=F32)


def fam_offset(o, s):
    def make(rng, n, d, nq):
        return (F32(o) + F32(s) * rng.standard_normal((n, d), dtype=F32)).astype(F32), (F32(o) + F32(s) * rng.standard_normal((nq, d), dtype=F32)).astype(F32)
    return make


def fam_dupgroups(rng, n, d, nq):
    # groups of 40 copies of a centre, each copy 1e-3 noise away: 40 > k + 16 rows inside the contraction's rounding
    centres = rng.standard_normal(((n + 39) // 40, d), dtype=F32)
    rows = (np.repeat(centres, 40, axis=0)[:n] + F32(1e-3) * rng.standard_normal((n, d), dtype=F32)).astype(F32)
    q = (centres[rng.integers(0, min(centres.shape[0], max(1, n // 40)), nq)] + F32(1e-3) * rng.standard_normal((nq, d), dtype=F32)).astype(F32)
    return rows, q


def fam_repeated(rng, n, d, nq):
    # one row repeated 300 times among Gaussian rows: exact ties far beyond kk; the answer is the lowest slots
    rows = rng.standard_normal((n, d), dtype=F32)
    r = rows[0].copy()
    at = rng.choice(n, size=min(n, 300), replace=False)
    rows[at] = r
    q = rng.standard_normal((nq, d), dtype=F32)
    q[: (nq + 1) // 2] = r
    return rows, q


def fam_lattice(rng, n, d, nq):
    return rng.integers(-2, 3, (n, d)).astype(F32), rng.integers(-2, 3, (nq, d)).astype(F32)


def fam_scaled(rng, n, d, nq):
    # cosine: 300 scaled copies lambda c of one vector, zero rows, Gaussian rows; queries c, scaled c, zero, Gaussian
    rows = rng.standard_normal((n, d), dtype=F32)
    c = rng.standard_normal(d, dtype=F32)
    m = min(n, 300)
    at = rng.choice(n, size=m, replace=False)
    rows[at] = (c[None, :] * rng.uniform(0.01, 100.0, m).astype(F32)[:, None]).astype(F32)
    rows[rng.choice(n, size=min(n, 20), replace=False)] = 0
    q = rng.standard_normal((nq, d), dtype=F32)
    q[: (nq + 2) // 3] = (c[None, :] * rng.uniform(0.5, 2.0, (nq + 2) // 3).astype(F32)[:, None]).astype(F32)
    if nq > 2:
        q[-1] = 0
    return rows, q


def fam_bits(rng, n, w, nq):
    # a dozen bit patterns, each row one of them: popcount ties everywhere
    pats = rng.integers(0, 2 ** 32, size=(12, w), dtype=np.uint32)
    return pats[rng.integers(0, 12, n)].copy(), pats[rng.integers(0, 12, nq)].copy()


def fam_scaled_by(fam, s):
    return lambda rng, n, d, nq: tuple((a * F32(s)).astype(F32) for a in fam(rng, n, d, nq))


FAMILIES = {"gauss": fam_gauss, "offset10": fam_offset(10, 0.01), "offset100": fam_offset(100, 0.1), "dupgroups": fam_dupgroups,
            "repeated": fam_repeated, "lattice": fam_lattice, "scaled": fam_scaled, "bits": fam_bits,
            # i8 storage keeps trunc(100 x) in [-100, 100]: rows whose integers fill that range, and a common offset of 90 +- 2
            "i8gauss": fam_scaled_by(fam_gauss, 0.3), "i8offset": fam_offset(0.9, 0.02),
            # the edges of the f32 range (tests/value_range.py): norms^2 of 2^-85 and 2^117, denormal squares, sums that overflow
            "tiny": fam_scaled_by(fam_gauss, 2.0 ** -45), "huge": fam_scaled_by(fam_gauss, 2.0 ** 55), "denorm": fam_scaled_by(fam_gauss, 1e-20),
            "edge": STRICT["l2_edge"][2]}


# ---- the referee's own check against float64 (exact64, pair_rounding: tests/value_range.py) -----------------------------------------
def referee(oracle, cores, metric, storage, rows, queries, k):
    """oracle.bruteforce in the storage's sum mode over the stored values; checked against float64: the referee's k-th distance is
    within the pair kernel's rounding of the float64 k-th distance (order statistics move no more than the values do)"""
    if metric == "hamming":
        sr, sq, mode = rows, queries, oracle.SUM_WAVE64
    elif storage == "f16":
        sr, sq, mode = oracle.round_f16(rows), oracle.round_f16(queries), oracle.SUM_WAVE64_F16
    elif storage == "i8":
        sr, sq, mode = oracle.quantize_i8(rows), oracle.quantize_i8(queries), oracle.SUM_I8
    else:
        sr, sq, mode = rows, queries, oracle.SUM_WAVE64
    ids, dists = oracle.bruteforce(sr, sq, k, metric, mode, cores)
    kk = min(k, rows.shape[0])
    dims = padded_dims(rows.shape[1]) * (32 if metric == "hamming" else 1)
    for q0 in range(0, sq.shape[0], 128):
        d64 = exact64(metric, sr, sq[q0:q0 + 128])
        kth = np.partition(d64, kk - 1, axis=1)[:, kk - 1]
        got = dists[q0:q0 + 128, kk - 1].astype(np.float64)  # (a k-th distance above FLT_MAX is +inf: within_rounding)
        with np.errstate(invalid="ignore"):
            assert np.all(within_rounding(metric, got, kth, dims)), ("referee off float64", q0, np.max(np.abs(got - kth) - pair_rounding(metric, kth, dims)))
    return ids, dists, sr


def index_of(capi, metric, storage, rows, stored):
    d = rows.shape[1]
    ix = capi.GpuIndex(metric, d, M=4, ef_construction=8, seed=1, quantization=storage)
    ix.import_graph(stored if storage == "i8" else rows, empty_graph(rows.shape[0]))  # rows only: the exact search ignores the graph
    return ix


def run_case(capi, oracle, cores, monkeypatch, family, metric, n, d, nq, k, storage="f32", fused=True, seed=0):
    rng = np.random.default_rng([seed, n, d, nq, k])
    rows, queries = FAMILIES[family](rng, n, d, nq)
    ids, dists, stored = referee(oracle, cores, metric, storage, rows, queries, k)
    ix = index_of(capi, metric, storage, rows, stored)
    monkeypatch.setenv("LANTERN_GPU_DENSE_FUSED", "1" if fused else "0")
    before = capi.exact_knn_stats()
    slots, got = ix.exact_search(queries, k)
    after = capi.exact_knn_stats()
    bad = np.nonzero(np.any(slots != ids, axis=1) | np.any(got.view(np.uint32) != dists.view(np.uint32), axis=1))[0]
    assert bad.size == 0, (f"{bad.size} of {nq} queries differ from the brute force", bad[:8].tolist(), slots[bad[0]][:12].tolist(), ids[bad[0]][:12].tolist())
    ix.close()
    st = {key: after[key] - before[key] for key in after}
    st["range_refused"] = range_refusals(metric, stored, queries if storage == "f32" else None, k, dists[:, -1], padded_dims(d)) if metric != "hamming" else 0
    return st


def range_refusals(metric, rows, queries, k, dk, dims):
    """how many of the call's queries k_certify's RANGE rules refuse whatever the contraction found (tests/exact_knn_bound.py certify with
    tau = +inf).  Read off dense.cpp exact_knn_run / bruteforce.hip k_certify: one cosine ROW norm^2 outside [2^-60, 2^60] raises
    flag[nq] and the host clears every query's certificate -- all of the call's queries; a QUERY norm out of range, |q|^2 >= 2^120 and the
    l2sq rule (2 qa + sqrt(dup))^2 >= 2^120 are tested per query and refuse that query alone -- and only where the survivor list is full:
    with fewer than kk = k + 16 rows every row is a survivor and k_certify passes the query before it looks at a norm (certify's tau =
    None).  Norms in float64 here, in f32 on the device: a query within 2^-10 of a threshold is not counted."""
    if queries is None:
        return 0
    with np.errstate(over="ignore"):
        rn = (rows.astype(np.float64) ** 2).sum(1)
        qn = (queries.astype(np.float64) ** 2).sum(1)
    if metric == "cos" and np.any((rn != 0) & ((rn < 2.0 ** -61) | (rn > 2.0 ** 61))):
        return len(qn)
    if rows.shape[0] < k + 16:
        return 0
    slack = 1.0 + 2.0 ** -10
    return sum(1 for q2, d in zip(qn, dk.astype(np.float64))
               if not any(certify(metric, np.inf, dd, qq, dims) for qq in (q2 / slack, q2 * slack) for dd in (d / slack, d * slack)))


# (family, metric, n, d, nq, k): a list over the edges, not the product -- n: 1, fewer than k, the fused path's start (kSeedCols =
# 4096), the 64k chunk edges; d: the BK = 32 K-tail and the group widths; nq: the 128-row tile and the 1024-query block (QT)
CASES = [
    ("gauss", "l2sq", 1, 3, 1, 1),
    ("gauss", "l2sq", 9, 31, 127, 10),
    ("gauss", "cos", 4096, 32, 128, 100),
    ("gauss", "l2sq", 4097, 33, 129, 240),
    ("gauss", "l2sq", 65537, 128, 1025, 10),
    ("gauss", "cos", 131073, 33, 16, 10),
    ("offset10", "l2sq", 4000, 128, 16, 10),
    ("offset10", "l2sq", 4097, 1, 129, 10),
    ("offset10", "l2sq", 65536, 33, 128, 100),
    ("offset100", "l2sq", 4096, 768, 127, 10),
    ("offset100", "l2sq", 131073, 32, 16, 1),
    ("offset100", "cos", 20000, 31, 64, 10),
    ("dupgroups", "l2sq", 4000, 128, 16, 10),
    ("dupgroups", "l2sq", 65537, 3, 64, 100),
    ("dupgroups", "cos", 8000, 2000, 16, 10),
    ("repeated", "l2sq", 4097, 128, 8, 240),
    ("repeated", "cos", 9000, 33, 8, 10),
    ("lattice", "l2sq", 65537, 31, 128, 10),
    ("lattice", "l2sq", 9, 3, 1025, 10),
    ("scaled", "cos", 4097, 128, 129, 10),
    ("scaled", "cos", 20000, 3, 16, 100),
    ("bits", "hamming", 4097, 4, 128, 10),
    ("bits", "hamming", 65537, 25, 16, 240),
    # the edges of the f32 range; RANGE_ALL: the cases in which the certificate's range rules refuse every query of the call
    ("tiny", "cos", 4097, 33, 64, 10),       # row norms^2 ~ 2^-85 < 2^-60: flag[nq], every query falls back
    ("huge", "cos", 4097, 128, 64, 10),      # row norms^2 ~ 2^117 > 2^60: the same
    ("huge", "l2sq", 4097, 128, 64, 10),     # (2 qa + sqrt(dup))^2 >= 2^120, a per-query rule that every query of this set meets
    ("tiny", "l2sq", 4097, 33, 129, 10),
    ("denorm", "l2sq", 4097, 128, 16, 10),   # every distance below the bound's absolute term 4 (d + 8) 2^-126
    ("edge", "l2sq", 4000, 31, 16, 10),      # |q|^2 >= 1e36 chi^2_31 > 2^120, +inf distances: contraction keys inf and inf - inf
    ("huge", "l2sq", 65537, 33, 16, 100),
]
RANGE_ALL = {("tiny", "cos", 4097), ("huge", "cos", 4097), ("huge", "l2sq", 4097), ("edge", "l2sq", 4000)}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("family,metric,n,d,nq,k", CASES, ids=[f"{c[0]}-{c[1]}-n{c[2]}-d{c[3]}-q{c[4]}-k{c[5]}" for c in CASES])
def test_exact_search_is_the_brute_force(capi, oracle, cores, monkeypatch, family, metric, n, d, nq, k, fused):
    st = run_case(capi, oracle, cores, monkeypatch, family, metric, n, d, nq, k, fused=fused)
    assert st["queries"] == nq and st["certified"] + st["fallback"] == nq
    assert st["fallback"] >= st["range_refused"], st  # (the range rules refuse whatever the contraction found)
    if (family, metric, n) in RANGE_ALL:
        assert st["range_refused"] == nq and st["fallback"] == nq, st


QUANT_CASES = [("f16", "gauss", "l2sq", 20000, 128, 64, 10), ("f16", "offset10", "l2sq", 20000, 128, 64, 10), ("f16", "gauss", "cos", 4097, 33, 129, 100),
               ("f16", "offset100", "cos", 9000, 31, 32, 10), ("i8", "i8gauss", "l2sq", 20000, 128, 64, 10), ("i8", "i8offset", "l2sq", 20000, 128, 64, 10),
               ("i8", "i8gauss", "cos", 4097, 33, 129, 100), ("i8", "i8offset", "cos", 9000, 31, 32, 10)]


@pytest.mark.parametrize("storage,family,metric,n,d,nq,k", QUANT_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-n{c[3]}-d{c[4]}" for c in QUANT_CASES])
def test_exact_search_on_quantised_storage_is_the_brute_force(capi, oracle, cores, monkeypatch, storage, family, metric, n, d, nq, k):
    run_case(capi, oracle, cores, monkeypatch, family, metric, n, d, nq, k, storage=storage)


def test_k_above_240_is_refused(capi):
    rows = np.random.default_rng(0).standard_normal((300, 8), dtype=F32)
    ix = index_of(capi, "l2sq", "f32", rows, rows)
    ix.exact_search(rows[:2], 240)
    with pytest.raises(capi.LanternGpuError, match="k <= 240"):
        ix.exact_search(rows[:2], 241)


# ---- the certificate's counters ----------------------------------------------------------------------------------------
def test_offset_rows_take_the_fallback_and_gaussian_rows_do_not(capi, oracle, cores, monkeypatch):
    st = run_case(capi, oracle, cores, monkeypatch, "offset10", "l2sq", 4000, 128, 16, 10)
    assert st["fallback"] >= 1
    for family, metric, n, d in [("gauss", "l2sq", 65537, 128), ("gauss", "cos", 65537, 128)]:
        st = run_case(capi, oracle, cores, monkeypatch, family, metric, n, d, 256, 10)
        assert st["fallback"] == 0 and st["certified"] == 256, (family, metric, st)


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_clustered_rows_are_certified_at_size(capi, monkeypatch, metric):
    from lantern_amd import synth

    n, d, nq = 131073, 768, 256
    make = synth.query_maker("clustered", d)
    rows, queries = make(np.random.default_rng(3), n), make(np.random.default_rng(4), nq)
    ix = index_of(capi, metric, "f32", rows, rows)
    before = capi.exact_knn_stats()
    slots, dists = ix.exact_search(queries, 10)
    after = capi.exact_knn_stats()
    assert after["fallback"] - before["fallback"] == 0 and after["certified"] - before["certified"] == nq
    # spot check against float64: the 10th distance within the pair kernel's rounding
    d64 = exact64(metric, rows, queries[:8])
    kth = np.sort(d64, axis=1)[:, 9]
    assert np.all(np.abs(dists[:8, 9] - kth) <= pair_rounding(metric, kth, d) * 2)


def test_certified_calls_issue_the_same_contraction_launches(capi, oracle, cores, monkeypatch):
    # the launches of the contraction (rows x cols, fused) follow from the shape alone -- certified or not, the certificate and the
    # fallback add no contraction launch
    n, d, nq, k = 140000, 64, 1100, 10
    rng = np.random.default_rng(1)
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
    for family, fallback in (("gauss", False), ("offset10", True)):
        rows, queries = FAMILIES[family](rng, n, d, nq)
        ix = index_of(capi, "l2sq", "f32", rows, rows)
        before = capi.exact_knn_stats()
        capi.dense_profile(True)
        ix.exact_search(queries, k)
        got = [(r["rows"], r["cols"], r["fused"]) for r in capi.dense_profile(False)]
        after = capi.exact_knn_stats()
        assert got == want, family
        assert (after["fallback"] > before["fallback"]) == fallback, family
        ix.close()


# ---- assign_to_clusters and PQ encoding: k = 1, first minimum wins ------------------------------------------------------
def test_assign_to_clusters_offset_subvectors(capi, oracle):
    rng = np.random.default_rng(7)
    n, row_dims, start, sub, C = 200, 40, 9, 12, 256
    data = (F32(30) + F32(0.01) * rng.standard_normal((n, row_dims), dtype=F32)).astype(F32)
    centers = np.ascontiguousarray(data[rng.choice(n, C - 1, replace=n < C - 1), start:start + sub])
    centers = np.concatenate([centers, centers[5:6]])  # a duplicated centroid: the first one must win
    for metric in ("l2sq", "cos"):
        idx, dist = capi.assign_to_clusters(data, centers, metric, start, sub)
        want_i, want_d = [], []
        for i in range(n):
            best, bd = 0, None
            for c in range(C):  # the reference's strict-< loop over usearch_distance, in the pair kernel's order
                dd = oracle.distance(data[i, start:start + sub], centers[c], metric, oracle.SUM_WAVE64)
                if bd is None or dd < bd:
                    best, bd = c, dd
            want_i.append(best)
            want_d.append(bd)
        assert np.array_equal(idx, np.array(want_i, np.uint32)), (metric, int(np.sum(idx != np.array(want_i))))
        assert np.array_equal(dist.view(np.uint32), np.array(want_d, F32).view(np.uint32)), metric
        assert not np.any(idx == C - 1)


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_pq_encoding_of_offset_rows(capi, oracle, metric):
    rng = np.random.default_rng(11)
    n, d, S, C = 1500, 96, 8, 64
    base = (F32(10) + F32(0.01) * rng.standard_normal((n, d), dtype=F32)).astype(F32)
    cb = base[rng.choice(n, C, replace=False)].copy()  # closely spaced centroids: drawn from the rows themselves
    cb[3] = cb[2]  # a duplicated centroid
    codes, _ = quantize_reference(oracle, base, cb, S, metric)
    ix = capi.GpuIndex(metric, d, M=8, ef_construction=32, ef=32, seed=5, pq_codebook=cb, num_subvectors=S)
    ix.set_add_batch(256, 16)
    ix.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    assert np.array_equal(ix.export_codes(), codes), int(np.sum(ix.export_codes() != codes))
    ix.close()


# ---- the bound on the hardware ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb", [(1, 1), (127, 257), (129, 127), (257, 129)])
@pytest.mark.parametrize("d", [1, 3, 31, 33, 128, 768])
def test_contraction_is_within_the_bound(capi, na, nb, d):
    # distance_matrix(exact_order=False) is the contraction of the exact k-NN; |d~ - delta| <= E(q, b) on every family
    dims = padded_dims(d)
    for fi, family in enumerate(["gauss", "offset10", "offset100", "dupgroups", "repeated", "lattice", "scaled"]):
        rng = np.random.default_rng([fi, na, nb, d])
        rows, a = FAMILIES[family](rng, nb, d, na)
        for metric in ("l2sq", "cos"):
            got = capi.distance_matrix(a, rows, metric, exact_order=False).astype(np.float64)
            ref = exact64(metric, rows, a)
            if metric == "l2sq":
                qn, bn = np.sqrt((a.astype(np.float64) ** 2).sum(1)), np.sqrt((rows.astype(np.float64) ** 2).sum(1))
                E = mfma_error_l2(qn[:, None], bn[None, :], dims)
            else:
                E = np.full(ref.shape, mfma_error_cos(dims))
            over = np.abs(got - ref) - E
            assert np.all(over <= 0), (family, metric, float(np.max(over)), float(np.max(np.abs(got - ref))))
