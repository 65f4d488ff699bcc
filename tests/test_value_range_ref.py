"""The oracle on the strict families of tests/value_range.py: its device-order distances (SUM_WAVE64, SUM_WAVE64_F16) are within the
project's tolerance of float64 at every row width, and the AVX2 form and the scalar restatement give the same bits -- so that a GPU
test which demands the oracle's bits demands the right ones.  No GPU needed."""
import numpy as np
import pytest

from tests import value_range as vr

DIMS = [1, 3, 33, 128, 768, 2000]
NA, NB = 7, 33  # queries x rows per shape: every scale of a family meets every other


def oracle_matrix(oracle, metric, rows, queries, mode):
    return np.array([[oracle.distance(q, r, metric, mode) for r in rows] for q in queries], dtype=np.float32)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("family,metric", vr.F32_PAIRS + vr.F16_STRICT, ids=[f"{f}-{m}" for f, m in vr.F32_PAIRS + vr.F16_STRICT])
def test_oracle_is_within_the_tolerance_of_float64(oracle, family, metric, d):
    rows, queries = vr.strict_data(family, NB, d, NA)
    f16 = vr.STRICT[family][1] == "f16"
    if f16:
        rows, queries, mode = oracle.round_f16(rows), oracle.round_f16(queries), oracle.SUM_WAVE64_F16
    else:
        mode = oracle.SUM_WAVE64
    try:
        oracle.set_wave_simd(True)
        simd = oracle_matrix(oracle, metric, rows, queries, mode)
        oracle.set_wave_simd(False)
        scalar = oracle_matrix(oracle, metric, rows, queries, mode)
    finally:
        oracle.set_wave_simd(True)
    assert np.array_equal(simd.view(np.uint32), scalar.view(np.uint32)), "the AVX2 form and the scalar restatement differ"
    if not vr.in_domain(family, metric):  # an l2sq family under cosine: the two forms agree, nothing more is claimed
        return
    assert not np.any(np.isnan(simd)) and not np.any(np.isneginf(simd)), "a strict family gave a NaN or -inf"
    ref = vr.exact64(metric, rows, queries, direct=True)
    ok = vr.within_rounding(metric, simd, ref, d)
    bad = np.argwhere(~ok)
    assert bad.size == 0, (family, metric, d, [(int(i), int(j), float(simd[i, j]), float(ref[i, j])) for i, j in bad[:4]])


def test_the_families_reach_the_edges_they_name(oracle):
    """the data really is hostile: denormal squares, +inf next to finite distances, denormal halves as stored operands"""
    rows, q = vr.strict_data("l2_denorm", NB, 128, NA)
    sq = rows * rows
    assert np.all(sq < np.finfo(np.float32).tiny) and np.mean(sq > 0) > 0.9  # (the smallest components' squares are 0 even as denormals)
    rows, q = vr.strict_data("l2_edge", NB, 33, NA)
    dm = oracle_matrix(oracle, "l2sq", rows, q, oracle.SUM_WAVE64)
    assert np.any(np.isposinf(dm)) and np.any(np.isfinite(dm))
    rows, q = vr.strict_data("l2_mixed", NB, 128, NA)
    dm = oracle_matrix(oracle, "l2sq", rows, q, oracle.SUM_WAVE64)
    assert np.any(np.isposinf(dm)) and np.any(dm == 0) and not np.any(rows[NB // 2])
    rows, q = vr.strict_data("f16_denorm", NB, 33, NA)
    h = np.abs(oracle.round_f16(rows))
    assert np.any((h > 0) & (h < 2.0 ** -14)) and np.any(h > 4.9e4) and np.all(np.isfinite(h))
    rows, q = vr.strict_data("cos_mixed", NB, 33, NA)
    assert np.any(~rows.any(axis=1)) and not q[-1].any()


def test_within_rounding_at_the_top_of_the_range():
    g = vr.gamma(8 + 8)
    top = vr.FLT_MAX
    got = np.array([np.inf, top, np.inf, top, np.inf, np.nan, 1.0], dtype=np.float32)
    ref = np.array([top * (1 + 2 * g), top * (1 + 2 * g), top * (1 + g / 2), top * (1 + g / 2), top / 2, 1.0, 1.0])
    assert vr.within_rounding("l2sq", got, ref, 8).tolist() == [True, False, True, True, False, False, True]


def test_loose_pairs_have_the_classes_they_are_built_for(oracle):
    rng = np.random.default_rng(1)
    seen = set()
    for name, a, b in vr.loose_pairs(rng, 33):
        for metric in ("l2sq", "cos"):
            got = vr.value_class(oracle.distance(a, b, metric, oracle.SUM_WAVE64))
            seen.add(got)
            if not name.startswith("finite_1e19"):
                assert got == vr.class64(metric, a, b), (name, metric, got)
    assert {"nan", "+inf", "num"} <= seen
