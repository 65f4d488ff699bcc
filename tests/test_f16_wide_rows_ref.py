"""f16 storage on rows of 1017 .. 2000 dimensions, without a device.  An f16 row holds 8 scalars per 16-byte chunk, so these are the rows of
128 .. 250 chunks: the ones device_common.hpp group_lanes_for gives to 64 lanes.  tests/test_gpu_f16_wide_rows.py holds the device to the
oracle's SUM_WAVE64_F16 bits at these widths; here the oracle itself is held to float64 with the project's tolerance (DESIGN.md 4.1,
tests/value_range.py), shown to be sensitive to the summation order it pins, and the launch plans (lantern_gpu_plan_search,
lantern_gpu_plan_insert) are held to the shapes the device tests rely on: no int8 screen for f16 rows however wide, the latency-bound
shape for a small batch, four rows per group for a middling one, the classic two-row shape beyond."""
import numpy as np
import pytest

from tests import value_range as vr
from tests.test_insert_plan import BASE as INSERT_BASE

# 128 chunks with one half in the last, 128 full, 129; 191 / 192 / 193 (three to four chunks per lane, and a row-load block boundary); the cap
WIDE = [1017, 1024, 1025, 1528, 1536, 1537, 2000]
NA, NB = 7, 33
M_COS, M_L2SQ, F16 = 1, 3, 100
PATH_CLASSIC, PATH_SPEC2 = 2, 4  # tests/test_search_plan.py PATHS


def f16_chunks(d):
    return (d + 7) // 8


def oracle_matrix(oracle, metric, rows, queries, mode):
    return np.array([[oracle.distance(q, r, metric, mode) for r in rows] for q in queries], dtype=np.float32)


def gaussian_pairs(d):
    rng = np.random.default_rng(d)
    return (rng.standard_normal((NB, d), dtype=np.float32) * np.float32(0.4)).astype(np.float32), (rng.standard_normal((NA, d), dtype=np.float32) * np.float32(0.4)).astype(np.float32)


# ---- 1. the oracle against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDE)
def test_these_widths_are_the_64_lane_rows(oracle, d):
    """the oracle's chunk rule (oracle/metrics.c group_lanes) at 8 scalars per chunk: lo_wave_group_lanes takes f32 dimensions, four
    per chunk, so an f16 row of c chunks groups as an f32 row of 4 c dimensions does"""
    c = f16_chunks(d)
    assert 128 <= c <= 250
    assert oracle.lib().lo_wave_group_lanes(4 * c) == 64
    if d == WIDE[0]:  # one dimension less is 127 chunks: 32 lanes, the widest row the suite had
        assert f16_chunks(d - 1) == 127 and oracle.lib().lo_wave_group_lanes(4 * 127) == 32
        assert oracle.lib().lo_wave_group_lanes(4 * f16_chunks(1000)) == 32


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("d", WIDE)
def test_oracle_f16_order_is_within_the_tolerance_of_float64(oracle, metric, d):
    for name, (rows, queries) in (("gauss", gaussian_pairs(d)), ("f16_denorm", vr.strict_data("f16_denorm", NB, d, NA))):
        sr, sq = oracle.round_f16(rows), oracle.round_f16(queries)
        got = oracle_matrix(oracle, metric, sr, sq, oracle.SUM_WAVE64_F16)
        assert not np.any(np.isnan(got)) and not np.any(np.isneginf(got))
        ref = vr.exact64(metric, sr, sq, direct=True)
        ok = vr.within_rounding(metric, got, ref, d)
        bad = np.argwhere(~ok)
        assert bad.size == 0, (name, metric, d, [(int(i), int(j), float(got[i, j]), float(ref[i, j])) for i, j in bad[:4]])
        if name == "f16_denorm":
            h = np.abs(sr)
            assert np.any((h > 0) & (h < 2.0 ** -14)) and np.any(h > 4.9e4), "the family lost its denormal or top-of-range halves"
            continue
        # the same stored values summed four per chunk (the f32 rows' order) are other bits: the comparison sees the order it pins
        other = oracle_matrix(oracle, metric, sr, sq, oracle.SUM_WAVE64)
        assert np.all(vr.within_rounding(metric, other, ref, d))
        assert np.any(other.view(np.uint32) != got.view(np.uint32)), (metric, d, "SUM_WAVE64 and SUM_WAVE64_F16 agree on every pair")


# ---- 2. the plans -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def search_fields(capi, **over):
    f = dict.fromkeys(capi.PLAN_SEARCH_IN, 0)
    f.update(M=16, M0=32, n=1500, ef_default=64, num_cus=256, search_vis_slots=-1, k=10, env_wide_rows=-1)
    f.update(over)
    return f


@pytest.mark.parametrize("mcode", [M_L2SQ + F16, M_COS + F16], ids=["l2sq_f16", "cos_f16"])
@pytest.mark.parametrize("chunks", [128, 192, 193, 250])
def test_search_plans_of_wide_f16_rows(capi, chunks, mcode):
    base = search_fields(capi, chunks=chunks, mcode=mcode)
    # rows of >= 128 chunks, an index that claims a screen table: the metric alone keeps the launch off the int8 screen
    for nq in (40, 700, 1100):
        out, why = capi.plan_search(dict(base, nq=nq, screen=1))
        assert why is None and out["screen_lds"] == 0, (nq, out)
    out, why = capi.plan_search(dict(base, nq=1100, screen=1, mcode=mcode - F16))
    assert why is None and out["screen_lds"] > 0, "the f32 twin of this launch screens: the assertion above tests the metric gate"
    out, why = capi.plan_search(dict(base, nq=40))
    assert why is None and out["path"] == PATH_SPEC2 and out["took_spec"] == 1 and out["waves"] == 11 and out["wide_rows"] == 0, out
    assert out["spec_prefetch"] == 1 and out["spec_cache"] == 128  # (64 lanes: one list word per lane, M0 = 32 fits)
    out, why = capi.plan_search(dict(base, nq=700))
    assert why is None and out["path"] == PATH_CLASSIC and out["spec"] == 0 and out["waves"] == 4 and out["wide_rows"] == 1, out
    out, why = capi.plan_search(dict(base, nq=1100))
    assert why is None and out["path"] == PATH_CLASSIC and out["spec"] == 0 and out["waves"] == 4 and out["wide_rows"] == 0, out
    for nq, path in ((40, PATH_SPEC2), (700, PATH_CLASSIC), (1100, PATH_CLASSIC)):
        for top in (64, 128, 200):
            out, why = capi.plan_search(dict(base, nq=nq, each=1, max_expansion=top, k=top))
            assert why is None and out["expansion"] == top, (nq, top, why)
            assert out["path"] == (path if top <= 128 else PATH_CLASSIC), (nq, top, out)  # (the LDS list has no latency-bound form)


@pytest.mark.parametrize("mcode", [M_L2SQ + F16, M_COS + F16], ids=["l2sq_f16", "cos_f16"])
@pytest.mark.parametrize("chunks", [128, 192, 193, 250])
def test_insert_plans_of_wide_f16_rows_are_unscreened(capi, chunks, mcode):
    f = dict(INSERT_BASE, mcode=mcode, chunks=chunks, screen_table=1)
    out, why = capi.plan_insert(f)
    assert why is None and out["screened"] == 0 and out["screen_lds"] == 0, out
    assert capi.plan_insert(dict(f, mcode=mcode - F16))[0]["screened"] == 1  # (the f32 twin is screened: the metric is what decides)
