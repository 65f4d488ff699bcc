"""The screened exact pass of a filtered call, without a device (include/lantern_gpu.h "THE SCREENED EXACT PASS"):
lantern_gpu_plan_filtered_screen is the decision the call's own plan takes and the carve the launcher asks for."""
import pytest

from tests.test_filtered_dense_plan import COS, HAMMING, L2SQ, capi  # noqa: F401 (the metric codes; capi: the module's fixture)


def test_reasons_in_the_order_a_call_meets_them(capi):
    """every input wrong at once, then mended one by one: the reason named is always the first one still standing"""
    bad = dict(on=0, mcode=L2SQ + 100, chunks=127, table=False, compact=True, kk=10)
    mend = [("on", 1, "off"), ("mcode", L2SQ, "metric"), ("chunks", 128, "width"), ("table", True, "no_table"), ("compact", False, "compact")]
    for name, good, why in mend:
        p = capi.plan_filtered_screen(**bad)
        assert p == {"taken": False, "why": why, "lds": 0, "per_cu": 0}
        bad[name] = good
    assert capi.plan_filtered_screen(**bad)["why"] == "taken"
    # a list that fits today's carve of the 160 KiB and not the screened one keeps today's kernel
    assert capi.plan_filtered_screen(1, L2SQ, 128, kk=9900)["why"] == "taken" and capi.plan_filtered_screen(1, L2SQ, 128, kk=9990)["why"] == "lds"


@pytest.mark.parametrize("mcode", [L2SQ, COS, L2SQ + 100, COS + 100, L2SQ + 200, COS + 200, HAMMING])
def test_taken_only_for_f32_l2sq_and_cos_with_the_table(capi, mcode):
    f32 = mcode in (L2SQ, COS)
    assert capi.plan_filtered_screen(1, mcode, 192)["taken"] == f32
    assert capi.plan_filtered_screen(1, mcode, 192)["why"] == ("taken" if f32 else "metric")
    assert not capi.plan_filtered_screen(1, mcode, 192, table=False)["taken"] and not capi.plan_filtered_screen(0, mcode, 192)["taken"]


@pytest.mark.parametrize("d", [509, 768, 2000])
@pytest.mark.parametrize("kk", [1, 10, 17, 300])
def test_carve_bytes(capi, d, kk):
    """the exact pass's carve at 2 * 512 / 64 = 16 rows per round, the query's screen block, the survivor queue"""
    up16 = lambda x: (x + 15) // 16 * 16
    chunks, rows = (d + 3) // 4, 16
    scalars = 28 * 4
    exact = chunks * 16 + 2 * up16(kk * 8) + 2 * up16(rows * 8) + up16(rows * 4) + scalars  # query row, list + merge target, new keys (+ sorted), new ids
    screen = 16 + (chunks + 3) // 4 * 32  # three scalars (+ pad), then 16 B of h and 16 B of l per screen chunk
    queue = 128 * 4  # a power of two >= 15 left over + 64 of a screen round
    p = capi.plan_filtered_screen(1, L2SQ, chunks, kk=kk)
    assert p["taken"] and p["lds"] == exact + screen + queue
    assert p["per_cu"] == min(2, 160 * 1024 // p["lds"])
