"""lantern_gpu_plan_delete_compact: whether unlink and compaction run on a compact pq index's code rows, and the compaction's bytes, as a
pure function (include/lantern_gpu.h "Deleting rows"; DESIGN.md 4.11, 4.12 "Compact pq indexes").  No device."""
import ctypes

import pytest

from lantern_amd import capi

M_COS, M_L2SQ, M_HAMMING, M_F16, M_PQD = 1, 3, 8, 100, 600
# 768-d rows in 96 subvectors of 8 dimensions (cps = 2, inv = 2^16 / 2), M = 16: 1M rows of which 900 000 live
BIG = dict(mcode=M_L2SQ, chunks=192, M0=32, M=16, on=True, compact=True, pqd_inv=32768, code_row_bytes=128, num_subvectors=96, cap=1_000_000,
           code_rows=1_000_000, upper_cap=70_000, live=900_000, upper_blocks=63_000, capacity=0)
# cosine, 64-d in 16 subvectors, M = 4: compacted at 700 rows in a capacity of 1000, 500 live, the call asks for a capacity of 800
COS = dict(mcode=M_COS, chunks=16, M0=8, M=4, on=True, compact=True, pqd_inv=65536, code_row_bytes=16, num_subvectors=16, cap=1000, code_rows=700,
           upper_cap=1024, live=500, upper_blocks=40, capacity=800)


@pytest.mark.parametrize("change,why", [({}, "served"), ({"on": False, "compact": False}, "off"), ({"on": False}, "off"),
                                        ({"compact": False, "pqd_inv": 0}, "stored"), ({"pqd_inv": 0, "mcode": M_HAMMING}, "no_decode"),
                                        ({"mcode": M_L2SQ + M_F16, "chunks": 4096}, "metric"), ({"mcode": M_L2SQ + M_PQD}, "metric"),
                                        ({"chunks": 4096}, "shape"), ({"mcode": M_COS}, "served")])
def test_the_reasons_in_the_order_the_call_meets_them(change, why):
    a = {**BIG, **change}
    p = capi.plan_delete_compact(**a)
    assert (p["why"], p["served"]) == (why, why == "served")
    if p["served"]:
        assert (p["mcode"], p["lanes"], p["expand_bytes"]) == (a["mcode"] + M_PQD, 64, 0)
    else:
        assert (p["mcode"], p["lds"], p["new_bytes"], p["peak_bytes"]) == (0, 0, 0, 0)
        assert p["expand_bytes"] == (a["cap"] * a["chunks"] * 16 if a["compact"] else 0)  # what the user would have to allocate instead


def test_the_bytes_count_code_rows():
    p = capi.plan_delete_compact(**BIG)
    # a slot: 32 x 4 list + 8 label + 1 level + 4 upper_off + 4 radius + 96 code bytes = 241; an upper block 16 x 4 + 4 = 68; a padded code row 128
    assert p["old_bytes"] == 1_000_000 * 241 + 70_000 * 68 + 1_000_000 * 128 == 373_760_000
    assert p["new_bytes"] == p["after_bytes"] == 900_000 * 241 + 63_000 * 68 + 900_000 * 128 == 336_384_000
    assert p["peak_bytes"] == 710_144_000 < 1_000_000 * 192 * 16  # old + new is a quarter of the f32 block an expansion allocates
    # LDS: keep, tomb 32 + 32 | offers 256 | round 256 | sums 4 words = 2320; p's decoded row 192 x 16; 256 code rows of 128 bytes
    assert (p["lds"], p["block_offers"]) == (2320 + 3072 + 32768, 256)
    c = capi.plan_delete_compact(**COS)
    # a slot: 8 x 4 + 8 + 1 + 4 + 4 + 4 norm + 16 code bytes = 69; an upper block 4 x 4 + 4 = 20; the padded code rows held 700, hold 800 after
    assert c["old_bytes"] == 1000 * 69 + 1024 * 20 + 700 * 16 == 100_680
    assert c["new_bytes"] == 800 * 69 + 40 * 20 + 800 * 16 == 68_800
    assert c["after_bytes"] == 800 * 69 + 40 * 20 + 500 * 16 == 64_000  # memory_usage counts the code rows in use
    assert c["peak_bytes"] == 169_480
    assert (c["lds"], c["block_offers"], c["lanes"], c["mcode"]) == ((16 + 256 + 256 + 4) * 4 + 16 * 16 + 256 * 16, 256, 8, M_COS + M_PQD)


def test_bad_inputs_the_switch_value_and_the_exports():
    for bad in [dict(chunks=0), dict(M0=1), dict(M=0), dict(M=33), dict(code_row_bytes=0), dict(code_row_bytes=24), dict(code_row_bytes=144),
                dict(num_subvectors=129), dict(pqd_inv=-1), dict(live=-1), dict(capacity=-1)]:
        with pytest.raises(capi.LanternGpuError, match="lantern_gpu: bad plan input"):
            capi.plan_delete_compact(**{**BIG, **bad})
    err = ctypes.c_char_p()
    for on in (2, -1):  # refused before the handle is looked at
        capi.lib().lantern_gpu_set_delete_compact(None, on, ctypes.byref(err))
        assert b"delete_compact must be 0 (unlink and compaction refuse a compact pq index) or 1 (they are served from the code rows)" in err.value
    for name in ("lantern_gpu_set_delete_compact", "lantern_gpu_delete_compact", "lantern_gpu_plan_delete_compact"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert {"set_delete_compact", "delete_compact"} <= set(dir(capi.GpuIndex))
