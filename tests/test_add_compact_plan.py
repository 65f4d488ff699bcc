"""lantern_gpu_plan_add_compact: whether an add or a reserve leaves a compact pq index compact, as a pure function (include/lantern_gpu.h;
DESIGN.md 4.7 "Compact pq indexes: adding").  No device.  insert_rows and usearch_reserve decide through this function.
"""
import ctypes

import pytest

from lantern_amd import capi

M_COS, M_L2SQ, M_HAMMING, M_F16, M_PQD = 1, 3, 8, 100, 600
CHUNKS, S16, INV, CAP = 192, 128, 8192, 10_000_000  # 768-d rows in 96 subvectors of 8 dimensions: cps = 2, inv = 2^16 / 2
ARGS = dict(mcode=M_L2SQ, chunks=CHUNKS, M0=32, efc=128, rows=1, cap=CAP, on=True, compact=True, pqd_inv=INV, code_row_bytes=S16)


@pytest.mark.parametrize("change,why", [({}, "served"), ({"on": False}, "off"), ({"compact": False}, "expanded"), ({"pqd_inv": 0}, "no_decode"),
                                        ({"mcode": M_HAMMING}, "metric"), ({"mcode": M_L2SQ + M_F16}, "metric"), ({"mcode": M_L2SQ + M_PQD}, "metric"),
                                        ({"collective": True}, "collective"), ({"pages": True}, "pages"), ({"efc": 200_000}, "shape"),
                                        ({"mcode": M_COS, "rows": 0}, "served"), ({"rows": 100_000, "efc": 160}, "served")])
def test_the_decision_and_its_reason(change, why):
    a = {**ARGS, **change}
    p = capi.plan_add_compact(**a)
    assert (p["why"], p["served"]) == (why, why == "served")
    if p["served"]:
        # the staging block is the call's only f32 rows: at most 65536 of them, never the capacity's block
        assert p["stage_rows"] == min(a["rows"], 65536) and p["stage_bytes"] == p["stage_rows"] * CHUNKS * 16 <= 65536 * CHUNKS * 16
        assert (p["mcode"], p["expand_bytes"], p["lanes"]) == (a["mcode"] + M_PQD, 0, 64)
        assert p["kpl"] == (2 if a["efc"] <= 128 else 0) and 0 < p["lds"] <= 160 * 1024
    else:
        assert (p["stage_bytes"], p["mcode"]) == (0, 0)
        assert p["expand_bytes"] == (CAP * CHUNKS * 16 if a["compact"] else 0)  # what the call decodes the index into


def test_bad_inputs_the_switch_value_and_the_exports():
    for bad in [dict(chunks=0), dict(M0=1), dict(efc=0), dict(rows=-1), dict(code_row_bytes=0), dict(code_row_bytes=24), dict(pqd_inv=-1), dict(waves=0)]:
        with pytest.raises(capi.LanternGpuError, match="lantern_gpu: bad plan input"):
            capi.plan_add_compact(**{**ARGS, **bad})
    err = ctypes.c_char_p()
    for on in (2, -1):  # refused before the handle is looked at
        capi.lib().lantern_gpu_set_add_compact(None, on, ctypes.byref(err))
        assert b"add_compact must be 0" in err.value
    for name in ("lantern_gpu_set_add_compact", "lantern_gpu_add_compact", "lantern_gpu_plan_add_compact"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert {"set_add_compact", "add_compact"} <= set(dir(capi.GpuIndex))
