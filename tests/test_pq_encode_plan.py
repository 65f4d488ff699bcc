"""The fused pq encoder's host side without a device (lantern_amd/csrc/pq_encode.hip): the five symbols, plan_pq_encode's decisions, and
lantern_gpu_pq_encode's refusals."""
import ctypes as C

import numpy as np
import pytest

SYMBOLS = ("lantern_gpu_set_pq_encode_fused", "lantern_gpu_pq_encode_fused", "lantern_gpu_plan_pq_encode", "lantern_gpu_last_pq_encode",
           "lantern_gpu_pq_encode")


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    return capi


def test_the_symbols_are_exported_and_bound(capi):
    raw = C.CDLL(capi.LIB_PATH)
    for name in SYMBOLS:
        assert name in capi.EXPORTS and hasattr(raw, name) and getattr(capi.lib(), name).argtypes is not None, name


@pytest.mark.parametrize("metric,dims,S,C,on,want", [
    # Lantern's usual shape: strips of 4 subvectors = one 128-byte line of the row, 32 KB of tables + 32 KB of rows
    ("l2sq", 768, 96, 256, True, {"why": "served", "strip": 4, "grid": (256, 24), "lds": 65536, "chunks": 2}),
    ("cos", 12, 4, 10, True, {"why": "served", "strip": 4, "grid": (256, 1), "lds": 4 * 10 * 16 + 256 * 12 * 4, "chunks": 1}),
    ("l2sq", 128, 4, 256, True, {"why": "served", "strip": 1, "grid": (256, 4), "lds": 65536, "chunks": 8}),
    ("l2sq", 100, 5, 255, True, {"why": "served", "strip": 1, "grid": (256, 5), "lds": 255 * 80 + 256 * 20 * 4, "chunks": 5}),
    ("l2sq", 144, 4, 16, True, {"why": "subdim"}),
    ("hamming", 768, 96, 256, True, {"why": "metric"}),
    ("l2sq", 768, 96, 257, True, {"why": "centroids"}),
    ("l2sq", 768, 96, 256, False, {"why": "off"}),
    ("hamming", 144, 4, 300, False, {"why": "off"}),  # the reasons in the order a call meets them
])
def test_plan(capi, metric, dims, S, C, on, want):
    p = capi.plan_pq_encode(metric, dims, S, C, rows=65536, on=on)
    served = want["why"] == "served"
    assert p["served"] == served and p["launches"] == (1 if served else 0) and p["lds"] <= 65536
    assert {k: p[k] for k in want} == want
    if not served:
        assert p["strip"] == 0 and p["grid"] == (0, 0) and p["lds"] == 0


def test_plan_refuses_shapes_no_index_has(capi):
    for dims, S, C in ((10, 4, 16), (0, 1, 16), (8, 0, 16), (8, 2, 0)):
        with pytest.raises(capi.LanternGpuError, match="bad plan input"):
            capi.plan_pq_encode("l2sq", dims, S, C)


def test_entry_validates_before_it_looks_for_a_device(capi):
    rows, cb = np.ones((3, 12), np.float32), np.ones((10, 12), np.float32)
    with pytest.raises(capi.LanternGpuError, match="needs cos or l2sq"):
        capi.pq_encode(rows, cb, 4, "hamming")
    with pytest.raises(capi.LanternGpuError, match="bad arguments"):
        capi.pq_encode(rows, cb, 5, "l2sq")  # 5 does not divide 12
    with pytest.raises(capi.LanternGpuError, match="bad arguments"):
        capi.pq_encode(rows, np.ones((257, 12), np.float32), 4, "l2sq")  # a code is a byte
    if capi.device_count() > 0:
        assert capi.pq_encode(rows, cb, 4, "l2sq")[0].shape == (3, 4)
    else:
        with pytest.raises(capi.LanternGpuError, match="no HIP device"):
            capi.pq_encode(rows, cb, 4, "l2sq")
