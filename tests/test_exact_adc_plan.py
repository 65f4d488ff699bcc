"""lantern_gpu_plan_exact_adc and the exports around it (include/lantern_gpu.h; DESIGN.md 4.5 "Compact pq indexes: ADC pre-selection"):
whether an exact search on the code rows pre-selects by table lookups, as a pure function; and the error model of the scan's keys
against the certificate's bound E (tests/exact_knn_bound.py), in numpy.  No device.
"""
import ctypes as C

import numpy as np
import pytest

from lantern_amd import capi
from tests.exact_knn_bound import mfma_error_cos, mfma_error_l2

M_COS, M_L2SQ, M_HAMMING = 1, 3, 8
# 768-d rows in 96 subvectors of 8 dimensions at the 128-byte row stride: cps = 2, inv = 2^16 / 2
ARGS = dict(mcode=M_L2SQ, chunks=192, nb=1_000_000, nq=64, k=10, on=True, compact=True, pqd_inv=32768, code_row_bytes=128, max_queries=64,
            subvectors=96, centroids=256)


@pytest.mark.parametrize("change, why", [
    ({}, "taken"), ({"nq": 1}, "taken"),
    ({"max_queries": 0}, "off"), ({"max_queries": 0, "compact": False}, "off"),
    ({"on": False}, "not_compact"), ({"compact": False}, "not_compact"), ({"pqd_inv": 0}, "not_compact"), ({"mcode": M_HAMMING}, "not_compact"),
    ({"nq": 65}, "many_queries"), ({"nq": 65, "centroids": 257}, "many_queries"),
    ({"centroids": 257}, "shape"), ({"subvectors": 144, "chunks": 288}, "shape"), ({"subvectors": 128}, "shape"), ({"subvectors": 7}, "shape"),
    ({"subvectors": 0}, "shape"), ({"nq": 2731, "max_queries": 4096}, "budget"), ({"nq": 2730, "max_queries": 4096}, "taken"),
])
def test_the_decision_and_its_reason_in_call_order(change, why):
    p = capi.plan_exact_adc(**{**ARGS, **change})
    assert (p["why"], p["taken"]) == (why, why == "taken")
    if why == "taken":
        nq = change.get("nq", 64)
        assert p == {"taken": True, "why": "taken", "T": 1, "block": 1024, "lds_bytes": 96 * 1024, "S16": 96, "table_bytes": nq * 96 * 1024}
    else:
        assert all(p[f] == 0 for f in ("T", "block", "lds_bytes", "S16", "table_bytes"))


@pytest.mark.parametrize("S, T", [(16, 4), (32, 4), (33, 2), (64, 2), (65, 1), (96, 1), (128, 1)])
def test_queries_per_workgroup_fill_160_kb(S, T):
    stride = 128 if 64 < S < 128 else (S + 15) // 16 * 16
    p = capi.plan_exact_adc(**{**ARGS, "chunks": S, "pqd_inv": 65536, "code_row_bytes": stride, "subvectors": S, "mcode": M_COS})
    S16 = (S + 15) // 16 * 16
    assert (p["why"], p["T"], p["S16"], p["lds_bytes"]) == ("taken", T, S16, T * S16 * 1024)


def test_exports_are_bound_and_refuse_bad_arguments_without_a_device():
    for name in ("lantern_gpu_set_exact_adc", "lantern_gpu_exact_adc", "lantern_gpu_plan_exact_adc", "lantern_gpu_exact_adc_stats"):
        assert name in capi.EXPORTS and getattr(capi.lib(), name).argtypes is not None
    assert hasattr(capi.GpuIndex, "set_exact_adc") and hasattr(capi.GpuIndex, "exact_adc")
    assert set(capi.exact_adc_stats()) == {"tables", "scans"}
    err = C.c_char_p()
    capi.lib().lantern_gpu_set_exact_adc(None, -1, C.byref(err))  # refused on the value, before the handle is looked at
    assert b"exact_adc must be 0" in err.value
    for bad in [dict(max_queries=-1), dict(subvectors=-1), dict(centroids=-1), dict(chunks=0), dict(code_row_bytes=24), dict(k=241)]:
        with pytest.raises(capi.LanternGpuError, match="lantern_gpu: bad plan input"):
            capi.plan_exact_adc(**{**ARGS, **bad})
    assert capi.lib().lantern_gpu_plan_exact_adc(None, None) == b"lantern_gpu: null plan array"


def fma32(a, b, acc):
    """fl32(a b + acc): the product of two f32 is exact in float64; the second rounding can differ from a true fma's by 2^-29 ulp"""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


FAMILIES = {"gaussian": lambda x: x, "offset": lambda x: 10 + 0.01 * x, "small": lambda x: 1e-3 * x, "large": lambda x: 3e4 * x}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("w, S", [(4, 2), (4, 16), (24, 4), (8, 96), (4, 128), (48, 16)])  # d = 8 .. 768
def test_scan_keys_are_within_the_certificates_bound(w, S, family):
    """an entry is w fmas over fl(q - c) (l2sq) or q c (cos), a key the f32 sum of S entries in ascending order"""
    rng = np.random.default_rng(w * 1000 + S)
    q = FAMILIES[family](rng.standard_normal((8, 1, S, w))).astype(np.float32)
    b = FAMILIES[family](rng.standard_normal((1, 300, S, w))).astype(np.float32)
    dims, q64, b64 = w * S, q.astype(np.float64), b.astype(np.float64)
    key = {"l2sq": np.zeros((8, 300), np.float32), "cos": np.zeros((8, 300), np.float32)}
    for s in range(S):
        e2, ed = np.zeros((8, 300), np.float32), np.zeros((8, 300), np.float32)
        for j in range(w):
            t = q[:, :, s, j] - b[:, :, s, j]  # (f32: one rounding)
            e2, ed = fma32(t, t, e2), fma32(q[:, :, s, j], b[:, :, s, j], ed)
        key["l2sq"], key["cos"] = key["l2sq"] + e2, key["cos"] + ed
    qn, bn = np.sqrt((q64 ** 2).sum((2, 3))), np.sqrt((b64 ** 2).sum((2, 3)))
    ref = {"l2sq": ((q64 - b64) ** 2).sum((2, 3)), "cos": 1 - (q64 * b64).sum((2, 3)) / (qn * bn)}
    inv = lambda n: np.float32(1) / np.sqrt((n * n).astype(np.float32))  # the epilogue's inverse roots of the f32 norms
    key["cos"] = np.float32(1) - key["cos"] * (inv(qn) * inv(bn))
    E = {"l2sq": mfma_error_l2(qn, bn, dims), "cos": mfma_error_cos(dims)}
    ld = np.longdouble  # the referee: float64 against extended precision first
    wide = {"l2sq": ((q.astype(ld) - b.astype(ld)) ** 2).sum((2, 3)),
            "cos": 1 - (q.astype(ld) * b.astype(ld)).sum((2, 3)) / np.sqrt((q.astype(ld) ** 2).sum((2, 3)) * (b.astype(ld) ** 2).sum((2, 3)))}
    for m in ("l2sq", "cos"):
        assert np.finfo(ld).eps < 2e-19 and (np.abs(ref[m] - wide[m]) <= 2.0 ** -20 * E[m]).all()
        assert (np.abs(key[m].astype(np.float64) - ref[m]) <= E[m]).all(), (np.abs(key[m] - ref[m]) / E[m]).max()
    # the tighter statement the derivation makes for l2sq: relative to delta, w + S + 2 roundings
    g = (w + S + 2) * 2.0 ** -24
    assert (np.abs(key["l2sq"] - ref["l2sq"]) <= g / (1 - g) * ref["l2sq"] + 4 * (dims + 8) * 2.0 ** -126).all()
