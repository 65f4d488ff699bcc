"""The native f16 / i8 contraction's host side without a device: the two exports exist and are bound, lantern_gpu_plan_dense's
arithmetic (operand kind, the f32 copy a call allocates, the dims the certificate is told, K steps per tile), and
lantern_gpu_distance_matrix's acceptance of f16 / i8 rows ahead of the device check."""
import numpy as np
import pytest

M_COS, M_L2SQ, M_HAMMING, M_COS_B1 = 1, 3, 8, 9
M_F16, M_I8 = 100, 200
CHUNK_ROWS = 65536  # base rows per contraction launch


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def test_the_exports_exist_and_are_bound(capi):
    for name in ("lantern_gpu_dense_kind_stats", "lantern_gpu_plan_dense"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    stats = capi.dense_kind_stats()
    assert len(stats) == 3 and all(isinstance(v, int) and v >= 0 for v in stats)


def test_plan_f16(capi):
    assert capi.plan_dense(M_COS + M_F16, 96, 1_000_000, 1) == {"kind": 1, "copy_bytes": 0, "dims": 2 * 768, "k_steps": 12}
    off = capi.plan_dense(M_COS + M_F16, 96, 1_000_000, 0)
    assert off == {"kind": 0, "copy_bytes": CHUNK_ROWS * 768 * 4, "dims": 768, "k_steps": 24}
    assert capi.plan_dense(M_L2SQ + M_F16, 96, 1000, 0)["copy_bytes"] == 1000 * 768 * 4  # fewer rows than a chunk


def test_plan_i8(capi):
    assert capi.plan_dense(M_L2SQ + M_I8, 48, 1_000_000, 1) == {"kind": 2, "copy_bytes": 0, "dims": 0, "k_steps": 6}
    assert capi.plan_dense(M_COS + M_I8, 48, 1_000_000, 1) == {"kind": 2, "copy_bytes": 0, "dims": 0, "k_steps": 6}
    off = capi.plan_dense(M_L2SQ + M_I8, 48, 1_000_000, 0)
    assert off == {"kind": 0, "copy_bytes": CHUNK_ROWS * 768 * 4, "dims": 768, "k_steps": 24}


@pytest.mark.parametrize("native", [-1, 0, 1])
def test_plan_f32_and_popcount_codes(capi, native):
    for mcode in (M_L2SQ, M_COS):
        assert capi.plan_dense(mcode, 192, 1_000_000, native) == {"kind": 0, "copy_bytes": 0, "dims": 768, "k_steps": 24}
    for mcode in (M_HAMMING, M_COS_B1):
        p = capi.plan_dense(mcode, 6, 1_000_000, native)
        assert p["kind"] == 0 and p["copy_bytes"] == 0 and p["dims"] == 0


def test_plan_at_the_slab_edge(capi):
    # a K step is 128 bytes of a row: 8 chunks
    for mcode in (M_L2SQ + M_F16, M_COS + M_I8):
        assert capi.plan_dense(mcode, 8, 5000, 1)["k_steps"] == 1
        assert capi.plan_dense(mcode, 9, 5000, 1)["k_steps"] == 2
    assert capi.plan_dense(M_L2SQ + M_F16, 1, 5000, 1) == {"kind": 1, "copy_bytes": 0, "dims": 16, "k_steps": 1}


def test_plan_refuses_nonsense(capi):
    with pytest.raises(capi.LanternGpuError, match="bad plan input"):
        capi.plan_dense(M_L2SQ, 0, 10)
    assert capi.lib().lantern_gpu_plan_dense(None, None) is not None


def test_distance_matrix_kinds_without_a_device(capi):
    if capi.device_count() > 0:
        pytest.skip("a device is present")
    a16, b16 = np.ones((2, 5), np.float16), np.ones((3, 5), np.float16)
    a8, b8 = np.ones((2, 5), np.int8), np.ones((3, 5), np.int8)
    for metric in ("cos", "l2sq"):
        for exact in (True, False):
            with pytest.raises(capi.LanternGpuError, match="no HIP device"):
                capi.distance_matrix(a16, b16, metric, exact_order=exact, kind="f16")
            with pytest.raises(capi.LanternGpuError, match="no HIP device"):
                capi.distance_matrix(a8, b8, metric, exact_order=exact, kind="i8")
        with pytest.raises(capi.LanternGpuError, match="no HIP device"):
            capi.distance(a16[0], b16[0], metric, kind="f16")


def test_other_kinds_are_still_refused(capi):
    # validation stays ahead of the device check: these texts come with or without a device
    fits = "scalar kind does not fit the metric"
    with pytest.raises(capi.LanternGpuError, match=fits):
        capi.distance_matrix(np.ones((2, 8), np.float16), np.ones((2, 8), np.float16), "hamming", kind="f16")
    with pytest.raises(capi.LanternGpuError, match=fits):
        capi.distance_matrix(np.ones((2, 8), np.int8), np.ones((2, 8), np.int8), "hamming", kind="i8")
    out, a = np.zeros((1, 1), np.float32), np.zeros(64, np.uint8)
    for kind, metric in ((capi.SCALAR_B1, capi.METRICS["l2sq"]), (2, capi.METRICS["l2sq"]), (2, capi.METRICS["cos"])):  # b1 with l2sq; f64
        with pytest.raises(capi.LanternGpuError, match=fits):
            capi._call("lantern_gpu_distance_matrix", capi._ptr(a), 1, capi._ptr(a), 1, kind, 8, metric, 1, capi._ptr(out))
