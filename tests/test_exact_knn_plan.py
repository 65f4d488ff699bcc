"""The plan of an exact k-NN call, without a device: lantern_gpu_plan_exact_knn (csrc/dense.cpp plan_exact_knn) at the sizes where the
launch sequence changes -- the 4096 seed columns, the 65536-row chunk, the 1024-query tile, the fused switch -- for every operand kind,
with the buffer sizes and offsets the call allocates by.  The expected step lists are written out: (queries, base rows, fused, first
base row) per contraction launch.  Every plan made here is also checked against lantern_gpu_plan_dense, which projects four of its
numbers."""
import pytest

M_COS, M_L2SQ, M_HAMMING, M_COS_B1 = 1, 3, 8, 9
M_F16, M_I8 = 100, 200
F, T = False, True


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def plan(capi, mcode, chunks, nb, nq, k=10, native=-1, fused=-1):
    p = capi.plan_exact_knn(mcode, chunks, nb, nq, k, native, fused)
    assert capi.plan_dense(mcode, chunks, nb, native) == {"kind": p["kind"], "copy_bytes": p["fb_bytes"], "dims": p["dims"], "k_steps": p["k_steps"]}
    return p


# ---- boundaries -----------------------------------------------------------------------------------------------------------------------
def test_the_seed_columns(capi):
    p = plan(capi, M_L2SQ, 1, 4096, 1)
    assert p["steps"] == [(1, 4096, F, 0)]
    assert (p["fused"], p["cand_bytes"], p["ldd"], p["dd_bytes"]) == (0, 0, 4096, 4096 * 4)
    p = plan(capi, M_L2SQ, 1, 4097, 1)
    assert p["steps"] == [(1, 4096, F, 0), (1, 1, T, 4096)]
    assert (p["fused"], p["cand_bytes"], p["ldd"], p["dd_bytes"]) == (1, 4096 * 8 + 4 + 16, 4096, 4096 * 4)
    assert (p["seed_cols"], p["cand_cap"], p["qtile"]) == (4096, 4096, 1024)


def test_the_chunk_of_base_rows(capi):
    p = plan(capi, M_COS, 1, 65536, 1)
    assert p["steps"] == [(1, 4096, F, 0), (1, 61440, T, 4096)] and p["chunk_rows"] == 65536
    p = plan(capi, M_COS, 1, 65537, 1)
    assert p["steps"] == [(1, 4096, F, 0), (1, 61440, T, 4096), (1, 1, T, 65536)] and p["chunk_rows"] == 65536
    assert plan(capi, M_COS, 1, 5000, 1)["chunk_rows"] == 5000


def test_the_query_tile(capi):
    assert plan(capi, M_L2SQ, 1, 4097, 1024)["steps"] == [(1024, 4096, F, 0), (1024, 1, T, 4096)]
    assert plan(capi, M_L2SQ, 1, 4097, 1025)["steps"] == [(1024, 4096, F, 0), (1024, 1, T, 4096), (1, 4096, F, 0), (1, 1, T, 4096)]
    # chunk-major, tile-minor
    assert plan(capi, M_L2SQ, 1, 65537, 1025)["steps"] == [(1024, 4096, F, 0), (1024, 61440, T, 4096), (1, 4096, F, 0), (1, 61440, T, 4096),
                                                           (1024, 1, T, 65536), (1, 1, T, 65536)]


def test_the_fused_switch(capi):
    p = plan(capi, M_L2SQ, 1, 65537, 1025, fused=0)
    assert p["steps"] == [(1024, 65536, F, 0), (1, 65536, F, 0), (1024, 1, F, 65536), (1, 1, F, 65536)]
    assert (p["fused"], p["cand_bytes"], p["ldd"], p["dd_bytes"]) == (0, 0, 65536, 1024 * 65536 * 4)
    p = plan(capi, M_L2SQ, 1, 5000, 3, fused=0)
    assert p["steps"] == [(3, 5000, F, 0)] and (p["ldd"], p["dd_bytes"]) == (5000, 3 * 5000 * 4)
    assert plan(capi, M_L2SQ, 1, 5000, 3, fused=1)["steps"] == plan(capi, M_L2SQ, 1, 5000, 3)["steps"] == [(3, 4096, F, 0), (3, 904, T, 4096)]


def test_the_shape_of_the_launch_sequence_tests(capi):
    # (n, nq) = (140000, 1100) of tests/test_gpu_exact_knn.py and test_gpu_dense_native.py: three chunks (the last of 8928 rows) by two
    # query tiles (1024 + 76) -- eight launches
    want = [(1024, 4096, F, 0), (1024, 61440, T, 4096), (76, 4096, F, 0), (76, 61440, T, 4096),
            (1024, 65536, T, 65536), (76, 65536, T, 65536), (1024, 8928, T, 131072), (76, 8928, T, 131072)]
    assert plan(capi, M_L2SQ, 16, 140000, 1100)["steps"] == want
    assert plan(capi, M_L2SQ + M_F16, 8, 140000, 1100, native=1)["steps"] == want


# ---- kinds ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mcode", [M_HAMMING, M_COS_B1])
@pytest.mark.parametrize("fused", [-1, 0, 1])
def test_popcount_metrics_are_never_fused(capi, mcode, fused):
    p = plan(capi, mcode, 2, 70000, 3, fused=fused)
    assert p["steps"] == [(3, 65536, F, 0), (3, 4464, F, 65536)]
    assert (p["bits"], p["fused"], p["exact_keys"], p["dims"], p["k_steps"], p["kind"], p["copy"]) == (1, 0, 1, 0, 0, 0, 0)
    assert (p["cand_bytes"], p["fq_bytes"], p["fb_bytes"], p["fchunks"]) == (0, 0, 0, 2)


@pytest.mark.parametrize("native", [-1, 1])
def test_quantised_rows_as_stored(capi, native):
    p = plan(capi, M_COS + M_F16, 96, 100000, 7, native=native)
    assert (p["kind"], p["copy"], p["fchunks"], p["dims"], p["exact_keys"], p["k_steps"], p["fq_bytes"], p["fb_bytes"]) == (1, 0, 96, 2 * 768, 0, 12, 0, 0)
    p = plan(capi, M_L2SQ + M_I8, 48, 100000, 7, native=native)
    assert (p["kind"], p["copy"], p["fchunks"], p["dims"], p["exact_keys"], p["k_steps"], p["fq_bytes"], p["fb_bytes"]) == (2, 0, 48, 0, 1, 6, 0, 0)
    assert p["bits"] == 0 and p["fused"] == 1


def test_quantised_rows_on_an_f32_copy(capi):
    p = plan(capi, M_COS + M_F16, 96, 100000, 7, native=0)
    assert (p["kind"], p["copy"], p["fchunks"], p["dims"], p["exact_keys"], p["k_steps"]) == (0, 1, 192, 768, 0, 24)
    assert (p["fq_bytes"], p["fb_bytes"]) == (7 * 768 * 4, 65536 * 768 * 4)
    p = plan(capi, M_L2SQ + M_I8, 48, 1000, 7, native=0)
    assert (p["kind"], p["copy"], p["fchunks"], p["dims"], p["exact_keys"], p["k_steps"]) == (0, 2, 192, 768, 0, 24)
    assert (p["fq_bytes"], p["fb_bytes"]) == (7 * 768 * 4, 1000 * 768 * 4)  # fewer rows than a chunk
    p = plan(capi, M_L2SQ, 192, 100000, 7, native=0)
    assert (p["kind"], p["copy"], p["fchunks"], p["dims"], p["fq_bytes"], p["fb_bytes"]) == (0, 0, 192, 768, 0, 0)


# ---- kk and the buffers ---------------------------------------------------------------------------------------------------------------
def test_kk(capi):
    assert plan(capi, M_L2SQ, 1, 5000, 1, k=1)["kk"] == 17
    assert plan(capi, M_L2SQ, 1, 5000, 1, k=240)["kk"] == 256


@pytest.mark.parametrize("nb,nq,k", [(4096, 1, 10), (4097, 1, 10), (70001, 1030, 240), (70000, 1030, 1), (1_000_000_000, 2, 10)])
def test_buffer_sizes_and_offsets(capi, nb, nq, k):
    p = plan(capi, M_L2SQ, 1, nb, nq, k=k)
    kk, nqt = k + 16, min(nq, 1024)
    assert p["aux_bytes"] == (nq + nb) * 4 + 8 + nq * kk * 8 + (nq + 1) * 4  # (one billion rows: above 32 bits, whole)
    assert (p["qn_off"], p["bn_off"]) == (0, nq * 4)
    assert p["best_off"] % 8 == 0 and (nq + nb) * 4 <= p["best_off"] <= (nq + nb) * 4 + 4
    assert p["flag_off"] == p["best_off"] + nq * kk * 8 and p["flag_off"] + (nq + 1) * 4 <= p["aux_bytes"]
    if nb > 4096:
        assert p["cand_bytes"] == nqt * 4096 * 8 + nqt * 4 + 16 and p["cnt_off"] == nqt * 4096 * 8
        assert p["dd_bytes"] == nqt * 4096 * 4
    else:
        assert p["cand_bytes"] == 0 and p["dd_bytes"] == nqt * nb * 4


# ---- bad input ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fields", [(-1, 1, 10, 1, 1), (1 << 31, 1, 10, 1, 1), (M_L2SQ, 0, 10, 1, 1), (M_L2SQ, (1 << 20) + 1, 10, 1, 1), (M_L2SQ, 1, -1, 1, 1),
                                    (M_L2SQ, 1, 10, -1, 1), (M_L2SQ, 1, 10, 1, 0), (M_L2SQ, 1, 10, 1, 241), (M_L2SQ, 1, 10, 1, -5)])
def test_fields_out_of_range_are_refused(capi, fields):
    with pytest.raises(capi.LanternGpuError, match="bad plan input"):
        capi.plan_exact_knn(*fields)


def test_rows_beyond_32_bits_and_null_arrays_are_refused(capi):
    for nb, nq in ((1 << 32, 1), (10, 1 << 32)):
        with pytest.raises(capi.LanternGpuError, match="do not fit the plan"):
            capi.plan_exact_knn(M_L2SQ, 1, nb, nq, 10)
    with pytest.raises(capi.LanternGpuError, match="f32 copy of a chunk of rows does not fit the plan"):
        capi.plan_exact_knn(M_L2SQ + M_I8, 2048, 70000, 1, 10, 0)
    import ctypes
    import numpy as np

    pin, out, count = np.array([M_L2SQ, 1, 10, 1, 1, -1, -1], np.int64), np.zeros(34, np.uint32), ctypes.c_size_t(0)
    fn = capi.lib().lantern_gpu_plan_exact_knn
    assert fn(None, capi._ptr(out), None, 0, ctypes.byref(count)) is not None
    assert fn(capi._ptr(pin), None, None, 0, ctypes.byref(count)) is not None
    assert fn(capi._ptr(pin), capi._ptr(out), None, 0, None) is not None
    assert fn(capi._ptr(pin), capi._ptr(out), None, 4, ctypes.byref(count)) is not None  # room for steps announced, no array
    assert fn(capi._ptr(pin), capi._ptr(out), None, 0, ctypes.byref(count)) is None and count.value == 1


def test_the_largest_call_is_planned_without_listing_its_steps(capi):
    # 65536 chunks by 4194304 query tiles, the first chunk's tiles twice: the steps are a count and a function of the index, not a list
    p = capi.plan_exact_knn(M_L2SQ, 1, (1 << 32) - 1, (1 << 32) - 1, 10)
    assert p["n_steps"] == 65536 * 4194304 + 4194304 and len(p["steps"]) == 1 << 20
    assert p["steps"][:3] == [(1024, 4096, F, 0), (1024, 61440, T, 4096), (1024, 4096, F, 0)]
    assert p["steps"][-1] == (1024, 61440, T, 4096)
