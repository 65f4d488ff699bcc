"""The C ABI of the per-query filtered search with per-query (k, ef, skip) (include/lantern_gpu.h "PER-QUERY FILTERS WITH PER-QUERY k, ef
AND skip") without a device: the symbols are exported and bound, and the first refusals of the documented order -- the lane, the
filter array, the index handle -- come before any device use.  (The refusals behind the handle need an index: tests/
test_gpu_filtered_each_params.py.)"""
import ctypes as C

import numpy as np
import pytest

NAMES = ["lantern_gpu_search_batch_filtered_each_params", "lantern_gpu_search_batch_filtered_each_params_lane",
         "lantern_gpu_search_batch_filtered_each_params_device", "lantern_gpu_last_filtered_each_params", "lantern_gpu_plan_filtered_params"]


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def call(capi, name, *args):
    err = C.c_char_p()
    getattr(capi.lib(), name)(*args, C.byref(err))
    return err.value.decode() if err.value is not None else None


def forms(capi, h, filters, nq, params, lane=0, k_stride=10):
    return {
        "lantern_gpu_search_batch_filtered_each_params": (h, filters, None, nq, capi.SCALAR_F32, params, k_stride, None, None, None),
        "lantern_gpu_search_batch_filtered_each_params_lane": (h, lane, filters, None, nq, capi.SCALAR_F32, params, k_stride, None, None, None),
        "lantern_gpu_search_batch_filtered_each_params_device": (h, filters, None, 512, nq, params, k_stride, None, None, None, None, None, None, None),
    }


def test_symbols_are_exported_and_bound(capi):
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in capi.EXPORTS, name
        assert getattr(capi.lib(), name).argtypes is not None, name
    for wrapper in ("search_batch_filtered_each_params", "search_batch_filtered_each_params_lane", "search_batch_filtered_each_params_device",
                    "last_filtered_each_params"):
        assert callable(getattr(capi.GpuIndex, wrapper)), wrapper
    assert callable(capi.plan_filtered_params) and len(capi.PLAN_FILTERED_IN) == 8


def test_the_handles_come_first_as_in_the_uniform_per_query_form(capi):
    junk = C.create_string_buffer(8192)
    nulls = (C.c_void_p * 4)()
    P = capi.query_params([(10, 64, 0)] * 4)
    bad = capi.query_params([(10, 64, 0)] * 4)
    bad["reserved"][2] = 1
    for params in (capi._ptr(P), capi._ptr(bad), None):  # (a bad parameter array does not speak before the handle does)
        for h, text in ((None, "null index handle"), (C.cast(junk, C.c_void_p), "not an index handle")):
            for name, args in forms(capi, h, nulls, 4, params).items():
                assert text in call(capi, name, *args), name
    for name, args in forms(capi, None, None, 3, capi._ptr(P)).items():
        assert "null filter array" in call(capi, name, *args), name
    for name, args in forms(capi, None, None, 0, None).items():
        assert "null index handle" in call(capi, name, *args), name  # no queries: no arrays needed, and the next check speaks
    # an entry that is no filter at all is named without an index, the first one
    arr = (C.c_void_p * 9)()
    arr[5] = arr[7] = C.addressof(junk)
    for name, args in forms(capi, None, arr, 9, None).items():
        e = call(capi, name, *args)
        assert "not a filter handle" in e and e.endswith("(filters[5])"), (name, e)
    for lane in (-1, 8):
        name = "lantern_gpu_search_batch_filtered_each_params_lane"
        assert "lane must be in [0, 8)" in call(capi, name, *forms(capi, None, None, 3, None, lane=lane)[name])
    shape = (C.c_uint32 * 4)(*([7] * 4))
    assert "null index handle" in call(capi, "lantern_gpu_last_filtered_each_params", None, shape)
    assert list(shape) == [7] * 4  # a refused call writes nothing


def test_the_wrappers_check_their_arrays(capi):
    with pytest.raises(ValueError, match="one parameter row per query"):
        capi.GpuIndex.search_batch_filtered_each_params_device(object(), [None] * 3, 0, 64, 3, [(1, 0, 0)], 1)


def test_fails_loudly_without_a_device(capi):
    if capi.device_count() > 0:  # (with a device the call is served: tests/test_gpu_filtered_each_params.py)
        return
    with pytest.raises(capi.LanternGpuError, match="no HIP device"):
        capi.GpuIndex("l2sq", 8).search_batch_filtered_each_params([None, None], np.zeros((2, 8), np.float32), [(1, 0, 0), (2, 0, 0)])
