"""CPU-side checks of the per-query filtered-search entry points: exported, bound, and refusing bad arguments before any device use
(the style of tests/test_filtered_search_abi.py)."""
import ctypes as C

import numpy as np
import pytest

NAMES = ["lantern_gpu_search_batch_filtered_each", "lantern_gpu_search_batch_filtered_each_device", "lantern_gpu_search_batch_filtered_each_lane",
         "lantern_gpu_last_filtered_each"]


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def call(capi, name, *args):
    err = C.c_char_p()
    out = getattr(capi.lib(), name)(*args, C.byref(err))
    return out, (err.value.decode() if err.value is not None else None)


def host(capi, h, filters, nq):
    return call(capi, "lantern_gpu_search_batch_filtered_each", h, filters, None, nq, capi.SCALAR_F32, 10, 0, None, None, None)[1]


def device(capi, h, filters, nq):
    return call(capi, "lantern_gpu_search_batch_filtered_each_device", h, filters, None, 512, nq, 10, 0, 0, None, None, None, None, None, None, None)[1]


def lane(capi, h, filters, nq, which=0):
    return call(capi, "lantern_gpu_search_batch_filtered_each_lane", h, which, filters, None, nq, capi.SCALAR_F32, 10, 0, None, None, None)[1]


def test_symbols_exported_and_bound(capi):
    raw = C.CDLL(capi.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in capi.EXPORTS, n
        assert getattr(capi.lib(), n).argtypes is not None, n
    for m in ("search_batch_filtered_each", "search_batch_filtered_each_device", "search_batch_filtered_each_lane", "last_filtered_each"):
        assert callable(getattr(capi.GpuIndex, m)), m


def test_null_and_foreign_index_handles_are_refused(capi):
    junk = C.create_string_buffer(4096)  # not an index: its first word is not the index magic
    nulls = (C.c_void_p * 4)()  # four unfiltered entries: a valid filter array
    for h in (None, C.cast(junk, C.c_void_p)):
        for e in (host(capi, h, nulls, 4), device(capi, h, nulls, 4), lane(capi, h, nulls, 4)):
            assert e and ("null index handle" in e or "not an index handle" in e), e
        shape = (C.c_uint32 * 6)(*([7] * 6))
        _, e = call(capi, "lantern_gpu_last_filtered_each", h, shape)
        assert e and ("null index handle" in e or "not an index handle" in e)
        assert list(shape) == [7] * 6  # a refused call writes nothing


def test_a_junk_entry_is_named_without_an_index(capi):
    """Which index an entry belongs to cannot be told without one; that an entry is no filter at all can, and its position is named --
    before any device use."""
    junk = C.create_string_buffer(4096)
    for pos in (0, 5, 8):
        arr = (C.c_void_p * 9)()
        arr[pos] = C.addressof(junk)
        if pos == 5:
            arr[7] = C.addressof(junk)  # the FIRST offender is named
        for e in (host(capi, None, arr, 9), device(capi, None, arr, 9), lane(capi, None, arr, 9)):
            assert e and "not a filter handle" in e and e.endswith("(filters[%d])" % pos), e
    for e in (host(capi, None, None, 3), device(capi, None, None, 3), lane(capi, None, None, 3)):
        assert e and "null filter array" in e, e
    for e in (host(capi, None, None, 0), device(capi, None, None, 0), lane(capi, None, None, 0)):
        assert e and "null index handle" in e, e  # no queries: no array needed, and the next check speaks


def test_lane_is_validated_first(capi):
    for which in (-1, 8, 100):
        e = lane(capi, None, None, 3, which)
        assert e and "lane must be in [0, 8)" in e


def test_wrapper_builds_the_handle_array(capi):
    arr = capi.GpuIndex._filter_array([None, 4096, None], 3)
    assert arr.dtype == np.uint64 and arr.tolist() == [0, 4096, 0]
    with pytest.raises(ValueError, match="one filter"):
        capi.GpuIndex._filter_array([None], 2)
    closed = capi.Filter(None, None)
    with pytest.raises(ValueError, match="closed Filter"):
        capi.GpuIndex._filter_array([closed], 1)
