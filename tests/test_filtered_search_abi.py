"""CPU-side checks of the filtered-search entry points: exported, bound, and refusing bad arguments before any device use."""
import ctypes as C

import pytest

NAMES = ["lantern_gpu_filter_from_labels", "lantern_gpu_filter_from_slot_bitmap", "lantern_gpu_filter_count", "lantern_gpu_filter_free",
         "lantern_gpu_set_filter_policy", "lantern_gpu_filter_stats", "lantern_gpu_last_filtered_launch", "lantern_gpu_search_batch_filtered",
         "lantern_gpu_search_batch_filtered_device", "lantern_gpu_cursor_search_filtered", "lantern_scan_set_filter"]


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


def test_symbols_exported_and_bound(capi):
    raw = C.CDLL(capi.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
        assert n in capi.EXPORTS, n
        assert getattr(capi.lib(), n).argtypes is not None, n
    assert capi.FILTER_SKIP_DELETED == 1
    for m in ("filter_from_labels", "filter_from_bitmap", "search_batch_filtered", "search_batch_filtered_device", "set_filter_policy",
              "filter_stats", "last_filtered_launch"):
        assert callable(getattr(capi.GpuIndex, m)), m
    assert callable(capi.Cursor.search_filtered) and callable(capi.Scan.set_filter)
    assert isinstance(capi.Filter.count, property) and callable(capi.Filter.close)


def test_null_and_foreign_index_handles_are_refused(capi):
    junk = C.create_string_buffer(4096)  # not an index: its first word is not the index magic
    labels = (C.c_uint64 * 3)(1, 2, 3)
    words = (C.c_uint32 * 1)(7)
    for h in (None, C.cast(junk, C.c_void_p)):
        f, e = call(capi, "lantern_gpu_filter_from_labels", h, labels, 3, 0)
        assert not f and e and ("null index handle" in e or "not an index handle" in e)
        f, e = call(capi, "lantern_gpu_filter_from_slot_bitmap", h, words, 1, 0)
        assert not f and e and ("null index handle" in e or "not an index handle" in e)
        _, e = call(capi, "lantern_gpu_filter_stats", h, None, None)
        assert e and "index handle" in e
        _, e = call(capi, "lantern_gpu_set_filter_policy", h, 0, 0, C.c_double(16.0))
        assert e and "index handle" in e
        shape = (C.c_uint32 * 6)(*([7] * 6))
        _, e = call(capi, "lantern_gpu_last_filtered_launch", h, shape)
        assert e and ("null index handle" in e or "not an index handle" in e)
        assert list(shape) == [7] * 6  # a refused call writes nothing


def test_null_and_foreign_filter_handles_are_refused(capi):
    junk = C.create_string_buffer(4096)
    for f in (None, C.cast(junk, C.c_void_p)):
        n, e = call(capi, "lantern_gpu_filter_count", f)
        assert n == 0 and e and ("null filter handle" in e or "not a filter handle" in e)
        _, e = call(capi, "lantern_gpu_search_batch_filtered", None, f, None, 1, capi.SCALAR_F32, 10, 0, None, None, None)
        assert e and "filter handle" in e
        _, e = call(capi, "lantern_gpu_search_batch_filtered_device", None, f, None, 512, 1, 10, 0, 0, None, None, None, None, None, None, None)
        assert e and "filter handle" in e
    capi.lib().lantern_gpu_filter_free(None)  # a no-op
    capi.lib().lantern_gpu_filter_free(C.cast(junk, C.c_void_p))  # not a filter: left alone


def test_policy_path_and_flags_are_validated_first(capi):
    for path in (-1, 3, 7):
        _, e = call(capi, "lantern_gpu_set_filter_policy", None, path, 0, C.c_double(16.0))
        assert e and "filter path must be 0 (auto), 1 (walk) or 2 (exact)" in e
    _, e = call(capi, "lantern_gpu_set_filter_policy", None, 0, 0, C.c_double(-1.0))
    assert e and "exact_factor" in e
    _, e = call(capi, "lantern_gpu_filter_from_labels", None, None, 0, 2)
    assert e and "unknown filter flags" in e
    _, e = call(capi, "lantern_gpu_filter_from_slot_bitmap", None, None, 4, 0)
    assert e and "null bitmap" in e
    _, e = call(capi, "lantern_scan_set_filter", None, None)
    assert e and "null scan" in e
    n, e = call(capi, "lantern_gpu_cursor_search_filtered", None, None, None, capi.SCALAR_F32, 10, 0, False, None, None)
    assert n == 0 and e and "null cursor" in e
