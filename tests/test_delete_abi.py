"""The delete entry points at the C boundary, without a device: they exist, the binding covers them, and every argument check
comes before any device use (as tests/test_capi_exports.py test_argument_validation_precedes_device_use)."""
import ctypes as C

import pytest

NAMES = ("lantern_gpu_remove_labels", "lantern_gpu_deleted_count", "lantern_gpu_unlink_deleted")


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def test_exports_exist_and_the_binding_covers_them(capi):
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in capi.EXPORTS
    assert [n for n, _ in capi.UnlinkStats._fields_] == ["tombstones_unlinked", "lists_repaired", "offers", "lists_cut", "request_evals",
                                                         "reprune_evals", "entry_moved"]
    assert C.sizeof(capi.UnlinkStats) == 56
    for method in ("remove_labels", "deleted_count", "unlink_deleted"):
        assert hasattr(capi.GpuIndex, method)


def test_null_and_foreign_handles_are_refused(capi):
    L = capi.lib()
    foreign = C.create_string_buffer(4096)  # readable memory that is no index
    labels = (C.c_uint64 * 2)(1, 2)
    for handle, text in ((None, b"null index handle"), (C.cast(foreign, C.c_void_p), b"not an index handle")):
        err, removed, st = C.c_char_p(), C.c_uint64(77), capi.UnlinkStats()
        L.lantern_gpu_remove_labels(handle, labels, 2, C.byref(removed), C.byref(err))
        assert text in err.value and removed.value == 0
        err = C.c_char_p()
        assert L.lantern_gpu_deleted_count(handle, C.byref(err)) == 0 and text in err.value
        err = C.c_char_p()
        st.offers = 5
        L.lantern_gpu_unlink_deleted(handle, C.byref(st), C.byref(err))
        assert text in err.value and st.offers == 0
        # a null stats pointer and a null removed pointer are accepted: the refusal is still the handle's
        err = C.c_char_p()
        L.lantern_gpu_unlink_deleted(handle, None, C.byref(err))
        assert text in err.value
        err = C.c_char_p()
        L.lantern_gpu_remove_labels(handle, labels, 2, None, C.byref(err))
        assert text in err.value
        L.lantern_gpu_remove_labels(handle, labels, 2, None, None)  # and a null error slot
        L.lantern_gpu_unlink_deleted(handle, None, None)


def test_null_labels_with_a_count_are_refused_before_the_handle_is_looked_at(capi):
    L = capi.lib()
    foreign = C.create_string_buffer(4096)
    for handle in (None, C.cast(foreign, C.c_void_p)):
        err, removed = C.c_char_p(), C.c_uint64(9)
        L.lantern_gpu_remove_labels(handle, None, 3, C.byref(removed), C.byref(err))
        assert b"null label array" in err.value and removed.value == 0
    # n == 0 with null labels is no argument error: the handle is what is refused
    err = C.c_char_p()
    L.lantern_gpu_remove_labels(None, None, 0, None, C.byref(err))
    assert b"null index handle" in err.value
