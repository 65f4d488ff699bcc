"""The C ABI of the int8 screen's diagnostics (include/lantern_gpu.h lantern_gpu_export_screen, lantern_gpu_screen_probe) without a
device: the symbols are exported and bound, a null or foreign handle is refused, a range or an argument that can be refused from the
arguments alone is refused before the handle is looked at, and nothing computes without a device.  (A range past the size of a live
index, and everything the two calls return, needs a device: tests/test_gpu_screen_rows.py.)"""
import ctypes as C

import numpy as np
import pytest

NAMES = ["lantern_gpu_export_screen", "lantern_gpu_screen_probe"]
SIZE_MAX = C.c_size_t(-1).value


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def call(capi, name, *args):
    err = C.c_char_p()
    out = getattr(capi.lib(), name)(*args, C.byref(err))
    return out, (err.value.decode() if err.value else None)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_symbols_are_exported_and_bound(capi):
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in capi.EXPORTS, name
        assert getattr(capi.lib(), name).argtypes is not None, name
    assert capi.lib().lantern_gpu_export_screen.restype is C.c_size_t
    for wrapper in ("export_screen", "screen_probe"):
        assert callable(getattr(capi.GpuIndex, wrapper))


def test_null_and_foreign_handles_are_refused(capi):
    junk = C.cast(C.create_string_buffer(8192), C.c_void_p)
    codes, meta, norms = np.full((2, 2048), 7, np.int8), np.full((2, 2), 7, np.float32), np.full(2, 7, np.float32)
    q, slots, out = np.zeros(512, np.float32), np.zeros(2, np.uint32), np.full(2, 7, np.uint8)
    for h, text in ((None, "null index handle"), (junk, "not an index handle")):
        got, err = call(capi, "lantern_gpu_export_screen", h, 0, 2, p(codes), p(meta), p(norms))
        assert got == 0 and text in err
        got, err = call(capi, "lantern_gpu_export_screen", h, 0, 0, None, None, None)  # (the size query of the wrapper)
        assert got == 0 and text in err
        _, err = call(capi, "lantern_gpu_screen_probe", h, p(q), p(slots), 2, 1.0, 256, p(out))
        assert text in err
    assert (codes == 7).all() and (meta == 7).all() and (norms == 7).all() and (out == 7).all()  # nothing was written


def test_a_range_that_cannot_lie_in_any_index_is_refused_before_the_handle_is_looked_at(capi):
    junk = C.cast(C.create_string_buffer(8192), C.c_void_p)
    for first, count in ((SIZE_MAX, 1), (1, SIZE_MAX), (SIZE_MAX, SIZE_MAX), (SIZE_MAX // 2 + 1, SIZE_MAX // 2 + 1)):
        for h in (None, junk):
            got, err = call(capi, "lantern_gpu_export_screen", h, first, count, None, None, None)
            assert got == 0 and "slot range out of the index" in err, (first, count)
    for h in (None, junk):  # the largest range that does not wrap gets as far as the handle
        _, err = call(capi, "lantern_gpu_export_screen", h, SIZE_MAX - 1, 1, None, None, None)
        assert "handle" in err


def test_probe_arguments_are_refused_before_the_handle_is_looked_at(capi):
    junk = C.cast(C.create_string_buffer(8192), C.c_void_p)
    q, slots, out = np.zeros(512, np.float32), np.zeros(65, np.uint32), np.zeros(65, np.uint8)
    _, err = call(capi, "lantern_gpu_screen_probe", junk, p(q), p(slots), 65, 1.0, 256, p(out))
    assert "at most 64 slots" in err
    for wg in (0, 64, 128, 255, 384, 1024, -256):
        _, err = call(capi, "lantern_gpu_screen_probe", junk, p(q), p(slots), 4, 1.0, wg, p(out))
        assert "workgroup must be 256 or 512" in err, wg
    for args in ((None, p(slots), 4, 1.0, 256, p(out)), (p(q), None, 4, 1.0, 256, p(out)), (p(q), p(slots), 4, 1.0, 512, None)):
        _, err = call(capi, "lantern_gpu_screen_probe", junk, *args)
        assert "null buffer" in err and "handle" not in err
    for wg in (256, 512):  # well-formed arguments get as far as the handle
        _, err = call(capi, "lantern_gpu_screen_probe", junk, p(q), p(slots), 64, 1.0, wg, p(out))
        assert "not an index handle" in err


def test_fails_loudly_without_a_device(capi):
    if capi.device_count() > 0:
        pytest.skip("a device is present")
    with pytest.raises(capi.LanternGpuError, match="no HIP device"):
        capi.GpuIndex("l2sq", 513).export_screen()
    with pytest.raises(capi.LanternGpuError, match="no HIP device"):
        capi.GpuIndex("cos", 513).screen_probe(np.zeros(513, np.float32), [0], 1.0)
