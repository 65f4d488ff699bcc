"""CPU-side checks of the seeded-walk entry points (include/lantern_gpu.h "Filtered search" 5): exported, bound, and refusing bad
arguments before any device use (the style of tests/test_filtered_each_abi.py)."""
import ctypes as C

import pytest

NAMES = ["lantern_gpu_set_filter_seeds", "lantern_gpu_last_filtered_seeds"]


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
    for m in ("set_filter_seeds", "last_filtered_seeds"):
        assert callable(getattr(capi.GpuIndex, m)), m


def test_more_than_4096_seeds_are_refused_before_the_handle_is_looked_at(capi):
    """The limit is checked first -- with no index at all, so no device was touched -- and its message names it."""
    junk = C.create_string_buffer(4096)
    for h in (None, C.cast(junk, C.c_void_p)):
        for seeds in (4097, 10**6, 2**40):
            _, e = call(capi, "lantern_gpu_set_filter_seeds", h, seeds)
            assert e and "4096" in e and "seeds" in e, e


def test_null_and_foreign_index_handles_are_refused(capi):
    junk = C.create_string_buffer(4096)  # not an index: its first word is not the index magic
    for h in (None, C.cast(junk, C.c_void_p)):
        for seeds in (0, 1, 256, 4096):  # values within the limit: the handle check speaks
            _, e = call(capi, "lantern_gpu_set_filter_seeds", h, seeds)
            assert e and ("null index handle" in e or "not an index handle" in e), e
        out = (C.c_uint32 * 4)(*([7] * 4))
        _, e = call(capi, "lantern_gpu_last_filtered_seeds", h, out)
        assert e and ("null index handle" in e or "not an index handle" in e), e
        assert list(out) == [7] * 4  # a refused call writes nothing
    assert junk.raw == b"\0" * 4096  # ... and nothing was written through the foreign pointer


def test_scan_server_tool_knows_the_flag(capi):
    import os
    import subprocess

    tool = os.path.join(os.path.dirname(capi.LIB_PATH), "lantern-scan-server")
    r = subprocess.run([tool, "--no-such-flag"], capture_output=True, text=True)
    assert r.returncode == 2 and "--filter-seeds" in r.stderr
