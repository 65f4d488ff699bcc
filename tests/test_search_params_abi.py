"""The C ABI of the per-query-parameter search (include/lantern_gpu.h "PER-QUERY k, ef AND skip") without a device: the symbols are
exported and bound, and everything that can be refused from the arguments alone is refused before a device is touched, naming the
first offending position."""
import ctypes as C

import numpy as np
import pytest

NAMES = ["lantern_gpu_search_batch_params", "lantern_gpu_search_batch_params_lane", "lantern_gpu_search_batch_params_lane_notify",
         "lantern_gpu_search_batch_params_device", "lantern_gpu_last_params_launch", "lantern_scan_server_start_params_fn"]


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def call(capi, name, *args):
    err = C.c_char_p()
    getattr(capi.lib(), name)(*args, C.byref(err))
    return err.value.decode() if err.value else None


class Args:
    def __init__(self, capi, nq=6, k_stride=10):
        self.nq, self.k_stride = nq, k_stride
        self.q = np.zeros((nq, 8), dtype=np.float32)
        self.P = capi.query_params([(1 + i, 0, i) for i in range(nq)])
        self.lab, self.dist, self.cnt = np.zeros((nq, k_stride), np.uint64), np.zeros((nq, k_stride), np.float32), np.zeros(nq, np.uint32)
        self.cb = capi.QUERIES_DONE_FN(lambda ctx, which, count: None)

    def forms(self, capi, h, lane=0, q=True, lab=True, params=True):
        p = lambda a, on=True: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
        host = (p(self.q, q), self.nq, 0, p(self.P, params), self.k_stride, p(self.lab, lab), p(self.dist), p(self.cnt))
        return {
            "lantern_gpu_search_batch_params": (h,) + host,
            "lantern_gpu_search_batch_params_lane": (h, lane) + host,
            "lantern_gpu_search_batch_params_lane_notify": (h, lane) + host + (C.cast(self.cb, C.c_void_p), None),
            "lantern_gpu_search_batch_params_device": (h, p(self.q, q), 32, self.nq, p(self.P, params), self.k_stride, p(self.lab, lab), p(self.dist), None,
                                                       p(self.cnt), None, None, None),
        }


def test_symbols_are_exported_and_bound(capi):
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in capi.EXPORTS, name
        assert getattr(capi.lib(), name).argtypes is not None, name
    assert capi.QUERY_PARAMS.itemsize == 16 and capi.QUERY_PARAMS.names == ("k", "ef", "skip", "reserved")
    P = capi.query_params([(10, 64, 3), (5,), (7, 20)])
    assert P.tolist() == [(10, 64, 3, 0), (5, 0, 0, 0), (7, 20, 0, 0)]
    for wrapper in ("search_batch_params", "search_batch_params_lane", "search_batch_params_lane_notify", "search_batch_params_device",
                    "last_params_launch"):
        assert callable(getattr(capi.GpuIndex, wrapper))


def test_null_and_foreign_handles_are_refused(capi):
    a = Args(capi)
    junk = C.create_string_buffer(8192)
    for name, args in a.forms(capi, None).items():
        assert "null index handle" in call(capi, name, *args), name
    for name, args in a.forms(capi, C.cast(junk, C.c_void_p)).items():
        assert "not an index handle" in call(capi, name, *args), name
    out = np.zeros(6, dtype=np.uint32)
    assert "null index handle" in call(capi, "lantern_gpu_last_params_launch", None, out.ctypes.data_as(C.c_void_p))
    assert "not an index handle" in call(capi, "lantern_gpu_last_params_launch", C.cast(junk, C.c_void_p), out.ctypes.data_as(C.c_void_p))


def test_bad_arguments_are_refused_before_the_handle_is_looked_at(capi):
    """(whatever the handle is: these messages come from the arguments alone, so they reach a caller without a device too)"""
    junk = C.cast(C.create_string_buffer(8192), C.c_void_p)
    a = Args(capi)
    for name in ("lantern_gpu_search_batch_params_lane", "lantern_gpu_search_batch_params_lane_notify"):
        for lane in (-1, 8):
            assert "lane must be in [0, 8)" in call(capi, name, *a.forms(capi, junk, lane=lane)[name]), name
    a.P["reserved"][4] = 7
    a.P["reserved"][5] = 1
    for name, args in a.forms(capi, junk).items():
        assert call(capi, name, *args).endswith("reserved parameter word must be 0 (params[4])"), name
    a = Args(capi, k_stride=3)  # k = 1 .. 6: position 3 is the first whose k = 4 does not fit
    for name, args in a.forms(capi, junk).items():
        assert call(capi, name, *args).endswith("k_stride is smaller than a query's k (params[3])"), name
    a = Args(capi)
    for name, args in a.forms(capi, junk, params=False).items():
        assert "null parameter array" in call(capi, name, *args), name
    for name, args in a.forms(capi, junk, q=False).items():
        if not name.endswith("_device"):
            assert "null" in call(capi, name, *args) and "handle" not in call(capi, name, *args), name
    for name, args in a.forms(capi, junk, lab=False).items():
        if not name.endswith("_device"):
            assert "null" in call(capi, name, *args) and "handle" not in call(capi, name, *args), name
    args = list(a.forms(capi, junk)["lantern_gpu_search_batch_params_lane_notify"])
    args[-2] = None  # no callback
    assert "null buffer or callback" in call(capi, "lantern_gpu_search_batch_params_lane_notify", *args)


def test_scan_server_params_fn_arguments(capi):
    err = C.c_char_p()
    fn = capi.BATCH_SEARCH_FN(lambda *a: 1)
    pfn = capi.BATCH_SEARCH_PARAMS_FN(lambda *a: 1)
    lib = capi.lib()
    assert lib.lantern_scan_server_start_params_fn(fn, C.cast(None, capi.BATCH_SEARCH_PARAMS_FN), None, 16, b"127.0.0.1", 0, 8, 100, C.byref(err)) is None
    assert b"bad scan server arguments" in err.value
    assert lib.lantern_scan_server_start_params_fn(fn, pfn, None, 0, b"127.0.0.1", 0, 8, 100, C.byref(err)) is None
    assert b"bad scan server arguments" in err.value


def test_fails_loudly_without_a_device(capi):
    if capi.device_count() > 0:
        pytest.skip("a device is present")
    with pytest.raises(capi.LanternGpuError, match="no HIP device"):
        capi.GpuIndex("l2sq", 8).search_batch_params(np.zeros((2, 8), np.float32), [(1, 0, 0), (2, 0, 0)])
