"""CPU-side checks of a filter's life-cycle entry points (lantern_gpu.h "A FILTER'S LIFE CYCLE"): exported, bound, refusing bad arguments
before any device use -- and the "LSRX" message against a server whose injected back end has no extension hook."""
import ctypes as C
import socket
import struct

import numpy as np
import pytest

from tests.test_scan_server_filtered import FakeFilters, q, raw_filter_reply

NAMES = ["lantern_gpu_filter_extend", "lantern_gpu_filter_combine", "lantern_gpu_filter_export", "lantern_gpu_filter_rows", "lantern_scan_client_extend_filter"]
HANDLE = ("null filter handle", "not a filter handle")


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
    assert capi.FILTER_EXTEND_ALL == 2 and capi.FILTER_OPS == {"and": 0, "or": 1, "andnot": 2}
    for m in ("extend", "combine", "export", "__and__", "__or__", "__sub__"):
        assert callable(getattr(capi.Filter, m)), m
    assert callable(capi.ScanClient.extend_filter)


def test_null_and_foreign_filter_handles_are_refused_by_all_three_calls(capi):
    junk = C.create_string_buffer(4096)  # not a filter: its first word is not the filter magic
    foreign = C.cast(junk, C.c_void_p)
    for f, msg in ((None, HANDLE[0]), (foreign, HANDLE[1])):
        out, e = call(capi, "lantern_gpu_filter_extend", None, f, None, 0, 0)
        assert not out and e and msg in e
        out, e = call(capi, "lantern_gpu_filter_extend", None, f, None, 0, capi.FILTER_EXTEND_ALL | capi.FILTER_SKIP_DELETED)
        assert not out and e and msg in e
        for op in (0, 1, 2):
            out, e = call(capi, "lantern_gpu_filter_combine", None, f, f, op)
            assert not out and e and msg in e
        words, slots = (C.c_uint32 * 4)(7, 7, 7, 7), (C.c_uint32 * 4)(9, 9, 9, 9)
        n, e = call(capi, "lantern_gpu_filter_export", f, words, 4, slots, 4)
        assert n == 0 and e and msg in e
        assert list(words) == [7] * 4 and list(slots) == [9] * 4  # a refused call writes nothing
        n, e = call(capi, "lantern_gpu_filter_rows", f)
        assert n == 0 and e and msg in e


def test_op_flags_and_nulls_are_refused_before_any_device_use(capi):
    labels = (C.c_uint64 * 3)(1, 2, 3)
    for op in (-1, 3, 99):
        out, e = call(capi, "lantern_gpu_filter_combine", None, None, None, op)
        assert not out and e and "filter op must be" in e
    for flags in (4, 8, 0x80000000, 7):
        out, e = call(capi, "lantern_gpu_filter_extend", None, None, None, 0, flags)
        assert not out and e and "unknown filter flags" in e
    out, e = call(capi, "lantern_gpu_filter_extend", None, None, None, 3, 0)
    assert not out and e and "null label array" in e
    out, e = call(capi, "lantern_gpu_filter_extend", None, None, labels, 3, capi.FILTER_EXTEND_ALL)
    assert not out and e and "takes no labels" in e
    out, e = call(capi, "lantern_gpu_filter_extend", None, None, labels, 0, capi.FILTER_EXTEND_ALL | capi.FILTER_SKIP_DELETED)
    assert not out and e and "takes no labels" in e


def test_client_extend_filter_refusals(capi):
    labels = (C.c_uint64 * 2)(1, 2)
    n, e = call(capi, "lantern_scan_client_extend_filter", None, labels, 2, 0)
    assert n == 0 and e and "not connected" in e
    n, e = call(capi, "lantern_scan_client_extend_filter", None, None, 0, capi.FILTER_EXTEND_ALL)
    assert n == 0 and e and "not connected" in e
    n, e = call(capi, "lantern_scan_client_extend_filter", None, labels, (1 << 24) + 1, 0)  # (refused before a label is read)
    assert n == 0 and e and "too many labels" in e
    n, e = call(capi, "lantern_scan_client_extend_filter", None, None, 2, 0)
    assert n == 0 and e and "null label array" in e
    n, e = call(capi, "lantern_scan_client_extend_filter", None, labels, 2, 4)
    assert n == 0 and e and "unknown filter flags" in e
    n, e = call(capi, "lantern_scan_client_extend_filter", None, labels, 2, capi.FILTER_EXTEND_ALL)
    assert n == 0 and e and "takes no labels" in e


def raw_extend(labels, flags=0, count=None):
    labels = np.asarray(labels, dtype=np.uint64)
    return struct.pack("<IIQ", 0x5852534C, flags, labels.size if count is None else count) + labels.tobytes()


def test_an_injected_back_end_answers_the_extension_with_an_error_frame(capi):
    be = FakeFilters()
    srv = be.server(capi, max_wait_us=100)
    c = capi.ScanClient(srv.host, srv.port)
    assert c.set_filter([3, 5, 8]) == 3
    before = c.search(q(4), 5)[0].tolist()
    assert before == [4003, 4005, 4008]
    with pytest.raises(capi.LanternGpuError, match="cannot extend a filter"):
        c.extend_filter([9])
    with pytest.raises(capi.LanternGpuError, match="cannot extend a filter"):
        c.extend_filter(all_new=True)
    assert c.search(q(4), 5)[0].tolist() == before  # the connection survives, its previous filter still answers
    assert len(be.made) == 1 and not be.freed
    # the raw message: an error frame, then the same connection goes on; bad flags are named as such
    s = socket.create_connection((srv.host, srv.port))
    s.sendall(raw_extend([1, 2, 3]))
    status, msg = raw_filter_reply(s)
    assert status != 0 and "cannot extend a filter" in msg
    s.sendall(raw_extend([], flags=4))
    status, msg = raw_filter_reply(s)
    assert status != 0 and "bad extension flags" in msg
    s.sendall(raw_extend([1], flags=2))  # every new row, and labels
    status, msg = raw_filter_reply(s)
    assert status != 0 and "bad extension flags" in msg
    s.sendall(raw_extend([], count=(1 << 24) + 1))  # over the label cap: the error frame, and the connection is closed
    status, msg = raw_filter_reply(s)
    assert status != 0 and "at most" in msg
    assert s.recv(1) == b""
    s.close()
    assert c.search(q(7), 5)[0].tolist() == [7003, 7005, 7008]
    c.close()
    srv.stop()
