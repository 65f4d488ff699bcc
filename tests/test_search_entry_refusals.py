"""What the batched-search entry points (lantern_gpu_search_batch*) refuse from their arguments alone, without a device: the
exact text, and which defect is named when two are present.  The texts are written out here; the refusals that need a live index
are in tests/test_gpu_search_entry_refusals.py.  (The style of tests/test_search_params_abi.py.)"""
import ctypes as C

import numpy as np
import pytest

NULL_H = "lantern_gpu: null index handle"
FOREIGN_H = "lantern_gpu: not an index handle (stale, freed or foreign pointer)"
LANE = "lantern_gpu: lane must be in [0, 8)"
NO_PARAMS = "lantern_gpu: null parameter array"
K_STRIDE = "lantern_gpu: k_stride is smaller than a query's k (params[%d])"
RESERVED = "lantern_gpu: a query's reserved parameter word must be 0 (params[%d])"
NO_FILTERS = "lantern_gpu: null filter array"
NOT_A_FILTER = "lantern_gpu: not a filter handle (stale, freed or foreign pointer)"
NO_FILTER = "lantern_gpu: null filter handle"
NULL_HOST = "lantern_gpu: null query or result pointer"
NULL_LANE = "lantern_gpu: null buffer"
NULL_NOTIFY = "lantern_gpu: null buffer or callback"

P = "lantern_gpu_search_batch"
PLAIN, PLAIN_LANE, PLAIN_NOTIFY = P, P + "_lane", P + "_lane_notify"
DEVICE, STRIDED = P + "_device", P + "_device_strided"
PARAMS, PARAMS_LANE, PARAMS_NOTIFY, PARAMS_DEVICE = P + "_params", P + "_params_lane", P + "_params_lane_notify", P + "_params_device"
FILTERED, FILTERED_DEVICE = P + "_filtered", P + "_filtered_device"
EACH, EACH_LANE, EACH_DEVICE = P + "_filtered_each", P + "_filtered_each_lane", P + "_filtered_each_device"
ALL = [PLAIN, PLAIN_LANE, PLAIN_NOTIFY, DEVICE, STRIDED, PARAMS, PARAMS_LANE, PARAMS_NOTIFY, PARAMS_DEVICE, FILTERED, FILTERED_DEVICE, EACH, EACH_LANE,
       EACH_DEVICE]
LANED = [PLAIN_LANE, PLAIN_NOTIFY, PARAMS_LANE, PARAMS_NOTIFY, EACH_LANE]
WITH_PARAMS = [PARAMS, PARAMS_LANE, PARAMS_NOTIFY, PARAMS_DEVICE]
WITH_FILTERS = [EACH, EACH_LANE, EACH_DEVICE]


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def said(capi, name, args):
    err = C.c_char_p()
    getattr(capi.lib(), name)(*args, C.byref(err))
    return err.value.decode() if err.value else None


JUNK = C.create_string_buffer(8192)  # neither an index nor a filter: its first word is no magic
LOOKS_LIKE_A_FILTER = C.create_string_buffer((0x4C414E5446494C54).to_bytes(8, "little") + bytes(4096))  # passes the handle check; never read further


class Call:
    """One call's arguments (rows of 8 f32), complete and well-formed unless a keyword says otherwise; `forms(h)` lays them out for every entry point."""

    def __init__(self, capi, nq=6, k=10, lane=0, q=True, lab=True, dist=True, params=True, filters=True, filter=LOOKS_LIKE_A_FILTER, cb=True, kind=None, stride=32):
        self.capi, self.nq, self.k, self.lane = capi, nq, k, lane
        self.q = np.zeros((max(nq, 1), 8), np.float32)
        self.lab, self.dist, self.cnt = np.zeros((max(nq, 1), max(k, 1)), np.uint64), np.zeros((max(nq, 1), max(k, 1)), np.float32), np.zeros(max(nq, 1), np.uint32)
        self.P = capi.query_params([(1 + i if k else 0, 0, i) for i in range(max(nq, 1))])  # k = 1 .. nq; a zero-width call asks for nothing
        self.filters = (C.c_void_p * max(nq, 1))()  # every query unfiltered
        self.done = capi.QUERIES_DONE_FN(lambda ctx, which, count: None)
        self.on = dict(q=q, lab=lab, dist=dist, params=params, filters=filters, cb=cb)
        self.device = None  # (d_queries, d_labels, d_distances, d_counts) for the device forms; the host arrays where nothing would read them
        self.filter, self.kind, self.stride = filter, capi.SCALAR_F32 if kind is None else kind, stride

    def forms(self, h):
        p = lambda a, key=None: a.ctypes.data_as(C.c_void_p) if key is None or self.on[key] else None  # noqa: E731
        f32, nq, k, lane, stride = self.kind, self.nq, self.k, self.lane, self.stride
        q, answers = p(self.q, "q"), (p(self.lab, "lab"), p(self.dist, "dist"), p(self.cnt))
        dq, dl, dd, dc = self.device or ((q,) + answers)
        dev = (dl, dd, None, dc, None, None, None)  # labels, distances, slots, counts, D, E, stream
        notify = (C.cast(self.done, C.c_void_p) if self.on["cb"] else None, None)
        params = p(self.P, "params")
        filters = C.cast(self.filters, C.c_void_p) if self.on["filters"] else None
        one = C.c_void_p(self.filter) if isinstance(self.filter, int) else C.cast(self.filter, C.c_void_p) if self.filter is not None else None
        return {
            PLAIN: (h, q, nq, f32, k, 0) + answers,
            PLAIN_LANE: (h, lane, q, nq, f32, k, 0) + answers,
            PLAIN_NOTIFY: (h, lane, q, nq, f32, k, 0) + answers + notify,
            DEVICE: (h, dq, nq, k, 0, 0) + dev,
            STRIDED: (h, dq, stride, nq, k, 0, 0) + dev,
            PARAMS: (h, q, nq, f32, params, k) + answers,
            PARAMS_LANE: (h, lane, q, nq, f32, params, k) + answers,
            PARAMS_NOTIFY: (h, lane, q, nq, f32, params, k) + answers + notify,
            PARAMS_DEVICE: (h, dq, stride, nq, params, k) + dev,
            FILTERED: (h, one, q, nq, f32, k, 0) + answers,
            FILTERED_DEVICE: (h, one, dq, stride, nq, k, 0, 0) + dev,
            EACH: (h, filters, q, nq, f32, k, 0) + answers,
            EACH_LANE: (h, lane, filters, q, nq, f32, k, 0) + answers,
            EACH_DEVICE: (h, filters, dq, stride, nq, k, 0, 0) + dev,
        }


def check(capi, call, h, expected, names=ALL):
    """`expected`: one text (None: no error) for every name, or {name: text} with "*" for the rest"""
    forms = call.forms(h)
    for name in names:
        want = expected.get(name, expected.get("*")) if isinstance(expected, dict) else expected
        assert said(capi, name, forms[name]) == want, name


def junk():
    return C.cast(JUNK, C.c_void_p)


def test_every_form_is_exported_and_bound(capi):
    assert len(set(ALL)) == 14
    for name in ALL:
        assert name in capi.EXPORTS and getattr(capi.lib(), name).argtypes is not None, name


def test_null_and_foreign_index_handles(capi):
    check(capi, Call(capi), None, NULL_H)
    check(capi, Call(capi), junk(), FOREIGN_H)
    # an empty batch is no excuse: the handle is looked at all the same
    check(capi, Call(capi, nq=0), None, NULL_H)
    check(capi, Call(capi, k=0), junk(), FOREIGN_H)


def test_bad_lane(capi):
    for lane in (8, -1):
        for h, handle_text in ((None, NULL_H), (junk(), FOREIGN_H)):
            # the plain lane forms look at the handle first, the others at the lane
            check(capi, Call(capi, lane=lane), h, {PLAIN_LANE: handle_text, PLAIN_NOTIFY: handle_text, "*": LANE}, LANED)
        # ... and the lane comes before everything else those three check without an index
        check(capi, Call(capi, lane=lane, params=False, q=False, cb=False), None, LANE, [PARAMS_LANE, PARAMS_NOTIFY])
        check(capi, Call(capi, lane=lane, filters=False), None, LANE, [EACH_LANE])


def test_parameter_tables(capi):
    for h in (None, junk()):
        check(capi, Call(capi, params=False), h, NO_PARAMS, WITH_PARAMS)
        c = Call(capi)
        c.P["reserved"][4] = 7
        c.P["reserved"][5] = 1
        check(capi, c, h, RESERVED % 4, WITH_PARAMS)
        c.P["k"][2] = 11  # both defects: the first offending position is named, with ITS defect
        check(capi, c, h, K_STRIDE % 2, WITH_PARAMS)
        check(capi, Call(capi, k=3), h, K_STRIDE % 3, WITH_PARAMS)  # k = 1 .. 6: position 3 is the first whose k = 4 does not fit
    check(capi, Call(capi, nq=0, params=False), None, NULL_H, WITH_PARAMS)  # no queries: no table needed


def test_filter_arrays(capi):
    for h in (None, junk()):
        check(capi, Call(capi, filters=False), h, NO_FILTERS, WITH_FILTERS)
    check(capi, Call(capi, nq=0, filters=False), None, NULL_H, WITH_FILTERS)  # no queries: no array needed
    for pos in (0, 3, 5):
        c = Call(capi)
        c.filters[pos] = C.addressof(JUNK)
        if pos == 3:
            c.filters[4] = C.addressof(JUNK)  # the FIRST offender is named
        # which index an entry belongs to cannot be told without one; that it is no filter at all can
        check(capi, c, None, NOT_A_FILTER + " (filters[%d])" % pos, WITH_FILTERS)
        check(capi, c, junk(), NOT_A_FILTER + " (filters[%d])" % pos, WITH_FILTERS)


def test_single_filter_handle_comes_before_the_index(capi):
    for h in (None, junk()):
        check(capi, Call(capi, filter=None), h, NO_FILTER, [FILTERED, FILTERED_DEVICE])
        check(capi, Call(capi, filter=JUNK), h, NOT_A_FILTER, [FILTERED, FILTERED_DEVICE])


def test_null_buffers_where_they_are_checked_before_the_handle(capi):
    texts = {PARAMS: NULL_HOST, PARAMS_LANE: NULL_LANE, PARAMS_NOTIFY: NULL_NOTIFY}
    for h in (None, junk()):
        for missing in ("q", "lab", "dist"):
            check(capi, Call(capi, **{missing: False}), h, texts, list(texts))
            check(capi, Call(capi, params=False, **{missing: False}), h, texts, list(texts))  # the buffers come before the table
        check(capi, Call(capi, cb=False), h, {PARAMS_NOTIFY: NULL_NOTIFY, PLAIN_NOTIFY: NULL_H if h is None else FOREIGN_H}, [PARAMS_NOTIFY, PLAIN_NOTIFY])
    # nothing is read or written for an empty batch, so nothing is missed; a missing callback still is while there are queries
    check(capi, Call(capi, nq=0, q=False, lab=False, dist=False, cb=False), None, NULL_H, list(texts))
    check(capi, Call(capi, k=0, q=False, lab=False, dist=False), None, NULL_H, list(texts))
    check(capi, Call(capi, k=0, cb=False), None, NULL_NOTIFY, [PARAMS_NOTIFY])


def test_null_buffers_elsewhere_wait_for_the_handle(capi):
    rest = [PLAIN, PLAIN_LANE, PLAIN_NOTIFY, FILTERED, EACH, EACH_LANE]
    check(capi, Call(capi, q=False, lab=False, dist=False), None, NULL_H, rest)
    check(capi, Call(capi, q=False, lab=False, dist=False), junk(), FOREIGN_H, rest)
