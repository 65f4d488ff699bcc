"""What the batched-search entry points refuse once they hold a live index (tests/test_search_entry_refusals.py has the rest): the exact
text, and which defect is named when two are present.  Needs an MI355X.

One index of 64 rows x 8 dims (f32, l2sq, M = 4), calls of 3 queries and k = 2.  A refused call launches nothing; the device forms are
given real device buffers all the same."""
import numpy as np
import pytest

from tests.test_search_entry_refusals import (ALL, DEVICE, EACH, EACH_DEVICE, EACH_LANE, FILTERED, FILTERED_DEVICE, LANE, NULL_HOST, NULL_LANE, NULL_NOTIFY,
                                              PARAMS, PARAMS_DEVICE, PARAMS_LANE, PARAMS_NOTIFY, PLAIN, PLAIN_LANE, PLAIN_NOTIFY, STRIDED, Call, check)

pytestmark = pytest.mark.gpu

KIND = "lantern_gpu: scalar kind of the queries does not match the index"
STRIDE = "lantern_gpu: the query row stride does not match the index's stored row stride (lantern_gpu_row_bytes)"
AMBIGUOUS = ("lantern_gpu: this index stores rows at a stride wider than the vector's own length (lantern_gpu_row_bytes): device-resident "
             "queries must be handed over with their stride, through lantern_gpu_search_batch_device_strided")
ANOTHER = "lantern_gpu: the filter belongs to another index (built over 64 rows; this index holds 64)"
HOST = [PLAIN, PLAIN_LANE, PLAIN_NOTIFY, PARAMS, PARAMS_LANE, PARAMS_NOTIFY, FILTERED, EACH, EACH_LANE]
KIND_BEFORE_BUFFERS = [PLAIN, PLAIN_LANE, PLAIN_NOTIFY, FILTERED, EACH, EACH_LANE]
NQ, K = 3, 2


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


class Live:
    def __init__(self, capi):
        from lantern_amd import hip

        rng = np.random.default_rng(5)
        self.capi = capi
        self.gpu, self.other = (capi.GpuIndex("l2sq", 8, M=4, ef_construction=16, ef=8, seed=1) for _ in range(2))
        for ix in (self.gpu, self.other):
            ix.add_many(np.arange(64, dtype=np.uint64) + 1, rng.standard_normal((64, 8), dtype=np.float32))
        self.mine, self.theirs = self.gpu.filter_from_labels(np.arange(1, 33)), self.other.filter_from_labels(np.arange(1, 33))
        self.bufs = [hip.Buffer(NQ * 32), hip.Buffer(NQ * K * 8), hip.Buffer(NQ * K * 4), hip.Buffer(NQ * 4)]
        self.bufs[0].zero()

    def call(self, **kw):
        kw.setdefault("nq", NQ)
        kw.setdefault("k", K)
        kw.setdefault("filter", self.mine.h)
        c = Call(self.capi, **kw)
        c.P["k"] = np.minimum(c.P["k"], c.k)  # (every table here is a good one)
        c.device = tuple(b.ptr for b in self.bufs)
        return c


@pytest.fixture(scope="module")
def live(capi):
    return Live(capi)


def test_kind_mismatch(capi, live):
    check(capi, live.call(kind=capi.SCALAR_B1), live.gpu.h, KIND, HOST)
    # ... named before a missing buffer, except where the buffers are looked at before the handle
    check(capi, live.call(kind=capi.SCALAR_B1, q=False, lab=False, dist=False), live.gpu.h,
          {PARAMS: NULL_HOST, PARAMS_LANE: NULL_LANE, PARAMS_NOTIFY: NULL_NOTIFY, "*": KIND}, HOST)
    # ... and before an empty batch is let go
    check(capi, live.call(kind=capi.SCALAR_B1, nq=0), live.gpu.h, KIND, HOST)
    check(capi, live.call(kind=capi.SCALAR_B1, k=0), live.gpu.h, KIND, KIND_BEFORE_BUFFERS)


def test_bad_lane_with_a_live_index(capi, live):
    for lane in (8, -1):
        check(capi, live.call(lane=lane, kind=capi.SCALAR_B1), live.gpu.h, LANE, [PLAIN_LANE, PLAIN_NOTIFY, PARAMS_LANE, PARAMS_NOTIFY, EACH_LANE])


def test_stride_mismatch_and_ambiguous_stride(capi, live):
    for stride in (16, 48, 0):
        check(capi, live.call(stride=stride), live.gpu.h, STRIDE, [STRIDED, PARAMS_DEVICE, FILTERED_DEVICE, EACH_DEVICE])
    # bit rows of 96 bytes are stored at a 128-byte stride: the form without a stride refuses, the strided one wants 128
    wide = capi.GpuIndex("hamming", 24, M=4, ef_construction=16, ef=8, seed=1)
    assert wide.row_bytes() == 128
    check(capi, live.call(), wide.h, AMBIGUOUS, [DEVICE])
    check(capi, live.call(stride=96), wide.h, STRIDE, [STRIDED, PARAMS_DEVICE, EACH_DEVICE])
    wide.close()


def test_null_buffers_after_the_handle(capi, live):
    texts = {PLAIN_LANE: NULL_LANE, PLAIN_NOTIFY: NULL_NOTIFY, FILTERED: NULL_HOST, EACH: NULL_HOST, EACH_LANE: NULL_LANE}
    for missing in ("q", "lab", "dist"):
        check(capi, live.call(**{missing: False}), live.gpu.h, texts, list(texts))
    check(capi, live.call(cb=False), live.gpu.h, NULL_NOTIFY, [PLAIN_NOTIFY])


def test_plain_form_refuses_null_buffers(capi, live):
    """NULL queries, labels or distances are refused, never read through (as lantern_gpu_search_batch_filtered refuses them)."""
    for missing in ("q", "lab", "dist"):
        check(capi, live.call(**{missing: False}), live.gpu.h, NULL_HOST, [PLAIN])


def test_filter_of_another_index(capi, live):
    check(capi, live.call(filter=live.theirs.h), live.gpu.h, ANOTHER, [FILTERED])
    c = live.call()
    c.filters[0], c.filters[1], c.filters[2] = live.mine.h, live.theirs.h, live.theirs.h
    check(capi, c, live.gpu.h, ANOTHER + " (filters[1])", [EACH, EACH_LANE])
    # the filters are looked at even where nothing would be searched
    c = live.call(k=0)
    c.filters[1] = live.theirs.h
    check(capi, c, live.gpu.h, ANOTHER + " (filters[1])", [EACH, EACH_LANE])


def test_empty_batches_return_silently(capi, live):
    before = live.gpu.counters()["search_queries"]
    rest = [n for n in ALL if n not in (PARAMS, PARAMS_LANE, PARAMS_NOTIFY, PARAMS_DEVICE)]
    calls = [(live.call(nq=0), ALL), (live.call(nq=0, q=False, params=False, filters=False), HOST),
             # (a params form's k_stride = 0 is the width of its answer rows, not an empty batch: it is launched)
             (live.call(k=0), rest), (live.call(k=0, q=False), [n for n in rest if n in HOST])]
    for c, names in calls:
        check(capi, c, live.gpu.h, None, names)
        assert not (c.lab.any() or c.dist.any() or c.cnt.any()), "an empty batch writes nothing"
    assert live.gpu.counters()["search_queries"] == before
