"""Every way a batch of queries reaches the search kernels gives the same answers: the three trips through the host
(lantern_amd/csrc/host_trip.hpp: the index's own block, a lane, device-resident) and lane_notify, with each launch that rides them.
Needs an MI355X.

One index of 2 000 x 32 (f32, l2sq, M = 8, ef = 32) and two batches on it, in this order: (nq, k) = (64, 10), then (5, 3) -- a lane's
staging block grows for the first and is reused, too large, by the second, and the 64-byte rounding of the block's regions falls
differently.  The device-resident strided form, copied down, is the reference; labels, distance bits and counts are equal, no
tolerance: the same kernels walk the same graph (a filter that allows every row, and no filter at all in the per-query form, are the
unfiltered walk: tests/test_gpu_filtered_search.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, LANES = 2000, 32, (0, 7)
SHAPES = [(64, 10), (5, 3)]


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


@pytest.fixture(scope="module")
def index(capi):
    rng = np.random.default_rng(11)
    gpu = capi.GpuIndex("l2sq", D, M=8, ef_construction=32, ef=32, seed=3)
    gpu.set_add_batch(256, 16)
    gpu.add_many(np.arange(N, dtype=np.uint64) + 1, rng.standard_normal((N, D), dtype=np.float32))
    return gpu, gpu.filter_from_bitmap(np.ones(N, dtype=bool)), rng


def device_strided(gpu, queries, k):
    from lantern_amd import hip

    nq = queries.shape[0]
    rows = gpu.device_query_rows(queries)
    dq, lab, dist, cnt = hip.Buffer.from_numpy(rows), hip.Buffer(nq * k * 8), hip.Buffer(nq * k * 4), hip.Buffer(nq * 4)
    gpu.search_batch_device(dq.ptr, nq, k, 0, 0, lab.ptr, dist.ptr, None, cnt.ptr, query_stride=rows.strides[0])
    hip.synchronize()
    return lab.download((nq, k), np.uint64), dist.download((nq, k), np.float32), cnt.download(nq, np.uint32)


def test_every_form_gives_the_device_forms_answers(capi, index):
    gpu, everything, rng = index
    for nq, k in SHAPES:
        queries = rng.standard_normal((nq, D), dtype=np.float32)
        want = device_strided(gpu, queries, k)
        assert np.all(want[2] == k) and np.all(want[0] > 0)  # full rows: nothing is equal for being empty
        table, nobody = [(k, 0, 0)] * nq, [None] * nq
        forms = {"search_batch": gpu.search_batch(queries, k)}
        for lane in LANES:
            forms[f"search_batch_lane({lane})"] = gpu.search_batch_lane(lane, queries, k)
            forms[f"search_batch_params_lane({lane})"] = gpu.search_batch_params_lane(lane, queries, table, k_stride=k)
            forms[f"search_batch_filtered_each_lane({lane})"] = gpu.search_batch_filtered_each_lane(lane, nobody, queries, k)
        forms["search_batch_lane_notify"] = gpu.search_batch_lane_notify(3, queries, k)[:3]
        forms["search_batch_params"] = gpu.search_batch_params(queries, table, k_stride=k)
        forms["search_batch_params_lane_notify"] = gpu.search_batch_params_lane_notify(3, queries, table, k_stride=k)[:3]
        forms["search_batch_filtered"] = gpu.search_batch_filtered(everything, queries, k)
        forms["search_batch_filtered_each"] = gpu.search_batch_filtered_each(nobody, queries, k)
        for name, (lab, dist, cnt) in forms.items():
            what = f"{name}, nq = {nq}, k = {k}"
            assert np.array_equal(lab, want[0]), what + ": labels differ"
            assert np.array_equal(dist.view(np.uint32), want[1].view(np.uint32)), what + ": distance bits differ"
            assert np.array_equal(cnt, want[2]), what + ": counts differ"
