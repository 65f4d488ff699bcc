"""The dense route of the filtered exact path, without a device (include/lantern_gpu.h "THE EXACT PATH'S DENSE ROUTE"):
lantern_gpu_plan_filtered_dense is the decision the call itself takes and the exact k-NN plan it then runs."""
import ctypes as C

import pytest

L2SQ, COS, HAMMING = 3, 1, 8  # usearch_metric_kind_t: the metric codes of f32 / bit rows (+ 100: f16 storage, + 200: i8)


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def test_decision_on_each_side_of_every_condition(capi):
    plan = lambda **kw: capi.plan_filtered_dense(**{**dict(mcode=L2SQ, chunks=32, allowed=5000, nq=64, k=10, skip=0, min_queries=64), **kw})
    p = plan()
    assert p["taken"] and p["why"] == "taken" and p["kk"] == 26
    # the setting: 0 is off
    p = plan(min_queries=0)
    assert not p["taken"] and p["why"] == "off" and p["n_steps"] == 0 and p["steps"] == [] and p["gather_bytes"] == 0 and p["kk"] == 0
    # nq = m - 1 / m
    assert plan(nq=63)["why"] == "few_queries" and not plan(nq=63)["taken"]
    assert plan(nq=64)["taken"] and plan(nq=1, min_queries=1)["taken"]
    # k + skip = 240 / 241, by k and by skip
    assert plan(k=240)["taken"] and plan(k=240)["kk"] == 256
    assert plan(k=10, skip=230)["taken"] and plan(k=10, skip=230)["kk"] == 256
    assert plan(k=241)["why"] == "wide" and plan(k=10, skip=231)["why"] == "wide" and not plan(k=10, skip=231)["taken"]
    # a compact pq index; a query on the walk path
    assert plan(compact=True)["why"] == "compact" and not plan(compact=True)["taken"]
    assert plan(exact=False)["why"] == "walk_path" and not plan(exact=False)["taken"]
    # nothing to launch
    assert plan(allowed=0)["why"] == "empty" and plan(nq=0)["why"] == "empty" and plan(k=0)["why"] == "empty"


@pytest.mark.parametrize("allowed", [1, 4095, 4096, 4097, 65535, 65536, 65537, 200000])
@pytest.mark.parametrize("nq", [3, 1024, 1025])
@pytest.mark.parametrize("fused", [-1, 0, 1])
def test_steps_are_the_exact_knn_plans(capi, allowed, nq, fused):
    for mcode, chunks in ((L2SQ, 2), (COS + 100, 96), (L2SQ + 200, 48), (HAMMING, 6)):
        for k, skip in ((10, 0), (10, 20), (1, 239)):
            mine = capi.plan_filtered_dense(mcode, chunks, allowed, nq, k, skip, min_queries=1, fused=fused)
            knn = capi.plan_exact_knn(mcode, chunks, allowed, nq, k + skip, fused=fused)
            assert mine["taken"]
            assert mine["n_steps"] == knn["n_steps"] and mine["steps"] == knn["steps"]
            assert mine["kk"] == knn["kk"] == k + skip + 16
            assert mine["gather_rows"] == knn["chunk_rows"] == min(allowed, 65536)


def test_buffer_sizes(capi):
    # one chunk of rows as stored; one norm word per allowed row, none for bit rows
    p = capi.plan_filtered_dense(L2SQ, 192, 100000, 256, 10, min_queries=1)
    assert p["gather_rows"] == 65536 and p["gather_bytes"] == 65536 * 192 * 16 and p["norm_bytes"] == 400000
    p = capi.plan_filtered_dense(L2SQ, 192, 300, 256, 10, min_queries=1)
    assert p["gather_rows"] == 300 and p["gather_bytes"] == 300 * 192 * 16 and p["norm_bytes"] == 1200
    p = capi.plan_filtered_dense(L2SQ + 100, 96, 70000, 8, 10, min_queries=1)  # f16 rows: gathered as stored
    assert p["gather_bytes"] == 65536 * 96 * 16 and p["norm_bytes"] == 280000
    p = capi.plan_filtered_dense(L2SQ + 100, 96, 70000, 8, 10, min_queries=1, native=0)  # ... also when they are dequantised afterwards
    assert p["gather_bytes"] == 65536 * 96 * 16 and p["norm_bytes"] == 280000
    p = capi.plan_filtered_dense(HAMMING, 6, 70000, 8, 10, min_queries=1)
    assert p["gather_bytes"] == 65536 * 6 * 16 and p["norm_bytes"] == 0
    # a gather buffer above 4 GiB keeps its high word (the largest row the plan accepts is far above any index's)
    p = capi.plan_filtered_dense(L2SQ, 8192, 70000, 8, 10, min_queries=1)
    assert p["gather_bytes"] == 65536 * 8192 * 16 > 2**32


def test_bad_input_is_refused_on_either_side_of_the_decision(capi):
    for mq in (0, 1):
        with pytest.raises(capi.LanternGpuError, match="bad plan input"):
            capi.plan_filtered_dense(L2SQ, 0, 100, 8, 10, min_queries=mq)
        with pytest.raises(capi.LanternGpuError, match="bad plan input"):
            capi.plan_filtered_dense(L2SQ, 2, -1, 8, 10, min_queries=mq)
    count = C.c_size_t(0)
    assert b"null plan array" in capi.lib().lantern_gpu_plan_filtered_dense(None, None, None, 0, C.byref(count))


def test_setter_getter_and_stats_refuse_a_foreign_handle(capi):
    junk = C.create_string_buffer(8192)
    h = C.cast(junk, C.c_void_p)
    err = C.c_char_p()
    capi.lib().lantern_gpu_set_filter_dense(h, 4, C.byref(err))
    assert err.value and b"not an index handle" in err.value
    err = C.c_char_p()
    assert capi.lib().lantern_gpu_filter_dense(h, C.byref(err)) == 0
    assert err.value and b"not an index handle" in err.value
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    err = C.c_char_p()
    capi.lib().lantern_gpu_filter_dense_stats(h, out, C.byref(err))
    assert err.value and b"not an index handle" in err.value and list(out) == [7, 7, 7, 7]
