"""The three forms of a filtered call against each other (include/lantern_gpu.h "Filtered search").  Needs an MI355X.

One small batch goes through the single-filter call, the per-query-filter call and the per-query-parameter call with uniform parameters:
every query's answer is the same bytes whichever form carried it, the launch records are those of the plan (lantern_gpu_plan_filtered_params),
and a batch of nothing but riders does in each form what that form does.  The restatement of tests/filtered_walk_ref.py is the arbiter of
the answers themselves in the suites of each form; here only the forms' agreement is at stake, so the index is built on the device.

Every case runs as the library stands, with the seeded walk (the table builder's single-filter caller) and with both dense routes (its
relaunch of refused queries, and the answer kernel's two callers).
"""
import re

import numpy as np
import pytest

from tests.test_gpu_filtered_each import EachDev
from tests.test_gpu_filtered_each_params import ParamsDev
from tests.test_gpu_filtered_search import same

pytestmark = pytest.mark.gpu

N, D, M, EF = 600, 24, 8, 64
K, SKIP = 5, 2
# exact iff allowed^2 <= factor * ef * n: 40 rows take the exact path at ef = 64 from a factor of 0.042 on, 450 rows walk below 5.27 (at the
# default of 5.6 the rule would send 450 rows of 600 down the exact path as well)
FACTOR = 1.0
MODES = ["plain", "seeded", "dense"]


class FormsDev(EachDev, ParamsDev):
    pass


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


_INDEX = {}


def index(capi, metric):
    """(gpu, queries, [empty, 3 rows, 40 rows, 450 rows]): built once per metric"""
    if metric not in _INDEX:
        rng = np.random.default_rng(600 + len(metric))
        base = rng.standard_normal((N, D), dtype=np.float32)
        queries = rng.standard_normal((9, D), dtype=np.float32)
        gpu = capi.GpuIndex(metric, D, M=M, ef_construction=32, ef=EF, seed=7)
        gpu.add_many(np.arange(N, dtype=np.uint64) + 1, base)
        gpu.flush()
        filt = []
        for count in (0, 3, 40, 450):
            a = np.zeros(N, dtype=bool)
            a[rng.permutation(N)[:count]] = True
            filt.append(gpu.filter_from_bitmap(a))
            assert filt[-1].count == count
        _INDEX[metric] = gpu, queries, filt
    return _INDEX[metric]


class mode_set:
    """the index's filter policy for one case, the defaults again behind it"""

    def __init__(self, gpu, mode):
        self.gpu, self.mode = gpu, mode

    def __enter__(self):
        self.gpu.set_filter_policy("auto", exact_factor=FACTOR)
        self.gpu.set_filter_seeds(8 if self.mode == "seeded" else 0)
        self.gpu.set_filter_dense(1 if self.mode == "dense" else 0)
        self.gpu.set_filter_dense_each(2 if self.mode == "dense" else 0)

    def __exit__(self, *exc):
        self.gpu.set_filter_policy("auto")
        self.gpu.set_filter_seeds(0)
        self.gpu.set_filter_dense(0)
        self.gpu.set_filter_dense_each(0)


def plan_of(capi, gpu, counts, seeds):
    fields = {"chunks": gpu.row_bytes() // 16, "M0": 2 * M, "n": N, "ef_default": EF, "path": 0, "cand_cap": 0, "exact_factor": FACTOR, "seeds": seeds}
    per, launch, why = capi.plan_filtered_params(fields, counts, [(K, EF, SKIP)] * len(counts))
    assert why is None, why
    return per, launch


def rows_of(out, qs, with_labels=True):
    """the answers of queries qs: slots, distances, counts, D, E -- and the labels"""
    return tuple(a[qs] for a in (out if with_labels else out[:5]))


def same_bytes(a, b):
    same(a, b)
    assert np.array_equal(a[5], b[5]), "labels differ"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_every_query_answers_alike_through_the_three_forms(capi, metric, mode):
    gpu, queries, filt = index(capi, metric)
    empty, f3, f40, f450 = filt
    filters = [empty, f3, f40, f450, None, f40, f450, None, f3]
    counts = [-1 if f is None else f.count for f in filters]
    seeds = 8 if mode == "seeded" else 0
    dev = FormsDev(gpu, queries, K)
    with mode_set(gpu, mode):
        each = dev.each(filters, ef=EF, skip=SKIP)
        regime = gpu.last_filtered_each()
        each_dense = gpu.last_filtered_each_dense()
        params = dev.each_params(filters, [(K, EF, SKIP)] * 9)
        carve = gpu.last_filtered_each_params()
        # 1. the per-query forms agree on every query, the NULL entries included; the single-filter form on the queries of its filter
        same_bytes(each, params)
        per, launch = plan_of(capi, gpu, counts, seeds)
        assert [q["path"] for q in per] == [0, 2, 2, 1, 1, 2, 1, 1, 2]
        assert (regime["walk"], regime["exact"], regime["unfiltered"], regime["empty"], regime["distinct_filters"]) == (4, 4, 2, 1, 4)
        if mode == "dense":  # (the groups: f3 twice, f40 twice; what the certificate refuses comes back into the exact launch)
            assert (each_dense["groups"], each_dense["queries"]) == (2, 4)
        else:
            assert each_dense["queries"] == 0
        # 2. the params call's carve is the plan's
        assert carve == {"largest_expansion": launch["walk"]["expansion"], "largest_cand_cap": launch["walk"]["cand_cap"],
                         "largest_exact_keys": launch["exact"]["expansion"], "k_zero": 0}
        assert carve["largest_expansion"] == EF and carve["largest_exact_keys"] == K + SKIP
        for f in filt:
            qs = [q for q in range(9) if filters[q] is f]
            single = dev.filtered(f, ef=EF, skip=SKIP)
            same_bytes(rows_of(single, qs), rows_of(each, qs))
            # 2. ... and the single-filter call's launch is the plan's for nine queries behind this filter
            shape = gpu.last_filtered_launch()
            _, solo = plan_of(capi, gpu, [f.count] * 9, seeds)
            want_path = None if f.count == 0 else "walk" if f is f450 else "exact"
            if mode == "dense" and shape["path"] == "dense":
                assert want_path == "exact" and shape["expansion"] == K + SKIP
                continue
            assert shape["path"] == want_path
            want = solo[want_path] if want_path else dict.fromkeys(solo["walk"], 0)
            assert (shape["expansion"], shape["cand_cap"], shape["lds_bytes"]) == (want["expansion"], want["cand_cap"], want["lds"])
            if want_path == "walk":
                assert shape["vis_slots"] == want["vis_slots_or_rows"]
            else:
                assert shape["vis_slots"] == 0
            if want_path == "walk":
                got = gpu.last_filtered_seeds()
                assert (got["seeded"], got["unseeded"]) == ((9, 0) if seeds else (0, 9))
        # the answers are answers: counts by the filters' sizes behind the skip
        assert list(each[2]) == [max(0, min(K, (N if c < 0 else c) - SKIP)) for c in counts]


def test_uniform_parameters_past_32_bits_are_refused_by_every_form(capi):
    """The plan's clamp (tests/test_filtered_params_plan.py) holds for the uniform forms, whose k, ef and skip are size_t: 2^32 + 1 is
    refused over budget before anything is queued, never planned as the 1 it would wrap to."""
    gpu, queries, filt = index(capi, "l2sq")
    f450 = filt[3]
    dev = FormsDev(gpu, queries, K)
    big = 2**32 + 1
    before = gpu.filter_stats()
    try:
        for forced, text, ask in (("walk", "ef/k exceed the 160 KiB LDS budget", {"ef": big}), ("walk", "ef/k exceed the 160 KiB LDS budget", {"skip": big}),
                                  ("exact", "k + skip exceed the 160 KiB LDS budget", {"skip": big})):
            gpu.set_filter_policy(forced)
            with pytest.raises(capi.LanternGpuError, match=re.escape(text)):
                dev.filtered(f450, **ask)
            with pytest.raises(capi.LanternGpuError, match=re.escape(text)):
                dev.each([f450] * 9, **ask)
        # a rider never looks at them, as ever
        same_bytes(dev.filtered(filt[0], ef=big, skip=big), dev.each_params([filt[0]] * 9, [(K, 64, 0)] * 9))
    finally:
        gpu.set_filter_policy("auto")
    assert gpu.filter_stats() == before


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_a_batch_of_riders_alone_by_form(capi, metric, mode):
    """3. Two queries, both behind the empty filter: the single-filter call and the parameter form answer without a launch, the uniform
    per-query form makes one exact launch that carries them."""
    gpu, queries, filt = index(capi, metric)
    empty = filt[0]
    dev = FormsDev(gpu, queries[:2], K)
    stats = lambda: (lambda s: (s["walk"], s["exact"]))(gpu.filter_stats())
    with mode_set(gpu, mode):
        before = stats()
        single = dev.filtered(empty, ef=EF, skip=SKIP)
        assert stats() == before
        shape = gpu.last_filtered_launch()
        assert shape["path"] is None and all(v == 0 for n, v in shape.items() if n != "path")
        each = dev.each([empty, empty], ef=EF, skip=SKIP)
        assert stats() == (before[0], before[1] + 1)
        regime = gpu.last_filtered_each()
        assert (regime["walk"], regime["exact"], regime["empty"], regime["launches"]) == (0, 0, 2, 1)
        before = stats()
        params = dev.each_params([empty, empty], [(K, EF, SKIP)] * 2)
        assert stats() == before
        regime = gpu.last_filtered_each()
        assert (regime["walk"], regime["exact"], regime["empty"], regime["launches"]) == (0, 0, 2, 0)
        same_bytes(single, each)
        same_bytes(single, params)
        assert not single[2].any() and np.isinf(single[1]).all() and not single[5].any()
        _, launch = plan_of(capi, gpu, [0, 0], 8 if mode == "seeded" else 0)
        assert launch["walk"]["queries"] == 0 and launch["exact"]["queries"] == 0
