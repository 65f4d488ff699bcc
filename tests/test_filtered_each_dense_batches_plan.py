"""The batches of a per-query-filter call's dense run, without a device (include/lantern_gpu.h "THAT RUN, BATCHED"):
lantern_gpu_plan_filtered_each_dense_batches is the plan the call itself runs.  Checked against a numpy restatement of "greedy, in plan
order, never across a chunk of 65 536 positions, every step alone fits"."""
import numpy as np
import pytest

L2SQ, COS, HAMMING = 3, 1, 8  # usearch_metric_kind_t (+ 100: f16 storage)
CHUNK, QTILE = 65536, 1024


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def groups_of(sizes):
    """(queries, rows) per group -> the plan's per-query inputs"""
    ids = np.concatenate([np.full(q, g) for g, (q, _) in enumerate(sizes)])
    counts = np.concatenate([np.full(q, r) for q, r in sizes])
    return ids, counts, np.ones(ids.size, np.uint8)


def restate(steps, capacity):
    batches, offs = [], []
    for i, (_, nqt, col0, cols) in enumerate(steps):
        floats = nqt * cols
        assert floats <= capacity
        if batches and batches[-1][2] + floats <= capacity and steps[batches[-1][0]][2] // CHUNK == col0 // CHUNK:
            first, count, packed, tiles = batches[-1]
        else:
            first, count, packed, tiles = i, 0, 0, 0
            batches.append(None)
        offs.append(packed)
        skinny = -(-cols // 256) if nqt <= 32 else 0
        big = 0 if nqt <= 32 else -(-nqt // 128) * -(-cols // 128)
        batches[-1] = (first, count + 1, packed + floats, tiles + skinny + big)
        offs[-1] = (offs[-1], skinny, big)
    return batches, offs


@pytest.mark.parametrize("sizes,capacity,n_batches", [
    ([(2, 50)] * 600, 0, 1),                                  # many tiny groups: one batch
    ([(10, 900)] * 3, 20000, 2),                              # three blocks of 0.45 of the capacity each: 2 + 1
    ([(2048, 40000)], 0, 2),                                  # two query tiles of one group, each the capacity: two batches in one chunk
    ([(40, 70000)], 0, 2),                                    # a segment across the chunk boundary: a batch per chunk
    ([(2, 50), (3, 70000), (2, 9)], 0, 2),                    # ... with neighbours on either side of it
    ([(129, 700), (33, 300), (129, 700), (40, 300)], 129 * 700, 4),  # a capacity passed in: every step is its own batch
    ([(1, 1), (32, 256), (33, 257), (128, 128), (129, 129)], 0, 1),  # tile counts at the shapes' edges
])
def test_batches(capi, sizes, capacity, n_batches):
    ids, counts, exact = groups_of(sizes)
    plan = capi.plan_filtered_each_dense(L2SQ, 4, 10, 0, 1, ids, counts, exact)
    got = capi.plan_filtered_each_dense_batches(L2SQ, 4, 10, 0, 1, ids, counts, exact, capacity=capacity)
    own = min(len(ids), QTILE) * min(int(plan["rows"]), CHUNK)
    assert got["why"] == "taken" and got["capacity"] == (capacity or own)
    batches, offs = restate(plan["steps"], got["capacity"])
    assert got["batches"] == batches and got["steps"] == offs and len(batches) == n_batches
    assert (got["skinny"], got["big"]) == (sum(s for _, s, _ in offs), sum(b for _, _, b in offs))


def test_tile_counts_and_refusals(capi):
    ids, counts, exact = groups_of([(1, 1), (32, 256), (33, 257), (128, 128), (129, 129)])
    got = capi.plan_filtered_each_dense_batches(COS, 4, 10, 0, 1, ids, counts, exact)
    assert [s[1:] for s in got["steps"]] == [(1, 0), (1, 0), (0, 3), (0, 1), (0, 4)]
    # not served: never an error, the reason says why
    why = lambda *a, **kw: capi.plan_filtered_each_dense_batches(*a, ids, counts, exact, **kw)["why"]
    assert why(L2SQ + 100, 4, 10, 0, 1) == "operands" and why(L2SQ + 100, 4, 10, 0, 1, native=0) == "operands" and why(HAMMING, 4, 10, 0, 1) == "operands"
    assert why(L2SQ, 4, 10, 0, 0) == "no_run" and why(L2SQ, 4, 10, 231, 1) == "no_run" and why(L2SQ, 65537, 10, 0, 1) == "wide_row"
    # a capacity that one step alone exceeds is refused
    with pytest.raises(capi.LanternGpuError, match="does not fit"):
        capi.plan_filtered_each_dense_batches(L2SQ, 4, 10, 0, 1, ids, counts, exact, capacity=129 * 129 - 1)
