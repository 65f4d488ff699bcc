"""The batched dense run of the per-query-filter calls on the device (lantern_gpu_set_filter_dense_each_batched; include/lantern_gpu.h
"THAT RUN, BATCHED", DESIGN.md 4.9 "Dense exact path, per-query filters: batched").  Needs an MI355X.

Every case runs one per-query-filter call three ways -- batched on, batched off, the dense route off -- and requires all six outputs
equal for every query (the answers are re-ranked in exact order behind a certificate: not a bit may differ), then checks batched on
against float64: l2sq on an integer lattice (every f32 distance exact: the top k + skip by (distance, slot) must be the slots, ties
included), cos within the numerics contract's 1e-5 * max(1, |ref|), slot sets equal except at a float64 near-tie of the cut (at most 1
query in 50, asserted).  Group g's filter allows the rows of its own range; the groups differ in size, so segments start unaligned.
The two cases of 1024-query tiles take every 16th query to float64 (all of them to the other two runs).
"""
import numpy as np
import pytest

from tests.test_gpu_filtered_dense import index_of, poison
from tests.test_gpu_filtered_search import Dev, same

pytestmark = pytest.mark.gpu

F32, EMPTY = np.float32, 0xFFFFFFFF
EDGES = [(1, 1), (31, 255), (32, 256), (33, 257), (129, 700)]  # (queries, rows) per group: both tile shapes and their edges


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def inputs(metric, sizes, d, seed, zeros=False):
    """rows and queries of the groups `sizes`; l2sq: rows from n / 2 lattice points in [-8, 8]^d, so that ties occur -- and no more
    of them than that: a query whose k-th and (k + skip + 16)-th distances tie is refused by the certificate and answered elsewhere"""
    rng = np.random.default_rng([seed, d, len(sizes)])
    n, nq = sum(r for _, r in sizes), sum(q for q, _ in sizes)
    if metric == "l2sq":
        pool = rng.integers(-8, 9, size=(max(2, n // 2), d)).astype(F32)
        rows, queries = pool[rng.integers(0, len(pool), n)], pool[rng.integers(0, len(pool), nq)] + rng.integers(-1, 2, size=(nq, d)).astype(F32)
        queries = np.clip(queries, -8, 8)
    else:
        rows, queries = rng.standard_normal((n, d), dtype=F32), rng.standard_normal((nq, d), dtype=F32)
        if zeros:  # the zero-norm rules: a zero row in the last group, whose first query is zero too
            rows[n - 3] = 0
            queries[nq - sizes[-1][0]] = 0
    return rows, queries


def reference(metric, rows, queries):
    """float64 distances of every query to every row"""
    r, q = rows.astype(np.float64), queries.astype(np.float64)
    if metric == "l2sq":
        return (q * q).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2.0 * (q @ r.T)
    nr, nq = np.sqrt((r * r).sum(1)), np.sqrt((q * q).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 - (q @ r.T) / (nq[:, None] * nr[None, :])
    d[(nq == 0)[:, None] | (nr == 0)[None, :]] = 1.0
    d[(nq == 0)[:, None] & (nr == 0)[None, :]] = 0.0
    return d


def near_ties(metric, sizes, rows, queries, kk, every=1):
    """per checked query: (query, first row of its group, its float64 distances to its group's rows, near-tie at the cut)"""
    out, q0, r0 = [], 0, 0
    for nq_g, n_g in sizes:
        dist = reference(metric, rows[r0:r0 + n_g], queries[q0:q0 + nq_g:every])
        for i, d in enumerate(dist):
            s = np.sort(d)
            tie = metric == "cos" and n_g > kk and s[kk] - s[kk - 1] <= 1e-5 * max(1.0, abs(s[kk - 1]))
            out.append((q0 + i * every, r0, d, tie))
        q0, r0 = q0 + nq_g, r0 + n_g
    return out


def run_case(capi, oracle, metric, sizes, d, k, skip, seed=1, zeros=False, every=1, storage="f32"):
    rows, queries = inputs(metric, sizes, d, seed, zeros)
    ix = index_of(capi, oracle, metric, storage, rows)
    filters, r0 = [], 0
    for nq_g, n_g in sizes:
        allowed = np.zeros(rows.shape[0], dtype=bool)
        allowed[r0:r0 + n_g] = True
        filters += [ix.filter_from_bitmap(allowed)] * nq_g
        r0 += n_g
    dev, got, launches = Dev(ix, queries, k), {}, {}
    for mode, (m, on) in dict(setting0=(0, 0), off=(1, 0), on=(1, 1)).items():
        ix.set_filter_dense_each(m)
        ix.set_filter_dense_each_batched(on)
        assert ix.filter_dense_each_batched() == on
        poison(dev)
        dev.gpu.search_batch_filtered_each_device(filters, dev.dq.ptr, dev.rows.strides[0], dev.nq, k, 0, skip, dev.lab.ptr, dev.dist.ptr, dev.slot.ptr,
                                                  dev.cnt.ptr, dev.D.ptr, dev.E.ptr)
        got[mode], launches[mode] = dev._out(), (ix.last_filtered_each_dense(), ix.last_filtered_each_dense_launches())
    for other in ("off", "setting0"):
        same(got["on"], got[other])
        assert np.array_equal(got["on"][5], got[other][5]), "labels differ"
    slots, dists, counts = got["on"][:3]
    kk, ties = k + skip, 0
    for q, r0, ref, tie in near_ties(metric, sizes, rows, queries, kk, every):
        order = np.lexsort((np.arange(ref.size), ref))[:kk][skip:]  # by (distance, slot)
        assert counts[q] == order.size and np.all(slots[q, order.size:] == EMPTY)
        mine = slots[q, :order.size].astype(np.int64) - r0
        if metric == "l2sq":
            assert np.array_equal(mine, order) and np.array_equal(dists[q, :order.size].astype(np.float64), ref[order]), q
        else:
            want = ref[order]
            assert np.all(np.abs(dists[q, :order.size] - want) <= 1e-5 * np.maximum(1.0, np.abs(want))), q
            ties += bool(tie)
            assert tie or set(mine) == set(order), q
    assert ties * 50 <= len(queries)
    dense = launches["on"][0]
    assert dense["queries"] == len(queries) and dense["certified"] * 2 >= dense["queries"], dense  # (what was compared is this run's, not the exact launch's)
    ix.close()
    return launches


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
@pytest.mark.parametrize("d", [4, 32, 36, 100])  # rows of 1, 8, 9 and 25 chunks: less than a K step, exactly one, one plus a tail, several plus a tail
def test_tile_edges_and_row_widths(capi, oracle, metric, d):
    launches = run_case(capi, oracle, metric, EDGES, d, 10, 0)
    dense, (con, sel, batches, skinny) = launches["on"][0], launches["on"][1].values()
    assert dense["steps"] == 5 and (con, sel, batches) == (1, 1, 1) and skinny == 1 + 1 + 1  # (33 and 129 queries: 128 x 128 tiles)
    assert tuple(launches["off"][1].values()) == (5, 5, 0, 0) and tuple(launches["setting0"][1].values()) == (0, 0, 0, 0)


@pytest.mark.parametrize("metric,k,skip,zeros", [("l2sq", 1, 0, False), ("l2sq", 10, 230, False), ("cos", 10, 230, False), ("cos", 5, 2, True)])
def test_width_and_zero_norms(capi, oracle, metric, k, skip, zeros):
    run_case(capi, oracle, metric, EDGES, 36, k, skip, seed=2, zeros=zeros)


def test_more_tiles_than_workgroups(capi, oracle):
    """600 groups of 2 queries over 47 .. 53 rows: one launch of each kind where the per-step run makes 600"""
    sizes = [(2, 47 + g % 7) for g in range(600)]
    launches = run_case(capi, oracle, "l2sq", sizes, 8, 10, 0, seed=3)
    assert launches["on"][0]["steps"] == 600 and tuple(launches["on"][1].values()) == (1, 1, 1, 600)
    assert launches["off"][0]["steps"] == 600 and tuple(launches["off"][1].values()) == (600, 600, 0, 0)


@pytest.mark.parametrize("sizes,batches,every", [
    ([(40, 70000)], 2, 1),        # a segment across the chunk boundary
    ([(1024, 30000)] * 3, 2, 16),  # 1024-query steps; their blocks fill the first chunk's batch to the last float
    ([(2048, 40000)], 2, 16),     # two batches in one chunk
])
def test_chunks_and_batches(capi, oracle, sizes, batches, every):
    launches = run_case(capi, oracle, "l2sq", sizes, 4, 10, 0, seed=4, every=every)
    assert tuple(launches["on"][1].values())[:3] == (batches, batches, batches)


def test_f16_rows_take_the_per_step_run(capi, oracle):
    sizes = [(3, 100), (40, 300)]
    ids, counts = np.repeat([0, 1], [3, 40]), np.repeat([100, 300], [3, 40])
    assert capi.plan_filtered_each_dense_batches(3 + 100, 5, 10, 0, 1, ids, counts, np.ones(43, np.uint8))["why"] == "operands"
    launches = run_case(capi, oracle, "l2sq", sizes, 36, 10, 0, seed=5, storage="f16")
    assert tuple(launches["on"][1].values()) == (2, 2, 0, 0) == tuple(launches["off"][1].values())
