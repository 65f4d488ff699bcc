"""A filter's life cycle on the device (lantern_gpu.h "A FILTER'S LIFE CYCLE"; filter_ops.hip): the slot list built by the device list
pass, two filters combined, a filter extended to the grown index -- and the extension through the scan-side service ("LSRX").  Needs an
MI355X.  Every comparison is exact: bitmaps and lists word for word against numpy (tests/filter_ops_ref.py), answers bit for bit
against a filter built fresh by filter_from_labels / filter_from_bitmap on the index as it stands."""
import time

import numpy as np
import pytest

from tests import filter_ops_ref as ref
from tests.test_gpu_filtered_search import CASES, Dev, oracle_index, same

pytestmark = pytest.mark.gpu

# one workgroup of the list kernels covers 256 words = 8192 slots (filter_ops.hpp kFilterListSpan); the scan over the workgroups'
# counts is rocPRIM's.  24581: four workgroups, the last one partly filled, an odd last word
SIZES = [1, 31, 32, 33, 127, 128, 129, 8191, 8192, 8193, 24581]
COMBINE_SIZES = [33, 129, 8193, 24581]
GROWTH = [(100, 101), (100, 129), (100, 400), (128, 133), (8190, 8195)]
ANSWER_CASES = [c for c in CASES if c[:3] in (("l2sq", 3000, 128), ("hamming", 3000, 24))]
MODES = [("walk", 0), ("exact", 0), ("walk", 64)]  # (policy, seeds)


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def small_index(capi, n, d=8, seed=1):
    """n rows of d-dimensional f32 built on the device; slot s carries label s + 1"""
    ix = capi.GpuIndex("l2sq", d, M=4, ef_construction=8, ef=8, seed=3)
    grow(ix, 0, n, d, seed)
    return ix


def grow(ix, n_old, n_new, d=8, seed=1):
    rng = np.random.default_rng(seed * 100003 + n_old)
    ix.add_many(np.arange(n_old, n_new, dtype=np.uint64) + 1, rng.standard_normal((n_new - n_old, d), dtype=np.float32))
    ix.flush()


@pytest.fixture(scope="module")
def indexes(capi):
    """the bitmap / list tests' indexes by size, built once"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = small_index(capi, n)
        return cache[n]

    return get


def labels_of(allowed):
    return ref.slots(allowed).astype(np.uint64) + 1


def check(f, allowed):
    """the filter's bitmap (every device word), list and count against the allow-set"""
    words, slots = f.export()
    assert f.rows == allowed.size and words.size == ref.words_for(allowed.size)
    assert np.array_equal(words, ref.pack(allowed)), "bitmap differs"  # (pack: zero past ceil(n / 32) up to the multiple of 4)
    assert np.array_equal(slots, ref.slots(allowed)), "slot list differs"
    assert f.count == slots.size == int(allowed.sum())
    assert f.resident_bytes == 4 * words.size + 4 * slots.size


def equal_filters(a, b):
    (wa, sa), (wb, sb) = a.export(), b.export()
    assert np.array_equal(wa, wb) and np.array_equal(sa, sb) and a.count == b.count and a.resident_bytes == b.resident_bytes


def answers(gpu, dev, f):
    out = []
    for policy, seeds in MODES:
        gpu.set_filter_policy(policy)
        gpu.set_filter_seeds(seeds)
        out.append(dev.filtered(f))
    gpu.set_filter_seeds(0)
    gpu.set_filter_policy("auto")
    return out


# ------------------------------------------------------------------------------------------------
# the list
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_list_of_both_constructors_equals_flatnonzero(capi, indexes, n):
    ix = indexes(n)
    for name in ref.PATTERNS:
        allowed = ref.pattern(name, n)
        check(ix.filter_from_bitmap(allowed), allowed)
        check(ix.filter_from_labels(labels_of(allowed)), allowed)


# ------------------------------------------------------------------------------------------------
# combine
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COMBINE_SIZES)
def test_combine_equals_numpy(capi, indexes, n):
    ix = indexes(n)
    sets = {name: ref.pattern(name, n, seed=1) for name in ref.PATTERNS}
    filters = {name: ix.filter_from_bitmap(a) if i % 2 else ix.filter_from_labels(labels_of(a)) for i, (name, a) in enumerate(sets.items())}
    for x in ref.PATTERNS:
        for y in ref.PATTERNS:
            for op in ref.OPS:
                check(filters[x].combine(filters[y], op), ref.combine(sets[x], sets[y], op))
    a, b = filters["half"], filters["third"]
    check(a & b, sets["half"] & sets["third"])
    check(a | b, sets["half"] | sets["third"])
    check(a - b, sets["half"] & ~sets["third"])
    same_again = a & a
    equal_filters(same_again, a)
    assert same_again.h != a.h
    equal_filters(a | filters["everything"], filters["everything"])
    check(a - a, np.zeros(n, dtype=bool))


def test_empty_combination_answers_without_a_launch(capi, indexes):
    ix = indexes(8193)
    a = ix.filter_from_bitmap(ref.pattern("half", 8193))
    none = a - a
    assert none.count == 0
    before = ix.filter_stats()
    q = np.random.default_rng(2).standard_normal((5, 8), dtype=np.float32)
    lab, dist, cnt = ix.search_batch_filtered(none, q, 3)
    assert not cnt.any() and not lab.any() and np.all(np.isinf(dist))
    assert ix.filter_stats() == before and not any(ix.last_filtered_launch().values())


@pytest.mark.parametrize("metric,n,d,M,efc,ef,k", ANSWER_CASES)
def test_combined_filter_answers_as_the_bitmap_of_the_numpy_result(capi, oracle, metric, n, d, M, efc, ef, k):
    base, queries, g, gpu = oracle_index(capi, oracle, metric, n, d, M, efc, ef, 9)
    sa, sb = ref.pattern("half", n, seed=2), ref.pattern("third", n)
    fa, fb = gpu.filter_from_labels(labels_of(sa)), gpu.filter_from_bitmap(sb)
    dev = Dev(gpu, queries, k)
    for op in ref.OPS:
        want = ref.combine(sa, sb, op)
        combined, fresh = fa.combine(fb, op), gpu.filter_from_bitmap(want)
        check(combined, want)
        for got, exp in zip(answers(gpu, dev, combined), answers(gpu, dev, fresh)):
            same(got, exp)
            assert got[2].any()


def test_combine_refuses_foreign_and_stale_operands(capi):
    n = 129
    ix, other = small_index(capi, n), small_index(capi, n)
    a, b, alien = ix.filter_from_bitmap(ref.pattern("half", n)), ix.filter_from_bitmap(ref.pattern("third", n)), other.filter_from_bitmap(ref.pattern("third", n))
    for x, y in ((a, alien), (alien, a)):
        with pytest.raises(capi.LanternGpuError, match="another index"):
            capi._call("lantern_gpu_filter_combine", ix.h, x.h, y.h, 0)
    grow(ix, n, n + 1)
    fresh = ix.filter_from_bitmap(ref.pattern("third", n + 1))
    for x, y in ((a, fresh), (fresh, b)):
        with pytest.raises(capi.LanternGpuError, match="stale filter: built when the index held 129 rows, it now holds 130"):
            x & y
    check(fresh | fresh, ref.pattern("third", n + 1))


# ------------------------------------------------------------------------------------------------
# extend
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", GROWTH)
def test_extend_equals_a_fresh_filter_of_the_union(capi, n1, n2):
    rng = np.random.default_rng(n1 * 7 + n2)
    ix = small_index(capi, n1)
    old_set = rng.random(n1) < 0.5
    old_set[n1 - 1] = True  # (the last old slot: the bit just below the seam)
    L1 = rng.permutation(labels_of(old_set))
    f = ix.filter_from_labels(L1)
    check(f, old_set)
    current = f.extend(L1)  # a current filter: an equal copy under another handle
    equal_filters(current, f)
    assert current.h != f.h
    grow(ix, n1, n2)
    q = rng.standard_normal((2, 8), dtype=np.float32)
    with pytest.raises(capi.LanternGpuError, match=f"stale filter: built when the index held {n1} rows, it now holds {n2}"):
        ix.search_batch_filtered(f, q, 3)
    new_set = rng.random(n2 - n1) < 0.5
    new_set[0] = True  # (the first new slot: the bit just above the seam)
    L2 = rng.permutation(np.flatnonzero(new_set).astype(np.uint64) + n1 + 1)
    slot_labels = np.arange(n2, dtype=np.uint64) + 1
    ext, fresh = f.extend(L2), ix.filter_from_labels(np.concatenate([L1, L2]))
    check(ext, ref.extend(old_set, slot_labels, L2))
    equal_filters(ext, fresh)
    with pytest.raises(capi.LanternGpuError, match="stale filter"):  # nothing was extended behind the caller's back
        ix.search_batch_filtered(f, q, 3)
    lab = ix.search_batch_filtered(ext, q, 3)[0]
    assert np.array_equal(lab, ix.search_batch_filtered(fresh, q, 3)[0])
    # every new slot; no new slot (the count stays, and searches take the filter now)
    check(f.extend(all_new=True), ref.extend(old_set, slot_labels, all_new=True))
    kept = f.extend([])
    check(kept, ref.extend(old_set, slot_labels))
    assert kept.count == f.count
    assert np.all(np.isin(ix.search_batch_filtered(kept, q, 3)[0], np.concatenate([L1, np.zeros(1, dtype=np.uint64)])))
    # the old handle is still a filter: it reads, and it frees
    check(f, old_set)
    f.close()


def test_extend_skips_deleted_new_rows_and_keeps_the_snapshot_of_old_ones(capi):
    n1, n2 = 100, 140
    ix = small_index(capi, n1)
    old_set = ref.pattern("third", n1)
    f = ix.filter_from_labels(labels_of(old_set))
    grow(ix, n1, n2)
    assert ix.remove_labels([4, 121]) == 2  # slot 3: an old row the filter allows; slot 120: a new row
    slot_labels = np.arange(n2, dtype=np.uint64) + 1
    slot_labels[[3, 120]] = 0
    assert old_set[3]
    L2 = np.array([0, 111, 121, 131], dtype=np.uint64)  # label 0 among them: what the deleted row carries now
    check(f.extend(L2, skip_deleted=True), ref.extend(old_set, slot_labels, L2, skip_deleted=True))
    got = f.extend(L2, skip_deleted=True).export()[1].tolist()
    assert 3 in got and 110 in got and 130 in got and 120 not in got
    check(f.extend(L2), ref.extend(old_set, slot_labels, L2))  # without the flag label 0 is a label like any other
    assert 120 in f.extend(L2).export()[1].tolist()
    check(f.extend(all_new=True, skip_deleted=True), ref.extend(old_set, slot_labels, all_new=True, skip_deleted=True))


def test_extend_is_refused_across_a_compaction_and_for_another_index(capi):
    n = 200
    ix, other = small_index(capi, n), small_index(capi, n)
    allowed = ref.pattern("half", n)
    f = ix.filter_from_bitmap(allowed)
    with pytest.raises(capi.LanternGpuError, match="another index"):
        capi.Filter(other, capi._call("lantern_gpu_filter_extend", other.h, f.h, None, 0, 0))
    assert ix.remove_labels([7, 8, 9]) == 3
    ix.compact_deleted()
    grow(ix, n, n + 10)
    for kw in ({"labels": [201]}, {"all_new": True}):
        with pytest.raises(capi.LanternGpuError, match="stale filter: the index was compacted since the filter was built"):
            f.extend(**kw)
    check(f, allowed)  # the old handle still reads
    f.close()


def test_extended_filter_answers_as_a_fresh_one(capi):
    n1, n2, d, k = 3000, 3300, 128, 10
    rng = np.random.default_rng(11)
    gpu = capi.GpuIndex("l2sq", d, M=16, ef_construction=64, ef=64, seed=9)
    grow(gpu, 0, n1, d)
    L1 = labels_of(rng.random(n1) < 0.3)
    f = gpu.filter_from_labels(L1)
    grow(gpu, n1, n2, d)
    L2 = np.flatnonzero(rng.random(n2 - n1) < 0.3).astype(np.uint64) + n1 + 1
    ext, fresh = f.extend(L2), gpu.filter_from_labels(np.concatenate([L1, L2]))
    equal_filters(ext, fresh)
    dev = Dev(gpu, rng.standard_normal((64, d), dtype=np.float32), k)
    through_ext = answers(gpu, dev, ext)
    for got, exp in zip(through_ext, answers(gpu, dev, fresh)):
        same(got, exp)
        assert np.all(got[2] == k)
    slots, labels = through_ext[1][0], through_ext[1][5]  # (the exact path's)
    assert np.isin(labels, np.concatenate([L1, L2])).all() and (slots >= n1).any()  # allowed rows only, new ones among them


# ------------------------------------------------------------------------------------------------
# the service
# ------------------------------------------------------------------------------------------------
def test_the_service_extends_a_connections_filter_and_keeps_its_scan(capi):
    n, more, d, k = 3000, 50, 64, 10
    rng = np.random.default_rng(7)
    ix = capi.GpuIndex("l2sq", d, M=16, ef_construction=64, ef=64, seed=3)
    grow(ix, 0, n, d)
    q = rng.standard_normal(d, dtype=np.float32)
    srv = capi.ScanServer(index=ix, max_wait_us=200)
    c = capi.ScanClient(srv.host, srv.port)
    with pytest.raises(capi.LanternGpuError, match="no filter to extend"):
        c.extend_filter(all_new=True)
    evens = np.arange(2, n + 1, 2, dtype=np.uint64)
    assert c.set_filter(evens) == evens.size
    first = c.search(q, k)
    assert first[0].size == k and np.all(first[0] % 2 == 0)
    grow(ix, n, n + more, d)
    with pytest.raises(capi.LanternGpuError, match=f"stale filter: built when the index held {n} rows, it now holds {n + more}"):
        c.search_next(q, k)
    new_evens = np.arange(n + 2, n + more + 1, 2, dtype=np.uint64)
    with pytest.raises(capi.LanternGpuError, match="bad extension flags|unknown filter flags"):
        capi._call("lantern_scan_client_extend_filter", c.c, None, 0, 4)
    assert c.extend_filter(new_evens) == evens.size + new_evens.size
    fresh = ix.filter_from_labels(np.concatenate([evens, new_evens]))
    # the scan goes on where it stood: the hand-out history survived the extension (and the error frame), so the continuation is the
    # first k rows of the new filter's answer that the scan has not been handed yet
    top = ix.search_batch_filtered(fresh, q[None, :], 2 * k)
    keep = ~np.isin(top[0][0], first[0])
    nxt = c.search_next(q, k)
    assert np.array_equal(nxt[0], top[0][0][keep][:k]) and np.array_equal(nxt[1].view(np.uint32), top[1][0][keep][:k].view(np.uint32))
    assert not set(nxt[0].tolist()) & set(first[0].tolist())
    # the next searches and a continuation: page for page the direct cursor's through a freshly built filter, bit for bit
    cur = ix.cursor()
    want = [cur.search_filtered(fresh, q, k, streaming=p > 0) for p in range(3)]
    pages = [c.search(q, k)] + [c.search_next(q, k) for _ in range(2)]
    for have, exp in zip(pages, want):
        assert np.array_equal(have[0], exp[0]) and np.array_equal(have[1].view(np.uint32), exp[1].view(np.uint32))
    cur.close()
    t0 = time.perf_counter()
    while srv.filter_stats()["resident_bytes"] != fresh.resident_bytes and time.perf_counter() - t0 < 5:
        time.sleep(0.01)
    assert srv.filter_stats()["resident_bytes"] == fresh.resident_bytes  # the old filter is released: the one new filter's bytes
    c.close()
    srv.stop()
