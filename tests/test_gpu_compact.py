"""lantern_gpu_compact_deleted on the device (include/lantern_gpu.h "Deleting rows").  Nothing here is judged by recall: a
stable renumbering keeps the (distance, slot) order of the live slots, so the compacted index must be byte for byte the graph the numpy
restatement (tests/compact_ref.py) predicts and must answer every search with the labels, distance bits and counters the unlinked index
gave -- and the oracle gives on the compacted export."""
import numpy as np
import pytest

from tests import compact_ref
from tests import filtered_walk_ref as ref
from tests.filtered_regimes import stored_rows
from tests.test_gpu_delete import EF, EFC, build, graphs_equal, make_rows, random_share

pytestmark = pytest.mark.gpu
EMPTY = compact_ref.EMPTY


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0
    return capi


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def pq_kw(base):
    from tests.test_gpu_quantized_indexes import make_codebook

    return dict(pq_codebook=make_codebook(np.random.default_rng(0), base, 8, 32), num_subvectors=8)


def compact_and_check(capi, ix, fresh, capacity=0):
    """ix is unlinked.  Export, compact, export: every comparison of case 1.  Returns (graph after, rows after, slot_map, stats)."""
    before = ix.export_graph(with_vectors=True)
    screen = ix.export_screen()
    codes = ix.export_codes() if ix.pq_S else None
    mem_before = sum(ix.memory_usage())
    want, want_rows, want_map = compact_ref.compact(before, before["vectors"])
    plan_map, plan_off, live, blocks = capi.plan_compact(before["labels"], before["levels"])
    st, slot_map = ix.compact_deleted(capacity)
    after = ix.export_graph(with_vectors=True)
    print(f"n {before['labels'].size} -> {live}: {st}")
    graphs_equal(after, want)  # levels, nbr0, upper_off, upper_nbr, labels, entry_slot, max_level: edge for edge and in order
    assert same_bytes(after["vectors"], want_rows)
    assert np.array_equal(slot_map, plan_map) and np.array_equal(slot_map, want_map) and np.array_equal(after["upper_off"], plan_off)
    assert len(ix) == live and ix.deleted_count == 0
    assert (st["rows_before"], st["rows_after"]) == (before["labels"].size, live)
    assert (st["upper_blocks_before"], st["upper_blocks_after"]) == (before["upper_nbr"].shape[0], blocks)
    assert st["bytes_before"] == mem_before and st["bytes_after"] == sum(ix.memory_usage()) and st["bytes_after"] < st["bytes_before"]
    assert st["bytes_moved"] > 0 and all(v == 0 for v in st["unlink"].values())  # (the caller unlinked)
    keep = np.flatnonzero(before["labels"] != 0)
    if screen["row_bytes"]:  # the int8 screen and its metadata follow the map bit for bit
        now = ix.export_screen()
        assert now["row_bytes"] == screen["row_bytes"] and same_bytes(now["codes"], screen["codes"][keep]) and same_bytes(now["meta"], screen["meta"][keep])
        assert (screen["norms"] is None) == (now["norms"] is None) and (screen["norms"] is None or same_bytes(now["norms"], screen["norms"][keep]))
    if codes is not None:
        assert same_bytes(ix.export_codes(), codes[keep])
    total = ix.checksum()
    other = fresh()
    other.import_graph(want_rows, want)
    assert other.checksum() == total
    st2, map2 = ix.compact_deleted()  # a second call: zeros, the identity, nothing moves
    assert all(v == 0 for k, v in st2.items() if k != "unlink") and all(v == 0 for v in st2["unlink"].values())
    assert np.array_equal(map2, np.arange(live)) and ix.checksum() == total
    return after, want_rows, slot_map, st


def run_case(capi, metric, storage, d, M, n, dead, pq=False, also_without_unlink=False, base=None):
    base = make_rows(metric, d, n, d + M) if base is None else base
    kw = pq_kw(base) if pq else {}
    quant = "f32" if pq else storage
    dead = np.unique(np.asarray(dead, dtype=np.int64))
    ix = build(capi, metric, quant, base, M, **kw)
    assert ix.remove_labels(dead + 1) == dead.size
    ix.unlink_deleted()
    fresh = lambda: capi.GpuIndex(metric, d, M=M, ef_construction=EFC, ef=EF, seed=11, quantization=quant, **kw)
    out = compact_and_check(capi, ix, fresh)
    if also_without_unlink:  # the call unlinks by itself: the same graph, and the unlink's stats say it ran
        twin = build(capi, metric, quant, base, M, **kw)
        twin.remove_labels(dead + 1)
        st, _ = twin.compact_deleted()
        assert twin.checksum() == ix.checksum() and st["unlink"]["tombstones_unlinked"] > 0 and st["unlink"]["lists_repaired"] > 0
    return ix, base, out


# Chosen by row width and deletion pattern: 3 f32 (one 16-byte unit per row, many rows per wave), 16 (64 B), 100 (400 B: tiles end inside
# rows), 300 (1200 B), 512 (2 KiB, the narrowest row with the int8 screen: 128-byte screen rows), 768 (3 KiB rows, 192-byte screen rows),
# f16 and i8 rows, bit rows at the widened 128-byte stride, and 8-byte pq code rows (the byte form of the row kernel).
CASES = [
    ("l2sq", "f32", 3, 4, 700), ("cos", "f32", 16, 2, 1000), ("l2sq", "f32", 100, 4, 777), ("cos", "f32", 300, 16, 800),
    ("l2sq", "f32", 512, 16, 600), ("cos", "f32", 768, 4, 800), ("l2sq", "f16", 64, 4, 1000), ("cos", "i8", 100, 16, 1000),
    ("hamming", "f32", 24, 4, 1000),
    ("l2sq", "f32", 64, 33, 1500),  # lists of W = 66 (and 33 above) in k_compact_lists: a tile of 256 entries ends inside a list
]


@pytest.mark.parametrize("metric,storage,d,M,n", CASES)
def test_compacted_graph_is_the_restatement(capi, metric, storage, d, M, n):
    ix, _, (after, _, _, _) = run_case(capi, metric, storage, d, M, n, random_share(n, 0.3), also_without_unlink=(d == 16))
    if d >= 512:
        assert ix.export_screen()["row_bytes"] > 0  # the case is about the screen


def hubs_neighbours(capi, base, hub, M):
    """every row a hub's list names, the hubs themselves kept: their lists empty out and are refilled from the offers"""
    g = build(capi, "l2sq", "f32", base, M).export_graph()
    named = np.unique(np.concatenate([g["nbr0"][s][g["nbr0"][s] != EMPTY] for s in hub]))
    return np.setdiff1d(named, hub)


@pytest.mark.parametrize("pattern", ["30 % of the other rows", "the hubs' neighbours"])
def test_compacted_graph_with_lists_of_130(capi, pattern):
    """tests/test_gpu_long_lists.py's hubs at M = 65: W = 130 (and 65 above) in k_compact_lists -- a list spans two tiles of 256
    entries -- after the unlink of tests/test_gpu_delete.py's hubs case, and after one that takes every neighbour of every hub."""
    from tests.test_gpu_long_lists import hubs

    n, d, M = 1200, 128, 65
    base, hub = hubs(n, d, 8, d + M)
    rest = np.setdiff1d(np.arange(n), hub)
    dead = rest[random_share(rest.size, 0.3)] if pattern.startswith("30") else hubs_neighbours(capi, base, hub, M)
    assert dead.size > 0 and not np.intersect1d(dead, hub).size
    ix, _, (after, _, slot_map, _) = run_case(capi, "l2sq", "f32", d, M, n, dead, base=base)
    live = n - np.unique(dead).size
    assert (slot_map == EMPTY).sum() == np.unique(dead).size and len(ix) == live
    for key in ("nbr0", "upper_nbr"):  # no dangling entry: a list names live rows of the new numbering or is padding, padding last
        named = after[key] != EMPTY
        assert (after[key][named] < live).all() and not (named[:, 1:] & ~named[:, :-1]).any(), key
    assert (after["nbr0"][slot_map[hub]] != EMPTY).any(axis=1).all()  # the hubs are linked again


def test_compacted_pq_index_codes_follow_the_map(capi):
    ix, _, _ = run_case(capi, "l2sq", "f32", 64, 8, 600, random_share(600, 0.3), pq=True)
    assert ix.pq_S == 8


def entry_and_top(capi, metric, d, M, n):
    g = build(capi, metric, "f32", make_rows(metric, d, n, d + M), M).export_graph()
    top = np.flatnonzero(g["levels"] >= max(1, int(g["max_level"]) - 1))
    return np.union1d(top, [int(g["entry_slot"])])


@pytest.mark.parametrize("pattern", ["1 %", "90 %", "first and last", "run of 300", "entry and top levels"])
def test_deletion_patterns_on_the_16d_case(capi, pattern):
    metric, d, M, n = "cos", 16, 2, 1000
    dead = {"1 %": lambda: random_share(n, 0.01), "90 %": lambda: random_share(n, 0.9), "first and last": lambda: [0, n - 1],
            "run of 300": lambda: np.arange(350, 650), "entry and top levels": lambda: entry_and_top(capi, metric, d, M, n)}[pattern]()
    ix, _, (after, _, slot_map, _) = run_case(capi, metric, "f32", d, M, n, dead)
    assert (slot_map == EMPTY).sum() == np.unique(dead).size


# ---------------------------------------------------------------------------------------------------------------------------------
# searches are unchanged bit for bit; the index keeps growing as the oracle does
# ---------------------------------------------------------------------------------------------------------------------------------
def every_search(capi, ix, queries, k, allowed_slots, n_now):
    from lantern_amd import hip

    nq = queries.shape[0]
    out = {}
    dq = ix.device_query_rows(queries)
    bq = hip.Buffer.from_numpy(dq)
    lab, dist, D, E = hip.Buffer(nq * k * 8), hip.Buffer(nq * k * 4), hip.Buffer(nq * 8), hip.Buffer(nq * 8)
    ix.search_batch_device(bq.ptr, nq, k, 0, 0, lab.ptr, dist.ptr, None, None, D.ptr, E.ptr, query_stride=dq.strides[0])
    hip.synchronize()
    out["device"] = (lab.download((nq, k), np.uint64), dist.download((nq, k), np.float32), D.download(nq, np.uint64), E.download(nq, np.uint64))
    out["batch"] = ix.search_batch(queries, k)
    out["lone"] = [ix.search(q, k) for q in queries[:8]]
    # the exact search ranges over every stored row, tombstones included: the first k LIVE rows of a longer answer
    labels_now = ix.export_graph()["labels"]
    e_slots, e_dists = ix.exact_search(queries, 8 * k)
    live_hit = labels_now[e_slots.astype(np.int64)] != 0
    assert (live_hit.sum(1) >= k).all()
    first = np.argsort(~live_hit, axis=1, kind="stable")[:, :k]
    out["exact"] = (np.take_along_axis(e_slots, first, 1), np.take_along_axis(e_dists, first, 1))
    allowed = np.zeros(n_now, dtype=bool)
    allowed[allowed_slots] = True
    f = ix.filter_from_bitmap(allowed)
    for path in ("walk", "exact"):
        ix.set_filter_policy(path)
        out["filtered " + path] = ix.search_batch_filtered(f, queries, k)
    ix.set_filter_policy("auto")
    f.close()
    return out, allowed


def assert_same_answers(a, b, slot_map):
    for key in a:
        if key == "exact":  # slots, not labels: through the map
            assert np.array_equal(slot_map[a[key][0]], b[key][0]) and same_bytes(a[key][1], b[key][1]), key
        elif key == "lone":
            assert all(same_bytes(x[0], y[0]) and same_bytes(x[1], y[1]) for x, y in zip(a[key], b[key])), key
        else:
            assert all(same_bytes(x, y) for x, y in zip(a[key], b[key])), key


@pytest.mark.parametrize("metric,storage,d,M", [("l2sq", "f32", 768, 16), ("cos", "f16", 64, 4)])
def test_searches_unchanged_and_growth_as_the_oracle(capi, oracle, cores, metric, storage, d, M):
    n, nq, k = 1200, 100, 10
    base = make_rows(metric, d, n + 300, 51)
    queries = make_rows(metric, d, nq, 52)
    rows_all, q_s, ometric, mode = stored_rows(oracle, storage, metric, base, queries)
    ix = build(capi, metric, storage, base[:n], M)
    dead = np.sort(random_share(n, 0.3))
    ix.remove_labels(dead + 1)
    ix.unlink_deleted()
    live_old = np.flatnonzero(ix.export_graph()["labels"] != 0)
    before, _ = every_search(capi, ix, queries, k, live_old[::2], n)
    fresh = lambda: capi.GpuIndex(metric, d, M=M, ef_construction=EFC, ef=EF, seed=11, quantization=storage)
    after, _, slot_map, _ = compact_and_check(capi, ix, fresh)
    live = live_old.size
    got, allowed = every_search(capi, ix, queries, k, slot_map[live_old[::2]], live)  # the filter rebuilt through slot_map
    assert_same_answers(before, got, slot_map)
    # ... and the oracle on the compacted export, not only the code's own earlier answer
    rows_live = rows_all[:n][live_old]
    ora = oracle.OracleIndex.from_graph(metric, rows_live, after, M, EFC, EF, 11, mode, borrow=False)
    o_lab, o_dist, _, o_D, o_E = ora.search_batch(q_s, k, EF, 4)
    lab, dist, D, E = got["device"]
    assert np.array_equal(lab, o_lab) and same_bytes(dist, o_dist) and np.array_equal(D, o_D) and np.array_equal(E, o_E)
    assert np.array_equal(got["batch"][0], o_lab) and same_bytes(got["batch"][1], o_dist)
    assert all(np.array_equal(l, o_lab[i]) and same_bytes(dd, o_dist[i]) for i, (l, dd) in enumerate(got["lone"]))
    ids, dd = oracle.bruteforce(rows_live, q_s, k, ometric, mode, cores)
    assert np.array_equal(got["exact"][0], ids) and same_bytes(got["exact"][1], dd)
    dm = ref.distance_matrix(oracle, rows_live, q_s, ometric, mode, cores)
    for path in ("walk", "exact"):
        slots, dists, counts, _, _ = ref.search(after, dm, allowed, M, k, EF, path=path)
        f_lab, f_dist, f_cnt = got["filtered " + path]
        assert np.array_equal(f_cnt, counts) and (counts == k).all(), path
        assert np.array_equal(f_lab, after["labels"][slots.astype(np.int64)]) and same_bytes(f_dist, dists.astype(np.float32)), path
    # the index keeps growing as the oracle does: 300 more rows with the (256, 16) plan, edge for edge
    more = np.arange(n, n + 300, dtype=np.uint64) + 1
    ix.add_many(more, base[n:])
    ora.add_planned(more, rows_all[n:], 256, 16)
    grown = ix.export_graph()
    graphs_equal(grown, ora.export_graph())
    # delete 20 % again, compact again: case 1's comparison holds a second time
    again = random_share(len(ix), 0.2, seed=6)
    assert ix.remove_labels(grown["labels"][again]) == again.size
    ix.unlink_deleted()
    compact_and_check(capi, ix, fresh)


# ---------------------------------------------------------------------------------------------------------------------------------
# stale handles
# ---------------------------------------------------------------------------------------------------------------------------------
def test_stale_filters_and_cursors_are_refused(capi):
    n, d, M = 1000, 16, 8
    base = make_rows("l2sq", d, n + 5, 61)
    q = make_rows("l2sq", d, 8, 62)
    ix = build(capi, "l2sq", "f32", base[:n], M)
    f = ix.filter_from_bitmap(np.ones(n, dtype=bool))
    cur, fresh_cur = ix.cursor(), ix.cursor()
    page1, _ = cur.search(q[0], 5)
    own1, _ = ix.search(q[1], 5)  # the handle's own scan (usearch_search_ef): renumbered, it goes on
    ix.remove_labels(np.arange(5, dtype=np.uint64) + 1)
    st, slot_map = ix.compact_deleted()
    assert st["rows_after"] == n - 5
    with pytest.raises(capi.LanternGpuError, match="the index was compacted since the filter was built"):
        ix.search_batch_filtered(f, q, 5)
    ix.add_many(np.arange(n, n + 5, dtype=np.uint64) + 1, base[n:])  # the size is the filter's again: still another epoch
    assert len(ix) == n
    with pytest.raises(capi.LanternGpuError, match="the index was compacted since the filter was built"):
        ix.search_batch_filtered(f, q, 5)
    with pytest.raises(capi.LanternGpuError, match="the index was compacted: rescan"):
        cur.search(q[0], 5, streaming=True)
    with pytest.raises(capi.LanternGpuError, match="the index was compacted: rescan"):
        cur.search_filtered(ix.filter_from_bitmap(np.ones(n, dtype=bool)), q[0], 5, streaming=True)
    again, _ = cur.search(q[0], 5)  # a non-streaming search starts the scan over, and it serves again
    page2, _ = cur.search(q[0], 5, streaming=True)
    assert len(again) == 5 and len(page2) == 5 and not set(again) & set(page2)
    a, _ = fresh_cur.search(q[2], 5)  # a cursor that had handed out nothing adopts the new epoch
    b, _ = fresh_cur.search(q[2], 5, streaming=True)
    assert len(a) == 5 and len(b) == 5 and not set(a) & set(b)
    own2, _ = ix.search(q[1], 5, streaming=True)
    assert len(own2) == 5 and not set(own1) & set(own2)
    for c in (cur, fresh_cur):
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------------------
def test_nothing_deleted_is_a_no_op(capi):
    n, d = 300, 16
    ix = build(capi, "l2sq", "f32", make_rows("l2sq", d, n, 81), 8)
    total, cap, mem = ix.checksum(), ix.capacity, ix.memory_usage()
    f = ix.filter_from_bitmap(np.ones(n, dtype=bool))
    st, slot_map = ix.compact_deleted(capacity=5000)
    assert all(v == 0 for k, v in st.items() if k != "unlink") and all(v == 0 for v in st["unlink"].values())
    assert np.array_equal(slot_map, np.arange(n)) and (ix.checksum(), ix.capacity, ix.memory_usage()) == (total, cap, mem)
    assert ix.search_batch_filtered(f, make_rows("l2sq", d, 4, 82), 5)[2].tolist() == [5] * 4  # the epoch did not move
    empty = capi.GpuIndex("l2sq", d, M=8)
    st, slot_map = empty.compact_deleted()
    assert st["rows_before"] == 0 and slot_map.size == 0


def test_everything_deleted_leaves_an_empty_index_that_builds_as_a_fresh_one(capi, oracle):
    n, d, M = 300, 16, 8
    base = make_rows("l2sq", d, n + 200, 83)
    ix = build(capi, "l2sq", "f32", base[:n], M)
    assert ix.remove_labels(np.arange(n, dtype=np.uint64) + 1) == n
    st, slot_map = ix.compact_deleted()
    assert (st["rows_before"], st["rows_after"], st["upper_blocks_after"]) == (n, 0, 0) and (slot_map == EMPTY).all()
    assert len(ix) == 0 and ix.capacity == 0 and sum(ix.memory_usage()) == 0 and st["bytes_after"] == 0
    gi = ix.graph_info()
    assert (int(gi.size), int(gi.max_level)) == (0, -1) and int(gi.entry_slot) in (EMPTY, -1)
    lab, dist = ix.search(base[0], 5)
    assert len(lab) == 0
    labels = np.arange(200, dtype=np.uint64) + 1000
    ix.add_many(labels, base[n:])
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=EFC, ef=EF, seed=11, sum_mode=oracle.SUM_WAVE64)
    ora.add_planned(labels, base[n:], 256, 16)
    graphs_equal(ix.export_graph(), ora.export_graph())


def test_capacity_is_kept_for_the_rows_to_come(capi):
    n, d, M = 600, 100, 8
    base = make_rows("l2sq", d, n + 300, 84)
    ix = build(capi, "l2sq", "f32", base[:n], M)
    ix.remove_labels(random_share(n, 0.5) + 1)
    st, _ = ix.compact_deleted(capacity=700)
    assert st["rows_after"] == 300 and ix.capacity == 700
    mem = ix.memory_usage()
    assert sum(mem) == st["bytes_after"] and mem[0] == 700 * ix.row_bytes()
    ix.add_many(np.arange(n, n + 300, dtype=np.uint64) + 1, base[n:])
    assert len(ix) == 600 and ix.capacity == 700 and ix.memory_usage()[0] == mem[0]  # the rows were not reallocated
    save = ix.save_buffer()  # a file of the compacted, regrown index loads into the same graph
    again = capi.GpuIndex("l2sq", d, M=M, ef_construction=EFC, ef=EF, seed=11)
    again.load_buffer(save)
    assert again.checksum() == ix.checksum() and len(again) == 600


def test_refusals(capi):
    from tests.pg_pages import PageStore

    n, d, M = 300, 16, 8
    base = make_rows("l2sq", d, n, 71)
    pages = PageStore(capi, build(capi, "l2sq", "f32", base, M).save_buffer(), d * 4, M)
    mirror = capi.GpuIndex("l2sq", d, M=M, ef_construction=EFC, ef=EF, seed=11, retriever=pages.retriever)
    mirror.view_mem_lazy(pages.header)
    assert mirror.remove_labels([1, 2, 3]) == 3
    with pytest.raises(capi.LanternGpuError, match="compaction does not run on a page-attached index"):
        mirror.compact_deleted()
    rows = make_rows("l2sq", 64, 600, 4)
    pq = build(capi, "l2sq", "f32", rows, 8, **pq_kw(rows))
    pq.pq_compact()
    dead = random_share(600, 0.25)
    pq.remove_labels(dead + 1)
    with pytest.raises(capi.LanternGpuError, match=r"compaction does not run on a compact pq index: expand it first \(lantern_gpu_pq_expand\)"):
        pq.compact_deleted()
    pq.pq_expand()
    st, slot_map = pq.compact_deleted()
    assert st["rows_after"] == 600 - dead.size == len(pq) and st["unlink"]["tombstones_unlinked"] == dead.size
    lab, _, cnt = pq.search_batch(rows[:16], 5)
    assert (cnt == 5).all() and not (lab == 0).any()
