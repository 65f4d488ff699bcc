"""Deleting rows on the device (include/lantern_gpu.h "Deleting rows"): lantern_gpu_remove_labels against numpy, and
lantern_gpu_unlink_deleted against its CPU restatement (tests/unlink_ref.py) on the exported graph -- lists edge for edge and in order
at every level, the entry, max_level and every stat the restatement defines.  PARITY UNPINNED BY THE REFERENCE beyond the label reset
(delete.c:52-61) and the golden case (hnsw_delete.out:28-55)."""
import json
import os

import numpy as np
import pytest

from tests import unlink_ref
from tests.filtered_regimes import stored_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EFC, EF = 64, 40


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0
    return capi


def make_rows(metric, d, n, seed, identical=0):
    rng = np.random.default_rng(seed)
    if metric == "hamming":
        base = rng.integers(0, 2**32, (n, d), dtype=np.uint64).astype(np.uint32)
    else:
        base = (np.float32(0.4) * rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32)
    if identical:
        base[100:100 + identical] = base[100]
    return base


def build(capi, metric, storage, base, M, **kw):
    n, d = base.shape
    ix = capi.GpuIndex(metric, d, M=M, ef_construction=EFC, ef=EF, seed=11, quantization=storage, **kw)
    ix.set_add_batch(256, 16)
    ix.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    return ix


def graphs_equal(a, b):
    for key in ("levels", "nbr0", "upper_off", "upper_nbr", "labels"):
        assert np.array_equal(a[key], b[key]), key
    assert (a["entry_slot"], a["max_level"]) == (b["entry_slot"], b["max_level"])


def remove_and_unlink(capi, oracle, metric, storage, base, M, dead_slots, **kw):
    """Build (kw: a pq codebook), remove, unlink; every comparison with the restatement and every invariant.  Returns what the
    follow-up tests use; "want_stats" are the restatement's own (reprunes, max_kept: what the device does not count)."""
    n = base.shape[0]
    ix = build(capi, metric, storage, base, M, **kw)
    dead_slots = np.unique(np.asarray(dead_slots, dtype=np.int64))
    assert ix.remove_labels(dead_slots + 1) == dead_slots.size and ix.deleted_count == dead_slots.size
    before = ix.export_graph(with_vectors=bool(ix.pq_S))
    assert np.array_equal(np.flatnonzero(before["labels"] == 0), dead_slots)
    if ix.pq_S:  # an expanded pq index is the f32 index of its decoded rows (tests/test_gpu_quantized_indexes.py)
        rows_s, ometric, mode = before.pop("vectors"), metric, oracle.SUM_WAVE64
    else:
        rows_s, _, ometric, mode = (base, None, "hamming", oracle.SUM_SEQ) if metric == "hamming" else stored_rows(oracle, storage, metric, base, base[:1])
    dist = unlink_ref.pair_matrix(oracle, rows_s, ometric, mode, 8)
    want, wst = unlink_ref.unlink(before, dist, M)
    st = ix.unlink_deleted()
    after = ix.export_graph()
    print(f"{metric} {storage} {base.shape} M={M} dead={dead_slots.size}: {st}; the restatement: reprunes {wst['reprunes']} max_kept {wst['max_kept']}")
    graphs_equal(after, want)
    assert {k: st[k] for k in unlink_ref.STATS} == {k: wst[k] for k in unlink_ref.STATS}
    assert (st["reprune_evals"] > 0) == (wst["reprunes"] > 0)
    unlink_ref.check_invariants(before, after, M)
    sum_before = ix.checksum()
    assert all(v == 0 for v in ix.unlink_deleted().values()) and ix.checksum() == sum_before  # a second call changes nothing
    return dict(ix=ix, after=after, rows=rows_s, ometric=ometric, mode=mode, stats=st, want_stats=wst, dead=dead_slots)


def random_share(n, share, seed=5):
    return np.random.default_rng(seed).choice(n, max(1, int(round(n * share))), replace=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# removal
# ---------------------------------------------------------------------------------------------------------------------------------
def test_remove_labels_counts_and_mirrors(capi, oracle):
    n, d = 1000, 16
    base = make_rows("l2sq", d, n, 1)
    ix = build(capi, "l2sq", "f32", base, 8)
    labels = np.arange(n, dtype=np.uint64) + 1
    g0, sum0 = ix.export_graph(), ix.checksum()
    assert ix.deleted_count == 0 and ix.remove_labels([]) == 0 and ix.checksum() == sum0
    rng = np.random.default_rng(2)
    first = rng.choice(labels, 150, replace=False)
    assert ix.remove_labels(first) == 150
    second = np.concatenate([rng.choice(labels, 200, replace=False), first[:40], [0, 0, 5000, 2**40 + 3, 2**63], first[:40]]).astype(np.uint64)
    rng.shuffle(second)  # duplicates, strangers, 0 and labels removed before: none of them counts
    expect = np.setdiff1d(np.intersect1d(second, labels), first)
    assert ix.remove_labels(second) == expect.size
    gone = np.union1d(first, expect)
    want_labels = np.where(np.isin(labels, gone), 0, labels).astype(np.uint64)
    assert ix.deleted_count == gone.size == int((want_labels == 0).sum())
    g1 = ix.export_graph()
    assert np.array_equal(g1["labels"], want_labels)  # the host mirror
    for key in ("levels", "nbr0", "upper_off", "upper_nbr"):
        assert np.array_equal(g0[key], g1[key]), key  # only labels changed
    again = capi.GpuIndex("l2sq", d, M=8, ef_construction=EFC, ef=EF, seed=11)
    again.load_buffer(ix.save_buffer())
    assert np.array_equal(again.export_graph()["labels"], want_labels) and again.deleted_count == gone.size and again.checksum() == ix.checksum()
    assert ix.save_stream() == ix.save_buffer()
    # a search returns label 0 for exactly the removed slots it reaches (the device's own label array)
    queries = make_rows("l2sq", d, 64, 3)
    ora = oracle.OracleIndex.from_graph("l2sq", base, g1, 8, EFC, EF, 11, oracle.SUM_WAVE64)
    o_lab, o_dist, o_slots, _, _ = ora.search_batch(queries, 10, EF, 4)
    lab, dist, _ = ix.search_batch(queries, 10)
    assert np.array_equal(lab, o_lab) and np.array_equal(dist, o_dist)
    assert np.array_equal(lab == 0, want_labels[o_slots.astype(np.int64)] == 0) and (lab == 0).any()
    # a filter that skips deleted rows is a snapshot of the labels at its build
    f = ix.filter_from_bitmap(np.ones(n, dtype=bool), skip_deleted=True)
    assert f.count == n - gone.size
    flab, _, _ = ix.search_batch_filtered(f, queries, 10)
    assert not (flab == 0).any()


def test_golden_delete_case_through_the_scan(capi):
    with open(os.path.join(ROOT, "tests", "golden", "delete_cases.json")) as fh:
        c = json.load(fh)["small_world_partial"]
    rows = np.array(c["v"], dtype=np.float32)
    labels = np.arange(len(rows), dtype=np.uint64) + 1
    name = {int(l): i for l, i in zip(labels, c["ids"])}
    ix = capi.GpuIndex("l2sq", 3, M=c["M"], ef_construction=128, ef=64, seed=7)
    ix.add_many(labels, rows)
    q = np.array(c["query"], dtype=np.float32)

    def fetch(limit):
        s = capi.Scan(ix, init_k=10)
        s.rescan(q)
        out = [name[int(l)] for l in s.fetch(limit)]
        s.end()
        return out

    got = fetch(c["limit"])
    assert got[0] == c["before"]["first"] and sorted(got[1:]) == sorted(c["before"]["then_any_order"])
    dead = [l for l in labels if name[int(l)] in c["deleted"]["ids"]]
    assert ix.remove_labels(dead) == 3
    assert fetch(c["limit"]) == c["after_vacuum"]["rows"]  # scan.c:296-300 drops label 0
    assert ix.unlink_deleted()["tombstones_unlinked"] == 3
    assert fetch(c["limit"]) == c["after_vacuum"]["rows"]


@pytest.mark.parametrize("storage", ["f16", "i8", "b1", "pq"])
def test_removal_on_every_index_kind_changes_labels_only(capi, storage):
    n, d = 600, 64
    base = make_rows("l2sq", d, n, 4)
    if storage == "pq":
        from tests.test_gpu_quantized_indexes import make_codebook

        ix = build(capi, "l2sq", "f32", base, 8, pq_codebook=make_codebook(np.random.default_rng(0), base, 8, 32), num_subvectors=8)
        ix.pq_compact()
    else:
        ix = build(capi, "l2sq", storage, base, 8)
    g0 = ix.export_graph()
    dead = random_share(n, 0.25)
    assert ix.remove_labels(dead + 1) == dead.size and ix.deleted_count == dead.size
    g1 = ix.export_graph()
    for key in ("levels", "nbr0", "upper_off", "upper_nbr"):
        assert np.array_equal(g0[key], g1[key]), key
    assert np.array_equal(np.flatnonzero(g1["labels"] == 0), np.sort(dead))
    lab, _, _ = ix.search_batch(base[:32], 5)
    assert (lab == 0).any()
    if storage == "pq":
        with pytest.raises(capi.LanternGpuError, match=r"unlink does not run on a compact pq index: expand it first \(lantern_gpu_pq_expand\)"):
            ix.unlink_deleted()
        ix.pq_expand()
        assert ix.unlink_deleted()["tombstones_unlinked"] == dead.size


# ---------------------------------------------------------------------------------------------------------------------------------
# parity of the unlink
# ---------------------------------------------------------------------------------------------------------------------------------
# rows of d = 3, 16 and 100 f32 scalars (1, 4 and 25 chunks) are read by 8 lanes, 200 (50 chunks) by 16, 300 (75) by 32 and 768 (192, the
# int8 screen present) by 64: every instantiation width of k_unlink_requests.  M 2 and 4 give many upper levels and full lists.
CASES = [
    ("l2sq", "f32", 3, 4, 700, 0.30), ("cos", "f32", 3, 2, 700, 0.30),
    ("l2sq", "f32", 16, 2, 1000, 0.30), ("cos", "f32", 16, 16, 1000, 0.01), ("l2sq", "f32", 16, 4, 1000, 0.90),
    ("l2sq", "f32", 100, 4, 1200, 0.90), ("cos", "f32", 100, 16, 1000, 0.30), ("l2sq", "f32", 100, 2, 900, 0.01),
    ("l2sq", "f32", 200, 4, 1000, 0.30), ("cos", "f32", 200, 16, 800, 0.30), ("cos", "f32", 300, 4, 1000, 0.30), ("l2sq", "f32", 300, 16, 800, 0.90),
    ("l2sq", "f32", 768, 16, 1500, 0.90), ("cos", "f32", 768, 4, 800, 0.30), ("l2sq", "f32", 768, 2, 600, 0.30), ("cos", "f32", 768, 16, 900, 0.01),
    ("l2sq", "f16", 64, 4, 1000, 0.30), ("cos", "f16", 64, 16, 1000, 0.90), ("l2sq", "i8", 64, 2, 1000, 0.30), ("cos", "i8", 64, 16, 1000, 0.30),
    ("hamming", "f32", 24, 4, 1000, 0.30), ("hamming", "f32", 24, 16, 1000, 0.90),
    # The unlink hands its offers to the build's grouping pass and launch_revlink (kernels.hip), with inputs no build produces: no radius
    # on record and up to cut(cap) requests per list.  One case per reverse-link class the cases above do not reach; the restatement's
    # re-prunes on the oracle's build of the same rows (the device's graph: same batch plan) are next to each case.
    # k_revlink_pairs at 4, 6 and 8 chunks per lane (d = 1021: 256 chunks; 1536: 384; 2000: 500)
    ("l2sq", "f32", 1021, 4, 800, 0.30), ("cos", "f32", 1021, 4, 800, 0.30),   # 704, 1210 re-prunes
    ("l2sq", "f32", 1536, 4, 700, 0.30), ("cos", "f32", 1536, 4, 700, 0.30),   # 696, 1045
    ("l2sq", "f32", 2000, 4, 600, 0.30), ("cos", "f32", 2000, 4, 600, 0.30),   # 631, 903
    ("l2sq", "f32", 512, 40, 600, 0.30),    # the generic k_revlink (82 rows of 2 KiB do not fit the staged kernel): 493, the longest kept list 80
    ("l2sq", "f32", 64, 32, 1500, 0.30),    # k_revlink_staged without chain mode, cap 64: 1956, max_kept 64
    ("l2sq", "f32", 64, 33, 1500, 0.30),    # ... cap 66, the heuristic's second kept slot per lane: 2137, max_kept 66
    ("hamming", "f32", 560, 24, 700, 0.30),  # 140 chunks, cap 48: staged, in chain mode, on wide bit rows: 2981
    ("l2sq", "b1", 200, 4, 1000, 0.30), ("cos", "b1", 200, 4, 1000, 0.30),  # sign-bit rows (hamming / cos_b1 on 7 words): 1644, 1237
]
MIN_MAX_KEPT = {33: 64, 65: 128}  # M -> what the longest list a re-prune of the restatement left must exceed: kpos[1], kpos[2] of k_revlink_staged


@pytest.mark.parametrize("metric,storage,d,M,n,share", CASES)
def test_unlink_equals_the_restatement(capi, oracle, metric, storage, d, M, n, share):
    base = make_rows(metric, d, n, d + M)
    r = remove_and_unlink(capi, oracle, metric, storage, base, M, random_share(n, share))
    if share >= 0.3 and (M <= 4 or M >= 24):
        assert r["stats"]["reprune_evals"] > 0  # full lists: the re-prune path ran
    if M in MIN_MAX_KEPT:  # on the restatement alone
        assert r["want_stats"]["max_kept"] > MIN_MAX_KEPT[M], r["want_stats"]


def test_unlink_on_hubs_with_lists_of_130(capi, oracle):
    """tests/test_gpu_long_lists.py's hubs at M = 65 (cap 130: k_revlink_staged, the heuristic's third kept slot per lane).  The
    tombstones are 30 % of the rows that are not hubs, so the hubs' full lists lose about 39 entries each and are offered the
    neighbours of those.  Measured on the restatement over the oracle's build: 6787 re-prunes, max_kept 130."""
    from tests.test_gpu_long_lists import hubs

    n, d, M = 1200, 128, 65
    base, hub = hubs(n, d, 8, d + M)
    rest = np.setdiff1d(np.arange(n), hub)
    r = remove_and_unlink(capi, oracle, "l2sq", "f32", base, M, rest[random_share(rest.size, 0.3)])
    assert r["want_stats"]["max_kept"] > MIN_MAX_KEPT[M], r["want_stats"]
    assert r["stats"]["reprune_evals"] > 0


def test_unlink_on_an_expanded_pq_index(capi, oracle):
    """pq rows (S = 8, C = 32, d = 64): the expanded index holds the decodings, and the unlink is the restatement over those --
    the exported vectors, in the f32 order (SUM_WAVE64) --, not only a count of tombstones."""
    from tests.test_gpu_quantized_indexes import make_codebook

    n, d, M = 1000, 64, 4
    base = make_rows("l2sq", d, n, d + M)
    cb = make_codebook(np.random.default_rng(0), base, 8, 32)
    r = remove_and_unlink(capi, oracle, "l2sq", "f32", base, M, random_share(n, 0.3), pq_codebook=cb, num_subvectors=8)
    assert r["ix"].pq_S == 8 and not np.array_equal(r["rows"], base)
    assert r["stats"]["reprune_evals"] > 0


def test_unlink_entry_node_isolated_node_and_adjacent_tombstones(capi, oracle):
    n, d, M = 1000, 16, 4
    base = make_rows("l2sq", d, n, 21)
    g = build(capi, "l2sq", "f32", base, M).export_graph()
    entry = int(g["entry_slot"])
    v = next(s for s in range(n) if s != entry and entry not in unlink_ref.get_list(g, s, 0, M) and len(unlink_ref.get_list(g, s, 0, M)) >= 3)
    nb = unlink_ref.get_list(g, v, 0, M)  # every neighbour of v goes, v stays
    a = next(s for s in range(n) if s not in nb and s != v and s != entry)
    pair = [a, next(x for x in unlink_ref.get_list(g, a, 0, M) if x != v)]  # two adjacent tombstones
    r = remove_and_unlink(capi, oracle, "l2sq", "f32", base, M, [entry] + nb + pair)
    assert r["stats"]["entry_moved"] == 1 and r["after"]["entry_slot"] != entry
    assert r["after"]["labels"][r["after"]["entry_slot"]] != 0


def test_unlink_with_identical_rows(capi, oracle):
    """200 identical rows: every distance among them ties, the order is tie_mix's."""
    for metric, M in (("l2sq", 4), ("cos", 16)):
        base = make_rows(metric, 16, 1000, 31, identical=200)
        dead = np.union1d(random_share(1000, 0.3), np.arange(100, 300, 3))
        remove_and_unlink(capi, oracle, metric, "f32", base, M, dead)


def cut_case(oracle, M=16, d=100, n=1500):
    """M 16: cut(0) = 256 offers need a list most of whose 32 entries are tombstones with mostly live lists of their own.  A random
    share s of deletions gives a list about 1024 s (1 - s) candidates before duplicates -- at most 256, 92 at 90 % -- so it never
    reaches the cut; deleting only the neighbours of a few nodes does.  The restatement on the oracle's build (the device's graph:
    same batch plan) says how many lists are cut.
    M 17 and 32: cut(0) = 8 x 2 M = 272 and 512, the other branch of unlink_cut; there the neighbours of the three longest level-0
    lists go (a stable argsort of the lengths), those three nodes stay."""
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=EFC, ef=EF, seed=11, sum_mode=oracle.SUM_WAVE64)
    if M == 16:
        base = make_rows("l2sq", d, n, 41)
        ora.add_planned(np.arange(n, dtype=np.uint64) + 1, base, 256, 16)
        g = ora.export_graph()
        full = [s for s in range(n) if len(unlink_ref.get_list(g, s, 0, M)) == 2 * M][:3]
    else:
        base = make_rows("l2sq", d, n, d + M)
        ora.add_planned(np.arange(n, dtype=np.uint64) + 1, base, 256, 16)
        g = ora.export_graph()
        full = [int(s) for s in np.argsort(-(g["nbr0"] != unlink_ref.EMPTY).sum(axis=1), kind="stable")[:3]]
    dead = np.unique(np.concatenate([unlink_ref.get_list(g, s, 0, M) for s in full]))
    return base, np.setdiff1d(dead, full)


# M, d, n, cut(0), and on the oracle's graph: the lists the restatement cuts, its re-prunes
CUT_CASES = [(16, 100, 1500, 256, None, None), (17, 64, 1500, 272, 3, 2616), (32, 64, 1500, 512, 3, 1759)]


@pytest.mark.parametrize("M,d,n,cut,lists_cut,reprunes", CUT_CASES, ids=[f"M{c[0]}" for c in CUT_CASES])
def test_unlink_cuts_the_offers_at_256(capi, oracle, M, d, n, cut, lists_cut, reprunes):
    """... or at 8 cap, whichever is more"""
    assert unlink_ref.cut_of(0, M) == cut
    base, dead = cut_case(oracle, M, d, n)
    r = remove_and_unlink(capi, oracle, "l2sq", "f32", base, M, dead)
    assert r["stats"]["lists_cut"] > 0
    if lists_cut is not None:  # (the restatement ran on the device's graph: the oracle's, if the build is right)
        assert (r["want_stats"]["lists_cut"], r["want_stats"]["reprunes"]) == (lists_cut, reprunes)


# ---------------------------------------------------------------------------------------------------------------------------------
# the graph still works
# ---------------------------------------------------------------------------------------------------------------------------------
# d = 1021, M = 4: k_revlink_pairs, whose re-prunes keep a state across batches (the radii on record) -- the unlink resets it, and the
# 300 rows added afterwards build on the reset; d = 64, M = 32: lists of 64 (k_revlink_staged without chain mode) before and after
@pytest.mark.parametrize("metric,storage,d,M", [("l2sq", "f32", 768, 16), ("cos", "f16", 64, 4), ("l2sq", "f32", 1021, 4), ("l2sq", "f32", 64, 32)])
def test_unlinked_graph_searches_and_grows_as_the_oracle_on_the_same_graph(capi, oracle, metric, storage, d, M):
    from lantern_amd import hip

    n, nq, k = 1200, 100, 10
    base = make_rows(metric, d, n + 300, 51)
    queries = make_rows(metric, d, nq, 52)
    r = remove_and_unlink(capi, oracle, metric, storage, base[:n], M, random_share(n, 0.3))
    ix, after = r["ix"], r["after"]
    rows_all, q_s, _, mode = stored_rows(oracle, storage, metric, base, queries)
    ora = oracle.OracleIndex.from_graph(metric, rows_all[:n], after, M, EFC, EF, 11, mode, borrow=False)
    o_lab, o_dist, _, o_D, o_E = ora.search_batch(q_s, k, EF, 4)
    assert not (o_lab == 0).any()
    # the batch, with D and E
    dq = ix.device_query_rows(queries)
    bq = hip.Buffer.from_numpy(dq)
    lab, dist, D, E = hip.Buffer(nq * k * 8), hip.Buffer(nq * k * 4), hip.Buffer(nq * 8), hip.Buffer(nq * 8)
    ix.search_batch_device(bq.ptr, nq, k, 0, 0, lab.ptr, dist.ptr, None, None, D.ptr, E.ptr, query_stride=dq.strides[0])
    hip.synchronize()
    assert np.array_equal(lab.download((nq, k), np.uint64), o_lab) and np.array_equal(dist.download((nq, k), np.float32), o_dist)
    assert np.array_equal(D.download(nq, np.uint64), o_D) and np.array_equal(E.download(nq, np.uint64), o_E)
    h_lab, h_dist, _ = ix.search_batch(queries, k)
    assert np.array_equal(h_lab, o_lab) and np.array_equal(h_dist, o_dist)
    # the lone query and the cursor
    l1, d1 = ix.search(queries[0], k)
    assert np.array_equal(l1, o_lab[0]) and np.array_equal(d1, o_dist[0])
    cur = ix.cursor()
    c1, cd1 = cur.search(queries[1], 5)
    c2, _ = cur.search(queries[1], 5, streaming=True)
    assert np.array_equal(c1, o_lab[1][:5]) and np.array_equal(cd1, o_dist[1][:5]) and not set(c1) & set(c2) and 0 not in set(c2)
    cur.close()
    # 300 more rows: the oracle on the same graph, the same batch plan, edge for edge
    more = np.arange(n, n + 300, dtype=np.uint64) + 1
    ix.add_many(more, base[n:])
    ora.add_planned(more, rows_all[n:], 256, 16)
    graphs_equal(ix.export_graph(), ora.export_graph())
    assert ix.deleted_count == r["dead"].size


# ---------------------------------------------------------------------------------------------------------------------------------
# existing handles and refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_filter_and_cursor_made_before_the_unlink_still_serve(capi, oracle):
    n, d, M = 1000, 16, 8
    base = make_rows("l2sq", d, n, 61)
    q = make_rows("l2sq", d, 8, 62)
    ix = build(capi, "l2sq", "f32", base, M)
    dead = random_share(n, 0.3)
    ix.remove_labels(dead + 1)
    allowed = np.zeros(n, dtype=bool)
    allowed[::2] = True
    f = ix.filter_from_bitmap(allowed, skip_deleted=True)
    cur = ix.cursor()
    page1, _ = cur.search(q[0], 5)
    ix.unlink_deleted()
    g = ix.export_graph()
    page2, _ = cur.search(q[0], 5, streaming=True)
    assert len(page2) == 5 and not set(page1) & set(page2) and 0 not in set(page2)
    lab, dist, cnt = ix.search_batch_filtered(f, q, 10)
    ok = allowed & (g["labels"] != 0)
    assert (cnt == 10).all() and ok[lab.astype(np.int64) - 1].all()
    from tests import filtered_walk_ref as ref

    dm = ref.distance_matrix(oracle, base, q, "l2sq", oracle.SUM_WAVE64)
    ix.set_filter_policy("walk")
    lab, dist, cnt = ix.search_batch_filtered(f, q, 10)
    slots, dists, counts, _, _ = ref.search(g, dm, ok, M, 10, EF)
    assert np.array_equal(lab.astype(np.int64) - 1, slots.astype(np.int64)) and np.array_equal(dist, dists)
    cur.close()


def test_unlink_refuses_a_page_attached_index(capi):
    from tests.pg_pages import PageStore

    n, d, M = 300, 16, 8
    base = make_rows("l2sq", d, n, 71)
    pages = PageStore(capi, build(capi, "l2sq", "f32", base, M).save_buffer(), d * 4, M)
    mirror = capi.GpuIndex("l2sq", d, M=M, ef_construction=EFC, ef=EF, seed=11, retriever=pages.retriever)
    mirror.view_mem_lazy(pages.header)
    assert mirror.remove_labels([1, 2, 3]) == 3 and mirror.deleted_count == 3  # removal serves a mirror
    with pytest.raises(capi.LanternGpuError, match="unlink does not run on a page-attached index"):
        mirror.unlink_deleted()


def test_nothing_live_and_empty_index(capi):
    n, d = 300, 16
    base = make_rows("l2sq", d, n, 81)
    ix = build(capi, "l2sq", "f32", base, 8)
    before = ix.checksum()
    assert ix.unlink_deleted() == dict.fromkeys(ix.unlink_deleted(), 0)  # nothing deleted
    assert ix.remove_labels(np.arange(n, dtype=np.uint64) + 1) == n
    removed_sum = ix.checksum()
    assert removed_sum != before
    assert all(v == 0 for v in ix.unlink_deleted().values()) and ix.checksum() == removed_sum  # nothing live: nothing changes
    empty = capi.GpuIndex("l2sq", d, M=8)
    assert empty.remove_labels([1, 2]) == 0 and empty.deleted_count == 0 and all(v == 0 for v in empty.unlink_deleted().values())
