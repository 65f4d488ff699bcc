"""The dense route of a per-query-filter call, without a device (include/lantern_gpu.h "THE DENSE ROUTE FOR PER-QUERY-FILTER CALLS",
DESIGN.md 4.9): lantern_gpu_plan_filtered_each_dense is the plan the call itself runs -- which queries form dense groups, the order the
run holds them in, the segments of the concatenated slot list and the contraction steps.  Checked against a numpy restatement."""
import ctypes as C
import json
import os

import numpy as np
import pytest

L2SQ, COS, HAMMING, COS_B1 = 3, 1, 8, 9  # usearch_metric_kind_t, and cosine over the bits of a b1 index (+ 100: f16 storage, + 200: i8)
NONE = 0xFFFFFFFF
CHUNK, QTILE = 65536, 1024


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def restate(k, skip, m, ids, counts, exact, compact=False):
    """the grouping as the header states it: (why, group per query, order, qoff, seg)"""
    nq = len(ids)
    nothing = lambda why: (why, [NONE] * nq, [], [0], [0])
    if m == 0:
        return nothing("off")
    if k + skip > 240:
        return nothing("wide")
    if compact:
        return nothing("compact")
    by_id = {}
    for i in range(nq):
        if exact[i] and ids[i] >= 0 and counts[i] > 0 and k > 0:
            by_id.setdefault(ids[i], []).append(i)
    groups = sorted((qs for qs in by_id.values() if len(qs) >= m), key=lambda qs: qs[0])
    if not groups:
        return nothing("no_group")
    if sum(counts[qs[0]] for qs in groups) > 0xFFFFFFFF:
        return nothing("too_many_rows")
    group, order, qoff, seg = [NONE] * nq, [], [0], [0]
    for g, qs in enumerate(groups):
        for q in qs:
            group[q] = g
        order += qs
        qoff.append(len(order))
        seg.append(seg[-1] + counts[qs[0]])
    return "taken", group, order, qoff, seg


def check_steps(steps, qoff, seg):
    """every (dense query, position of its own segment) pair in exactly one step and no other pair in any; no step across a chunk of
    65 536 positions or over 1024 queries; chunk-major"""
    qoff, seg = np.asarray(qoff, np.int64), np.asarray(seg, np.int64)
    total = int(seg[-1])
    chunk_rows = min(total, CHUNK)
    cover = {}  # (group, first query of the tile, queries) -> [(col0, cols)]
    area, last_chunk = 0, 0
    for q0, nqt, col0, cols in steps:
        assert 1 <= nqt <= QTILE and cols >= 1
        g = int(np.searchsorted(qoff, q0, side="right")) - 1
        assert qoff[g] <= q0 and q0 + nqt <= qoff[g + 1], "a step's queries belong to one group"
        assert seg[g] <= col0 and col0 + cols <= seg[g + 1], "a step's positions belong to its group's segment"
        assert col0 // chunk_rows == (col0 + cols - 1) // chunk_rows, "a step crosses a chunk"
        assert col0 // chunk_rows >= last_chunk, "steps are chunk-major"
        last_chunk = col0 // chunk_rows
        assert (q0 - qoff[g]) % QTILE == 0 and (nqt == QTILE or q0 + nqt == qoff[g + 1]), "tiles of 1024 queries from the group's first"
        cover.setdefault((g, q0, nqt), []).append((col0, cols))
        area += nqt * cols
    want = 0
    for g in range(len(seg) - 1):
        for q0 in range(int(qoff[g]), int(qoff[g + 1]), QTILE):
            nqt = min(QTILE, int(qoff[g + 1]) - q0)
            at = int(seg[g])
            for col0, cols in sorted(cover.get((g, q0, nqt), [])):
                assert col0 == at, "a tile's steps tile its segment without gap or overlap"
                at += cols
            assert at == seg[g + 1]
            want += nqt * int(seg[g + 1] - seg[g])
    assert area == want


def plan_and_check(capi, k, skip, m, ids, counts, exact, compact=False, mcode=L2SQ, chunks=8):
    p = capi.plan_filtered_each_dense(mcode, chunks, k, skip, m, ids, counts, exact, compact=compact)
    why, group, order, qoff, seg = restate(k, skip, m, list(ids), list(counts), list(exact), compact)
    assert p["why"] == why
    assert p["group"] == group and p["order"] == order
    if why != "taken":
        assert p["groups"] == 0 and p["queries"] == 0 and p["kk"] == 0 and p["rows"] == 0 and p["n_steps"] == 0 and p["steps"] == [] and p["seg"] == []
        return p
    assert p["groups"] == len(seg) - 1 and p["queries"] == len(order) and p["seg"] == seg and p["rows"] == seg[-1]
    assert p["kk"] == k + skip + 16 and p["gather_rows"] == min(seg[-1], CHUNK)
    assert p["n_steps"] == len(p["steps"])
    check_steps(p["steps"], qoff, seg)
    return p


@pytest.mark.parametrize("seed", range(12))
def test_random_calls_against_the_restatement(capi, seed):
    rng = np.random.default_rng([41, seed])
    nq = int(rng.integers(1, 3000))
    n_ids = int(rng.integers(1, 12))
    id_count = rng.choice([0, 1, 37, 500, 4097, 65530, 65536, 70000, 200000], size=n_ids)
    # a few ids stand behind most queries, so that groups pass 1024 queries; the entries are interleaved, not sorted by id
    which = rng.integers(-1, n_ids, size=nq) if seed % 2 else np.minimum(rng.geometric(0.5, size=nq) - 2, n_ids - 1)
    ids = np.where(which < 0, -1, which * 7 + 3).astype(np.int64)
    counts = np.where(which < 0, 0, id_count[np.maximum(which, 0)]).astype(np.int64)
    exact = (rng.random(nq) < 0.8) & (which >= 0)
    m = int(rng.choice([1, 2, 5, 40]))
    p = plan_and_check(capi, 10, int(rng.integers(0, 20)), m, ids, counts, exact)
    # NULL, empty and walk-path entries are never grouped
    for i in range(nq):
        if ids[i] < 0 or counts[i] == 0 or not exact[i]:
            assert p["group"][i] == NONE


def test_order_is_first_appearance_then_call_order(capi):
    # id 9 appears first at query 1, id 4 at query 0 -- and again at the end, not adjacent; id 5 has too few queries
    ids = [4, 9, 9, 5, 4, -1, 9, 4]
    counts = [30, 20, 20, 10, 30, 0, 20, 30]
    p = plan_and_check(capi, 10, 0, 2, ids, counts, [1] * 8)
    assert p["order"] == [0, 4, 7, 1, 2, 6] and p["seg"] == [0, 30, 50]
    assert p["group"] == [0, 1, 1, NONE, 0, NONE, 1, 0]
    assert p["steps"] == [(0, 3, 0, 30), (3, 3, 30, 20)]


def test_min_group_edge(capi):
    ids, counts = [1, 2, 1, 2, 1, 2, 2], [50] * 7
    p = plan_and_check(capi, 10, 0, 4, ids, counts, [1] * 7)  # id 1: m - 1 queries, id 2: m
    assert p["groups"] == 1 and p["order"] == [1, 3, 5, 6]
    assert plan_and_check(capi, 10, 0, 5, ids, counts, [1] * 7)["why"] == "no_group"
    assert plan_and_check(capi, 10, 0, 3, ids, counts, [1] * 7)["groups"] == 2
    # a walk-path query does not count towards its handle's group
    assert plan_and_check(capi, 10, 0, 4, ids, counts, [1, 1, 1, 0, 1, 1, 1])["why"] == "no_group"


def test_call_level_reasons(capi):
    ids, counts, exact = [3, 3, 3], [100, 100, 100], [1, 1, 1]
    assert plan_and_check(capi, 10, 0, 0, ids, counts, exact)["why"] == "off"
    assert plan_and_check(capi, 10, 230, 1, ids, counts, exact)["kk"] == 256  # k + skip = 240
    assert plan_and_check(capi, 240, 0, 1, ids, counts, exact)["why"] == "taken"
    assert plan_and_check(capi, 10, 231, 1, ids, counts, exact)["why"] == "wide"  # 241
    assert plan_and_check(capi, 241, 0, 1, ids, counts, exact)["why"] == "wide"
    assert plan_and_check(capi, 10, 0, 1, ids, counts, exact, compact=True)["why"] == "compact"
    assert plan_and_check(capi, 10, 0, 0, ids, counts, exact, compact=True)["why"] == "off"  # the switch comes first
    assert plan_and_check(capi, 10, 0, 1, [-1, -1], [0, 0], [0, 0])["why"] == "no_group"
    assert plan_and_check(capi, 10, 0, 1, [5, 5], [0, 0], [1, 1])["why"] == "no_group"  # an empty filter
    assert plan_and_check(capi, 10, 0, 1, [], [], [])["why"] == "no_group"
    # two groups of 2^31 rows: 2^32 positions do not fit
    assert plan_and_check(capi, 10, 0, 1, [1, 2], [2**31, 2**31], [1, 1])["why"] == "too_many_rows"
    assert plan_and_check(capi, 10, 0, 1, [1, 2], [2**31, 2**31 - 1], [1, 1])["rows"] == 2**32 - 1


def test_segment_across_a_chunk_and_tile_edge(capi):
    # the second segment straddles position 65 536: two steps for each of its tiles; 1025 queries are two tiles
    ids = [1] * 3 + [2] * 1025
    counts = [65530] * 3 + [20] * 1025
    p = plan_and_check(capi, 10, 0, 2, ids, counts, [1] * 1028)
    assert p["steps"] == [(0, 3, 0, 65530), (3, 1024, 65530, 6), (1027, 1, 65530, 6), (3, 1024, 65536, 14), (1027, 1, 65536, 14)]
    assert p["gather_rows"] == 65536


@pytest.mark.parametrize("mcode,chunks", [(L2SQ, 2), (COS + 100, 96), (L2SQ + 200, 48), (HAMMING, 6), (COS_B1, 2)])
def test_row_kinds_and_bad_input(capi, mcode, chunks):
    plan_and_check(capi, 10, 3, 2, [1, 1, 2, 2, 2], [100, 100, 70000, 70000, 70000], [1] * 5, mcode=mcode, chunks=chunks)
    for m in (0, 1):
        with pytest.raises(capi.LanternGpuError, match="bad plan input"):
            capi.plan_filtered_each_dense(mcode, 0, 10, 0, m, [1], [5], [1])
        with pytest.raises(capi.LanternGpuError, match="bad plan input"):
            capi.plan_filtered_each_dense(mcode, chunks, 10, 0, m, [1], [-1], [1])
        with pytest.raises(capi.LanternGpuError, match="bad plan input"):
            capi.plan_filtered_each_dense(mcode, chunks, 10, 0, m, [-2], [5], [1])
    count = C.c_size_t(0)
    assert b"null plan array" in capi.lib().lantern_gpu_plan_filtered_each_dense(None, None, 0, None, None, None, None, None, 0, C.byref(count))


def test_setter_getter_and_diagnostic_refuse_a_foreign_handle(capi):
    junk = C.create_string_buffer(8192)
    h = C.cast(junk, C.c_void_p)
    err = C.c_char_p()
    capi.lib().lantern_gpu_set_filter_dense_each(h, 4, C.byref(err))
    assert err.value and b"not an index handle" in err.value
    err = C.c_char_p()
    assert capi.lib().lantern_gpu_filter_dense_each(h, C.byref(err)) == 0
    assert err.value and b"not an index handle" in err.value
    out = (C.c_uint32 * 6)(*([7] * 6))
    err = C.c_char_p()
    capi.lib().lantern_gpu_last_filtered_each_dense(h, out, C.byref(err))
    assert err.value and b"not an index handle" in err.value and list(out) == [7] * 6


def test_the_two_existing_plans_are_unchanged(capi):
    """lantern_gpu_plan_exact_knn and lantern_gpu_plan_filtered_dense on a few inputs, as recorded from the commit before the explicit
    step list (tests/golden/dense_plans_before_each_dense.json)"""
    with open(os.path.join(os.path.dirname(__file__), "golden", "dense_plans_before_each_dense.json")) as fh:
        rec = json.load(fh)
    assert len(rec["exact_knn"]) >= 6 and len(rec["filtered_dense"]) >= 6
    for args, want in rec["exact_knn"]:
        got = capi.plan_exact_knn(*args)
        got["steps"] = [list(s) for s in got["steps"]]
        assert got == want, args
    for args, want in rec["filtered_dense"]:
        got = capi.plan_filtered_dense(*args)
        got["steps"] = [list(s) for s in got["steps"]]
        assert got == want, args
