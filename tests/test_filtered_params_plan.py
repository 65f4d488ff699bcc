"""lantern_gpu_plan_filtered_params: the plan of a per-query filtered call with per-query (k, ef, skip) -- path, expansion and C per query,
the two selection lists and the two launches' carves -- as a pure function (include/lantern_gpu.h).  No device.

The entry points plan through this function, so what is asserted here is what launches.
"""
import numpy as np
import pytest

from lantern_amd import capi

LDS = 160 * 1024
FACTOR = 5.6
BASE = {"chunks": 32, "M0": 32, "n": 3000, "ef_default": 64, "path": 0, "cand_cap": 0, "exact_factor": FACTOR, "seeds": 0}  # 128-d f32 rows, M = 16


def plan(counts, params, **over):
    return capi.plan_filtered_params({**BASE, **over}, counts, params)


def one(count, k, ef, skip=0, **over):
    per, launch, why = plan([count], [(k, ef, skip)], **over)
    assert why is None, why
    return per[0], launch


def walk_base(e, **over):
    """B(e) of the header: the walk's LDS beside `next` and the visited set, read off a one-query plan."""
    q, launch = one(-1, 1, e, **over)
    w = launch["walk"]
    assert q["path"] == 1 and w["expansion"] == e
    return w["lds"] - 16 * w["cand_cap"] - 4 * w["vis_slots_or_rows"]


def test_the_path_flips_with_a_querys_own_ef():
    n, count = 3000, 1000
    threshold = count * count / (FACTOR * n)  # exact iff count^2 <= factor * ef * n
    assert 32 < threshold <= 64
    per, launch, why = plan([count, count, count], [(10, 32), (10, 64), (10, 0)], n=n)
    assert why is None
    assert [q["path"] for q in per] == [1, 2, 2]  # (ef 0: the index's default, 64)
    assert launch["walk"]["queries"] == 1 and launch["exact"]["queries"] == 2
    per, _, _ = plan([count], [(10, 0)], n=n, ef_default=32)
    assert per[0]["path"] == 1
    # the rule does not look at k or skip
    per, _, _ = plan([count, count], [(500, 32, 100), (1, 64, 0)], n=n)
    assert [q["path"] for q in per] == [1, 2]
    # forced paths; a NULL entry walks whatever the policy
    per, _, _ = plan([count, 5, -1], [(10, 64), (10, 64), (10, 64)], n=n, path=1)
    assert [q["path"] for q in per] == [1, 1, 1]
    per, _, _ = plan([count, 2999, -1], [(10, 32), (10, 32), (10, 32)], n=n, path=2)
    assert [q["path"] for q in per] == [2, 2, 1]


@pytest.mark.parametrize("exp,want", [(1, 256), (64, 256), (65, 260), (300, 1200)])
def test_the_automatic_cap_switches_from_256_to_four_expansions(exp, want):
    q, launch = one(-1, 1, exp)
    assert (q["path"], q["expansion"], q["cand_cap"]) == (1, exp, want)
    assert (launch["walk"]["expansion"], launch["walk"]["cand_cap"]) == (exp, want)
    q, _ = one(-1, exp, 1)  # the expansion is max(ef, k + skip)
    assert (q["expansion"], q["cand_cap"]) == (exp, want)
    q, _ = one(-1, 1, 1, skip=exp - 1)
    assert (q["expansion"], q["cand_cap"]) == (exp, want)


def test_an_explicit_cap_is_raised_to_the_expansion():
    per, launch, why = plan([-1, -1, -1], [(10, 64), (10, 100), (10, 300)], cand_cap=100)
    assert why is None
    assert [q["cand_cap"] for q in per] == [100, 100, 300]
    assert [q["expansion"] for q in per] == [64, 100, 300]
    assert (launch["walk"]["expansion"], launch["walk"]["cand_cap"]) == (300, 300)


def test_every_query_is_planned_as_its_one_query_call_and_the_carve_is_the_largest():
    rng = np.random.default_rng(3)
    counts = [int(c) for c in rng.choice([-1, 0, 1, 30, 300, 1000, 3000], size=40)]
    params = [(int(rng.choice([0, 1, 5, 10, 300])), int(rng.choice([0, 1, 32, 64, 65, 400])), int(rng.choice([0, 0, 10, 1500]))) for _ in counts]  # (expansions below 2000: no cap binds)
    for over in ({}, {"path": 1}, {"path": 2}, {"cand_cap": 90}, {"chunks": 192, "M0": 64}):
        per, launch, why = plan(counts, params, **over)
        assert why is None
        walk, exact = [], []
        for i, (c, p) in enumerate(zip(counts, params)):
            q, solo = one(c, *p, **over)
            assert {n: per[i][n] for n in ("path", "expansion", "cand_cap")} == {n: q[n] for n in ("path", "expansion", "cand_cap")}, (i, c, p)
            if p[0] == 0 or c == 0:
                assert q == {"path": 0, "expansion": 0, "cand_cap": 0, "position": 0}
                assert solo["walk"]["queries"] == 0 and solo["exact"]["queries"] == 0  # alone: nothing is launched
            (walk if q["path"] == 1 else exact if q["path"] == 2 else []).append(i)
        riders = len(counts) - len(walk) - len(exact)
        assert walk and riders and (exact or over.get("path") == 1)
        w, e = launch["walk"], launch["exact"]
        # the riders ride in the exact launch, or in the walk launch when no query takes the exact path
        assert w["queries"] == len(walk) + (0 if exact else riders) and e["queries"] == (len(exact) + riders if exact else 0)
        assert w["expansion"] == max(per[i]["expansion"] for i in walk) and w["cand_cap"] == max(per[i]["cand_cap"] for i in walk)
        assert 0 < w["lds"] <= LDS and w["per_cu"] == max(1, min(4, LDS // w["lds"]))
        # the launch's carve is that of a query with the launch's largest expansion and (an explicit) largest cap
        _, solo = one(-1, 1, w["expansion"], **{**over, "path": 1, "cand_cap": w["cand_cap"]})
        assert solo["walk"] == {**w, "queries": 1}
        if exact:
            assert e["expansion"] == max(per[i]["expansion"] for i in exact) and e["cand_cap"] == 0
            assert 0 < e["lds"] <= LDS and e["per_cu"] == max(1, min(4, LDS // e["lds"]))
            _, solo = one(5, e["expansion"], 1, **{**over, "path": 2})
            assert solo["exact"] == {**e, "queries": 1}
        else:
            assert e == dict.fromkeys(e, 0)
        # the orders: walk by expansion descending, exact by allowed count descending, both stable; the riders behind, in batch order
        order = sorted(walk, key=lambda i: -per[i]["expansion"])
        assert [per[i]["position"] for i in order] == list(range(len(walk)))
        order = sorted(exact, key=lambda i: -counts[i])
        assert [per[i]["position"] for i in order] == list(range(len(exact)))
        rest = [i for i in range(len(counts)) if per[i]["path"] == 0]
        first = len(exact) if exact else len(walk)
        assert [per[i]["position"] for i in rest] == list(range(first, first + riders))


def test_riders_take_the_walk_launch_when_nothing_is_exact_and_no_launch_alone():
    per, launch, why = plan([-1, 0, 500, 2000], [(10, 64), (10, 64), (0, 64), (10, 64)], path=1)
    assert why is None
    assert [q["path"] for q in per] == [1, 0, 0, 1]
    assert launch["walk"]["queries"] == 4 and launch["exact"]["queries"] == 0
    assert [q["position"] for q in per] == [0, 2, 3, 1]
    per, launch, why = plan([0, 500, -1], [(10, 64), (0, 64), (0, 0)])
    assert why is None and all(q == {"path": 0, "expansion": 0, "cand_cap": 0, "position": 0} for q in per)
    assert launch["walk"]["queries"] == 0 and launch["exact"]["queries"] == 0
    # an empty index: no query has a path
    per, launch, why = plan([-1, 0], [(10, 64), (10, 64)], n=0)
    assert why is None and [q["path"] for q in per] == [0, 0] and launch["walk"]["queries"] == 0
    # no query at all
    per, launch, why = plan([], [])
    assert why is None and per == [] and launch["walk"]["queries"] == 0 and launch["exact"]["queries"] == 0
    # a rider's parameters are never refused: the single-filter call answers an empty filter without looking at them
    per, launch, why = plan([0, -1], [(10**6, 10**6, 10**6), (0, 10**6, 10**6)])
    assert why is None


WALK_TEXT = "lantern_gpu: ef/k exceed the 160 KiB LDS budget of the filtered search kernel"
EXACT_TEXT = "lantern_gpu: k + skip exceed the 160 KiB LDS budget of the exact filtered search kernel"
CAP_TEXT = "lantern_gpu: the candidate cap exceeds the 160 KiB LDS budget of the filtered search kernel"
JOINT_TEXT = ("lantern_gpu: the queries fit the 160 KiB LDS budget of the filtered search kernel one by one, but the largest expansion and the largest "
              "candidate cap of the batch do not fit together: split the batch")


def test_a_query_over_the_budget_refuses_the_call_and_is_named():
    b0 = walk_base(1) - 32
    e_fit = max(e for e in range(4000, 5200) if walk_base_formula(b0, e) + 16 * e <= LDS)
    assert one(-1, 1, e_fit)[0]["cand_cap"] == e_fit  # the last expansion that fits leaves `next` exactly its own size
    fine = (10, 64)
    _, _, why = plan([-1, -1, -1], [fine, (1, e_fit + 1), fine])
    assert why == WALK_TEXT + " (params[1])"
    _, _, why = plan([-1, -1], [(5, 10, e_fit + 1 - 5), fine])
    assert why == WALK_TEXT + " (params[0])"
    _, _, why = plan([30, 30], [fine, (2**32 - 1, 64, 2**32 - 1)], path=2)  # (k + skip beyond 32 bits does not wrap into something that fits)
    assert why == EXACT_TEXT + " (params[1])"
    kk_fit = max(kk for kk in range(9000, 11000) if plan([30], [(kk, 1)], path=2)[2] is None)
    _, _, why = plan([30, 30], [fine, (1, 1, kk_fit)], path=2)
    assert why == EXACT_TEXT + " (params[1])"
    _, _, why = plan([-1, -1], [fine, fine], cand_cap=20000)
    assert why == CAP_TEXT + " (params[0])"
    # two offenders: the first in batch order is named, whatever its kind; and a query's own refusal comes before the joint one
    _, _, why = plan([30, -1, -1], [(1, 1, kk_fit), (1, e_fit + 1), fine], n=3000)
    assert why == EXACT_TEXT + " (params[0])"
    _, _, why = plan([-1, 30, -1], [(1, e_fit + 1), (1, 1, kk_fit), fine], n=3000)
    assert why == WALK_TEXT + " (params[0])"
    _, _, why = plan([-1, -1, -1], [(1, 4900), (1, 1800), (1, e_fit + 1)])
    assert why == WALK_TEXT + " (params[2])"


def walk_base_formula(b0, e):
    """B(e) = B(0) + 2 ceil16(8 e): the header's formula, B(0) read off the function."""
    return b0 + 2 * ((8 * e + 15) // 16 * 16)


@pytest.mark.parametrize("over", [{}, {"chunks": 192, "M0": 32}], ids=["128d", "768d"])
def test_the_joint_carve_is_refused_at_its_stated_boundary(over):
    b0 = walk_base(1, **over) - 32
    for e in (1, 64, 65, 300, 1999, 4000):
        assert walk_base(e, **over) == walk_base_formula(b0, e)
    # where a query's own cap starts to bind: 80 e > 163840 - B(0)
    e_bind = (LDS - b0) // 80 + 1
    assert 1900 < e_bind < 2100
    assert one(-1, 1, e_bind - 1, **over)[0]["cand_cap"] == 4 * (e_bind - 1)
    assert one(-1, 1, e_bind + 8, **over)[0]["cand_cap"] < 4 * (e_bind + 8)
    # below that no batch is refused: the largest C belongs to the largest expansion
    _, launch, why = plan([-1] * 4, [(1, 1), (1, 300), (1, e_bind - 1), (10, 64)], **over)
    assert why is None and launch["walk"]["cand_cap"] == 4 * (e_bind - 1)
    # a long scan of expansion 4900 leaves `next` room_a keys; a second query is accepted up to C = room_a and refused from room_a + 1
    e_a = 4900
    room_a = (LDS - walk_base_formula(b0, e_a)) // 16
    q, launch = one(-1, 1, e_a, **over)
    assert q["cand_cap"] == room_a < 4 * e_a
    e_b = room_a // 4
    per, launch, why = plan([-1, 500], [(1, e_a), (1, e_b)], **{**over, "path": 1})
    assert why is None
    assert (launch["walk"]["expansion"], launch["walk"]["cand_cap"]) == (e_a, room_a)
    assert launch["walk"]["lds"] == walk_base_formula(b0, e_a) + 16 * room_a <= LDS and launch["walk"]["vis_slots_or_rows"] == 0
    for counts in ([-1, 500], [500, -1]):  # (either order: the carve joins the batch's largest of each)
        params = [(1, e_a), (1, e_b + 1)] if counts[0] == -1 else [(1, e_b + 1), (1, e_a)]
        assert all(plan([c], [p], **{**over, "path": 1})[2] is None for c, p in zip(counts, params))  # each fits alone
        _, _, why = plan(counts, params, **{**over, "path": 1})
        assert why == JOINT_TEXT
    assert walk_base_formula(b0, e_a) + 16 * 4 * (e_b + 1) > LDS
    # two long scans of different lengths, each with the cap its own room allows: the shorter one's is the larger
    assert one(-1, 1, 3010, **over)[0]["cand_cap"] > one(-1, 1, 3300, **over)[0]["cand_cap"]
    assert plan([-1, -1], [(1, 3300), (1, 3010)], **over)[2] == JOINT_TEXT
    assert plan([-1, -1], [(1, 3010), (10, 64, 3000)], **over)[2] is None  # (the same expansion: one carve)
    # an explicit cap never meets it: the query of the largest expansion has the largest C too
    _, launch, why = plan([-1, -1], [(1, e_a), (1, e_b + 1)], **{**over, "cand_cap": 300})
    assert why is None and launch["walk"]["cand_cap"] == e_a
    # the exact path has no joint refusal: its carve is its largest query's
    _, launch, why = plan([30, 30], [(9000, 1), (1, 1, 8999)], **{**over, "path": 2})
    assert why is None and launch["exact"]["expansion"] == 9000


def test_the_visited_set_follows_the_launch_carve():
    """vis_slots by the uniform call's rule, from the launch's carve: the LDS target of 64 KiB shrinks it as the lists grow."""
    _, small = one(-1, 10, 64)
    assert small["walk"]["vis_slots_or_rows"] == 2048 and small["walk"]["per_cu"] >= 2
    per, launch, why = plan([-1, -1], [(10, 64), (10, 64, 3000)])
    assert why is None
    _, alone = one(-1, 10, 64, 3000)
    assert launch["walk"] == {**alone["walk"], "queries": 2}
    assert launch["walk"]["vis_slots_or_rows"] < 2048
    # the exact launch: rows per round = 2 per group of lanes, 512 threads
    _, e = one(30, 10, 64, path=2)
    assert e["exact"]["vis_slots_or_rows"] > 0 and e["exact"]["vis_slots_or_rows"] % 2 == 0 and e["exact"]["cand_cap"] == 0


def test_null_arrays_are_refused():
    lib = capi.lib()
    a = np.zeros(8, dtype=np.int64)
    launch = np.zeros((2, 6), dtype=np.uint32)
    assert lib.lantern_gpu_plan_filtered_params(None, None, None, 0, None, capi._ptr(launch)) == b"lantern_gpu: null array"
    assert lib.lantern_gpu_plan_filtered_params(capi._ptr(a), None, None, 1, None, capi._ptr(launch)) == b"lantern_gpu: null array"
    assert lib.lantern_gpu_plan_filtered_params(capi._ptr(a), None, None, 0, None, capi._ptr(launch)) is None
