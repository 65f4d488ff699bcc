"""lantern_gpu_plan_filtered_compact: the plan of a filtered call on a compact pq index served under lantern_gpu_set_filter_compact, as a
pure function (include/lantern_gpu.h; DESIGN.md 4.9 "Compact pq indexes").  No device.

The entry points plan through this function, so what is asserted here is what launches.  Rows decoded on the fly plan as the expanded
index does, field for field; ADC puts the per-query table (16 KiB per code chunk) in front of everything else in the same 160 KiB.
"""
import numpy as np
import pytest

from lantern_amd import capi

LDS = 160 * 1024
FACTOR = 5.6
WALK_OVER = "lantern_gpu: ef/k exceed the 160 KiB LDS budget of the filtered search kernel"
EXACT_OVER = "lantern_gpu: k + skip exceed the 160 KiB LDS budget of the exact filtered search kernel"
# 256-d rows in 128 subvectors (8 code chunks: the 128 KiB table), M = 16
BIG = {"chunks": 64, "M0": 32, "n": 1200, "ef_default": 64, "path": 0, "cand_cap": 0, "exact_factor": FACTOR, "seeds": 0, "code_chunks": 8}
# 60-d rows in 6 subvectors (1 code chunk), M = 4
SMALL = {"chunks": 15, "M0": 8, "n": 1500, "ef_default": 100, "path": 0, "cand_cap": 0, "exact_factor": FACTOR, "seeds": 0, "code_chunks": 1}


def up16(x):
    return (x + 15) // 16 * 16


def walk_lds(f, e, C, vis):
    """table | raw query row | top and its merge target | a hop's new keys, their sorted copy and ids | scalars | visited set | next and its merge target"""
    M0 = f["M0"]
    return f["code_chunks"] * 16384 + f["chunks"] * 16 + 2 * up16(8 * e) + 2 * up16(8 * M0) + up16(4 * M0) + 112 + 4 * vis + 16 + 16 * C


def exact_lds(f, kk, rows=64):
    return f["code_chunks"] * 16384 + f["chunks"] * 16 + 2 * up16(8 * kk) + 2 * up16(8 * rows) + up16(4 * rows) + 112


def plan(fields, counts, params, **over):
    return capi.plan_filtered_compact({**fields, **over}, counts, params)


def test_the_decode_path_plans_as_the_expanded_index_field_for_field():
    rng = np.random.default_rng(3)
    counts = [int(c) for c in rng.choice([-1, 0, 1, 30, 300, 1000, 3000], size=40)]
    params = [(int(rng.choice([0, 1, 5, 10, 300])), int(rng.choice([0, 1, 32, 64, 65, 400, 1200])), int(rng.choice([0, 0, 10, 1500]))) for _ in counts]
    for over in ({}, {"path": 1}, {"path": 2}, {"cand_cap": 90}, {"chunks": 192, "M0": 64}, {"chunks": 6, "M0": 16}, {"seeds": 16}):
        f = {"chunks": 32, "M0": 32, "n": 3000, "ef_default": 64, "path": 0, "cand_cap": 0, "exact_factor": FACTOR, "seeds": 0, **over}
        per, launch, why = capi.plan_filtered_compact({**f, "code_chunks": 0}, counts, params)
        per0, launch0, why0 = capi.plan_filtered_params(f, counts, params)
        assert why == why0 is None
        assert per == per0
        for name in ("walk", "exact"):
            assert launch[name].pop("table_bytes") == 0
            assert launch[name] == launch0[name]
    # ... and is refused where, and as, the expanded index is
    for bad in ([(10**5, 10**5, 0)], [(10, 64, 0), (10**5, 64, 0), (10**5, 10**5, 0)]):
        f = {"chunks": 32, "M0": 32, "n": 3000, "ef_default": 64, "path": 0, "cand_cap": 0, "exact_factor": FACTOR, "seeds": 0}
        for forced in (1, 2):
            a = capi.plan_filtered_compact({**f, "path": forced, "code_chunks": 0}, [100] * len(bad), bad)[2]
            b = capi.plan_filtered_params({**f, "path": forced}, [100] * len(bad), bad)[2]
            assert a == b and a is not None


def test_adc_the_128_kib_table_leaves_room_for_the_default_search():
    per, launch, why = plan(BIG, [700, 30], [(10, 64, 0), (10, 64, 0)])
    assert why is None
    assert [q["path"] for q in per] == [1, 2]  # 30^2 <= 5.6 * 64 * 1200 < 700^2
    w, x = launch["walk"], launch["exact"]
    assert w["table_bytes"] == x["table_bytes"] == 8 * 16384
    assert (w["expansion"], w["cand_cap"]) == (64, 256) and w["vis_slots_or_rows"] == 2048
    assert w["lds"] == walk_lds(BIG, 64, 256, 2048) <= LDS
    assert x["expansion"] == 10 and x["vis_slots_or_rows"] == 64  # two rows per 8-lane group of four waves
    assert x["lds"] == exact_lds(BIG, 10) <= LDS
    assert w["per_cu"] == x["per_cu"] == 1  # 2 x LDS > 160 KiB


def test_adc_one_code_chunk():
    per, launch, why = plan(SMALL, [1000, 20, -1, 0], [(10, 0, 0), (10, 0, 0), (5, 0, 2), (10, 0, 0)])
    assert why is None
    assert [q["path"] for q in per] == [1, 2, 1, 0]
    w, x = launch["walk"], launch["exact"]
    assert w["table_bytes"] == x["table_bytes"] == 16384
    assert (w["expansion"], w["cand_cap"], w["vis_slots_or_rows"]) == (100, 400, 2048)
    assert w["lds"] == walk_lds(SMALL, 100, 400, 2048)
    assert x["lds"] == exact_lds(SMALL, 10)
    assert w["per_cu"] == min(4, LDS // w["lds"]) >= 2 and x["per_cu"] == 4
    assert "a code row has 1 to 8 chunks" in plan(SMALL, [1], [(1, 1, 0)], code_chunks=9)[2]


@pytest.mark.parametrize("fields", [BIG, SMALL, {**BIG, "code_chunks": 6, "chunks": 192}], ids=["128KiB", "16KiB", "96KiB"])
def test_adc_table_bytes_and_the_budget(fields):
    for e in (1, 64, 200, 500):
        per, launch, why = plan(fields, [-1], [(1, e, 0)])
        assert why is None
        w = launch["walk"]
        assert w["table_bytes"] == fields["code_chunks"] * 16384
        assert w["lds"] == walk_lds(fields, e, per[0]["cand_cap"], w["vis_slots_or_rows"]) <= LDS
        assert w["vis_slots_or_rows"] <= 2048 and (w["vis_slots_or_rows"] == 0 or w["vis_slots_or_rows"] >= 4 * fields["M0"])
        if w["vis_slots_or_rows"] < 2048:  # what fits: 256 slots more would not
            assert walk_lds(fields, e, per[0]["cand_cap"], w["vis_slots_or_rows"] + 256) > LDS
        assert w["per_cu"] == max(1, min(4, LDS // w["lds"]))
        assert (w["per_cu"] == 1) == (2 * w["lds"] > LDS)


def test_adc_an_expansion_past_the_room_beside_the_table_is_refused():
    fits = lambda e: walk_lds(BIG, e, e, 0) <= LDS  # noqa: E731 -- next holds at least the expansion
    e = 1
    while fits(e + 1):
        e += 1
    assert 500 < e < 2000
    per, launch, why = plan(BIG, [-1], [(10, e, 0)])
    assert why is None and per[0]["expansion"] == e and per[0]["cand_cap"] >= e
    assert launch["walk"]["lds"] <= LDS and launch["walk"]["vis_slots_or_rows"] == 0  # next took the room: the HBM bitmap alone
    assert plan(BIG, [-1], [(10, e + 1, 0)])[2] == WALK_OVER + " (params[0])"
    assert plan(BIG, [-1, 600], [(10, 64, 0), (e + 1, 0, 0)], path=1)[2] == WALK_OVER + " (params[1])"
    # the same expansion fits an index whose table is smaller
    assert plan(SMALL, [-1], [(10, e + 1, 0)])[2] is None


def test_adc_k_plus_skip_past_the_room_on_the_exact_path_is_refused():
    kk = 1
    while exact_lds(BIG, kk + 1) <= LDS:
        kk += 1
    assert 1000 < kk < 3000
    per, launch, why = plan(BIG, [5], [(kk - 7, 64, 7)])
    assert why is None and per[0]["path"] == 2 and launch["exact"]["expansion"] == kk and launch["exact"]["lds"] == exact_lds(BIG, kk)
    assert plan(BIG, [5], [(kk - 6, 64, 7)])[2] == EXACT_OVER + " (params[0])"
    assert plan(BIG, [5, 5, 5], [(1, 64, 0), (0, 64, 0), (kk + 1, 64, 0)])[2] == EXACT_OVER + " (params[2])"


def test_adc_the_joint_refusal_of_a_params_batch():
    # beside the 128 KiB table a query's automatic C is capped by its room early: expansion 800 gets C 1136, expansion 400 gets 1536 --
    # each fits alone, the joint carve (800 with 1536) does not
    a, b = (10, 800, 0), (10, 400, 0)
    for row in (a, b):
        per, launch, why = plan(BIG, [-1], [row])
        assert why is None and launch["walk"]["lds"] <= LDS
    ca = plan(BIG, [-1], [a])[0][0]["cand_cap"]
    cb = plan(BIG, [-1], [b])[0][0]["cand_cap"]
    assert (ca, cb) == ((LDS - walk_lds(BIG, 800, 0, 0)) // 16, (LDS - walk_lds(BIG, 400, 0, 0)) // 16) == (1136, 1536)
    assert walk_lds(BIG, 800, 1536, 0) > LDS
    why = plan(BIG, [-1, 600], [a, b], path=1)[2]
    assert why is not None and why.endswith("do not fit together: split the batch")
    assert plan(BIG, [-1, 600], [a, (10, 64, 0)], path=1)[2] is None
