"""The list prefetch of the screened search launches (walk.hpp search_level_reg, SearchArgs::list_prefetch) in the plan, without a
device: lantern_gpu_plan_search_screen_prefetch against tests/golden/search_plan_prefetch_cases.json -- rows recorded from the library
of the commit BEFORE the switch existed (lantern_gpu_plan_search_screen for the search launches, lantern_gpu_plan_insert for the
insertion ones).  The switch may set its own field and nothing else: every launch is planned in every other field as it was, a launch
that does not screen (latency-bound, LDS list, instrumented, short rows, f16 / i8 / bit rows, compact pq by either path, an index
without a screen table) never fetches ahead whatever LANTERN_GPU_SCREEN_LIST_PREFETCH says, and the insertion plan has not moved.
(The filtered launches have no plan of their own to show: they read neither the field nor the switch.)"""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_plan_prefetch_cases.json")
SWITCH = (-1, 0, 1)  # LANTERN_GPU_SCREEN_LIST_PREFETCH: unset, 0, 1


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def golden():
    return json.load(open(GOLDEN))


def plan(capi, row, switch):
    f = dict(zip(capi.PLAN_SEARCH_IN, row["in"]), screen=row["screen"], screen_list_prefetch=switch)
    return capi.plan_search(f)


def test_the_committed_rows_cover_the_launches_the_switch_must_not_reach():
    rs = golden()["search"]
    paths = {r["out"][0] for r in rs if r["refusal"] is None}
    assert paths >= {0, 1, 2, 3, 4}  # ADC, decode on the fly, classic, spec 1, spec 2
    assert any(r["out"][12] for r in rs) and any(r["screen"] and not r["out"][12] and r["refusal"] is None for r in rs)
    assert any(r["out"][11] for r in rs) and any(r["refusal"] for r in rs)  # the LDS list; a refusal
    assert len(golden()["insert"]) >= 30


def test_every_field_but_its_own_is_planned_as_before(capi):
    for r in golden()["search"]:
        for switch in SWITCH:
            out, why = plan(capi, r, switch)
            assert why == r["refusal"], (r["tag"], switch)
            if why is not None:
                assert out["expansion"] == r["out"][2] and out["list_prefetch"] == 0, r["tag"]
                continue
            assert [out[n] for n in capi.PLAN_SEARCH_OUT + ("screen_lds",)] == r["out"], (r["tag"], r["screen"], switch)


def test_only_a_launch_that_screens_fetches_ahead_and_the_switch_decides(capi):
    on_by_default = None
    for r in golden()["search"]:
        if r["refusal"] is not None:
            continue
        got = {s: plan(capi, r, s)[0]["list_prefetch"] for s in SWITCH}
        screens, M0 = r["out"][12] != 0, r["in"][2]
        if not screens or M0 > 64:  # (a list of more than 64 entries is no single request of the visit wave)
            assert got == {-1: 0, 0: 0, 1: 0}, (r["tag"], r["screen"], got)
            continue
        assert got[0] == 0 and got[1] == 1 and got[-1] in (0, 1), (r["tag"], got)
        assert on_by_default in (None, got[-1]), r["tag"]  # one default for every screened launch
        on_by_default = got[-1]
    assert on_by_default is not None


def test_the_older_entry_points_answer_as_before(capi):
    for r in golden()["search"]:
        f = dict(zip(capi.PLAN_SEARCH_IN, r["in"]), screen=r["screen"])
        out, why = capi.plan_search(f)
        assert why == r["refusal"]
        if why is None:
            assert [out[n] for n in capi.PLAN_SEARCH_OUT + ("screen_lds",)] == r["out"], r["tag"]
            assert "list_prefetch" not in out
        if not r["screen"] and why is None:
            assert [capi.plan_search(r["in"])[0][n] for n in capi.PLAN_SEARCH_OUT] == r["out"][:12], r["tag"]


def test_the_insertion_launches_are_planned_as_before(capi):
    for r in golden()["insert"]:
        out, why = capi.plan_insert(r["in"])
        assert why == r["refusal"] and [out[n] for n in capi.PLAN_INSERT_OUT] == r["out"], r["tag"]


def test_the_symbol_is_exported_and_bound(capi):
    import ctypes as C

    raw = C.CDLL(capi.LIB_PATH)
    name = "lantern_gpu_plan_search_screen_prefetch"
    assert hasattr(raw, name) and name in capi.EXPORTS and getattr(capi.lib(), name).argtypes is not None
    assert capi.lib().lantern_gpu_plan_search_screen_prefetch(None, None) == b"lantern_gpu: null array"
