"""The shape of the unfiltered search launch, without a device: lantern_gpu_plan_search (csrc/search_plan.cpp plan_search) against
tests/golden/search_plan_cases.json -- rows recorded from a sweep in which every launch the planned code made was compared, kernel
argument by kernel argument, with what the code before the plan existed launched for the same index, call and environment.  A row is
{"in": the 31 input fields, "out": the 12 output fields, "refusal": the text or null, "tag": what the row is there for}."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_plan_cases.json")
REFUSAL_WALK = "lantern_gpu: ef/k exceed the 160 KiB LDS budget of the search kernel"
REFUSAL_ADC = "lantern_gpu: ef/k exceed the 160 KiB LDS budget of the ADC search kernel"
PATHS = {"adc": 0, "pqd": 1, "classic": 2, "spec1": 3, "spec2": 4}


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def rows():
    return json.load(open(GOLDEN))


def test_the_committed_rows_cover_every_path_and_refusal():
    rs = rows()
    assert len(rs) >= 40
    assert {r["out"][0] for r in rs if r["refusal"] is None} == set(PATHS.values())
    assert {r["refusal"] for r in rs} == {None, REFUSAL_WALK, REFUSAL_ADC}
    assert any(r["in"][19] and r["refusal"] for r in rs) and any(r["in"][19] and r["refusal"] is None for r in rs)  # the per-query form
    assert all(len(r["in"]) == 31 and len(r["out"]) == 12 for r in rs)


def test_plan_search_reproduces_the_committed_rows(capi):
    checked = 0
    for r in rows():
        out, why = capi.plan_search(r["in"])
        assert why == r["refusal"], r
        if why is None:
            assert [out[n] for n in capi.PLAN_SEARCH_OUT] == r["out"], r
        else:
            assert out["expansion"] == r["out"][2], r
        checked += 1
    assert checked == len(rows()) == 88


def test_the_refusal_texts(capi):
    base = dict.fromkeys(capi.PLAN_SEARCH_IN, 0)
    base.update(chunks=192, M=16, M0=32, mcode=3, n=100000, ef_default=64, num_cus=256, search_vis_slots=-1, nq=8192, k=10, env_wide_rows=-1)
    out, why = capi.plan_search(dict(base, ef=20000))
    assert why == REFUSAL_WALK and out["expansion"] == 20000
    assert capi.plan_search(dict(base, each=1, max_expansion=20000))[1] == REFUSAL_WALK
    out, why = capi.plan_search(dict(base, ef=20000, pq_compact=1, pq_S16=96))
    assert why == REFUSAL_ADC
    # ... and an accepted launch of each family: no text
    out, why = capi.plan_search(base)
    assert why is None and out["path"] == PATHS["classic"] and out["expansion"] == 64 and out["waves"] == 4 and out["grid"] == 256 * 6
    out, why = capi.plan_search(dict(base, nq=1, waves=-8))
    assert why is None and out["path"] == PATHS["spec2"] and out["waves"] == 11 and out["grid"] == 1 and out["took_spec"] == 1
    out, why = capi.plan_search(dict(base, pq_compact=1, pq_S16=96))
    assert why is None and out["path"] == PATHS["adc"]
