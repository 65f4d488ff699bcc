"""The ledger of the unfiltered search kernels' instantiations (tests/search_cells.py), without a device:
  * the k_search / k_search_adc host stubs in the built library are exactly CELLS and PROF_CELLS -- an instantiation added without a row fails
    here, and so does a row for an instantiation that does not exist;
  * every cell has a recipe, and the restated launcher rule puts every recipe on its cell;
  * the pure planner (lantern_gpu_plan_search*) accepts every recipe and answers the path, spec, wide_rows, lds_list, expansion and screen
    the recipe claims, on machines of 32, 64, 256 and 304 compute units.
tests/test_gpu_search_cells.py launches every recipe on the device.
"""
import re
import shutil
import subprocess

import pytest

from tests import search_cells as sc

STUB = re.compile(r"\b(k_search|k_search_adc)<([^<>]*)>")


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def _arg(text):
    text = re.sub(r"^\((?:int|bool)\)", "", text.strip())
    return {"true": 1, "false": 0}[text] if text in ("true", "false") else int(text)


def library_cells(path):
    """The instantiations of k_search and k_search_adc in the library's symbol table, as cells with the templates' defaults filled in."""
    nm = shutil.which("nm")
    assert nm, "nm (binutils) is needed to read the library's symbol table"
    text = subprocess.run([nm, "-C", path], check=True, capture_output=True, text=True).stdout
    cells = set()
    for name, args in STUB.findall(text):
        a = [_arg(x) for x in args.split(",")]
        if name == "k_search":  # <METRIC, G, PROF = false, ROWS = 2, KPL = 1, SPEC = 0, EACH = false>
            a += [0, 2, 1, 0, 0][len(a) - 2:]
            assert len(a) == 7, args
            cells.add((sc.K_SEARCH, *a))
        else:  # <METRIC, KPL, SPEC = 0, EACH = false>
            a += [0, 0][len(a) - 2:]
            assert len(a) == 4, args
            cells.add((sc.K_SEARCH_ADC, a[0], 8, 0, 0, a[1], a[2], a[3]))
    return cells


def test_the_library_holds_exactly_the_cells_of_the_ledger(capi):
    got = library_cells(capi.LIB_PATH)
    want = set(sc.CELLS) | set(sc.PROF_CELLS)
    assert len(want) == 542 + 15
    missing, extra = sorted(want - got), sorted(got - want)
    assert not missing, f"{len(missing)} cells of the ledger are not in the library, first {missing[:5]}"
    assert not extra, f"{len(extra)} instantiations in the library have no row in the ledger, first {extra[:5]}"
    assert len([c for c in got if c[0] == sc.K_SEARCH]) == 537 and len([c for c in got if c[0] == sc.K_SEARCH_ADC]) == 20


def test_every_cell_has_recipes_that_land_on_it():
    for cell in sc.CELLS:
        rs = sc.recipes(cell)
        assert rs and sc.recipe(cell) == rs[0]
        for r in rs:
            assert sc.cell_of(r) == cell, (cell, r)
            assert r["inst"] in sc.INSTANCES and r["nq"] in (40, 64) and r["ef"] in (24, 100, 160)
            assert "LANTERN_GPU_WIDE_ROWS" not in r["env"]
            if r["each"]:  # one expansion class, carved for the class's top
                exp = [max(ef or sc.EF_DEFAULT, k + skip) for k, ef, skip in sc.params_of(r)]
                cls = {0 if e <= 64 else 1 if e <= 128 else 2 for e in exp}
                assert len(cls) == 1 and max(exp) == r["ef"] and len(set(sc.params_of(r))) >= 12
    # the levers the issue names are all used somewhere
    every = [r for c in sc.CELLS for r in sc.recipes(c)]
    assert any(r["env"].get("LANTERN_GPU_LDS_LIST") == "1" for r in every)
    assert any(r["nq"] == 64 and sc.cell_of(r)[4] == 2 for r in every)  # the four-row plan that falls through to two rows
    assert {r["screen"] for r in every} == {None, True, False}
    assert sum(sc.holds_screen_path(c) for c in sc.CELLS) == 16  # 2 metrics x ROWS {2, 4} x KPL {1, 2} x EACH {0, 1}


@pytest.mark.parametrize("num_cus", [32, 64, 256, 304])
def test_the_planner_agrees_with_every_recipe(capi, num_cus):
    for cell in sc.CELLS:
        for r in sc.recipes(cell):
            plan, refusal = capi.plan_search(sc.plan_fields(r, num_cus))
            assert refusal is None, (cell, r, refusal)
            claim = sc.plan_claim(r)
            screens = claim.pop("screens", None)
            assert {k: plan[k] for k in claim} == claim, (cell, r, plan)
            if screens is not None:
                assert (plan["screen_lds"] != 0) == screens, (cell, r, plan)
            assert plan["took_spec"] == int(claim["spec"] != 0)


def test_the_record_of_launches_is_empty_without_a_launch(capi):
    import numpy as np

    made, cells = capi.last_search_cells()
    assert made == 0 and cells == []
    assert capi.lib().lantern_gpu_last_search_cells(None, 0) == 0
    out = np.full(10, 7, dtype=np.uint32)
    assert capi.lib().lantern_gpu_last_search_cells(out.ctypes.data, 1) == 0 and np.all(out == 7)
