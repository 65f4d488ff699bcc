"""The instantiations of the unfiltered search kernels (k_search: search_kernel.hpp, k_search_adc: search_adc_kernel.hip) that the launchers
reach, and for each of them a way to reach it through the C ABI.  No device: tests/test_search_cells.py pins CELLS to the library's own symbol
table and every recipe to the pure planner; tests/test_gpu_search_cells.py launches every cell and compares it with the oracle and float64.

Test infrastructure, not part of the product.

A CELL is the template argument list of one compiled kernel, (kernel, METRIC, G, PROF, ROWS, KPL, SPEC, EACH) with kernel 1 = k_search and
2 = k_search_adc -- words [0..7] of a row of lantern_gpu_last_search_cells.  k_search_adc has no G, PROF or ROWS: its cells carry G = 8
(the lanes of a code row's group), PROF = ROWS = 0, as the library reports them.

A RECIPE is a dict of the levers of one launch:
  inst     the index: (metric code, G), see INSTANCES
  nq       40 or 64 queries
  waves    lantern_gpu_set_search_shape: 4 (the classic kernel) or 0 (automatic: what lets the latency-bound shapes in)
  env      the switches search_env reads on every call: LANTERN_GPU_SPEC, _LDS_LIST, _PQ_ADC, _ADC_SPEC (absent = unset)
  ef       24 / 100 / 160: one key per lane, two keys per lane, the LDS list
  each     False: lantern_gpu_search_batch_device; True: lantern_gpu_search_batch_params_device with a list inside ONE expansion class
  screen   None, or for the cells that hold the int8 screen's code path: True (an index with a screen) / False (built under
           LANTERN_GPU_SCREEN=0)
LANTERN_GPU_WIDE_ROWS is read once per process: no recipe relies on it.
"""
from __future__ import annotations

import itertools

K_SEARCH, K_SEARCH_ADC = 1, 2
M_COS, M_L2SQ, M_HAMMING, M_COS_B1 = 1, 3, 8, 9  # device_common.hpp
M_F16, M_I8, M_ADC, M_PQD = 100, 200, 400, 600
CODES = (M_COS, M_L2SQ, M_HAMMING, M_COS_B1, M_F16 + M_COS, M_F16 + M_L2SQ, M_I8 + M_COS, M_I8 + M_L2SQ, M_PQD + M_COS, M_PQD + M_L2SQ)
FOUR_ROW_CODES = (M_COS, M_L2SQ, M_HAMMING, M_F16 + M_COS, M_F16 + M_L2SQ, M_PQD + M_COS, M_PQD + M_L2SQ)  # search_launch.hpp: no i8, no cos over b1
ADC_CODES = (M_ADC + M_COS, M_ADC + M_L2SQ)
GS = (8, 16, 32, 64)
SPEC_ROWS = {8: 1, 16: 1, 32: 2, 64: 4}  # search_launch.hpp LGPU_SPEC_ROWS


def _cells():
    out = []
    # classic, two rows in flight
    out += [(K_SEARCH, m, g, 0, 2, kpl, 0, each) for m in CODES for g in GS for kpl in (1, 2, 0) for each in (0, 1)]
    # classic, four rows in flight (the small batch)
    out += [(K_SEARCH, m, 64, 0, 4, kpl, 0, each) for m in FOUR_ROW_CODES for kpl in (1, 2, 0) for each in (0, 1)]
    # latency-bound: spec 1, spec 2, spec 2 per query
    out += [(K_SEARCH, m, g, 0, SPEC_ROWS[g], kpl, spec, each) for m in CODES for g in GS for kpl in (1, 2) for spec, each in ((1, 0), (2, 0), (2, 1))]
    # ADC over the code rows
    out += [(K_SEARCH_ADC, m, 8, 0, 0, kpl, spec, each) for m in ADC_CODES for kpl, spec in ((1, 0), (2, 0), (0, 0), (1, 2), (2, 2)) for each in (0, 1)]
    return out


def _prof_cells():
    out = [(K_SEARCH, m, g, 1, 2, kpl, 0, 0) for m, g in ((M_L2SQ, 64), (M_L2SQ, 16), (M_COS, 64)) for kpl in (1, 2, 0)]
    out += [(K_SEARCH, m, g, 1, rows, 1, spec, 0) for m, g, rows in ((M_L2SQ, 16, 1), (M_L2SQ, 64, 4), (M_COS, 64, 4)) for spec in (1, 2)]
    return out


CELLS = tuple(_cells())
PROF_CELLS = tuple(_prof_cells())
assert len(CELLS) == len(set(CELLS)) == 542 and len(PROF_CELLS) == len(set(PROF_CELLS)) == 15

# ---- the indexes: one per (metric code, G), rows of a ragged width away from the load-block boundaries ---------------------------------
CHUNKS = {8: 9, 16: 49, 32: 97, 64: 193}  # 16-byte chunks of a stored row
N, M, EF_DEFAULT = 500, 8, 24
PQD_SHAPES = {8: (96, 8, 16), 16: (160, 20, 12), 32: (320, 20, 16), 64: (768, 96, 8)}  # G -> (d, subvectors, centroids): whole chunks per subvector
ADC_SHAPES = {M_ADC + M_L2SQ: (60, 6, 10), M_ADC + M_COS: (100, 20, 37)}                # (d, subvectors, centroids): a ragged subvector width


def _instance(m, g):
    """{storage, metric, d, chunks[, S, C]} of the index behind (metric code, G); d = f32 scalars, u32 words for hamming."""
    c = CHUNKS[g]
    metric = "hamming" if m == M_HAMMING else "cos" if m % 100 in (M_COS, M_COS_B1) else "l2sq"
    if m in ADC_CODES:
        d, S, C = ADC_SHAPES[m]
        return {"storage": "adc", "metric": metric, "d": d, "chunks": (d + 3) // 4, "S": S, "C": C}
    if m >= M_PQD:
        d, S, C = PQD_SHAPES[g]
        return {"storage": "pqd", "metric": metric, "d": d, "chunks": d // 4, "S": S, "C": C}
    if m >= M_I8:
        return {"storage": "i8", "metric": metric, "d": 16 * c - 5, "chunks": c}
    if m >= M_F16:
        return {"storage": "f16", "metric": metric, "d": 8 * c - 3, "chunks": c}
    if m == M_COS_B1:
        return {"storage": "b1", "metric": metric, "d": 128 * c - 37, "chunks": c}
    return {"storage": "f32", "metric": metric, "d": 4 * c - 1, "chunks": c}  # (hamming: 4c - 1 words)


INSTANCES = {(m, g): _instance(m, g) for m, g in itertools.product(CODES, GS)}
INSTANCES.update({(m, 8): _instance(m, 8) for m in ADC_CODES})
assert len(INSTANCES) == 42


def instance_id(key):
    i = INSTANCES[key]
    return f"{i['storage']}-{i['metric']}-m{key[0]}-G{key[1]}"


def group_lanes_for(chunks):
    """device_common.hpp"""
    return 64 if chunks >= 128 else 32 if chunks >= 64 else 16 if chunks >= 32 else 8


for (_m, _g), _i in INSTANCES.items():
    assert _i["storage"] == "adc" or group_lanes_for(_i["chunks"]) == _g, (_m, _g, _i)

EF_OF_KPL = {1: 24, 2: 100, 0: 160}


def holds_screen_path(cell):
    """search_kernel.hpp SCREEN: the instantiations that contain the int8 screen's code beside the plain walk's"""
    kernel, m, g, prof, rows, kpl, spec, each = cell
    return kernel == K_SEARCH and m in (M_L2SQ, M_COS) and g == 64 and not prof and spec == 0 and kpl > 0


def has_screen(r):
    """None: the recipe's index is of a kind that never has an int8 screen; else whether it has one (index.cpp: f32 l2sq / cos rows of >= 128
    chunks, unless it was made under LANTERN_GPU_SCREEN=0)."""
    m, g = r["inst"]
    return r["screen"] is not False if m in (M_L2SQ, M_COS) and g == 64 else None


def _recipe(cell, **kw):
    r = {"inst": (cell[1], cell[2]), "nq": 40, "waves": 4, "env": {}, "ef": EF_OF_KPL[cell[5]], "each": bool(cell[7]), "screen": None}
    r.update(kw)
    return r


def recipes(cell):
    """Every recipe of a cell of CELLS, the plainest first."""
    kernel, m, g, prof, rows, kpl, spec, each = cell
    assert cell in CELLS
    out = []
    if kernel == K_SEARCH_ADC:
        env = {"LANTERN_GPU_PQ_ADC": "1", "LANTERN_GPU_ADC_SPEC": "1" if spec else "0"}
        out.append(_recipe(cell, waves=0, env=env))
        if kpl == 0:  # the second way into the LDS list
            out.append(_recipe(cell, waves=0, env=dict(env, LANTERN_GPU_LDS_LIST="1"), ef=EF_OF_KPL[1]))
        return out
    if spec:
        return [_recipe(cell, waves=0, env={"LANTERN_GPU_SPEC": str(spec)})]
    out.append(_recipe(cell, nq=64 if rows == 4 else 40))
    if kpl == 0:
        out.append(_recipe(cell, nq=64 if rows == 4 else 40, env={"LANTERN_GPU_LDS_LIST": "1"}, ef=EF_OF_KPL[1]))
    if rows == 2 and g == 64 and m not in FOUR_ROW_CODES:  # a four-row launch is planned and falls through to the two-row kernel
        out.append(_recipe(cell, nq=64))
    if holds_screen_path(cell):  # both code paths of the instantiation
        out = [dict(r, screen=s) for r in out for s in (True, False)]
    return out


def recipe(cell):
    return recipes(cell)[0]


def cell_of(r):
    """The launcher's rule, restated: the cell a recipe must land on (search_plan.cpp plan_search, search_launch.hpp, search_adc_kernel.hip)."""
    m, g = r["inst"]
    env, ef, each = r["env"], r["ef"], int(r["each"])
    lds_list = env.get("LANTERN_GPU_LDS_LIST", "0") != "0"
    kpl = 0 if lds_list else 1 if ef <= 64 else 2 if ef <= 128 else 0
    if m in ADC_CODES:
        assert env.get("LANTERN_GPU_PQ_ADC") == "1"
        spec = 2 if r["waves"] <= 0 and ef <= 128 and not lds_list and env.get("LANTERN_GPU_ADC_SPEC", "0") != "0" else 0
        return (K_SEARCH_ADC, m, 8, 0, 0, kpl, spec, each)
    spec = 0
    if r["waves"] <= 0 and ef <= 128 and not lds_list and "LANTERN_GPU_SPEC" in env:
        spec = int(env["LANTERN_GPU_SPEC"])
        if each:
            spec = 2 if spec >= 2 else 0
    if spec:
        return (K_SEARCH, m, g, 0, SPEC_ROWS[g], kpl, spec, each)
    wide = r["nq"] >= 64 and r["nq"] * 4 <= 16 * 16  # true from 16 CUs up at four waves per query
    rows = 4 if wide and g == 64 and m in FOUR_ROW_CODES else 2
    return (K_SEARCH, m, g, 0, rows, kpl, 0, each)


# ---- what the pure planner must say of a recipe --------------------------------------------------------------------------------------
PATH_ADC, PATH_PQD, PATH_CLASSIC, PATH_SPEC1, PATH_SPEC2 = 0, 1, 2, 3, 4  # index.hpp SearchPath


def params_of(r):
    """The (k, ef, skip) rows of a per-query recipe: k in {1, 5, 10}, skip in {0, 3}, ef the class's top, a smaller one inside the class, or
    (first class only: the index's default lies in it) 0.  Every list holds its class's top, so the launch is carved for r["ef"]."""
    top = r["ef"]
    efs = (top, 0, top - 7) if top == EF_DEFAULT else (top, top - 7)
    grid = [(k, ef, skip) for skip in (0, 3) for ef in efs for k in (1, 5, 10)]
    return [grid[i % len(grid)] for i in range(r["nq"])]


def plan_fields(r, num_cus):
    """capi.plan_search's input for a recipe on a machine of num_cus compute units."""
    m, g = r["inst"]
    i, env = INSTANCES[(m, g)], r["env"]
    pq = i["storage"] in ("pqd", "adc")
    s16 = 0
    if pq:
        s16 = (i["S"] + 15) // 16 * 16
        s16 = 128 if 64 < s16 < 128 else s16
    f = {"chunks": i["chunks"], "M": M, "M0": 2 * M, "mcode": m % 100 if pq else m, "n": N, "ef_default": EF_DEFAULT, "num_cus": num_cus,
         "pq_compact": int(pq), "pqd_inv": 1 if i["storage"] == "pqd" else 0, "pq_S16": s16, "search_vis_slots": -1, "search_max_wg": 0,
         "phase_profile": 0, "spec_profile": 0, "nq": r["nq"], "k": 10, "ef": 0 if r["each"] else r["ef"], "skip": 0, "waves": r["waves"],
         "each": int(r["each"]), "max_expansion": r["ef"] if r["each"] else 0,
         "env_spec_set": int("LANTERN_GPU_SPEC" in env), "env_spec": int(env.get("LANTERN_GPU_SPEC", 0)),
         "env_adc_spec_set": int("LANTERN_GPU_ADC_SPEC" in env), "env_adc_spec": int(env.get("LANTERN_GPU_ADC_SPEC", 0)),
         "env_pq_adc": int(env.get("LANTERN_GPU_PQ_ADC", 0)), "env_spec_waves": 0, "env_lds_list": int(env.get("LANTERN_GPU_LDS_LIST", 0)),
         "env_wide_rows": -1, "reserved_29": 0, "env_waves_per_cu": 0}
    if has_screen(r) is not None:
        f["screen"] = int(has_screen(r))
    return f


def plan_claim(r):
    """{path, spec, wide_rows, lds_list, expansion[, screens]} the planner must answer for a recipe, derived from the cell it lands on."""
    kernel, m, g, prof, rows, kpl, spec, each = cell_of(r)
    lds_list = int(r["env"].get("LANTERN_GPU_LDS_LIST", "0") != "0")
    if kernel == K_SEARCH_ADC:
        path = PATH_ADC
    elif m >= M_PQD:
        path = PATH_PQD
    else:
        path = {0: PATH_CLASSIC, 1: PATH_SPEC1, 2: PATH_SPEC2}[spec]
    wide = int(kernel == K_SEARCH and spec == 0 and r["nq"] >= 64)  # (planned for every kind: the launcher falls through where it has no four rows)
    claim = {"path": path, "spec": spec, "wide_rows": wide, "lds_list": lds_list, "expansion": r["ef"]}
    if has_screen(r) is not None:  # the launch screens only in the cells that hold the screen's code path, on an index that has a screen
        claim["screens"] = bool(r["screen"])
    return claim
