"""The shape of a batch's k_insert launch, without a device: lantern_gpu_plan_insert (csrc/insert_batch.cpp plan_insert) says which launches
test their level-0 candidates on the int8 row copy, and what the query's int8 planes cost the LDS visited set.  The unscreened
answers are held to the arithmetic run_batch did before the plan existed, restated below; the screened ones to the 31 KB budget.
lantern_gpu_set_insert_screen's argument checks need no device either."""
import ctypes as C

import numpy as np
import pytest

M_COS, M_L2SQ, M_HAMMING, F16, I8 = 1, 3, 8, 100, 200
S_SCALARS = 28  # walk.hpp


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def up16(x):
    return (x + 15) & ~15


def walk_lds_bytes(chunks, ef_cap, cap_max, vis_slots):  # walk.hpp
    return chunks * 16 + 2 * up16(ef_cap * 8) + 2 * up16(cap_max * 8) + up16(cap_max * 4) + S_SCALARS * 4 + vis_slots * 4


def spec_lds_bytes(M0, prefetch, cache_entries):  # walk_spec.hpp
    return 2 * M0 * M0 * 4 + cache_entries * M0 * 4 + up16(cache_entries * 4) if prefetch else 0


def group_lanes_for(chunks):  # device_common.hpp
    return 64 if chunks >= 128 else 32 if chunks >= 64 else 16 if chunks >= 32 else 8


def before_the_plan(f):
    """(lone walk, vis_slots, LDS bytes) as run_batch computed them: the lone walk for a handful of rows of an f32 l2sq / cosine index,
    8192 slots (or the environment's) shrunk 256 at a time to 31 KB (96 KB in the lone shape), none below 4 * M0"""
    lone = bool(f["lone_ok"]) and f["rows"] <= 2 * f["num_cus"] and f["mcode"] in (M_L2SQ, M_COS) and f["efc"] <= 128 and 2 <= f["M0"] <= 64 and not f["lds_list"]
    ivis = 8192 if f["vis_slots_env"] < 0 else f["vis_slots_env"] // 4 * 4
    G = group_lanes_for(f["chunks"])
    LW = 1 if G >= 32 else 2 if G == 16 else 4
    prefetch = 1 if lone and f["M0"] % LW == 0 and f["M0"] <= G * LW else 0
    cache = 128 if prefetch else 0

    def lds(vis):
        return walk_lds_bytes(f["chunks"], f["efc"], f["M0"], vis) + (spec_lds_bytes(f["M0"], prefetch, cache) if lone else 0)

    while ivis and lds(ivis) > (96 if lone else 31) * 1024:
        ivis = ivis - 256 if ivis > 256 else 0
    if ivis and ivis < 4 * f["M0"]:
        ivis = 0
    return lone, ivis, lds(ivis)


def screen_query_lds_bytes(chunks):  # device_common.hpp
    return 16 + (chunks + 3) // 4 * 32


BASE = dict(mcode=M_L2SQ, chunks=192, M0=32, efc=128, rows=4096, num_cus=256, waves=4, screen_table=1, mode=1, lds_list=0, only_upper=0, lone_ok=1,
            vis_slots_env=-1)
SCREENED = [dict(BASE, mcode=m, chunks=c, efc=e) for m in (M_L2SQ, M_COS) for c in (128, 192, 500) for e in (40, 128)]
UNSCREENED = {
    "chunks 127": dict(BASE, chunks=127), "chunks 127 cos": dict(BASE, chunks=127, mcode=M_COS),
    "efc 129": dict(BASE, efc=129), "efc 200": dict(BASE, efc=200), "efc 200 cos": dict(BASE, efc=200, mcode=M_COS),
    "f16 l2sq": dict(BASE, mcode=M_L2SQ + F16), "f16 cos": dict(BASE, mcode=M_COS + F16), "i8 l2sq": dict(BASE, mcode=M_L2SQ + I8),
    "i8 cos": dict(BASE, mcode=M_COS + I8), "hamming": dict(BASE, mcode=M_HAMMING),
    "no table": dict(BASE, screen_table=0), "mode 0": dict(BASE, mode=0), "mode 0 cos efc 40": dict(BASE, mode=0, mcode=M_COS, efc=40),
    "lds_list": dict(BASE, lds_list=1), "only_upper": dict(BASE, only_upper=1, lone_ok=0),
    "lone walk 512 rows": dict(BASE, rows=512), "lone walk 1 row": dict(BASE, rows=1), "lone walk cos efc 40": dict(BASE, rows=300, mcode=M_COS, efc=40),
    "one wave": dict(BASE, waves=1),
    # (and shapes no screen reaches, for the arithmetic alone)
    "short rows": dict(BASE, chunks=32, M0=64, efc=64), "tuned set": dict(BASE, vis_slots_env=1000, mode=0), "no set": dict(BASE, vis_slots_env=0, mode=0),
    "a set smaller than 4 M0": dict(BASE, vis_slots_env=100, mode=0),
}


@pytest.mark.parametrize("f", SCREENED, ids=lambda f: f"m{f['mcode']}-c{f['chunks']}-efc{f['efc']}")
def test_the_qualifying_launches_are_screened_within_the_budget(capi, f):
    out, why = capi.plan_insert(f)
    assert why is None and out["screened"] == 1 and out["lone"] == 0
    planes = screen_query_lds_bytes(f["chunks"])
    assert out["screen_lds"] == planes
    _, vis0, lds0 = before_the_plan(f)
    assert out["lds"] <= 31 * 1024
    assert out["lds"] == walk_lds_bytes(f["chunks"], f["efc"], f["M0"], out["vis_slots"]) + planes
    # the planes come out of the visited set, in its steps of 256 slots: no more of them than the planes' bytes require
    assert out["vis_slots"] % 4 == 0 and vis0 - (planes + 1023) // 1024 * 256 <= out["vis_slots"] <= vis0
    assert out["vis_slots"] >= 4 * f["M0"]  # (every case here keeps a set)
    if out["vis_slots"] < vis0:  # ... and one step more would have fitted only without them
        assert walk_lds_bytes(f["chunks"], f["efc"], f["M0"], out["vis_slots"] + 256) + planes > 31 * 1024


@pytest.mark.parametrize("name", sorted(UNSCREENED))
def test_every_other_launch_is_planned_as_before(capi, name):
    f = UNSCREENED[name]
    out, why = capi.plan_insert(f)
    lone, vis, lds = before_the_plan(f)
    assert why is None and out["screened"] == 0 and out["screen_lds"] == 0, name
    assert (out["lone"], out["vis_slots"], out["lds"]) == (int(lone), vis, lds), name
    if name.startswith("lone walk"):
        assert out["lone"] == 1 and out["spec_prefetch"] == 1 and out["spec_cache"] == 128
    else:
        assert out["lone"] == 0 and out["spec_prefetch"] == 0 and out["spec_cache"] == 0


def test_one_condition_at_a_time(capi):
    """BASE is screened; each single change of UNSCREENED's first block switches it off, and the batch size switches at 2 x CUs"""
    assert capi.plan_insert(BASE)[0]["screened"] == 1
    assert capi.plan_insert(dict(BASE, rows=2 * 256))[0] == dict(capi.plan_insert(dict(BASE, rows=512))[0], lone=1, screened=0)
    assert capi.plan_insert(dict(BASE, rows=2 * 256 + 1))[0]["screened"] == 1
    assert capi.plan_insert(dict(BASE, rows=100, lone_ok=0))[0]["screened"] == 1  # (a rank of a work-sharded build walks no lone walk)
    assert capi.plan_insert(dict(BASE, waves=2))[0]["screened"] == 1
    assert capi.plan_insert(dict(BASE, mode=2))[0]["screened"] == 0  # (the setter refuses it; the plan knows 1 only)


def test_the_refusal_and_null_arrays(capi):
    out, why = capi.plan_insert(dict(BASE, efc=20000, mode=0))
    assert why == "lantern_gpu: ef_construction/dimensions exceed the 160 KiB LDS budget"
    a, o = np.zeros(13, np.int64), np.zeros(7, np.uint32)
    assert capi.lib().lantern_gpu_plan_insert(None, o.ctypes.data_as(C.c_void_p)) == b"lantern_gpu: null array"
    assert capi.lib().lantern_gpu_plan_insert(a.ctypes.data_as(C.c_void_p), None) == b"lantern_gpu: null array"


def test_symbols_are_exported_and_bound(capi):
    raw = C.CDLL(capi.LIB_PATH)
    for name in ("lantern_gpu_set_insert_screen", "lantern_gpu_insert_screen_stats", "lantern_gpu_plan_insert"):
        assert hasattr(raw, name) and name in capi.EXPORTS, name
        assert getattr(capi.lib(), name).argtypes is not None, name
    for wrapper in ("set_insert_screen", "insert_screen_stats"):
        assert callable(getattr(capi.GpuIndex, wrapper))
    assert len(capi.PLAN_INSERT_IN) == 13 and len(capi.PLAN_INSERT_OUT) == 7


def test_set_insert_screen_validates_before_any_device_use(capi):
    junk = C.cast(C.create_string_buffer(8192), C.c_void_p)
    err = C.c_char_p()
    for h in (None, junk):  # a mode that is neither value is refused whatever the handle, with both values named
        for mode in (2, -1, 3, 255):
            capi.lib().lantern_gpu_set_insert_screen(h, mode, C.byref(err))
            assert err.value and b"0 (off)" in err.value and b"1 (on)" in err.value and b"handle" not in err.value, mode
    for mode in (0, 1):  # a valid mode gets as far as the handle
        capi.lib().lantern_gpu_set_insert_screen(None, mode, C.byref(err))
        assert b"null index handle" in err.value
        capi.lib().lantern_gpu_set_insert_screen(junk, mode, C.byref(err))
        assert b"not an index handle" in err.value
    out = np.full(4, 7, np.uint64)
    for h, text in ((None, b"null index handle"), (junk, b"not an index handle")):
        capi.lib().lantern_gpu_insert_screen_stats(h, out.ctypes.data_as(C.c_void_p), C.byref(err))
        assert text in err.value and (out == 0).all()
        out[:] = 7
    capi.lib().lantern_gpu_insert_screen_stats(junk, None, C.byref(err))
    assert b"null array" in err.value
    assert junk.value and C.string_at(junk, 8192) == b"\0" * 8192  # nothing was written through the foreign pointer

