"""lantern_gpu_compact_deleted at the C boundary and its arithmetic, without a device: the exports exist, the binding covers them, bad
handles are refused before any device use, and lantern_gpu_plan_compact equals the numpy restatement (tests/compact_ref.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import compact_ref

NAMES = ("lantern_gpu_compact_deleted", "lantern_gpu_plan_compact")


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def test_exports_exist_and_the_binding_covers_them(capi):
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in capi.EXPORTS
    assert [n for n, _ in capi.CompactStats._fields_] == ["unlink", "rows_before", "rows_after", "upper_blocks_before", "upper_blocks_after",
                                                          "bytes_before", "bytes_after", "bytes_moved"]
    assert C.sizeof(capi.CompactStats) == 56 + 7 * 8 == 112
    assert hasattr(capi.GpuIndex, "compact_deleted") and hasattr(capi, "plan_compact")


def test_null_and_foreign_handles_are_refused(capi):
    L = capi.lib()
    foreign = C.create_string_buffer(4096)  # readable memory that is no index
    slot_map = (C.c_uint32 * 4)(9, 9, 9, 9)
    for handle, text in ((None, b"null index handle"), (C.cast(foreign, C.c_void_p), b"not an index handle")):
        err, st = C.c_char_p(), capi.CompactStats()
        st.bytes_moved, st.unlink.offers = 5, 6
        L.lantern_gpu_compact_deleted(handle, 0, slot_map, C.byref(st), C.byref(err))
        assert text in err.value and bytes(st) == bytes(112) and list(slot_map) == [9, 9, 9, 9]
        err = C.c_char_p()
        L.lantern_gpu_compact_deleted(handle, 10, None, None, C.byref(err))  # null outputs are accepted: the refusal is still the handle's
        assert text in err.value
        L.lantern_gpu_compact_deleted(handle, 0, None, None, None)  # and a null error slot


def patterns(n, rng):
    every = np.arange(n)
    yield "nothing dead", every[:0]
    yield "everything dead", every
    yield "first and last", np.unique([0, n - 1])
    yield "alternating", every[::2]
    yield "alternating, odd slots", every[1::2]
    yield "one long run", every[n // 4:n // 4 + max(1, n // 2)]
    yield "random 30 %", rng.choice(n, max(1, n * 3 // 10), replace=False)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_plan_equals_the_numpy_restatement(capi, n):
    rng = np.random.default_rng(n)
    levels = np.minimum(rng.geometric(0.5, n) - 1, 5).astype(np.uint8)  # about half the nodes have upper blocks, an eighth has level >= 3
    labels = (np.arange(n, dtype=np.uint64) * 7 + 1) | (np.uint64(1) << np.uint64(40))
    for name, dead in patterns(n, rng):
        lab, lev = labels.copy(), levels.copy()
        lab[dead] = 0
        if dead.size and dead.size < n:
            lev[dead[:3]] = [4, 2, 3][:min(3, dead.size)]  # nodes of level >= 2 among the dead: upper_off shifts by more than a block
            assert lev[dead].max() >= 2
        want_map, want_off, want_live, want_blocks = compact_ref.plan(lab, lev)
        got_map, got_off, live, blocks = capi.plan_compact(lab, lev)
        assert (live, blocks) == (want_live, want_blocks) == (n - dead.size, int(lev[lab != 0].sum())), name
        assert np.array_equal(got_map, want_map) and np.array_equal(got_off, want_off), name
        # the definition itself, not only the restatement: stable, dense, dead slots unmapped
        keep = np.flatnonzero(lab != 0)
        assert np.array_equal(got_map[keep], np.arange(keep.size)) and (got_map[dead] == compact_ref.EMPTY).all(), name
        assert got_off.size == keep.size and (keep.size == 0 or got_off[0] == 0), name


def test_plan_takes_null_outputs_and_refuses_null_inputs(capi):
    L = capi.lib()
    lab, lev = (C.c_uint64 * 3)(5, 0, 6), (C.c_uint8 * 3)(1, 2, 3)
    err, live, blocks = C.c_char_p(), C.c_uint64(9), C.c_uint64(9)
    L.lantern_gpu_plan_compact(lab, lev, 3, None, None, C.byref(live), C.byref(blocks), C.byref(err))
    assert err.value is None and (live.value, blocks.value) == (2, 4)
    L.lantern_gpu_plan_compact(None, lev, 3, None, None, C.byref(live), C.byref(blocks), C.byref(err))
    assert b"null label or level array" in err.value and (live.value, blocks.value) == (0, 0)
    err = C.c_char_p()
    L.lantern_gpu_plan_compact(None, None, 0, None, None, C.byref(live), None, C.byref(err))  # n == 0: nothing to read
    assert err.value is None and live.value == 0


def test_restatement_of_the_whole_renumbering_on_a_small_graph():
    """compact_ref.compact on a graph worked out by hand: 5 slots, slots 1 and 3 deleted, M = 2."""
    E = compact_ref.EMPTY
    g = {
        "labels": np.array([10, 0, 30, 0, 50], dtype=np.uint64), "levels": np.array([0, 2, 1, 0, 1], dtype=np.uint8),
        "nbr0": np.array([[2, 4, E, E], [E, E, E, E], [4, 0, E, E], [E, E, E, E], [0, 2, E, E]], dtype=np.uint32),
        "upper_off": np.array([E, 0, 2, E, 3], dtype=np.uint32),
        "upper_nbr": np.array([[E, E], [E, E], [4, E], [2, E]], dtype=np.uint32), "entry_slot": 4, "max_level": 1,
    }
    rows = np.arange(10, dtype=np.float32).reshape(5, 2)
    out, live_rows, slot_map = compact_ref.compact(g, rows)
    assert slot_map.tolist() == [0, E, 1, E, 2] and live_rows.tolist() == [[0, 1], [4, 5], [8, 9]]
    assert out["labels"].tolist() == [10, 30, 50] and out["levels"].tolist() == [0, 1, 1] and out["upper_off"].tolist() == [0, 0, 1]
    assert out["nbr0"].tolist() == [[1, 2, E, E], [2, 0, E, E], [0, 1, E, E]] and out["upper_nbr"].tolist() == [[2, E], [1, E]]
    assert (out["entry_slot"], out["max_level"]) == (2, 1)
    g["nbr0"][0, 0] = 1  # a live list that names a tombstone is not a state the compaction accepts
    with pytest.raises(AssertionError, match="names a tombstone"):
        compact_ref.compact(g)
