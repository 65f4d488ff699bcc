"""The frame around one new vector's walk (lantern_amd/csrc/insert_frame.hpp), on both kernels that share it.  Needs an MI355X.

The frame's behaviours: (a) more batch members than workgroups -- the next member comes by ticket, or by stride under
LANTERN_GPU_TICKETS=0: the same graph; (b) exact ties at the smallest distance of a level's result: the next level's start is the
tie_mix minimum, not keys[0]; (c) a node whose level is above the graph's max_level: the levels above the old top stay empty and the
entry point moves.  The kernels: k_insert_spec, the lone walk (f32 rows, batches of <= 2 x CUs rows), and k_insert (every f16 batch --
the lone walk has no f16 form -- and f32 batches above 2 x CUs rows, there in its screened instantiation).

Which test pinned which cell before this file (the rest of the cells are pinned here):
  lone walk  (a)  none: a batch of <= CUs rows has a workgroup per member, and no small build has a larger one
             (b)  none on purpose; test_gpu_parity.py::test_build_matches_oracle_edge_for_edge[(l2sq, 300, 5, 2, 10)] by chance
             (c)  test_gpu_scans_and_inserts.py::test_add_with_level_is_usearch_add_at_that_level
  k_insert   (a)  tickets: test_gpu_visited_regimes.py (a grid capped by set_search_shape); LANTERN_GPU_TICKETS=0: none
             (b)  none; (c) none (every caller-drawn level went through an f32 index)
  k_insert, screened: the graph and the counts  test_gpu_insert_screen.py (d >= 509, n = 6000, batches of 2048)
Pinned elsewhere and not here: the b_begin sub-range (test_gpu_sharded_build.py, the work-sharded build), only_upper (the same
file, the row-sharded build), the environment switches (test_gpu_env_switches.py, test_gpu_visited_regimes.py,
test_gpu_visited_undo_probe.py).

Every graph is compared edge for edge with the oracle's batch-synchronous build over the same rows and plan (OracleIndex.add_planned,
OracleIndex.add at a given level), through export_graph, as the build-parity tests of test_gpu_parity.py do.  No tolerance.
insert_screen_stats says which kernel ran: it counts k_insert launches, and the lone walk is not one.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import LABEL0

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
GRAPH_ARRAYS = ("levels", "labels", "upper_off", "nbr0", "upper_nbr")
KINDS = {"f32": "lone walk", "f16": "k_insert"}  # the kernel a SMALL batch takes, by storage


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def same_graph(got, want, what):
    assert got["entry_slot"] == want["entry_slot"] and got["max_level"] == want["max_level"], what
    for name in GRAPH_ARRAYS:
        assert np.array_equal(got[name], want[name]), f"{what}: {name} differs"


def run_steps(ix, rows, steps, plan=None):
    """steps: ("many", lo, hi) -- rows [lo, hi) under the batch plan -- or ("level", i, level) -- row i alone at a caller-drawn level.
    `plan`: the oracle (which takes the plan with every call); None: a device index (which has it set)."""
    labels = np.arange(len(rows), dtype=np.uint64) + LABEL0
    for kind, a, b in steps:
        if kind == "level":
            ix.add(labels[a], rows[a], level=b)
        elif plan:
            ix.add_planned(labels[a:b], rows[a:b], max_batch=plan[0], min_ratio=plan[1])
        else:
            ix.add_many(labels[a:b], rows[a:b])
        if not plan:
            ix.flush()


def oracle_build(oracle, metric, rows, quant, M, efc, plan, steps, cores=1):
    stored, mode = (oracle.round_f16(rows), oracle.SUM_WAVE64_F16) if quant == "f16" else (rows, oracle.SUM_WAVE64)
    ora = oracle.OracleIndex(metric, rows.shape[1], M=M, ef_construction=efc, ef=32, seed=13, sum_mode=mode)
    ora.set_build_threads(cores)
    run_steps(ora, stored, steps, plan)
    return ora


def device_build(capi, metric, rows, quant, M, efc, plan, steps, max_wg=0):
    gpu = capi.GpuIndex(metric, rows.shape[1], M=M, ef_construction=efc, ef=32, seed=13, quantization=quant)
    gpu.set_add_batch(*plan)
    gpu.set_insert_screen(1)  # (the initial mode; only the large f32 case below has launches that qualify)
    if max_wg:
        gpu.set_search_shape(0, max_wg)  # caps k_insert's grid; the lone walk's is min(rows, CUs) whatever the cap
    run_steps(gpu, rows, steps)
    assert len(gpu) == len(rows)
    return gpu


def took(gpu, quant):
    """the kernel the index's batches went through, from the k_insert launch counts: small f32 batches never reach k_insert, f16 batches always do"""
    s = gpu.insert_screen_stats()
    assert s[0] == 0 and s[2] == 0 and s[3] == 0, s  # (rows of 5 chunks, f16 rows: no launch screens)
    assert (s[1] > 0) == (quant == "f16"), (KINDS[quant], s)
    return s


def twin_rows(n, d, seed):
    """n rows of which every one is stored twice, next to its twin: a later row sees the two at the same distance"""
    return np.repeat(np.random.default_rng(seed).standard_normal((n // 2, d), dtype=np.float32), 2, axis=0)


def with_and_without_tickets(capi, monkeypatch, *args, **kw):
    """the same build under the ticket and under LANTERN_GPU_TICKETS=0 (read when an index is made)"""
    monkeypatch.delenv("LANTERN_GPU_TICKETS", raising=False)
    ticket = device_build(capi, *args, **kw)
    monkeypatch.setenv("LANTERN_GPU_TICKETS", "0")
    stride = device_build(capi, *args, **kw)
    monkeypatch.delenv("LANTERN_GPU_TICKETS")
    return ticket, stride


# ---- (a) more batch members than workgroups ----------------------------------------------------------------------------------
def test_k_insert_hands_members_out_by_ticket_or_by_stride(capi, oracle, monkeypatch):
    """f16 rows of 20 dimensions (3 chunks: the 8-lane instantiations): every batch is a k_insert launch of at most 3 workgroups, and from
    64 rows on a batch has 4 .. 25 members"""
    n, d, M, efc, plan = 400, 20, 4, 24, (64, 16)
    rows = twin_rows(n, d, 1)
    steps = [("many", 0, n)]
    want = oracle_build(oracle, "l2sq", rows, "f16", M, efc, plan, steps).export_graph()
    ticket, stride = with_and_without_tickets(capi, monkeypatch, "l2sq", rows, "f16", M, efc, plan, steps, max_wg=3)
    for gpu, what in ((ticket, "ticket"), (stride, "LANTERN_GPU_TICKETS=0")):
        took(gpu, "f16")
        same_graph(gpu.export_graph(), want, what)
    assert ticket.checksum() == stride.checksum()


def test_both_kernels_at_size_with_the_screened_instantiation(capi, oracle, cores, monkeypatch):
    """f32 rows of 512 dimensions (128 chunks), efc 40, batches of at most one sixteenth of the graph: from 4112 rows on a batch has more
    than 256 members -- the lone walk's workgroups are one per CU, so the rest come by ticket -- and from 8208 rows on more than 512 =
    2 x CUs: k_insert, here capped at 3 workgroups, in its screened instantiation (one key per lane of the list wave)."""
    n, d, M, efc, plan = 9800, 512, 8, 40, (1024, 16)
    rows = np.random.default_rng(2).standard_normal((n, d), dtype=np.float32)
    steps = [("many", 0, n)]
    want = oracle_build(oracle, "l2sq", rows, "f32", M, efc, plan, steps, cores).export_graph()
    ticket, stride = with_and_without_tickets(capi, monkeypatch, "l2sq", rows, "f32", M, efc, plan, steps, max_wg=3)
    for gpu, what in ((ticket, "ticket"), (stride, "LANTERN_GPU_TICKETS=0")):
        screened, plain, tested, rejected = gpu.insert_screen_stats()
        print(f"{what}: k_insert launches screened {screened} plain {plain}, rows tested {tested} rejected {rejected}")
        assert screened + plain > 0, "no batch reached k_insert"
        assert screened > 0 and tested > 0 and rejected > 0 and tested >= rejected
        same_graph(gpu.export_graph(), want, what)
    assert ticket.insert_screen_stats() == stride.insert_screen_stats()
    assert ticket.checksum() == stride.checksum()


# ---- (b) exact ties at the smallest distance ---------------------------------------------------------------------------------
@pytest.mark.parametrize("quant", list(KINDS))
def test_the_next_level_starts_at_the_tie_mix_minimum(capi, oracle, quant):
    """every row stored twice; M = 4: a quarter of the nodes have upper levels, whose results hand a start to the level below.  f32 rows
    of 20 dimensions are 5 chunks, f16 rows 3: the 8-lane instantiations."""
    n, d, M, efc, plan = 400, 20, 4, 24, (64, 16)
    rows = twin_rows(n, d, 3)
    steps = [("many", 0, n)]
    want = oracle_build(oracle, "l2sq", rows, quant, M, efc, plan, steps).export_graph()
    assert np.count_nonzero(want["levels"]) >= n // 8, "too few nodes with an upper level for the tie rule to matter"
    gpu = device_build(capi, "l2sq", rows, quant, M, efc, plan, steps)
    took(gpu, quant)
    same_graph(gpu.export_graph(), want, KINDS[quant])


# ---- (c) a node above the graph's top level ----------------------------------------------------------------------------------
@pytest.mark.parametrize("quant", list(KINDS))
def test_a_node_above_the_top_level_leaves_the_new_levels_empty(capi, oracle, quant):
    n, more, d, M, efc, plan = 300, 100, 20, 4, 24, (64, 16)
    rows = twin_rows(n + more + 2, d, 4)[: n + more + 1]
    before = oracle_build(oracle, "l2sq", rows[:n], quant, M, efc, plan, [("many", 0, n)])
    top = before.max_level
    assert top >= 1
    steps = [("many", 0, n), ("level", n, top + 2)]
    gpu = device_build(capi, "l2sq", rows[: n + 1], quant, M, efc, plan, steps)
    g = gpu.export_graph()
    same_graph(g, oracle_build(oracle, "l2sq", rows[: n + 1], quant, M, efc, plan, steps).export_graph(), KINDS[quant])
    assert g["entry_slot"] == n and g["max_level"] == top + 2 and g["levels"][n] == top + 2
    lists = g["upper_nbr"][g["upper_off"][n]: g["upper_off"][n] + top + 2]  # the node's lists of levels 1 .. top + 2
    assert np.all(lists[top:] == EMPTY), "a level above the old top is not empty"
    assert np.all(lists[:top, 0] != EMPTY), "a level the graph had was not linked"
    # ... and the build goes on from the new entry point
    steps.append(("many", n + 1, n + 1 + more))
    gpu = device_build(capi, "l2sq", rows, quant, M, efc, plan, steps)
    took(gpu, quant)
    same_graph(gpu.export_graph(), oracle_build(oracle, "l2sq", rows, quant, M, efc, plan, steps).export_graph(), KINDS[quant] + ", the build after")
