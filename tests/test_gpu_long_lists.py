"""Neighbour lists of 62 .. 160 entries (M 31 .. 80, M0 = 2 M): the build's reverse-link kernels and the search walks, held to the oracle
edge for edge and bit for bit.  Needs an MI355X.

The rest of the suite compares builds with the oracle almost only at M <= 16.  Past that, k_revlink_staged (kernels.hip) changes twice:
a list longer than 62 entries has no chain mode (every request to a full list is a full re-prune), and its heuristic keeps the kept
entries x, x + 64, x + 128 of lane x in kpos[0 .. 2], so slots 1 and 2 carry anything only when a re-prune keeps more than 64 or 128
entries.  k_connect takes its refine() branch for M > 16, and a search on M0 > 64 is the classic walk with more than one wave-pass per
list.  The cases below are the smallest at which the ORACLE's graph has full lists of each length; every case first asserts that on
the oracle alone, and that launch_revlink sends the shape to the class the case is here for.

Two data families: Gaussian rows (tests/test_gpu_delete.make_rows) and `hubs` -- a few rows near the origin, the rest on the unit
sphere.  A sphere row is nearer a hub (about 1) than any other sphere row (about 2), so every later row links to a hub, the hub's list
overflows, and the heuristic keeps the whole of it: long kept lists, which Gaussian rows give only by the handful.

No tolerance anywhere: lists in order, the entry, max_level, labels, distance bits, D and E."""
import numpy as np
import pytest

from tests.filtered_regimes import stored_rows
from tests.test_gpu_delete import make_rows
from tests.test_gpu_f16_wide_rows import Answers, assert_answers, assert_same_graph, bits
from tests.test_gpu_hamming_wide_rows import revlink_class

pytestmark = pytest.mark.gpu

LABEL0 = 1
SEED, EF, NQ, K = 11, 40, 64, 10
PLAN = (256, 16)
EMPTY = 0xFFFFFFFF
SCALARS_PER_CHUNK = {"f32": 4, "f16": 8, "i8": 16}


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def hubs(n, d, h, seed):
    """(rows, the sorted slots of the h hubs): unit rows, h of them shrunk to length 0.05"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    idx = rng.choice(n, h, replace=False)
    x[idx] *= np.float32(0.05)
    return np.ascontiguousarray(x), np.sort(idx)


def rows_of(family, metric, n, d, M):
    """the case's rows: seed d + M"""
    if family == "gauss":
        return make_rows(metric, d, n, d + M)
    return hubs(n, d, int(family[len("hubs"):]), d + M)[0]


def list_lengths(nbr):
    return (np.asarray(nbr) != EMPTY).sum(axis=1)


# family, metric, storage, n, d, M, efc, the reverse-link class, full level-0 lists in the oracle's graph (measured: plan (256, 16))
CASES = [
    ("hubs8", "l2sq", "f32", 1000, 64, 31, 64, "staged", 8),     # cap 62: the longest list with chain mode
    ("hubs8", "l2sq", "f32", 1000, 64, 32, 64, "staged", 5),     # cap 64: no chain; slot 0 of kpos full
    ("hubs8", "l2sq", "f32", 1000, 64, 33, 80, "staged", 5),     # cap 66: slot 1
    ("hubs8", "l2sq", "f32", 1200, 64, 64, 160, "staged", 2),    # cap 128: slot 1 full; efc > 128: the insertion walk's list in LDS
    ("hubs8", "l2sq", "f32", 1200, 128, 65, 160, "staged", 2),   # cap 130: slot 2; about 140 KB of the 150 KB the staged kernel may take
    ("hubs4", "l2sq", "f32", 1500, 96, 80, 200, "generic", 1),   # cap 160: about 166 KB, past it: the generic k_revlink
    ("gauss", "cos", "f32", 1500, 16, 40, 96, "staged", 3),
    ("gauss", "l2sq", "f32", 1500, 64, 32, 64, "staged", 3),
    ("hubs8", "l2sq", "f16", 1000, 64, 32, 64, "staged", 5),     # the M = 32 hubs case on halves and on int8 rows
    ("hubs8", "l2sq", "i8", 1000, 64, 32, 64, "staged", 5),
]
IDS = [f"{c[0]}-{c[1]}-{c[2]}-{c[3]}x{c[4]}-M{c[5]}" for c in CASES]


def build_pair(capi, oracle, cores, case, plan):
    """(the rows as the oracle holds them, the oracle's index, the device's), both built with `plan`; the reference-only checks"""
    family, metric, storage, n, d, M, efc, kernel, full = case
    base = rows_of(family, metric, n, d, M)
    rows_s, _, ometric, mode = stored_rows(oracle, storage, metric, base, base[:1])
    labels = np.arange(n, dtype=np.uint64) + LABEL0
    ora = oracle.OracleIndex(ometric, d, M=M, ef_construction=efc, ef=EF, seed=SEED, sum_mode=mode)
    ora.set_build_threads(cores)
    ora.add_planned(labels, rows_s, *plan)
    go = ora.export_graph()
    # non-vacuity, on the reference alone: a list of 2 M entries exists, and the shape is in the class the case names
    n_full = int((list_lengths(go["nbr0"]) == 2 * M).sum())
    print(f"{family} {metric} {storage} {n}x{d} M={M} plan={plan}: {n_full} level-0 lists of length {2 * M}")
    assert n_full >= 1, "the oracle's graph has no full level-0 list: the case is vacuous"
    if plan == PLAN:
        assert n_full == full, "the measured count next to the case is stale"
    chunks = -(-d // SCALARS_PER_CHUNK[storage])
    assert revlink_class(chunks, 2 * M) == kernel
    gpu = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=EF, seed=SEED, quantization=storage)
    gpu.set_add_batch(*plan)
    gpu.add_many(labels, base)
    gpu.flush()
    assert len(gpu) == n
    return base, rows_s, ometric, mode, ora, go, gpu


def assert_built_alike(gpu, go, kernel):
    gg = gpu.export_graph()
    assert_same_graph(gg, go)  # the entry, max_level, levels, labels, upper_off, nbr0, upper_nbr
    c = gpu.counters()
    print(f"add_revlink_evals {c['add_revlink_evals']} add_reprunes {c['add_reprunes']}")
    # k_revlink_staged counts its re-prunes; the generic k_revlink counts its distance evaluations alone (the comment in
    # tests/test_gpu_hamming_wide_rows.py) -- so the counters also say which of the two ran
    assert c["add_revlink_evals"] > 0, "no full list was re-pruned"
    assert (c["add_reprunes"] == 0) == (kernel == "generic"), c
    return gg


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_build_and_search_with_long_lists(capi, oracle, cores, case):
    family, metric, storage, n, d, M, efc, kernel, _ = case
    base, rows_s, ometric, mode, ora, go, gpu = build_pair(capi, oracle, cores, case, PLAN)
    gg = assert_built_alike(gpu, go, kernel)
    # 64 queries on the same graph: M0 > 64 is refused by the speculative and the prefetching walks, so past M = 32 every
    # search below is the classic walk, with more than one wave-pass per list
    queries = make_rows(metric, d, NQ, d + M + 1)
    _, q_s, _, _ = stored_rows(oracle, storage, metric, base[:1], queries)
    want = oracle.OracleIndex.from_graph(ometric, rows_s, gg, M, efc, EF, SEED, mode).search_batch(q_s, K, EF, cores)
    dev = Answers(gpu, queries, K)
    for waves in (4, 8):
        gpu.set_search_shape(waves)
        assert_answers(dev.search(NQ), want, NQ, f"waves={waves}")
    gpu.set_search_shape(0)
    lab, dist, _ = gpu.search_batch(queries, K)
    assert np.array_equal(lab, want[0]) and np.array_equal(bits(dist), bits(want[1]))
    l1, d1 = gpu.search(queries[0], K)
    assert len(l1) == K and np.array_equal(l1, want[0][0]) and np.array_equal(bits(d1), bits(want[1][0]))
    gpu.close()


# the two shapes whose re-prunes keep more than 64 and more than 128 entries, in the other batch plans: every row alone, and small batches
@pytest.mark.parametrize("plan", [(1, 1), (64, 4)])
@pytest.mark.parametrize("case", [c for c in CASES if c[5] in (33, 65)], ids=[i for c, i in zip(CASES, IDS) if c[5] in (33, 65)])
def test_build_with_long_lists_in_the_other_plans(capi, oracle, cores, case, plan):
    *_, go, gpu = build_pair(capi, oracle, cores, case, plan)
    assert_built_alike(gpu, go, case[7])
    gpu.close()


def test_upper_level_lists_of_63_entries(capi, oracle):
    """M = 63: an upper list's cap is 63, the first without chain mode.  Levels drawn by the index cannot fill an upper list of that
    length at any size a test can afford -- a row reaches level 1 with probability 1 / 63, so 63 links to one level-1 node want
    some 63 x 63 rows even if every one of them picked it -- so the levels are assigned: 600 hubs rows added one by one with
    add(label, row, level), 150 of them on level 1 and the two hubs first among those, on both sides."""
    n, d, M, efc = 600, 64, 63, 64
    base, hub = hubs(n, d, 2, d + M)
    levels = np.zeros(n, dtype=np.int64)
    levels[hub] = 1
    rest = np.setdiff1d(np.arange(n), hub)
    levels[np.random.default_rng(d + M + 1).choice(rest, 150 - hub.size, replace=False)] = 1
    order = np.concatenate([hub, rest])  # the hubs are in the graph before any row that will link to them
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=efc, ef=EF, seed=SEED, sum_mode=oracle.SUM_WAVE64)
    gpu = capi.GpuIndex("l2sq", d, M=M, ef_construction=efc, ef=EF, seed=SEED)
    gpu.set_add_batch(1, 1)
    for s in order:
        ora.add(int(s) + LABEL0, base[s], level=int(levels[s]))
        gpu.add(int(s) + LABEL0, base[s], level=int(levels[s]))
    go, gg = ora.export_graph(), gpu.export_graph()
    upper = list_lengths(go["upper_nbr"])
    print(f"upper lists: {upper.size}, of length 63: {int((upper == M).sum())}; level-0 lists of length 126: {int((list_lengths(go['nbr0']) == 2 * M).sum())}")
    assert int(go["max_level"]) == 1 and upper.size == 150 and (upper == M).any(), "no upper list of the oracle's graph reaches 63"
    assert_same_graph(gg, go)
    assert gpu.counters()["add_reprunes"] > 0
    gpu.close()
