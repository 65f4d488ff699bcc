"""The screen phase's block loads (walk.hpp hop_distances_screened: eight lanes per int8 row, the row requested in blocks of chunks per
lane before the first is consumed) at the smallest shapes at which they can go wrong: the shortest screened row, a partial last screen
word, a row that is no multiple of the group width, rows of several blocks with a partial last one; hops with fewer new rows than
groups (M = 4) and with several rounds of groups (M = 32, M0 = 64).  The screened classic walk must equal the oracle on the exported
graph in every label, distance bit, D and E, and the screen must have run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NQ, K = 3000, 96, 10
# d: chunks / screen chunks -- 509: 128 / 32 (smallest screened row, partial last f32 chunk) | 513: 129 / 33 (partial screen word, not a
# multiple of the group width) | 768: 192 / 48 (the headline row) | 1021: 256 / 64 (a long row) | 2000: 500 / 125 (multi-block rows,
# partial last block)
DIMS = (509, 513, 768, 1021, 2000)
MS = (4, 16, 32)
DATA = ("gaussian", "scaled_down", "scaled_up", "duplicates", "indexed_queries")
STRICT = ("gaussian",)  # elsewhere the bound may legitimately reject nothing: only 0 < exact <= logical is required


@pytest.fixture(scope="module")
def libs():
    from lantern_amd import build, capi
    from oracle import binding as oracle

    build.build()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi, oracle


def make(data, d):
    rng = np.random.default_rng(1000 + d)
    base = rng.standard_normal((N, d), dtype=np.float32)
    queries = rng.standard_normal((NQ, d), dtype=np.float32)
    if data == "scaled_down":
        base, queries = base * np.float32(1e-3), queries * np.float32(1e-3)
    elif data == "scaled_up":
        base, queries = base * np.float32(1e3), queries * np.float32(1e3)
    elif data == "duplicates":  # every row once more: ties in every list, and distance-0 pairs in the graph
        base = np.concatenate([base[: N // 2], base[: N // 2]])
    elif data == "indexed_queries":
        queries = base[rng.choice(N, NQ, replace=False)].copy()
    return np.ascontiguousarray(base), np.ascontiguousarray(queries)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("d", DIMS)
def test_blocked_screen_equals_the_oracle(libs, d, M, data):
    capi, oracle = libs
    base, queries = make(data, d)
    ix = capi.GpuIndex("l2sq", d, M=M, ef_construction=64, ef=64, seed=1)
    ix.set_add_batch(512, 16)
    ix.add_many(np.arange(N, dtype=np.uint64) + 1, base)
    ix.flush()
    ora = oracle.OracleIndex.from_graph("l2sq", base, ix.export_graph(), M, 64, 64, 1, oracle.SUM_WAVE64)
    expect = {ef: ora.search_batch(queries, K, ef) for ef in (10, 64, 128)}  # once, shared by both shapes
    for waves in (4, 8):  # the classic walk, which the screen serves
        ix.set_search_shape(waves)
        for ef in (10, 64, 128):
            o_lab, o_dist, _, o_D, o_E = expect[ef]
            c0, s0 = ix.counters(), ix.screen_stats()
            lab, dist, _ = ix.search_batch(queries, K, ef)
            c1, s1 = ix.counters(), ix.screen_stats()
            tag = (d, M, data, waves, ef)
            assert np.array_equal(lab, o_lab), tag
            assert np.array_equal(dist.view(np.uint32), o_dist.view(np.uint32)), tag
            assert c1["search_dist_evals"] - c0["search_dist_evals"] == int(o_D.sum()), tag
            assert c1["search_expansions"] - c0["search_expansions"] == int(o_E.sum()), tag
            logical, exact = s1[0] - s0[0], s1[1] - s0[1]
            assert logical == int(o_D.sum()), tag
            if data in STRICT:
                assert 0 < exact < logical, (tag, logical, exact)  # the screen ran, and rejected rows
            else:
                assert 0 < exact <= logical, (tag, logical, exact)
