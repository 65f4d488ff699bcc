"""The int8 screen of the f32 l2sq walk (walk.hpp hop_distances_screened) changes which rows are READ, never an
answer: with the screen on and off (LANTERN_GPU_SCREEN=0, child processes) every id, distance bit, count and D / E is the same; the
screened walk still equals the oracle; and the screen does reject most rows of a walk at size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def probe(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LANTERN_GPU_")}
    env.update(extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "screen_probe.py")], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    line = next((json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")), None)
    assert p.returncode == 0 and line, (extra, p.stdout[-1500:], p.stderr[-1500:])
    return line


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def test_screen_is_result_neutral(capi):
    on, off = probe({}), probe({"LANTERN_GPU_SCREEN": "0"})
    son, soff = on.pop("screen"), off.pop("screen")
    assert on == off
    # the comparison is not vacuous: with the screen on, every index it serves rejected rows in the walks above (and still read some
    # in f32); with it off, nothing was screened
    # (rows with one 1e4 component: every other value quantises to 0, r is ~||row||, and the bound rejects nothing -- correctly; there
    # the screened walk ran, read every row in f32, and still had to answer the same)
    for tag, st in son.items():
        if st["screened"] and tag.startswith("outlier"):
            assert 0 < st["exact"] <= st["logical"], (tag, st)
        elif st["screened"]:
            assert 0 < st["exact"] < st["logical"], (tag, st)
        else:
            assert st["logical"] == 0, (tag, st)
    assert all(st["logical"] == 0 for st in soff.values()), soff
    assert on["gaussian_768_inserted_found"] >= 0.9, "rows inserted after the build were not found at distance 0"


def test_screened_walk_equals_the_oracle(capi):
    from oracle import binding as oracle

    rng = np.random.default_rng(2)
    n, d, k = 4000, 768, 10
    base = rng.standard_normal((n, d), dtype=np.float32)
    queries = rng.standard_normal((128, d), dtype=np.float32)
    ix = capi.GpuIndex("l2sq", d, M=16, ef_construction=64, ef=64, seed=1)
    ix.set_add_batch(512, 16)
    ix.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    ix.flush()
    g = ix.export_graph()
    ora = oracle.OracleIndex.from_graph("l2sq", base, g, 16, 64, 64, 1, oracle.SUM_WAVE64)
    for waves in (4, 8):  # the classic walk, which the screen serves (a small batch would otherwise take walk_spec.hpp's walk)
        ix.set_search_shape(waves)
        for ef in (10, 64, 128):
            c0, s0 = ix.counters(), ix.screen_stats()
            lab, dist, _ = ix.search_batch(queries, k, ef)
            c1, s1 = ix.counters(), ix.screen_stats()
            o_lab, o_dist, _, o_D, o_E = ora.search_batch(queries, k, ef)
            assert np.array_equal(lab, o_lab) and np.array_equal(dist.view(np.uint32), o_dist.view(np.uint32)), (waves, ef)
            assert c1["search_dist_evals"] - c0["search_dist_evals"] == int(o_D.sum()), (waves, ef)
            assert c1["search_expansions"] - c0["search_expansions"] == int(o_E.sum()), (waves, ef)
            logical, exact = s1[0] - s0[0], s1[1] - s0[1]
            assert logical == int(o_D.sum()) and 0 < exact < logical, (waves, ef, logical, exact)  # the screen ran, and rejected rows


def test_screen_prunes_most_rows_at_size(capi):
    rng = np.random.default_rng(7)
    n, d = 200_000, 768
    base = rng.standard_normal((n, d), dtype=np.float32)
    queries = rng.standard_normal((2048, d), dtype=np.float32)
    ix = capi.GpuIndex("l2sq", d, M=16, ef_construction=128, ef=64, seed=1)
    ix.set_add_batch(16384, 16)
    ix.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    ix.flush()
    ix.search_batch(queries, 10)
    logical, exact = ix.screen_stats()
    assert logical == ix.counters()["search_dist_evals"]
    assert 0 < exact < 0.35 * logical, (logical, exact)
