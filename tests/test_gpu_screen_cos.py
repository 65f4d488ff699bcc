"""The int8 screen of the f32 cosine walk (walk.hpp hop_distances_screened<M_COS>) changes which rows are READ, never an
answer: with the screen on and off (LANTERN_GPU_SCREEN=0, child processes) every id, distance bit, count and D / E is the same; the
screened walk still equals the oracle, also in the per-query-parameter form; and at size the cosine bound rejects about as many rows as
the l2sq bound does on the same rows normalised (there the two metrics order the rows alike)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEAK = ("common_mean", "mixed_scale")  # the probe's families whose bound is weak by construction: 0 < exact <= logical

# test_cosine_screen_prunes_at_size: the cosine share of rows read in f32 may be at most this multiple of the l2sq share measured in the
# same test.  On unit rows the l2sq bound leaves a slack of about 1.41 rho in cosine units and the cosine bound rho + 2 e, so the two
# shares should be about equal; twice the l2sq share is where the bound would be looser than its mathematics (which also
# says what a device run has to record before this margin is tightened)
COS_SHARE_CAP = 2.0


def probe(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LANTERN_GPU_")}
    env.update(extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "screen_cos_probe.py")], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    line = next((json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")), None)
    assert p.returncode == 0 and line, (extra, p.stdout[-1500:], p.stderr[-1500:])
    return line


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def test_cosine_screen_is_result_neutral(capi):
    on, off = probe({}), probe({"LANTERN_GPU_SCREEN": "0"})
    son, soff = on.pop("screen"), off.pop("screen")
    assert on == off
    # the comparison is not vacuous: with the screen on, every index it serves rejected rows in the walks above (and still read some
    # in f32); with it off, or at d = 504, nothing was screened.  Rows with a common mean and rows whose norms leave the range in which
    # the screen rejects have a weak bound by construction: there the screened walk ran, and still had to answer the same.
    for tag, st in son.items():
        if st["screened"] and tag.startswith(WEAK):
            assert 0 < st["exact"] <= st["logical"], (tag, st)
        elif st["screened"]:
            assert 0 < st["exact"] < st["logical"], (tag, st)
        else:
            assert st["logical"] == 0, (tag, st)
    assert any(st["screened"] for st in son.values()) and not all(st["screened"] for st in son.values())
    assert all(st["logical"] == 0 for st in soff.values()), soff
    assert on["gaussian_768_inserted_found"] >= 0.9, "rows inserted after the build were not found at their self-distance"


@pytest.mark.parametrize("data", ["gaussian", "clustered"])
def test_screened_cosine_walk_equals_the_oracle(capi, data):
    from oracle import binding as oracle

    rng = np.random.default_rng(2)
    n, d, k = 4000, 768, 10
    if data == "gaussian":
        base = rng.standard_normal((n, d), dtype=np.float32)
        queries = rng.standard_normal((128, d), dtype=np.float32)
    else:
        centres = rng.standard_normal((16, d), dtype=np.float32) * 4
        base = (centres[rng.integers(0, 16, n)] + rng.standard_normal((n, d), dtype=np.float32) * 0.5).astype(np.float32)
        queries = (centres[rng.integers(0, 16, 128)] + rng.standard_normal((128, d), dtype=np.float32) * 0.5).astype(np.float32)
    ix = capi.GpuIndex("cos", d, M=16, ef_construction=64, ef=64, seed=1)
    ix.set_add_batch(512, 16)
    ix.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    ix.flush()
    g = ix.export_graph()
    ora = oracle.OracleIndex.from_graph("cos", base, g, 16, 64, 64, 1, oracle.SUM_WAVE64)
    expect = {ef: ora.search_batch(queries, k, ef) for ef in (10, 64, 128)}  # once, shared by both shapes
    for waves in (4, 8):  # the classic walk, which the screen serves (a small batch would otherwise take walk_spec.hpp's walk)
        ix.set_search_shape(waves)
        for ef in (10, 64, 128):
            c0, s0 = ix.counters(), ix.screen_stats()
            lab, dist, _ = ix.search_batch(queries, k, ef)
            c1, s1 = ix.counters(), ix.screen_stats()
            o_lab, o_dist, _, o_D, o_E = expect[ef]
            assert np.array_equal(lab, o_lab) and np.array_equal(dist.view(np.uint32), o_dist.view(np.uint32)), (data, waves, ef)
            assert c1["search_dist_evals"] - c0["search_dist_evals"] == int(o_D.sum()), (data, waves, ef)
            assert c1["search_expansions"] - c0["search_expansions"] == int(o_E.sum()), (data, waves, ef)
            logical, exact = s1[0] - s0[0], s1[1] - s0[1]
            assert logical == int(o_D.sum()) and 0 < exact < logical, (data, waves, ef, logical, exact)  # the screen ran, and rejected rows


@pytest.mark.parametrize("screen", ["1", "0"])
def test_screened_cosine_index_with_per_query_parameters(capi, oracle, screen, monkeypatch):
    from tests.test_gpu_search_params import Case, check, small_mix

    monkeypatch.setenv("LANTERN_GPU_SCREEN", screen)
    nq = 1400  # (the screen is part of the bandwidth-bound walk: more than two queries per CU in both classes)
    case = Case(capi, oracle, "cos", 2500, 512, 16, 64, nq)
    params = small_mix(nq, (1, 10, 40, 65, 100), (0, 64, 128), (0, 7))
    before = case.gpu.screen_stats()
    got = case.params(params)
    regime = case.gpu.last_params_launch()
    assert regime["launches"] == 2 and not regime["spec"], regime
    check(got, case.want(params), f"cos screen={screen}")
    after = case.gpu.screen_stats()
    if screen == "1":
        assert after[0] > before[0] and after[1] - before[1] < after[0] - before[0]  # rows were rejected on the screen copy
    else:
        assert after == before == (0, 0)


def test_cosine_screen_prunes_at_size(capi):
    """200 000 x 768 Gaussian rows: a cosine index on the rows and an l2sq index on the rows normalised to unit length, where the
    cosine distance is half the l2sq distance and the two orders agree.  Both screens must reject rows, and the share of rows the
    cosine screen still reads in f32 is held against the l2sq share of the same run, not against an absolute."""
    rng = np.random.default_rng(7)
    n, d = 200_000, 768
    base = rng.standard_normal((n, d), dtype=np.float32)
    queries = rng.standard_normal((2048, d), dtype=np.float32)
    unit = (base / np.linalg.norm(base.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    unit_q = (queries / np.linalg.norm(queries.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    share = {}
    for metric, rows, qs in (("cos", base, queries), ("l2sq", unit, unit_q)):
        ix = capi.GpuIndex(metric, d, M=16, ef_construction=128, ef=64, seed=1)
        ix.set_add_batch(16384, 16)
        ix.add_many(np.arange(n, dtype=np.uint64) + 1, rows)
        ix.flush()
        ix.search_batch(qs, 10)
        logical, exact = ix.screen_stats()
        assert logical == ix.counters()["search_dist_evals"]
        assert 0 < exact < logical, (metric, logical, exact)
        share[metric] = exact / logical
        ix.close()
    print(f"share of rows read in f32: cos {share['cos']:.4f}, l2sq on the normalised rows {share['l2sq']:.4f}, "
          f"ratio {share['cos'] / share['l2sq']:.3f}")
    assert share["cos"] <= COS_SHARE_CAP * share["l2sq"], share
