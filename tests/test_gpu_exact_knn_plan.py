"""An exact k-NN call launches what its plan lists (csrc/dense.cpp: plan_exact_knn, then exact_knn_run walks the plan's steps): at the
smallest shapes that cross each boundary of the plan -- the seed columns, the chunk of base rows with the query tile, the fused switch,
every operand kind -- the contraction launches recorded on the device are lantern_gpu_plan_exact_knn's step list, the launch counter
of the plan's operand kind moves by the number of steps, no query takes the fallback, and the answers are the brute force's.  Rows of
four dimensions (two words for hamming): the contraction costs nothing."""
import functools

import numpy as np
import pytest

from tests.test_gpu_exact_knn import FAMILIES, index_of, referee

pytestmark = pytest.mark.gpu

K = 10
MCODE = {("l2sq", "f32"): 3, ("cos", "f32"): 1, ("l2sq", "f16"): 103, ("cos", "i8"): 201, ("hamming", "f32"): 8}
FAMILY = {"f32": "gauss", "f16": "gauss", "i8": "i8gauss"}


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0
    return capi


@functools.lru_cache(maxsize=None)
def reference(oracle, cores, metric, storage, n, nq):
    """(rows, queries, the brute force's ids and distances, the rows as the index stores them): once per shape, shared by its switches"""
    rng = np.random.default_rng([n, nq, len(storage)])
    rows, queries = FAMILIES["bits" if metric == "hamming" else FAMILY[storage]](rng, n, 2 if metric == "hamming" else 4, nq)
    ids, dists, stored = referee(oracle, cores, metric, storage, rows, queries, K)
    for a in (rows, queries, ids, dists, stored):
        a.setflags(write=False)
    return rows, queries, ids, dists, stored


def check(capi, oracle, cores, monkeypatch, metric, storage, n, nq, native, fused):
    rows, queries, ids, dists, stored = reference(oracle, cores, metric, storage, n, nq)
    monkeypatch.setenv("LANTERN_GPU_DENSE_NATIVE", str(native))
    monkeypatch.setenv("LANTERN_GPU_DENSE_FUSED", str(fused))
    ix = index_of(capi, metric, storage, rows, stored)
    assert ix.row_bytes() == 16
    plan = capi.plan_exact_knn(MCODE[metric, storage], 1, n, nq, K, native, fused)
    stats, kinds = capi.exact_knn_stats(), capi.dense_kind_stats()
    capi.dense_profile(True)
    slots, got = ix.exact_search(queries, K)
    launches = [(r["rows"], r["cols"], r["fused"]) for r in capi.dense_profile(False)]
    after, moved = capi.exact_knn_stats(), [a - b for a, b in zip(capi.dense_kind_stats(), kinds)]
    ix.close()
    assert launches == [s[:3] for s in plan["steps"]]
    want = [0, 0, 0]
    if metric != "hamming":
        want[plan["kind"]] = len(plan["steps"])
    assert moved == want
    assert after["fallback"] == stats["fallback"] and after["certified"] - stats["certified"] == nq
    assert np.array_equal(slots, ids) and np.array_equal(got.view(np.uint32), dists.view(np.uint32))
    return plan


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "unfused"])
@pytest.mark.parametrize("n,nq", [(4096, 1), (4097, 1), (65537, 1025)])
def test_f32_calls_launch_their_plan(capi, oracle, cores, monkeypatch, n, nq, fused):
    plan = check(capi, oracle, cores, monkeypatch, "l2sq", "f32", n, nq, 1, fused)
    assert plan["kind"] == 0 and plan["fused"] == (1 if fused and n > 4096 else 0)


@pytest.mark.parametrize("native", [1, 0], ids=["native", "dequantised"])
def test_f16_calls_launch_their_plan(capi, oracle, cores, monkeypatch, native):
    plan = check(capi, oracle, cores, monkeypatch, "l2sq", "f16", 4097, 1, native, 1)
    assert (plan["kind"], plan["copy"]) == ((1, 0) if native else (0, 1)) and len(plan["steps"]) == 2


def test_i8_call_launches_its_plan(capi, oracle, cores, monkeypatch):
    plan = check(capi, oracle, cores, monkeypatch, "cos", "i8", 4097, 1, 1, 1)
    assert (plan["kind"], plan["exact_keys"]) == (2, 1) and len(plan["steps"]) == 2


def test_hamming_call_launches_its_plan(capi, oracle, cores, monkeypatch):
    plan = check(capi, oracle, cores, monkeypatch, "hamming", "f32", 5000, 3, 1, 1)
    assert plan["bits"] == 1 and plan["steps"] == [(3, 5000, False, 0)]
