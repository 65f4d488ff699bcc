"""The int8 screen in the insertion walk (csrc/insert_kernel.hip k_insert<.., SCREEN = true>; lantern_gpu_set_insert_screen): a build
whose level-0 candidates are tested on the int8 row copy first is, edge for edge, the build that reads every f32 row -- and the
oracle's.  Shapes: rows of >= 128 chunks (d >= 509), n = 6000 >> ef_construction so that level-0 lists are full, batches of up to
2048 rows (above 2 x CUs: k_insert, not the lone-insertion walk).  Every case reads its regime from insert_screen_stats:
(screened launches, unscreened launches, rows tested, rows rejected)."""
import threading

import numpy as np
import pytest

from tests.test_gpu_parity import LABEL0
from tests.test_screen_bound import adversarial

pytestmark = pytest.mark.gpu

N, M, SEED, PLAN = 6000, 8, 11, (2048, 2)
GRAPH_ARRAYS = ("levels", "labels", "upper_off", "nbr0", "upper_nbr")


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def rows_for(kind, n, d, seed):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((n, d), dtype=np.float32)
    centres = rng.standard_normal((16, d), dtype=np.float32)
    return (centres[rng.integers(0, 16, n)] + np.float32(0.35) * rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32)


def build(capi, metric, base, efc, mode, plan=PLAN, quantization="f32", reserve=None, parts=None):
    ix = capi.GpuIndex(metric, base.shape[1], M=M, ef_construction=efc, ef=64, seed=SEED, quantization=quantization)
    ix.set_add_batch(*plan)
    ix.set_insert_screen(mode)
    if reserve:
        ix.reserve(reserve)
    labels = np.arange(len(base), dtype=np.uint64) + LABEL0
    at = 0
    for count in parts or [len(base)]:
        ix.add_many(labels[at: at + count], base[at: at + count])
        at += count
    ix.flush()
    assert len(ix) == len(base)
    return ix


def same_graph(a, b, what):
    assert a["entry_slot"] == b["entry_slot"] and a["max_level"] == b["max_level"], what
    for name in GRAPH_ARRAYS:
        assert np.array_equal(a[name], b[name]), f"{what}: {name} differs"


def on_equals_off(capi, metric, base, efc, **kw):
    """both builds; mode 1 screened and rejected, mode 0 did neither, same graph, same checksum, same D.  -> (off, on)"""
    off, on = build(capi, metric, base, efc, 0, **kw), build(capi, metric, base, efc, 1, **kw)
    s0, s1 = off.insert_screen_stats(), on.insert_screen_stats()
    print(f"{metric} d={base.shape[1]} efc={efc}: off {s0} on {s1} rejected share {s1[3] / max(1, s1[2]):.3f}")
    assert s0[0] == 0 and s0[2] == 0 and s0[3] == 0 and s0[1] > 0
    assert s1[0] > 0 and s1[3] > 0 and s1[2] >= s1[3]
    assert s1[0] + s1[1] == s0[1]  # the same launches, some of them screened
    same_graph(on.export_graph(), off.export_graph(), "mode 1 against mode 0")
    assert on.checksum() == off.checksum()
    c0, c1 = off.counters(), on.counters()
    assert c1["add_walk_evals"] == c0["add_walk_evals"] and c1["add_expansions"] == c0["add_expansions"]  # rejected rows count as evaluated
    assert s1[2] <= c1["add_walk_evals"]
    return off, on


# ---- 1. on = off = oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "clusters"])
@pytest.mark.parametrize("efc", [40, 128])  # one and two keys per lane of the list wave
@pytest.mark.parametrize("metric,d", [("l2sq", 509), ("l2sq", 768), ("l2sq", 2000), ("cos", 512), ("cos", 768)])
def test_screened_build_is_the_unscreened_build(capi, oracle, metric, d, efc, kind):
    base = rows_for(kind, N, d, d + efc)
    off, on = on_equals_off(capi, metric, base, efc)
    if d != 768 or efc != 128:
        return
    # ... and the oracle's, edge for edge; searches of the screened-built index are the oracle's
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=64, seed=SEED, sum_mode=oracle.SUM_WAVE64)
    ora.add_planned(np.arange(N, dtype=np.uint64) + LABEL0, base, max_batch=PLAN[0], min_ratio=PLAN[1])
    same_graph(on.export_graph(), ora.export_graph(), "mode 1 against the oracle")
    from lantern_amd import hip

    nq, k = 64, 10
    queries = rows_for(kind, nq, d, 99)
    o_lab, o_dist, _, o_D, o_E = ora.search_batch(queries, k)
    qrows = on.device_query_rows(queries)
    dq = hip.Buffer.from_numpy(qrows)
    lab, dist, D, E = hip.Buffer(nq * k * 8), hip.Buffer(nq * k * 4), hip.Buffer(nq * 8), hip.Buffer(nq * 8)
    on.search_batch_device(dq.ptr, nq, k, 0, 0, lab.ptr, dist.ptr, None, None, D.ptr, E.ptr, query_stride=qrows.strides[0])
    hip.synchronize()
    assert np.array_equal(lab.download((nq, k), np.uint64), o_lab)
    assert np.array_equal(dist.download((nq, k), np.float32).view(np.uint32), o_dist.view(np.uint32))
    assert np.array_equal(D.download(nq, np.uint64), o_D) and np.array_equal(E.download(nq, np.uint64), o_E)


# ---- 2. regimes that stay unscreened ---------------------------------------------------------------------
@pytest.mark.parametrize("what,metric,d,efc,plan,quantization",
                         [("efc 200: the LDS list", "l2sq", 768, 200, PLAN, "f32"), ("d 504: 126 chunks, no table", "l2sq", 504, 64, PLAN, "f32"),
                          ("f16 rows", "cos", 768, 64, PLAN, "f16"), ("every batch takes the lone walk", "l2sq", 768, 64, (64, 1), "f32")])
def test_regimes_that_stay_unscreened(capi, what, metric, d, efc, plan, quantization):
    n = 1500 if plan != PLAN else N  # (batches of at most 64 rows: a shorter build)
    base = rows_for("gauss", n, d, 5)
    off, on = (build(capi, metric, base, efc, mode, plan=plan, quantization=quantization) for mode in (0, 1))
    s0, s1 = off.insert_screen_stats(), on.insert_screen_stats()
    assert s1[0] == 0 and s1[2] == 0 and s1[3] == 0 and s1 == s0, what
    assert (s1[1] == 0) == (plan != PLAN), what  # the lone walk is not a k_insert launch; every other regime is k_insert, unscreened
    same_graph(on.export_graph(), off.export_graph(), what)
    assert on.checksum() == off.checksum()


# ---- 3. adversarial values -------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_adversarial_rows_among_gaussian_ones(capi, oracle, metric):
    d = 768
    rng = np.random.default_rng(3)
    base = rows_for("gauss", N, d, 17)
    odd = list(adversarial(rng, d))
    g = rng.standard_normal(d).astype(np.float32)
    odd += [np.zeros(d, np.float32), g * np.float32(1e30), g * np.float32(1e-30)]
    for places in ((0,), (5, 400), (1, 2, 767)):
        r = rng.standard_normal(d).astype(np.float32)
        r[list(places)] = [np.float32(3e38) * (1 if i % 2 == 0 else -1) for i in range(len(places))]
        odd.append(r)
    # Rows that make a NaN distance are left out: a walk over NaN keys cannot be compared.  Which ones do is the
    # oracle's word, in the device's summation order: against itself, every odd row already kept and a few Gaussian rows.
    kept = []
    with np.errstate(over="ignore", invalid="ignore"):
        for r in odd:
            others = [r] + kept + [base[i] for i in range(0, 8)]
            if all(not np.isnan(oracle.distance(r, y, metric, oracle.SUM_WAVE64)) and not np.isnan(oracle.distance(y, r, metric, oracle.SUM_WAVE64)) for y in others):
                kept.append(r)
    assert len(kept) >= (9 if metric == "l2sq" else 5), len(kept)
    slots = np.linspace(3, N - 7, 4 * len(kept)).astype(int)  # each odd row four times: early (short lists) and late (full ones)
    for i, s in enumerate(slots):
        base[s] = kept[i % len(kept)]
    on_equals_off(capi, metric, base, 128)


# ---- 4. growth -------------------------------------------------------------------------------------------
def test_the_screen_table_grows_under_a_screened_build(capi):
    d = 768
    base = rows_for("gauss", 6500, d, 23)
    off, on = on_equals_off(capi, "l2sq", base, 64, reserve=4000, parts=[4000, 2500])
    assert on.capacity >= 6500
    whole = build(capi, "l2sq", base, 64, 0)
    a, b = on.export_screen(), whole.export_screen()
    assert a["row_bytes"] == b["row_bytes"] == (d // 4 + 3) // 4 * 16
    assert np.array_equal(a["codes"], b["codes"]) and np.array_equal(a["meta"].view(np.uint32), b["meta"].view(np.uint32))


# ---- 5. work-sharded build -------------------------------------------------------------------------------
def test_work_sharded_build_screens_and_gives_the_same_graph(capi):
    d, efc = 768, 64
    base = rows_for("gauss", N, d, 29)
    labels = np.arange(N, dtype=np.uint64) + LABEL0
    single = build(capi, "l2sq", base, efc, 0)
    comms = capi.Comm.local_world(2)
    out, errs = [None, None], []

    def run(r):
        try:
            comms[r].set_timeout(120)
            ix = capi.GpuIndex("l2sq", d, M=M, ef_construction=efc, ef=64, seed=SEED)
            ix.set_add_batch(*PLAN)
            ix.set_insert_screen(1)
            lo, hi = capi.shard_range(N, 2, r)
            ix.add_sharded(comms[r], labels[lo:hi], base[lo:hi])
            out[r] = ix
        except Exception as e:  # noqa: BLE001 -- reported below
            errs.append((r, repr(e)))

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for r, ix in enumerate(out):
        s = ix.insert_screen_stats()
        assert s[0] > 0 and s[3] > 0, (r, s)
        assert ix.checksum() == single.checksum(), r
