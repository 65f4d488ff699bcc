"""The integer form of the int8 screen on the DEVICE (walk.hpp screen_stage_query, hop_distances_screened) against its numpy
restatement (tests/test_screen_bound_int.py), through GpuIndex.screen_probe and distance_gather: single workgroups, indexes of at most
100 rows.  d = 509 is the first screened width with a ragged last chunk, 768 the workload's, 2000 the width where <X, c> over a group
leaves int32.

  1 the device's verdict is the integer restatement's a band of 2^-16 either side of the restatement's threshold (relative for l2sq,
    absolute for cosine): the integer sums are exact, and at most ~16 f32 roundings, amplified at most fourfold through the square,
    separate the two -- 64 u = 2^-18; the band is four times that
  2 rows whose codes are all +-127 against a query whose X are all 32639, d = 2000
  3 adversarial queries (an outlier, 1e-25, 1e25, zero, NaN, +inf) reject no row inside the radius; the last three reject nothing
  4 whole walks with the screen on and off are byte-identical in the shapes the other screen tests leave out, and the plan shows the
    planes' LDS block for the screened launch only"""
import numpy as np
import pytest

from tests import test_gpu_screen_rows as rows_mod
from tests import test_screen_bound_cos as cs
from tests import test_screen_bound_int as si

pytestmark = pytest.mark.gpu

F32 = np.float32
BAND = 2.0 ** -16
M_CODE = {"cos": 1, "l2sq": 3}


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def threshold(c, st, x, i, ra):
    """the integer restatement's compared value over the device's stored row i"""
    codes = c.codes[i, : c.d]
    if c.metric == "l2sq":
        return si.l2_threshold(st, codes, c.meta[i, 0], c.meta[i, 1], c.chunks)
    return si.cos_threshold(st, codes, c.meta[i, 0], c.meta[i, 1], ra, c.chunks)


def either_side(metric, thr):
    if metric == "l2sq":
        return F32(float(thr) * (1 - BAND)), F32(float(thr) * (1 + BAND))
    return F32(float(thr) - BAND), F32(float(thr) + BAND)


# ---- 1. the verdict against the integer restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("wg", [256, 512])
@pytest.mark.parametrize("d", [509, 768, 2000])
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_the_device_decides_as_the_integer_restatement(capi, metric, d, wg):
    c = rows_mod.case(capi, metric, d)
    gs = c.family("gaussian")
    checked = 0
    for x in rows_mod.gaussian_queries(d):
        ra = cs.rooted_norm(x) if metric == "cos" else None
        st = si.Staged(x, metric, ra=ra)
        assert st.ok
        for i in gs[::2] if wg == 512 else gs[1::2]:
            thr = threshold(c, st, x, i, ra)
            assert thr is not None and (metric == "cos" or float(thr) > 1.0)
            below, above = either_side(metric, thr)
            assert c.probe(x, [i], below, wg)[0], (i, "the device keeps a row the integer restatement rejects", float(thr))
            assert not c.probe(x, [i], above, wg)[0], (i, "the device rejects a row the integer restatement keeps", float(thr))
            checked += 1
    assert checked == 96


# ---- 2. the sums at the edge of int32 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wg", [256, 512])
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_rows_of_extreme_codes_against_a_query_of_extreme_planes(capi, metric, wg):
    d = 2000
    rng = np.random.default_rng(17)
    rows = np.concatenate([np.full((1, d), 3.0, F32), np.full((1, d), -1.0, F32), rng.standard_normal((30, d)).astype(F32)])
    ix = capi.GpuIndex(metric, d, M=8, ef_construction=32, ef=32, seed=3)
    ix.add_many(np.arange(len(rows), dtype=np.uint64) + 1, rows)
    ex = ix.export_screen()
    assert np.all(ex["codes"][0, :d] == 127) and np.all(ex["codes"][1, :d] == -127)
    x = np.ones(d, F32)
    ra = cs.rooted_norm(x) if metric == "cos" else None
    st = si.Staged(x, metric, ra=ra)
    assert np.all(st.X[:d] == si.XMAX)
    dist = ix.distance_gather(x, [0, 1])
    for i in (0, 1):
        ih, il, _ = si.row_sums(st, ex["codes"][i, :d])
        assert abs(256 * ih + il) == d * si.XMAX * 127 > 2 ** 32  # (the sum the device must not form in 32 bits)
        codes, m0, m1 = ex["codes"][i, :d], ex["meta"][i, 0], ex["meta"][i, 1]
        thr = si.l2_threshold(st, codes, m0, m1, 500) if metric == "l2sq" else si.cos_threshold(st, codes, m0, m1, ra, 500)
        assert thr is not None
        below, above = either_side(metric, thr)
        assert ix.screen_probe(x, [i], below, wg)[0] and not ix.screen_probe(x, [i], above, wg)[0], (i, float(thr))
        radii = [F32(0.5) * dist[i], F32(2) * dist[i]] if dist[i] > 0.5 else [F32(-0.01), F32(0.01)]
        for radius in radii:
            assert bool(ix.screen_probe(x, [i], radius, wg)[0]) == si.rejects(thr, radius), (i, float(radius), float(thr))
        assert ix.screen_probe(x, [i], radii[0], wg)[0] and not ix.screen_probe(x, [i], radii[1], wg)[0]
    ix.close()


# ---- 3. adversarial queries -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [509, 768, 2000])
@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_adversarial_queries_reject_no_row_inside_the_radius(capi, metric, d):
    c = rows_mod.case(capi, metric, d)
    rng = np.random.default_rng(d + 5)
    g = rng.standard_normal(d).astype(F32)
    out = g.copy(); out[d // 2] = F32(1e4)
    nan = g.copy(); nan[3] = F32(np.nan)
    inf = g.copy(); inf[d - 1] = F32(np.inf)
    queries = [("outlier", out), ("1e-25", g * F32(1e-25)), ("1e25", g * F32(1e25)), ("zero", np.zeros(d, F32)), ("nan", nan), ("inf", inf)]
    slots = np.arange(c.nfin)
    calls = 0
    for name, x in queries:
        with np.errstate(over="ignore", invalid="ignore"):
            dist = c.built.distance_gather(x, slots)
        fin = np.sort(dist[~np.isnan(dist)])
        with np.errstate(over="ignore"):
            radii = sorted({float(r) for r in (fin[:1].tolist() + fin[len(fin) // 2: len(fin) // 2 + 1].tolist() + fin[-1:].tolist())} |
                           {float(F32(2) * F32(r)) for r in fin[-1:].tolist() if r >= 0})
        for n_, radius in enumerate(radii):
            inside = [int(j) for j in np.argsort(-dist, kind="stable") if dist[j] <= radius][:64]
            if inside:
                got = c.built.screen_probe(x, inside, radius, 256 if n_ % 2 else 512)
                calls += 1
                assert not got.any(), (name, radius, [(c.fam[i], float(dist[i])) for i, r in zip(inside, got) if r])
        if name in ("zero", "nan", "inf"):
            assert not si.Staged(x, metric, ra=F32(1)).ok
            for n_, radius in enumerate((-np.inf, -1.0, 0.0, 1e-30, 1.0, 1e30)):
                assert not c.built.screen_probe(x, list(range(min(64, c.nfin))), radius, 256 if n_ % 2 else 512).any(), (name, radius)
    assert calls >= 6


# ---- 4. whole walks ---------------------------------------------------------------------------------------------------------------
N, D_, NQ, K = 3000, 513, 64, 10


def plan_of(capi, metric, screen, **over):
    f = dict.fromkeys(capi.PLAN_SEARCH_IN, 0)
    f.update(chunks=(D_ + 3) // 4, M=16, M0=32, mcode=M_CODE[metric], n=N, ef_default=64, num_cus=256, search_vis_slots=-1, nq=NQ, k=K, waves=4, env_wide_rows=-1, screen=screen)
    f.update(over)
    out, why = capi.plan_search(f)
    assert why is None
    return out


@pytest.mark.parametrize("metric", ["l2sq", "cos"])
def test_walks_with_the_screen_on_and_off_are_byte_identical(capi, metric, monkeypatch):
    from lantern_amd import hip

    rng = np.random.default_rng(23)
    centres = rng.standard_normal((12, D_), dtype=np.float32) * 2
    base = (centres[rng.integers(0, 12, N)] + rng.standard_normal((N, D_), dtype=np.float32)).astype(F32)
    queries = (centres[rng.integers(0, 12, NQ)] + rng.standard_normal((NQ, D_), dtype=np.float32)).astype(F32)
    monkeypatch.delenv("LANTERN_GPU_SPEC", raising=False)
    monkeypatch.delenv("LANTERN_GPU_SCREEN", raising=False)
    on = capi.GpuIndex(metric, D_, M=16, ef_construction=64, ef=64, seed=1)
    on.set_add_batch(512, 16)
    on.add_many(np.arange(N, dtype=np.uint64) + 1, base)
    on.flush()
    monkeypatch.setenv("LANTERN_GPU_SCREEN", "0")
    off = capi.GpuIndex(metric, D_, M=16, ef_construction=64, ef=64, seed=1)
    off.import_graph(base, on.export_graph())
    monkeypatch.delenv("LANTERN_GPU_SCREEN", raising=False)
    assert on.export_screen()["row_bytes"] == ((D_ + 3) // 4 + 3) // 4 * 16 and off.export_screen()["row_bytes"] == 0
    rows = on.device_query_rows(queries)
    stride = rows.strides[0]
    dq = hip.Buffer.from_numpy(rows)
    kinds = [("lab", 8, np.uint64, K), ("dist", 4, np.uint32, K), ("slot", 4, np.uint32, K), ("D", 8, np.uint64, 1), ("E", 8, np.uint64, 1)]
    bufs = {name: hip.Buffer(NQ * w * size) for name, size, _, w in kinds}

    def run(ix, waves, ef, each):
        ix.set_search_shape(waves)
        if each:
            params = [(K if q % 3 else 3, ef if q % 2 else ef // 2, q % 4) for q in range(NQ)]
            ix.search_batch_params_device(dq.ptr, stride, NQ, params, K, bufs["lab"].ptr, bufs["dist"].ptr, bufs["slot"].ptr, None, bufs["D"].ptr, bufs["E"].ptr)
        else:
            ix.search_batch_device(dq.ptr, NQ, K, ef, 0, bufs["lab"].ptr, bufs["dist"].ptr, bufs["slot"].ptr, None, bufs["D"].ptr, bufs["E"].ptr, query_stride=stride)
        hip.synchronize()
        return {name: bufs[name].download((NQ, w), dt).copy() for name, _, dt, w in kinds}

    for waves, ef, each in ((4, 64, False), (8, 64, False), (4, 128, False), (8, 128, False), (4, 64, True), (4, 128, True)):
        s0 = on.screen_stats()
        a, b = run(on, waves, ef, each), run(off, waves, ef, each)
        s1 = on.screen_stats()
        for name in a:
            assert np.array_equal(a[name], b[name]), (metric, waves, ef, each, name)
        assert s1[0] - s0[0] == int(a["D"].sum()) and 0 < s1[1] - s0[1] < s1[0] - s0[0], (metric, waves, ef, each, s0, s1)  # the screen ran, and rejected rows
    assert off.screen_stats() == (0, 0)
    # the plan: the planes' block in the screened launch, out of vis_slots; none without a screen, in the latency-bound shape, with the list in LDS
    block = 16 + ((D_ + 3) // 4 + 3) // 4 * 32
    for ef in (64, 128):
        with_, without = plan_of(capi, metric, 1, ef=ef), plan_of(capi, metric, 0, ef=ef)
        assert with_["screen_lds"] == block and without["screen_lds"] == 0
        assert with_["lds"] == without["lds"] + block - 4 * (without["vis_slots"] - with_["vis_slots"]) <= 26 * 1024
        assert 0 <= without["vis_slots"] - with_["vis_slots"] <= (block + 1023) // 1024 * 256
        assert {k: v for k, v in without.items() if k != "screen_lds"} == capi.plan_search({k: v for k, v in dict.fromkeys(capi.PLAN_SEARCH_IN, 0).items()} | dict(
            chunks=(D_ + 3) // 4, M=16, M0=32, mcode=M_CODE[metric], n=N, ef_default=64, num_cus=256, search_vis_slots=-1, nq=NQ, k=K, waves=4, env_wide_rows=-1, ef=ef))[0]
    assert plan_of(capi, metric, 1, waves=0)["screen_lds"] == 0 and plan_of(capi, metric, 1, waves=0)["spec"] == 2
    assert plan_of(capi, metric, 1, env_lds_list=1)["screen_lds"] == 0 and plan_of(capi, metric, 1, ef=200)["screen_lds"] == 0
    # a filtered launch of the same index carves what it carved without a screen
    allow = np.arange(1, N + 1, 3, dtype=np.uint64)
    shapes = []
    for ix in (on, off):
        f = ix.filter_from_labels(allow)
        ix.search_batch_filtered(f, queries, K, 64)
        shapes.append(ix.last_filtered_launch())
        f.close()
    assert shapes[0] == shapes[1] and shapes[0]["path"] is not None, shapes
    on.close()
    off.close()
