"""The visited set of the UNFILTERED walks where a workgroup takes its next query on the bitmap the previous walk wrote (walk.hpp
"visited set", VisUndo): every walk must hand its workgroup's HBM bitmap back all-zero, inside the launch.  Needs an MI355X.

Every case runs (1) a base line with one query per workgroup, (2) the same batch on W = 1 and W = 3 workgroups (set_search_shape: the
walks of a workgroup follow each other in one launch, by position or by ticket), (3) that launch again, (4) that launch with the queries
rolled by one, so that a bitmap meets a query other than the one that wrote it.  All must equal the oracle on the same graph -- slots,
labels, distance bits, counts, D and E, no tolerance -- and one another: a stale bit makes a walk take a row for visited, and D drops.

Each case states its launch through lantern_gpu_plan_search on the launch's own fields (vis_slots, kernel family, the int8 planes' block,
which instantiation of the classic kernel -- wide_rows: four rows in flight per group at 64 queries, two, the shape of a batch that fills the chip,
at 1088 --, grid = last_search_grid) and proves its regime -- every walk spills, keeps or overflows its undo log -- from the oracle's evaluation
counts (tests/visited_regimes.py; tests/test_visited_regimes_ref.py proves the same without a device).  LANTERN_GPU_VIS_UNDO is read once
per process: the forced overflows of the register-list walks are in tests/test_gpu_visited_undo_probe.py.
"""
import numpy as np
import pytest

from tests import visited_regimes as vr
from tests.test_gpu_search_params import small_mix

pytestmark = pytest.mark.gpu

LAUNCH_ENV = ("LANTERN_GPU_SPEC", "LANTERN_GPU_LDS_LIST", "LANTERN_GPU_PQ_ADC", "LANTERN_GPU_ADC_SPEC", "LANTERN_GPU_SPEC_WAVES", "LANTERN_GPU_SCREEN",
              "LANTERN_GPU_SCREEN_LIST_PREFETCH")


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


@pytest.fixture(scope="module")
def made():
    return {}


def set_env(monkeypatch, env):
    for name in LAUNCH_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def gpu_index(made, capi, monkeypatch, name, V):
    """the oracle's graph of index `name` on the device, made under LANTERN_GPU_VIS_SLOTS = V (read when an index is made); one per module"""
    if (name, V) not in made:
        ix = vr.index_of(name)
        set_env(monkeypatch, {})
        monkeypatch.setenv("LANTERN_GPU_VIS_SLOTS", str(V))
        gpu = capi.GpuIndex(ix["metric"], ix["d"], M=ix["M"], ef_construction=ix["efc"], ef=vr.EF_DEFAULT, seed=vr.INDEX_SEED, quantization=ix["storage"])
        gpu.import_graph(ix["base"], ix["g"])
        monkeypatch.delenv("LANTERN_GPU_VIS_SLOTS")
        assert (gpu.export_screen(0, 1)["row_bytes"] > 0) == (name in vr.SCREENED)
        made[(name, V)] = gpu
    return made[(name, V)]


def hand_back(gpu, queries, params, want, Ws, state, what, width=vr.K):
    """steps (1) .. (4) of the module's docstring; state(W) -> the plan of the launch with W workgroups (0: the default grid)"""
    A, B = vr.Launcher(gpu, queries, width), vr.Launcher(gpu, np.roll(queries, 1, axis=0), width)
    rolled_params, rolled_want = vr.roll_params(params), vr.rolled(want)
    try:
        gpu.set_search_shape(0, 0)
        base = A.run(params)
        assert gpu.last_search_grid() == state(0)["grid"], (what, gpu.last_search_grid())
        vr.check(base, want, f"{what}: one query per workgroup")
        for W in Ws:
            gpu.set_search_shape(0, max_workgroups=W)
            grid = state(W)["grid"]
            first = A.run(params)
            assert gpu.last_search_grid() == grid, (what, W, "the launch is not the one planned", gpu.last_search_grid(), grid)
            again = A.run(params)
            roll = B.run(rolled_params)
            assert gpu.last_search_grid() == grid
            vr.check(first, want, f"{what}: W = {W}")
            vr.check(again, want, f"{what}: W = {W}, the launch repeated")
            vr.check(roll, rolled_want, f"{what}: W = {W}, the queries rolled by one")
            vr.check(first, base, f"{what}: W = {W} against one query per workgroup")
            vr.check(again, first, f"{what}: W = {W}, the repeated launch against the first")
    finally:
        gpu.set_search_shape(0, 0)


# ------------------------------------------------------------------------------------------------
# the uniform launches: classic (plain and screened), the LDS list, the latency-bound walks, the row kinds, the natural log regimes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lid,V", [(lid, V) for lid, L in vr.LAUNCHES.items() for V in L["V"]], ids=lambda x: str(x))
def test_walks_hand_their_bitmap_back_inside_a_launch(capi, oracle, made, monkeypatch, lid, V):
    L = vr.LAUNCHES[lid]
    ix = vr.index_of(L["index"])
    gpu = gpu_index(made, capi, monkeypatch, L["index"], V)
    want = vr.reference(L["index"], L["ef"])
    vr.assert_regime(L["regime"], want[3], vr.descent(L["index"]), V)
    nq = L.get("nq", len(ix["oq"]))
    set_env(monkeypatch, L["env"])
    before = gpu.screen_stats()
    state = lambda W: vr.stated(capi, ix, V, W, nq, L["ef"], L["env"], L["path"], L["screen"], wide=vr.wide_of(L["path"], nq))  # noqa: E731
    hand_back(gpu, vr.tiled(ix["queries"], nq), L["ef"], vr.tiled(want, nq), L["W"], state, f"{lid} V = {V}")
    logical, exact = (a - b for a, b in zip(gpu.screen_stats(), before))
    if L["screen"]:  # the screened form of the walk ran (undo_apply<FRESH_ZERO>), and rejected rows
        assert 0 < exact < logical, (lid, logical, exact)


@pytest.mark.parametrize("V", [256, 0])
def test_more_than_twice_the_full_grid_of_queries(capi, oracle, made, monkeypatch, V):
    """2 x grid + 7 queries without a cap: every workgroup of the full classic grid takes a second and a third query, by ticket"""
    ix = vr.small_index("l2_64")
    gpu = gpu_index(made, capi, monkeypatch, "l2_64", V)
    set_env(monkeypatch, {})
    want = vr.reference("l2_64", 64)
    vr.assert_regime("within", want[3], vr.descent("l2_64"), V)
    full = vr.stated(capi, ix, V, 0, 10**6, 64, {}, "classic", 0)["grid"]
    nq = 2 * full + 7
    reps = -(-nq // vr.NQ)
    tiled = tuple(np.concatenate([a] * reps)[:nq] for a in want)
    big = vr.Launcher(gpu, np.tile(ix["queries"], (reps, 1))[:nq])
    gpu.set_search_shape(0, 0)
    for _ in range(2):
        got = big.run(64)
        assert gpu.last_search_grid() == full == vr.stated(capi, ix, V, 0, nq, 64, {}, "classic", 0)["grid"]
        vr.check(got, tiled, f"{nq} queries on {full} workgroups, V = {V}")


# ------------------------------------------------------------------------------------------------
# per-query parameters
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["0", None], ids=["LANTERN_GPU_SPEC=0", "LANTERN_GPU_SPEC unset"])
def test_per_query_parameter_launches(capi, oracle, made, monkeypatch, spec):
    """search_batch_params with three classes in one call (three launches, each on two workgroups), every walk past its 256 LDS slots"""
    V, width = 256, 129
    ix = vr.small_index("l2_64")
    gpu = gpu_index(made, capi, monkeypatch, "l2_64", V)
    params = tuple(small_mix(vr.NQ))
    want = vr.reference("l2_64", params)
    vr.assert_regime("within", want[3], vr.descent("l2_64"), V)
    env = vr.env_of(spec=spec)
    set_env(monkeypatch, env)
    hand_back(gpu, ix["queries"], params, want, (2,), lambda W: vr.stated_each(capi, ix, V, W, params, env, width), f"per-query, LANTERN_GPU_SPEC={spec}", width)
    regime = gpu.last_params_launch()
    assert regime["launches"] == 3 and regime["spec"] == (spec is None), regime


@pytest.mark.parametrize("V", [256, 0])
def test_natural_mixed_log_regimes_in_one_launch(capi, oracle, made, monkeypatch, V):
    """per-query ef 400 | 1000 by turns on the 30000 x 64 index: walks that clear their whole bitmap and walks that undo their log, on the
    same bitmaps in one launch -- W = 2 and the default grid"""
    ix = vr.big_index()
    gpu = gpu_index(made, capi, monkeypatch, "big", V)
    want = vr.reference("big", vr.BIG_MIXED)
    U = vr.descent("big")
    vr.assert_spills(want[3], U, V)
    vr.assert_mixed(want[3], U, V)
    set_env(monkeypatch, {})
    hand_back(gpu, ix["queries"], vr.BIG_MIXED, want, (2, 0), lambda W: vr.stated_each(capi, ix, V, W, vr.BIG_MIXED, {}, vr.K), f"big mixed V = {V}")
    assert gpu.last_params_launch()["launches"] == 1


# ------------------------------------------------------------------------------------------------
# a compact pq index: rows decoded on the fly, and ADC over the code bytes
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pq_index(capi, oracle):
    """Built on the device under LANTERN_GPU_VIS_SLOTS=256 (a pq index cannot be imported), compacted; the referee walks its exported graph
    over the decoded rows, and -- for ADC -- through set_pq_view in ADC's own summation order, as tests/test_gpu_quantized_indexes.py does."""
    from tests.test_gpu_quantized_indexes import make_codebook

    metric, n, d, S, C, M, efc = vr.PQ_SHAPE
    rng = np.random.default_rng(vr.DATA_SEED)
    base, queries = rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((vr.NQ, d), dtype=np.float32)
    cb = make_codebook(rng, base, S, C)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LANTERN_GPU_VIS_SLOTS", "256")
        gpu = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=vr.EF_DEFAULT, seed=vr.INDEX_SEED, pq_codebook=cb, num_subvectors=S)
    gpu.set_add_batch(256, 16)
    gpu.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    gpu.flush()
    codes = gpu.export_codes()
    g = gpu.export_graph(with_vectors=True)
    gpu.pq_compact()
    fields = {"name": "pq", "metric": metric, "n": n, "d": d, "M": M, "chunks": d // 4, "mcode": vr.M_CODE[metric], "queries": queries}

    def referee(adc):
        ora = oracle.OracleIndex.from_graph(metric, g["vectors"], g, M, efc, vr.EF_DEFAULT, vr.INDEX_SEED, oracle.SUM_WAVE64)
        if adc:
            ora.set_pq_view(cb, codes)
        lab, dist, slot, D, E = ora.search_batch(queries, vr.K, 64, vr.THREADS)
        return (slot, dist, np.full(vr.NQ, vr.K, dtype=np.uint32), D, E, lab), vr.descent_of(ora, queries)

    return gpu, fields, {False: referee(False), True: referee(True)}, (S + 15) // 16 * 16


@pytest.mark.parametrize("mode", ["decoded-classic", "decoded", "adc", "adc-classic"])
def test_compact_pq_walks(capi, pq_index, monkeypatch, mode):
    gpu, ix, referees, S16 = pq_index
    adc = mode.startswith("adc")
    want, U = referees[adc]
    V = 256
    vr.assert_regime("within", want[3], U, V)  # (the graph is the device's own: proven here, on its export)
    env = vr.env_of(spec=0 if mode == "decoded-classic" else None, pq_adc=int(adc))
    set_env(monkeypatch, env)
    if mode == "adc-classic":  # the 8-wave ADC walk (64 queries take the 3 + 8 wave shape unasked)
        monkeypatch.setenv("LANTERN_GPU_ADC_SPEC", "0")
    # (pqd_inv: any non-zero value says "subvectors of whole 16-byte chunks" to the plan; the ADC launch has the code rows' chunks)
    over = dict(pq_compact=1, pqd_inv=1, pq_S16=S16, env_adc_spec_set=int(mode == "adc-classic"))
    path = "adc" if adc else "pqd"

    def state(W):
        p = vr.stated(capi, ix, V, W, vr.NQ, 64, env, path, 0, **over)
        assert p["took_spec"] == int(mode in ("decoded", "adc")), (mode, p)
        return p

    hand_back(gpu, ix["queries"], 64, want, (1, 3), state, f"compact pq, {mode}")


# ------------------------------------------------------------------------------------------------
# the insertion walks: k_insert, plain and screened, on three workgroups
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,V", [(name, V) for name in vr.INSERTS for V in vr.INSERT_VIS[name]], ids=lambda x: str(x))
def test_capped_insertion_build_is_the_oracles_graph(capi, oracle, monkeypatch, name, V):
    """A batch of more than 2 x CUs rows walked by k_insert on THREE workgroups (set_search_shape caps the insertion grid too: index.cpp
    run_batch): a few hundred insertion walks follow each other on each bitmap.  The graph is the oracle's add_planned graph edge for edge,
    and the uncapped build's checksum."""
    metric, n, d, M, efc, first, screen = vr.INSERTS[name]
    o = vr.insert_oracle(name)
    assert o["big"] > 2 * vr.NUM_CUS
    # PROXY for the spill of the insertion walks (they have no oracle D): the oracle's search at ef = ef_construction for the batch's own rows,
    # on the graph the batch walks, evaluates more than V rows below the descent.  V = 0 needs none: every visit of a walk is a bitmap visit.
    assert V == 0 or o["batch"].min() > V
    set_env(monkeypatch, {})
    monkeypatch.setenv("LANTERN_GPU_INSERT_VIS_SLOTS", str(V))

    def build(W):
        ix = capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=vr.EF_DEFAULT, seed=vr.INDEX_SEED)
        try:
            ix.set_insert_screen(screen)
            ix.set_search_shape(0, max_workgroups=W)
            ix.set_add_batch(*vr.INSERT_FIRST_PLAN)
            ix.add_many(o["labels"][:first], o["base"][:first])
            ix.flush()
            ix.set_add_batch(*vr.INSERT_PLAN)
            ix.add_many(o["labels"][first:], o["base"][first:])
            ix.flush()
        finally:
            ix.set_search_shape(0, 0)
        return ix

    capped, free = build(vr.INSERT_W), build(0)
    for ix in (capped, free):
        screened, plain, tested, rejected = ix.insert_screen_stats()
        assert screened + plain >= 1, "no batch of the build went to k_insert"
        if screen:
            assert screened >= 1 and tested > 0 and 0 < rejected <= tested, (screened, plain, tested, rejected)
        else:
            assert screened == 0 and tested == 0
    vr.same_graph(capped.export_graph(), o["g"], f"{name} on {vr.INSERT_W} workgroups against the oracle")
    vr.same_graph(free.export_graph(), o["g"], f"{name} uncapped against the oracle")
    assert capped.checksum() == free.checksum()
