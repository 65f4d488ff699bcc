"""The regime conditions of the visited-set tests (tests/visited_regimes.py), on the oracle and the launch plan alone: the evaluation counts
that make every walk of tests/test_gpu_visited_regimes.py and tests/visited_undo_probe.py spill, keep its undo log, overflow it, or do
both in one launch -- and lantern_gpu_plan_search's word that each launch has the LDS visited set, the kernel family and the grid the case
means.  No device needed: a change of data, seed or plan cannot silently empty a GPU case, it fails here."""
import numpy as np
import pytest

from tests import visited_regimes as vr
from tests.test_gpu_search_params import small_mix


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import build, capi

    build.build()
    capi.lib()
    return capi


def counts(name, params):
    D = vr.reference(name, params)[3].astype(np.int64)
    return D, vr.descent(name)


@pytest.mark.parametrize("lid", list(vr.LAUNCHES))
def test_uniform_launches_are_in_their_regimes(capi, oracle, lid):
    L = vr.LAUNCHES[lid]
    ix = vr.index_of(L["index"])
    D, U = counts(L["index"], L["ef"])
    nq = L.get("nq", len(ix["oq"]))
    print(f"{lid}: D {D.min()} .. {D.max()}, U {U.min()} .. {U.max()}, D - U >= {(D - U).min()}")
    res = vr.reference(L["index"], L["ef"])
    assert len({tuple(r) for r in res[0].tolist()}) == len(ix["oq"])  # (all answers differ: a launch that mixed its queries up shows)
    for V in L["V"]:
        vr.assert_regime(L["regime"], D, U, V)
        for W in (0,) + tuple(L["W"]):
            p = vr.stated(capi, ix, V, W, nq, L["ef"], L["env"], L["path"], L["screen"], wide=vr.wide_of(L["path"], nq))
            assert p["grid"] == (W or nq) and p["expansion"] == L["ef"]
            assert p["lds_list"] == int("LANTERN_GPU_LDS_LIST" in L["env"])
    if lid == "classic-ef64":  # the batch of more than twice the full grid: the classic shape by itself
        full = vr.stated(capi, ix, 256, 0, 10**6, 64, {}, "classic", 0)["grid"]
        assert vr.stated(capi, ix, 256, 0, 2 * full + 7, 64, {}, "classic", 0)["grid"] == full == 6 * vr.NUM_CUS


def test_the_large_index_mixes_both_log_regimes_in_one_launch(capi, oracle):
    ix = vr.big_index()
    D, U = counts("big", vr.BIG_MIXED)
    for V in (256, 0):
        vr.assert_spills(D, U, V)
        over = vr.assert_mixed(D, U, V)
        assert np.array_equal(over, np.arange(len(D)) % 2 == 1)  # the ef = 1000 walks
        for W in (0, 2):
            p = vr.stated_each(capi, ix, V, W, vr.BIG_MIXED, {}, vr.K)
            assert p["grid"] == (W or len(D)) and p["expansion"] == 1000
    assert [c for c, _ in vr.classes_of(vr.BIG_MIXED)] == [0, 0, len(D)]  # both in the LDS-list class: one launch


def test_rolled_reference_is_the_reference_of_the_rolled_batch(oracle):
    ix = vr.small_index("l2_64")
    want = vr.rolled(vr.reference("l2_64", vr.PROBE_MIXED))
    got = vr.answers(ix["ora"], np.roll(ix["oq"], 1, axis=0), vr.roll_params(vr.PROBE_MIXED))
    vr.check(got, want, "rolled")
    assert vr.roll_params(vr.PROBE_MIXED)[0] == vr.PROBE_MIXED[-1] != vr.PROBE_MIXED[0]


def test_per_query_batch_spills_in_every_class(capi, oracle):
    params = tuple(small_mix(vr.NQ))
    D, U = counts("l2_64", params)
    vr.assert_regime("within", D, U, 256)
    assert all(c >= 8 for c, _ in vr.classes_of(params)), vr.classes_of(params)
    ix = vr.small_index("l2_64")
    for env in (vr.env_of(spec=0), {}):
        p = vr.stated_each(capi, ix, 256, 2, params, env, 129)
        assert p["grid"] == 2 and p["expansion"] == 136


@pytest.mark.parametrize("run", list(vr.PROBE_RUNS))
def test_probe_runs_are_in_their_regimes(capi, oracle, run):
    undo, V, regime = vr.PROBE_RUNS[run]
    cap = vr.MIXED_CAP if undo is None else undo
    for name in vr.PROBE_INDEXES:
        ix = vr.small_index(name)
        D, U = counts(name, 64)
        vr.assert_regime("overflow", D, U, V, cap)  # the uniform launches: every walk overflows, in every run
        De, _ = counts(name, vr.PROBE_MIXED)
        print(f"{run} {name}: ef 8 D {De[0::2].min()} .. {De[0::2].max()}, ef 64 D - U {(De - U)[1::2].min()} .. {(De - U)[1::2].max()}")
        if regime == "mixed":
            over = vr.assert_mixed(De, U, V, cap)
            assert np.array_equal(over, np.arange(vr.NQ) % 2 == 1)
        for family, env in vr.PROBE_FAMILIES.items():
            screened = family == "classic" and name in vr.SCREENED
            for W in vr.PROBE_W:
                assert vr.stated(capi, ix, V, W, vr.NQ, 64, env, family, screened, wide=vr.wide_of(family, vr.NQ))["grid"] == W
        for family, env in vr.PROBE_EACH_FAMILIES.items():
            screened = family == "classic" and name in vr.SCREENED
            for W in vr.PROBE_W:
                p = vr.stated_each(capi, ix, V, W, vr.PROBE_MIXED, env, vr.PROBE_K, screened)
                assert p["grid"] == W and p["path"] == vr.PATHS[family]
    assert [c for c, _ in vr.classes_of(vr.PROBE_MIXED)] == [vr.NQ, 0, 0]
    for name, ef in vr.PROBE_TILED:  # the screened walk with two rows per group: every walk overflows, in every run
        D, U = counts(name, ef)
        vr.assert_regime("overflow", D, U, V, cap)
        p = vr.stated(capi, vr.small_index(name), V, vr.INSERT_W, vr.TILED_NQ, ef, vr.env_of(spec=0), "classic", 1, wide=0)
        assert p["grid"] == vr.INSERT_W
    # the probe's build: every batch by k_insert on three workgroups.  PROXY (an insertion walk has no oracle D): the oracle's search at
    # ef = ef_construction on the finished graph
    proxy = vr.probe_insert_oracle()["finished"]
    if regime == "overflow":
        assert (proxy - V).min() > cap, (proxy.min(), V, cap)


@pytest.mark.parametrize("name", list(vr.INSERTS))
def test_insertion_builds_reach_k_insert_and_spill(oracle, name):
    metric, n, d, M, efc, first, screen = vr.INSERTS[name]
    o = vr.insert_oracle(name)
    assert o["big"] > 2 * vr.NUM_CUS  # plan_insert: more rows than the lone-insertion walk takes -- k_insert, whose grid the cap reaches
    print(f"{name}: batch of {o['big']}, finished-graph proxy D - U {o['finished'].min()} .. {o['finished'].max()}, "
          f"the batch's own rows on the graph they walk {o['batch'].min()} .. {o['batch'].max()}")
    for V in vr.INSERT_VIS[name]:
        # PROXY for the insertion walks' spill, on the graph the big batch walks (V = 0 needs none: every visit is a bitmap visit)
        assert V == 0 or o["batch"].min() > V
    assert max(o["batch"].max(), o["finished"].max()) + 1 + 256 <= vr.UNDO_WORDS  # (U <= 256: every log is kept)
