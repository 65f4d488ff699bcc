"""The indexes, launches and regime conditions of the visited-set tests of the UNFILTERED walks, shared by tests/test_visited_regimes_ref.py
(which proves every condition on the oracle and the launch plan alone, no device) and tests/test_gpu_visited_regimes.py,
tests/visited_undo_probe.py and tests/test_gpu_visited_undo_probe.py (which run the kernels in them).

Test infrastructure, not part of the product.  What the conditions are about (walk.hpp "visited set", VisUndo): a walk keeps its visited set
in V = vis_slots LDS slots and spills to its workgroup's HBM bitmap at three quarters; ids that go into the bitmap are appended to an undo
log of `cap` entries (kVisUndoWords, or LANTERN_GPU_VIS_UNDO) and the walk zeroes the words the log names when it ends -- or, past `cap`
ids, the whole bitmap.  A persistent workgroup starts its next query on that bitmap in the same launch, so a bit left behind makes the
next walk take a row for visited.  Per query, with
    D = the oracle's evaluation count at the query's expansion,
    U = the oracle's D of the same query at ef = 1, k = 1 (the greedy descent is part of every walk: U bounds the evaluations above level 0),
a walk records between D - U - V and D + 1 ids in its bitmap, so it
    spills                          if D - U > V            (V = 0: every visit is a bitmap visit, nothing to prove),
    keeps its log                   if D + 1 <= cap,
    overflows its log for certain   if D - U - V > cap,
and a launch is MIXED if at least 8 of its queries are on each side and none in between.  A missed condition is a failure, never a skip.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import filtered_regimes

UNDO_WORDS = filtered_regimes.UNDO_WORDS  # device_common.hpp kVisUndoWords
THREADS = filtered_regimes.THREADS
NUM_CUS = 256  # an MI355X; every planned grid is held to the launch's own (last_search_grid), so another chip fails loudly
NQ, K = 64, 10
DATA_SEED, INDEX_SEED, EF_DEFAULT = 5, 9, 64
EMPTY = 0xFFFFFFFF
PATHS = {"adc": 0, "pqd": 1, "classic": 2, "spec1": 3, "spec2": 4}  # tests/test_search_plan.py PATHS
M_CODE = {"cos": 1, "l2sq": 3, "hamming": 8}                        # device_common.hpp M_COS, M_L2SQ, M_HAMMING
M_STORAGE = {"f32": 0, "f16": 100, "i8": 200}                       # ... + M_F16, + M_I8

# name -> metric, n, d (f32 scalars; u32 words for hamming), M, efc, storage.  Gaussian rows, data seed 5, index seed 9, 64 queries.
SHAPES = {
    "l2_64": ("l2sq", 4000, 64, 16, 64, "f32"),     # 16 chunks: 8 lanes per row
    "l2_768": ("l2sq", 2500, 768, 16, 64, "f32"),   # 192 chunks: 64 lanes per row, an int8 screen
    "cos_768": ("cos", 2500, 768, 16, 64, "f32"),
    "f16_768": ("l2sq", 1500, 768, 16, 64, "f16"),
    "i8_256": ("cos", 1500, 256, 16, 64, "i8"),
    "b1_24": ("hamming", 3000, 24, 16, 64, "f32"),  # bit rows: 768 bits in 24 words
}
PQ_SHAPE = ("l2sq", 3000, 128, 32, 256, 8, 48)  # metric, n, d, S, C, M, efc: built on the device (a pq index cannot be imported)
# The insertion walks: metric, n, d, M, efc, rows of the first part, insert screen.  k_insert takes batches of MORE than 2 x CUs rows
# (insert_batch.cpp plan_insert: smaller ones go to the lone-insertion walk, whose grid set_search_shape does not cap), and under plan (512, 16)
# no batch of these builds has more than n / 16 rows.  So the first part is built under (512, 16) and the rest is added under (1024, 1):
# one batch of min(rows so far, 1024, rows left) > 512 rows, all of whose walks run on the first part's graph -- by k_insert, W workgroups.
INSERT_FIRST_PLAN, INSERT_PLAN, INSERT_W = (512, 16), (1024, 1), 3
INSERTS = {
    "ins_64": ("l2sq", 1200, 64, 8, 40, 600, 0),
    "ins_768": ("l2sq", 2500, 768, 4, 32, 1000, 1),  # batches of 1000 (k_insert, screened) and 500 rows (the lone walk)
}
# LANTERN_GPU_INSERT_VIS_SLOTS: 0, where every visit of a walk is a bitmap visit and nothing needs proving.  There is no 256 leg here: the
# big batch of ins_64 walks the FIRST PART's 600-row graph, on which the oracle's search at ef = 40 for the batch's own rows has D - U =
# 217 .. 326 -- not above 256 for every row (nor with 640 or 680 rows in the first part: 220, 246), so the spill of every walk cannot be
# shown.  The 256 leg of the insertion walks is the probe's build (PROBE_INSERT: plan (512, 16), every batch by k_insert).
INSERT_VIS = {"ins_64": (0,), "ins_768": (0,)}


def chunks_of(d, storage, metric):
    """16-byte chunks of a stored row (index.cpp usearch_init)"""
    words = d if metric == "hamming" else (d + 1) // 2 if storage == "f16" else (d + 3) // 4 if storage == "i8" else d
    chunks = (words + 3) // 4
    return 8 if metric == "hamming" and 4 < chunks < 8 else chunks


def gaussian(name, n, d, metric, storage):
    rng = np.random.default_rng(DATA_SEED)
    if metric == "hamming":
        return rng.integers(0, 2**32, size=(n, d), dtype=np.uint32), rng.integers(0, 2**32, size=(NQ, d), dtype=np.uint32)
    scale = np.float32(0.4 if storage == "i8" else 1.0)
    return rng.standard_normal((n, d), dtype=np.float32) * scale, rng.standard_normal((NQ, d), dtype=np.float32) * scale


@functools.lru_cache(maxsize=None)
def small_index(name):
    """{base: the stored values, queries: what the device is handed, oq: what the oracle is handed, ora, g, ...} of an oracle-built index"""
    from oracle import binding as oracle

    metric, n, d, M, efc, storage = SHAPES[name]
    base, queries = gaussian(name, n, d, metric, storage)
    if metric == "hamming":
        sb, sq, mode = base, queries, oracle.SUM_WAVE64
    else:
        sb, sq, _, mode = filtered_regimes.stored_rows(oracle, storage, metric, base, queries)
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=EF_DEFAULT, seed=INDEX_SEED, sum_mode=mode)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, sb)
    return {"name": name, "metric": metric, "n": n, "d": d, "M": M, "efc": efc, "storage": storage, "base": sb, "queries": queries, "oq": sq,
            "ora": ora, "g": ora.export_graph(), "chunks": chunks_of(d, storage, metric), "mcode": M_CODE[metric] + M_STORAGE[storage]}


def big_index():
    """filtered_regimes.big_index("gauss") in the form of small_index: 30000 x 64 l2sq, 48 queries"""
    ix = filtered_regimes.big_index("gauss")
    return {"name": "big", "metric": "l2sq", "n": filtered_regimes.N, "d": filtered_regimes.DIM, "M": filtered_regimes.M, "efc": filtered_regimes.EFC,
            "storage": "f32", "base": ix["base"], "queries": ix["queries"], "oq": ix["queries"], "ora": ix["ora"], "g": ix["g"],
            "chunks": filtered_regimes.DIM // 4, "mcode": M_CODE["l2sq"]}


def index_of(name):
    return big_index() if name == "big" else small_index(name)


def answers(ora, oq, params, width=None):
    """The oracle's answer per query with that query's own (k, ef, skip), laid out as the device lays it out:
    (slots, dists, counts, D, E, labels), rows `width` wide, the tail EMPTY / +inf / 0."""
    nq = len(params)
    width = max(p[0] for p in params) if width is None else width
    slots, dists = np.full((nq, width), EMPTY, dtype=np.uint32), np.full((nq, width), np.inf, dtype=np.float32)
    labs = np.zeros((nq, width), dtype=np.uint64)
    counts, D, E = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint64), np.zeros(nq, dtype=np.uint64)
    for q, (k, ef, skip) in enumerate(params):
        lab, dst, slt = ora.search(oq[q], k, ef, skip)
        c = len(lab)
        labs[q, :c], dists[q, :c], slots[q, :c], counts[q] = lab, dst, slt, c
        D[q], E[q] = ora.last_counters()
    return slots, dists, counts, D, E, labs


@functools.lru_cache(maxsize=None)
def reference(name, params):
    """answers() of index `name` for `params`: an int (a uniform launch at that ef, k = K) or a tuple of (k, ef, skip) per query"""
    ix = index_of(name)
    nq = len(ix["oq"])
    if isinstance(params, int):
        lab, dist, slot, D, E = ix["ora"].search_batch(ix["oq"], K, params, THREADS)
        return slot, dist, np.full(nq, K, dtype=np.uint32), D, E, lab
    return answers(ix["ora"], ix["oq"], params)


def descent_of(ora, oq):
    """U per query: the oracle's D at ef = 1, k = 1"""
    return ora.search_batch(oq, 1, 1, THREADS)[3].astype(np.int64)


@functools.lru_cache(maxsize=None)
def descent(name):
    ix = index_of(name)
    return descent_of(ix["ora"], ix["oq"])


def rolled(res, shift=1):
    """a reference answer for the batch rolled by `shift`: query i of the batch is query (i - shift) of the reference"""
    return tuple(np.roll(a, shift, axis=0) for a in res)


# ------------------------------------------------------------------------------------------------
# the conditions
# ------------------------------------------------------------------------------------------------
def assert_spills(D, U, V):
    D, U = np.asarray(D).astype(np.int64), np.asarray(U).astype(np.int64)
    assert V == 0 or (D - U).min() > V, ("spills", V, int((D - U).min()))


def assert_within(D, cap=UNDO_WORDS):
    D = np.asarray(D).astype(np.int64)
    assert D.max() + 1 <= cap, ("within", cap, int(D.max()))


def assert_overflows(D, U, V, cap=UNDO_WORDS):
    D, U = np.asarray(D).astype(np.int64), np.asarray(U).astype(np.int64)
    assert (D - U - V).min() > cap, ("overflow", cap, V, int((D - U - V).min()))


def assert_mixed(D, U, V, cap=UNDO_WORDS):
    """-> bool[nq]: the queries that overflow.  (A per-query launch walks its list by expansion, descending -- search_plan.cpp
    search_params_locked -- so inside a launch the clearing walks of a workgroup come first and hand over to the logged ones; a logged walk in
    front of a clearing one is the last walk of a launch and the first of the repeated launch on the same bitmap.)"""
    D, U = np.asarray(D).astype(np.int64), np.asarray(U).astype(np.int64)
    within, over = D + 1 <= cap, D - U - V > cap
    assert within.sum() >= 8 and over.sum() >= 8 and np.all(within | over), ("mixed", cap, V, np.sort(D).tolist())
    return over


def assert_regime(regime, D, U, V, cap=UNDO_WORDS):
    assert_spills(D, U, V)
    if regime == "within":
        assert_within(D, cap)
    elif regime == "overflow":
        assert_overflows(D, U, V, cap)
    else:
        assert regime == "mixed", regime
        assert_mixed(D, U, V, cap)


# ------------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------------
def env_of(spec=None, lds_list=0, pq_adc=0):
    """the environment of a launch: LANTERN_GPU_SPEC (None: unset), LANTERN_GPU_LDS_LIST, LANTERN_GPU_PQ_ADC"""
    e = {}
    if spec is not None:
        e["LANTERN_GPU_SPEC"] = str(spec)
    if lds_list:
        e["LANTERN_GPU_LDS_LIST"] = "1"
    if pq_adc:
        e["LANTERN_GPU_PQ_ADC"] = "1"
    return e


def plan(capi, ix, V, W, nq, ef, env, screen=0, k=K, **over):
    """lantern_gpu_plan_search on the launch's own fields: the index's, search_vis_slots = V, search_max_wg = W, the environment's, the screen.
    A refusal is a failure."""
    f = dict.fromkeys(capi.PLAN_SEARCH_IN, 0)
    spec = env.get("LANTERN_GPU_SPEC")
    f.update(chunks=ix["chunks"], M=ix["M"], M0=2 * ix["M"], mcode=ix["mcode"], n=ix["n"], ef_default=EF_DEFAULT, num_cus=NUM_CUS,
             search_vis_slots=V, search_max_wg=W, nq=nq, k=k, ef=ef, env_spec_set=int(spec is not None), env_spec=int(spec or 0),
             env_lds_list=int(env.get("LANTERN_GPU_LDS_LIST", 0)), env_pq_adc=int(env.get("LANTERN_GPU_PQ_ADC", 0)), env_wide_rows=-1, screen=screen)
    f.update(over)
    out, why = capi.plan_search(f)
    assert why is None, (why, f)
    return out


def stated(capi, ix, V, W, nq, ef, env, path, screened, k=K, wide=None, **over):
    """plan() of a launch, held to what the case means to run: the LDS visited set of V slots, the kernel family, whether the launch screens
    and -- `wide` 0 | 1, None: not said -- which instantiation of the classic kernel it is: two rows in flight per group (the shape of a batch
    that fills the chip: the headline kernel) or four (64 .. 4 x CUs queries; search_launch.hpp ROWS)"""
    p = plan(capi, ix, V, W, nq, ef, env, screen=int(ix["name"] in SCREENED), k=k, **over)
    assert p["vis_slots"] == V and p["path"] == PATHS[path] and (p["screen_lds"] > 0) == bool(screened), (ix["name"], V, W, nq, ef, env, p)
    assert wide is None or p["wide_rows"] == wide, (ix["name"], V, W, nq, ef, env, p)
    return p


TILED_NQ = 1088  # 17 x 64 queries: 4 waves x 1088 > 16 x CUs, so the classic launch has TWO rows in flight per group (plan: wide_rows = 0)


def wide_of(path, nq):
    """plan_search's rule for the four-row shape of the classic kernel on 256 CUs"""
    return int(path == "classic" and 64 <= nq and 4 * nq <= 16 * NUM_CUS)


def tiled(res, nq):
    """a reference answer (or a batch of queries) of m rows repeated to nq rows: row i is row i % m"""
    if isinstance(res, tuple):
        return tuple(tiled(a, nq) for a in res)
    return np.concatenate([res] * (-(-nq // res.shape[0])))[:nq]


def classes_of(params, ef_default=EF_DEFAULT):
    """[(queries, largest expansion)] of the three list-placement classes of a per-query call (search_plan.cpp search_params_locked)"""
    e = np.array([max(ef or ef_default, k + skip) for k, ef, skip in params])
    sel = (e <= 64, (e > 64) & (e <= 128), e > 128)
    return [(int(m.sum()), int(e[m].max()) if m.any() else 0) for m in sel]


def stated_each(capi, ix, V, W, params, env, width, screened=False, **over):
    """stated() of the LAST launch of a per-query call (the one last_search_grid speaks of): its highest non-empty class.  The register-list
    classes take the 3 + 8 wave shape unless LANTERN_GPU_SPEC=0 or they have more than two queries per CU; the LDS-list class is classic."""
    c = max(i for i, (count, _) in enumerate(classes_of(params)) if count)
    count, top = classes_of(params)[c]
    spec2 = c < 2 and env.get("LANTERN_GPU_SPEC") != "0" and count <= 2 * NUM_CUS
    return stated(capi, ix, V, W, count, 0, env, "spec2" if spec2 else "classic", screened and not spec2 and c < 2, k=width, each=1, max_expansion=top,
                  **over)


# The uniform launches of tests/test_gpu_visited_regimes.py: id -> index, family, V values, ef, environment, the launch screens, log regime, W values.
# Every walk of every one of them spills (or V = 0); `regime` is where its undo log ends up at the default capacity.
def _launches():
    out = {}
    for ef in (64, 128):  # one and two list keys per lane
        out[f"classic-ef{ef}"] = dict(index="l2_64", path="classic", V=(256, 0), ef=ef, env=env_of(spec=0), screen=0, regime="within", W=(1, 3))
        for name in ("l2_768", "cos_768"):  # the screened form of search_level_reg: undo_apply<FRESH_ZERO>
            out[f"screened-{name}-ef{ef}"] = dict(index=name, path="classic", V=(256, 0), ef=ef, env=env_of(spec=0), screen=1, regime="within", W=(1, 3))
            # ... and the headline instantiation (two rows per group, six workgroups per CU, 80 VGPRs): the 64 queries tiled to 1088
            out[f"screened-{name}-ef{ef}-nq{TILED_NQ}"] = dict(index=name, path="classic", V=(256, 0), ef=ef, env=env_of(spec=0), screen=1, regime="within",
                                                            W=(3,), nq=TILED_NQ)
    out["lds_list-ef200"] = dict(index="l2_64", path="classic", V=(256, 0), ef=200, env=env_of(spec=0), screen=0, regime="within", W=(1, 3))
    out["lds_list-forced-ef64"] = dict(index="l2_64", path="classic", V=(256, 0), ef=64, env=env_of(spec=0, lds_list=1), screen=0, regime="within", W=(1, 3))
    for spec in (1, 2):  # the latency-bound walks: 8 lanes per row, and 64 (the screen is not part of them)
        for name in ("l2_64", "cos_768"):
            out[f"spec{spec}-{name}"] = dict(index=name, path=f"spec{spec}", V=(256, 0), ef=64, env=env_of(spec=spec), screen=0, regime="within", W=(1, 3))
    for name in ("f16_768", "i8_256", "b1_24"):
        out[f"rows-{name}"] = dict(index=name, path="classic", V=(0,), ef=64, env=env_of(spec=0), screen=0, regime="within", W=(1,))
    # the natural log regimes on the 30000 x 64 index (48 queries): the LDS-list walk, W = 2 and the default grid (0)
    out["big-within-ef400"] = dict(index="big", path="classic", V=(256, 0), ef=400, env={}, screen=0, regime="within", W=(2, 0))
    out["big-overflow-ef1000"] = dict(index="big", path="classic", V=(256, 0), ef=1000, env={}, screen=0, regime="overflow", W=(2, 0))
    return out


LAUNCHES = _launches()
SCREENED = {"l2_768", "cos_768"}  # the indexes that hold an int8 screen (f32 l2sq / cos rows of >= 128 chunks)
BIG_MIXED = tuple((K, (400, 1000)[q % 2], 0) for q in range(filtered_regimes.NQ))  # per-query 400 | 1000 by turns: both in the LDS-list class

# ---- the forced regimes of tests/visited_undo_probe.py (LANTERN_GPU_VIS_UNDO is read once per process) ---------------------------
PROBE_INDEXES = ("l2_64", "l2_768", "cos_768")
PROBE_K = 5
PROBE_MIXED = tuple((PROBE_K, (8, 64)[q % 2], 0) for q in range(NQ))  # per-query ef 8 | 64 by turns: one class (one list key per lane)
# The cap of the mixed run, V = 0: D + 1 <= cap for the ef = 8 walks, D - U > cap for the ef = 64 walks, on all three indexes.  Measured
# on the oracle (tests/test_visited_regimes_ref.py asserts it): the ef = 8 walks have D = 251 .. 442 (l2_64), 214 .. 414 (l2_768), 235 .. 481 (cos_768); the ef = 64 walks have
# D - U = 1011 .. 1225, 932 .. 1045, 1061 .. 1285.  Any cap in 482 .. 931 separates them; 700 is the middle.
MIXED_CAP = 700
PROBE_RUNS = {  # id -> (LANTERN_GPU_VIS_UNDO, V, regime)
    "undo16-V256": (16, 256, "overflow"),
    "undo16-V0": (16, 0, "overflow"),
    "undo0-V256": (0, 256, "overflow"),
    "mixed-V0": (None, 0, "mixed"),  # None: MIXED_CAP
}
PROBE_FAMILIES = {"classic": env_of(spec=0), "spec1": env_of(spec=1), "spec2": env_of(spec=2)}  # (classic: screened on the 768-d indexes)
PROBE_EACH_FAMILIES = {"classic": env_of(spec=0), "spec2": env_of()}  # the per-query form has no spec 1; 64 queries take spec 2 unasked
PROBE_W = (1, 3)
PROBE_TILED = tuple((name, ef) for name in ("l2_768", "cos_768") for ef in (64, 128))  # screened, two rows per group: TILED_NQ queries on INSERT_W workgroups
PROBE_INSERT = ("l2sq", 1200, 64, 8, 40, (512, 16))  # the probe's capped build: LANTERN_GPU_INSERT_SPEC=0 sends every batch to k_insert


def roll_params(params, shift=1):
    return params if isinstance(params, int) else tuple(params[(q - shift) % len(params)] for q in range(len(params)))


# ------------------------------------------------------------------------------------------------
# the insertion walks
# ------------------------------------------------------------------------------------------------
def insert_rows(n, d):
    rng = np.random.default_rng(DATA_SEED)
    return rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((NQ, d), dtype=np.float32)


def insert_proxy(ora, queries, efc):
    """D - U per query of the oracle's search at ef = efc.  A PROXY for the insertion walks (they have no oracle D of their own): an
    insertion is the greedy descent and a level-0 walk at ef_construction from where it ends, as this search is."""
    D = ora.search_batch(queries, K, efc, THREADS)[3].astype(np.int64)
    return D - descent_of(ora, queries)


@functools.lru_cache(maxsize=None)
def insert_oracle(name):
    """{base, labels, g: the oracle's graph of the two-part build, finished: insert_proxy of fresh queries on the finished graph,
    batch: insert_proxy of the big batch's own rows on the graph they walk -- the first part's}"""
    from oracle import binding as oracle

    metric, n, d, M, efc, first, _ = INSERTS[name]
    base, queries = insert_rows(n, d)
    labels = np.arange(n, dtype=np.uint64) + 1
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=EF_DEFAULT, seed=INDEX_SEED, sum_mode=oracle.SUM_WAVE64)
    ora.add_planned(labels[:first], base[:first], *INSERT_FIRST_PLAN)
    big = min(first, INSERT_PLAN[0], n - first)  # lo_plan_batch: rows so far / min_ratio, at most max_batch, at most what is pending
    batch = insert_proxy(ora, base[first: first + big], efc)
    ora.add_planned(labels[first:], base[first:], *INSERT_PLAN)
    return {"base": base, "labels": labels, "g": ora.export_graph(), "finished": insert_proxy(ora, queries, efc), "batch": batch, "big": big}


@functools.lru_cache(maxsize=None)
def probe_insert_oracle():
    from oracle import binding as oracle

    metric, n, d, M, efc, plan_ = PROBE_INSERT
    base, queries = insert_rows(n, d)
    labels = np.arange(n, dtype=np.uint64) + 1
    ora = oracle.OracleIndex(metric, d, M=M, ef_construction=efc, ef=EF_DEFAULT, seed=INDEX_SEED, sum_mode=oracle.SUM_WAVE64)
    ora.add_planned(labels, base, *plan_)
    return {"base": base, "labels": labels, "g": ora.export_graph(), "finished": insert_proxy(ora, queries, efc)}


GRAPH_ARRAYS = ("levels", "labels", "upper_off", "nbr0", "upper_nbr")


def same_graph(a, b, what):
    assert int(a["entry_slot"]) == int(b["entry_slot"]) and int(a["max_level"]) == int(b["max_level"]), what
    for name in GRAPH_ARRAYS:
        assert np.array_equal(a[name], b[name]), f"{what}: {name} differs"


# ------------------------------------------------------------------------------------------------
# on the device
# ------------------------------------------------------------------------------------------------
class Launcher:
    """Device buffers for one batch of queries on one index.  run(ef) is a uniform launch at k = K, run(tuple of (k, ef, skip)) a
    per-query one; both give (slots, dists, counts, D, E, labels) and overwrite every buffer with 0xA5 first, so that whatever a launch
    leaves unwritten shows."""

    def __init__(self, gpu, queries, width=K):
        from lantern_amd import hip

        self.hip, self.gpu, self.width = hip, gpu, width
        self.rows = gpu.device_query_rows(queries)
        self.nq = nq = self.rows.shape[0]
        self.dq = hip.Buffer.from_numpy(self.rows)
        self.lab, self.dist, self.slot = hip.Buffer(nq * width * 8), hip.Buffer(nq * width * 4), hip.Buffer(nq * width * 4)
        self.cnt, self.D, self.E = hip.Buffer(nq * 4), hip.Buffer(nq * 8), hip.Buffer(nq * 8)

    def run(self, params):
        nq, w, stride = self.nq, self.width, self.rows.strides[0]
        for b in (self.lab, self.dist, self.slot, self.cnt, self.D, self.E):
            b.upload(np.full(b.nbytes, 0xA5, dtype=np.uint8))
        out = (self.lab.ptr, self.dist.ptr, self.slot.ptr, self.cnt.ptr, self.D.ptr, self.E.ptr)
        if isinstance(params, int):
            self.gpu.search_batch_device(self.dq.ptr, nq, w, params, 0, *out, query_stride=stride)
        else:
            assert len(params) == nq
            self.gpu.search_batch_params_device(self.dq.ptr, stride, nq, list(params), w, *out)
        self.hip.synchronize()
        return (self.slot.download((nq, w), np.uint32), self.dist.download((nq, w), np.float32), self.cnt.download(nq, np.uint32),
                self.D.download(nq, np.uint64), self.E.download(nq, np.uint64), self.lab.download((nq, w), np.uint64))


NAMES = ("slots", "distance bits", "counts", "D", "E", "labels")


def check(got, want, what):
    """slots, distance bits, counts, D, E and labels are equal, for every query"""
    for name, a, b in zip(NAMES, got, want):
        a, b = np.asarray(a), np.asarray(b)
        if name == "distance bits":
            a, b = a.view(np.uint32), b.view(np.uint32)
        if a.shape != b.shape or not np.array_equal(a, b):
            bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1)) if a.shape == b.shape else "shape"
            raise AssertionError(f"{what}: {name} differ for queries {bad if isinstance(bad, str) else bad[:8].tolist()} ({len(bad)} in all)")
