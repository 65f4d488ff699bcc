"""Every instantiation of the unfiltered search kernels that a launcher reaches (tests/search_cells.py CELLS: 542 compiled kernels),
launched once at least and compared with the oracle and with float64.  Needs an MI355X.

One test id is one small index -- a (metric code, lanes per row) pair, 40 of them, and the two ADC indexes -- and runs every recipe of every
cell of that index: 12 to 30 launches of 40 or 64 queries over 500 rows.  Per launch, in this order:
  1. the record: lantern_gpu_last_search_cells names exactly one launch, the cell the recipe claims (and whether it screened);
  2. the oracle: slots, labels, distance bits, counts, D and E are those of the oracle's walk on the same graph in the kind's summation
     order -- per query at that query's own (k, ef, skip) for the per-query form (tests/test_gpu_search_params.py Case.want);
  3. float64: every returned distance is within tests/value_range.within_rounding of the float64 distance between the stored query and the
     stored row it names (compact pq by decoding: the decoded row; ADC: the existing ADC test's 1e-5 * max(1, |d|) + 1e-6 to the decoded row).
The last test of the module asserts that the cells recorded over the whole module are CELLS.
"""
import numpy as np
import pytest

from tests import filtered_regimes as regimes
from tests import search_cells as sc
from tests import value_range as vr
from tests.test_gpu_quantized_indexes import make_codebook
from tests.test_gpu_search_params import Case, check

pytestmark = pytest.mark.gpu

EFC, SEED, K, NQ = 64, 9, 10, 64
SWITCHES = ("LANTERN_GPU_SPEC", "LANTERN_GPU_LDS_LIST", "LANTERN_GPU_PQ_ADC", "LANTERN_GPU_ADC_SPEC", "LANTERN_GPU_SPEC_WAVES", "LANTERN_GPU_SCREEN")
RAN, SEEN = set(), set()  # the instances run, and the cells recorded, in this process


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def data(key):
    """500 rows, 50 of them exact duplicates of 50 others (equal distances: the slot decides), and 64 queries, half of them rows of the set."""
    inst = sc.INSTANCES[key]
    rng = np.random.default_rng([key[0], key[1]])
    d = inst["d"]
    if inst["metric"] == "hamming":
        make = lambda m: rng.integers(0, 2**32, size=(m, d), dtype=np.uint32)  # noqa: E731
    else:
        shift = np.float32(0.1 if inst["storage"] == "b1" else 0.0)
        scale = np.float32(0.4 if inst["storage"] == "i8" else 1.0)
        make = lambda m: (rng.standard_normal((m, d), dtype=np.float32) - shift) * scale  # noqa: E731
    base = make(sc.N)
    base[250:300] = base[:50]
    queries = np.concatenate([base[rng.integers(0, sc.N, NQ // 2)], make(NQ - NQ // 2)])
    return base, queries, rng


def unpack(words, d):
    """the {0, 1} rows behind packed sign bits (most significant bit of each byte first)"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="big")[:, :d].astype(np.float64)


class Instance:
    """The index of a (metric code, G) on the device, the oracle over the same graph, and the float64 distances of its 64 queries."""

    def __init__(self, capi, oracle, key, screen=True):
        inst = sc.INSTANCES[key]
        storage, metric, d = inst["storage"], inst["metric"], inst["d"]
        base, queries, rng = data(key)
        labels = np.arange(sc.N, dtype=np.uint64) + 1
        self.key, self.capi, self.adc, self.dims = key, capi, storage == "adc", d * 32 if metric == "hamming" else d
        self.metric64 = metric
        if storage in ("pqd", "adc"):  # built on the device, then compacted; the oracle walks the decoded rows (ADC: through the table's sums)
            cb = make_codebook(rng, base, inst["S"], inst["C"])
            gpu = capi.GpuIndex(metric, d, M=sc.M, ef_construction=EFC, ef=sc.EF_DEFAULT, seed=SEED, pq_codebook=cb, num_subvectors=inst["S"])
            gpu.set_add_batch(256, 16)
            gpu.add_many(labels, base)
            codes = gpu.export_codes()
            g = gpu.export_graph(with_vectors=True)
            sb, sq = g["vectors"], queries
            ora = oracle.OracleIndex.from_graph(metric, sb, g, sc.M, EFC, sc.EF_DEFAULT, SEED, oracle.SUM_WAVE64)
            if self.adc:
                ora.set_pq_view(cb, codes)
            gpu.pq_compact()
            rows64, q64 = sb, sq
        elif storage == "b1":  # built on the device and exported: the stored rows are the packed sign bits
            sb, sq, ometric, mode = regimes.stored_rows(oracle, storage, metric, base, queries)
            gpu = capi.GpuIndex(metric, d, M=sc.M, ef_construction=EFC, ef=sc.EF_DEFAULT, seed=SEED, quantization="b1")
            gpu.add_many(labels, base)
            gpu.flush()
            g = gpu.export_graph(with_vectors=True)
            assert np.array_equal(g["vectors"], sb)
            ora = oracle.OracleIndex.from_graph(ometric, sb, g, sc.M, EFC, sc.EF_DEFAULT, SEED, mode)
            rows64, q64 = unpack(sb, d), unpack(sq, d)
        else:  # the oracle builds the graph over the stored values, the device imports it
            sb, sq, ometric, mode = regimes.stored_rows(oracle, storage, metric, base, queries)
            ora = oracle.OracleIndex(ometric, d, M=sc.M, ef_construction=EFC, ef=sc.EF_DEFAULT, seed=SEED, sum_mode=mode)
            ora.add_many(labels, sb)
            g = ora.export_graph()
            gpu = capi.GpuIndex(metric, d, M=sc.M, ef_construction=EFC, ef=sc.EF_DEFAULT, seed=SEED, quantization=storage)
            gpu.import_graph(sb, g)
            rows64, q64 = sb, sq
        self.gpu, self.ora, self.screen = gpu, ora, screen
        # [64][500], once; the differences themselves are summed: half the queries ARE rows, and their distance of exactly 0 has a bound of 0
        self.d64 = vr.exact64(metric, rows64, q64, direct=True)
        self.cases = {}
        for nq in (40, NQ):  # (tests/test_gpu_search_params.py Case: device buffers, the two entry points, the per-query oracle answer)
            c = Case.__new__(Case)
            c.capi, c.metric, c.n, c.ef, c.nq, c.queries, c.oq = capi, metric, sc.N, sc.EF_DEFAULT, nq, queries[:nq], sq[:nq]
            c.gpu, c.ora, c.labels = gpu, ora, g["labels"]
            c._dev()
            self.cases[nq] = c
        self.wants = {}

    def want(self, r):
        """The oracle's answer to a recipe: computed for 64 queries once per (entry point, expansion), the first nq rows of it."""
        at = (r["each"], r["ef"])
        if at not in self.wants:
            if r["each"]:
                self.wants[at] = self.cases[NQ].want(sc.params_of(dict(r, nq=NQ)), K)
            else:
                lab, dist, slot, D, E = self.ora.search_batch(self.cases[NQ].oq, K, r["ef"], regimes.THREADS)
                self.wants[at] = (slot, dist, np.full(NQ, K, dtype=np.uint32), D, E, lab)
        return tuple(a[:r["nq"]] for a in self.wants[at])

    def run(self, r, monkeypatch):
        capi, case = self.capi, self.cases[r["nq"]]
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in r["env"].items():
            monkeypatch.setenv(name, value)
        self.gpu.set_search_shape(r["waves"])
        capi.last_search_cells()
        got = case.params(sc.params_of(r), K) if r["each"] else case.uniform(K, r["ef"], 0)
        # 1. the record
        made, cells = capi.last_search_cells()
        cell = sc.cell_of(r)
        screens = int(self.screen and sc.holds_screen_path(cell))
        assert made == 1 and cells == [cell + (screens, r["nq"])], (r, made, cells)
        SEEN.add(cells[0][:8])
        # 2. the oracle
        check(got, self.want(r), f"{cell} by {r}")
        # 3. float64
        slots, dists, counts = got[0], got[1], got[2]
        valid = np.arange(K)[None, :] < counts[:, None]
        assert valid.any() and slots[valid].max() < sc.N
        q = np.broadcast_to(np.arange(r["nq"])[:, None], slots.shape)[valid]
        delta, d32 = self.d64[q, slots[valid]], dists[valid].astype(np.float64)
        if self.adc:
            ok = np.abs(d32 - delta) <= 1e-5 * np.maximum(1.0, np.abs(delta)) + 1e-6
        else:
            ok = vr.within_rounding(self.metric64, d32, delta, self.dims)
        assert np.all(ok), (cell, r, float(np.max(np.abs(d32 - delta))))
        return cells[0][:8]


@pytest.mark.parametrize("key", list(sc.INSTANCES), ids=[sc.instance_id(k) for k in sc.INSTANCES])
def test_every_cell_of_an_index_walks_as_the_oracle_does(capi, oracle, key, monkeypatch):
    RAN.add(key)
    mine = [c for c in sc.CELLS if (c[1], c[2]) == key]
    assert len(mine) in (10, 12, 18)
    two = any(sc.holds_screen_path(c) for c in mine)  # the f32 l2sq / cos rows of >= 128 chunks: with the int8 screen, and without
    made = {True: Instance(capi, oracle, key, True)}
    if two:
        monkeypatch.setenv("LANTERN_GPU_SCREEN", "0")
        made[False] = Instance(capi, oracle, key, False)
        monkeypatch.delenv("LANTERN_GPU_SCREEN")
    launched = set()
    try:
        for cell in mine:
            for r in sc.recipes(cell):
                assert made[r["screen"] is not False].run(r, monkeypatch) == cell
                launched.add(cell)
    finally:
        for inst in made.values():
            inst.gpu.set_search_shape(0)
    assert launched == set(mine)


def test_the_record_is_a_ring_of_this_threads_last_four_launches(capi, oracle, monkeypatch):
    import threading

    key = (sc.M_L2SQ, 8)
    inst = Instance(capi, oracle, key)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    inst.gpu.set_search_shape(4)
    case = inst.cases[40]
    capi.last_search_cells()
    # a per-query call over all three expansion classes: three launches, in class order, each with its own query count
    params = [(K, (24, 100, 160)[q % 3], 0) for q in range(40)]
    case.params(params, K)
    made, cells = capi.last_search_cells()
    assert made == 3 and [c[5] for c in cells] == [1, 2, 0] and [c[9] for c in cells] == [14, 13, 13]
    assert all(c[:5] == (sc.K_SEARCH, sc.M_L2SQ, 8, 0, 2) and c[6:9] == (0, 1, 0) for c in cells)
    assert capi.last_search_cells() == (0, [])  # reading resets
    # six launches: the count says six, the ring holds the last four, oldest first; a smaller cap keeps the oldest of those
    for ef in (24, 24, 100, 160, 24, 100):
        case.uniform(K, ef, 0)
    seen_elsewhere = []
    t = threading.Thread(target=lambda: seen_elsewhere.append(capi.last_search_cells()))
    t.start()
    t.join()
    assert seen_elsewhere == [(0, [])]  # another thread made no launch, and reading there takes nothing from here
    made, cells = capi.last_search_cells()
    assert made == 6 and [c[5] for c in cells] == [2, 0, 1, 2] and all(c[7] == 0 and c[9] == 40 for c in cells)
    for ef in (24, 100, 160):
        case.uniform(K, ef, 0)
    made, cells = capi.last_search_cells(cap=2)
    assert made == 3 and [c[5] for c in cells] == [1, 2]
    inst.gpu.set_search_shape(0)


def test_every_cell_was_launched():
    """The union over the module.  (A run of some ids only has nothing to say here: every id asserts its own cells.)"""
    if RAN != set(sc.INSTANCES):
        pytest.skip("only part of the module ran in this process: the union is asserted when all 42 indexes have run")
    assert SEEN == set(sc.CELLS), (sorted(set(sc.CELLS) - SEEN)[:5], sorted(SEEN - set(sc.CELLS))[:5])
