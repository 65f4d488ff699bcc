"""The frame around one query's walk (lantern_amd/csrc/query_frame.hpp), across the kernel families that share it.  Needs an MI355X.

The frame's behaviours: (a) the 0 / +inf / EMPTY tail of an answer row when k exceeds what the walk returns; (b) skip >= the walk's
count: count 0 and a full tail; (c) more queries than workgroups, with the ticket and with LANTERN_GPU_TICKETS=0: identical rows;
(d) NULL for any subset of the six output pointers: the others are written, nothing else is; (e) the done words, through the notify
form.  The families: the classic walk, the 3 + 8 wave walk, ADC over PQ codes, the filtered walk, the filtered exact path (no done
words there) -- each in its uniform and its per-query form.

Which test pinned which cell before this file (the rest of the cells are pinned here):
  classic, 3 + 8, per-query form   (a) (b) (c)  test_gpu_search_params.py: more_rows_wanted_than_the_index_has, more_queries_than_workgroups
                                   (e)          test_gpu_search_params.py: host_lane_and_notify_forms
  classic, 3 + 8, uniform form     (a) (c) (e)  test_gpu_parity.py, test_gpu_lane_notify.py (k <= n throughout: no skip >= count)
  ADC, both forms                  the answers  test_gpu_quantized_indexes.py, test_gpu_search_params.py: compact_pq_index_by_adc
  filtered walk / exact, uniform   (a) (b)      test_gpu_filtered_search.py: exact_path_is_bruteforce (skip 0 and 3), selective_walk
  filtered walk / exact, per-query (a) (c)      test_gpu_filtered_each.py: mixed_batch (a one-row and an empty filter), two_workgroups
  (d), any family                  none: every device-form test passes all six pointers
  LANTERN_GPU_TICKETS=0            test_gpu_parity.py, the classic uniform walk only

Every answer is compared with the restatement the family's own file uses: OracleIndex.search on the exported graph (in ADC's
summation order for the table walk), tests/filtered_walk_ref.py for the filtered kernels.  No tolerance: slots, distance bits,
labels, counts, D and E are equal.  Five queries on two workgroups, so three come by ticket.
"""
import numpy as np
import pytest

from tests import filtered_walk_ref as ref
from tests.test_gpu_search_params import Case, _pq_case

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
NQ = 5
NAMES = ("slots", "dists", "counts", "D", "E", "labels")  # (the order of Case.want and of filtered_walk_ref.search, labels last)
ALL = frozenset(NAMES)
MASKS = (ALL, frozenset({"dists"}), frozenset({"labels", "counts"}), frozenset({"slots", "D", "E"}))  # every pointer both given and NULL


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


class Outs:
    """Six device buffers for nq rows of `width`, filled with 0xA5 before a call so that whatever the call leaves unwritten shows."""

    KINDS = {"slots": (np.uint32, True), "dists": (np.float32, True), "counts": (np.uint32, False), "D": (np.uint64, False), "E": (np.uint64, False),
             "labels": (np.uint64, True)}

    def __init__(self, nq, width):
        from lantern_amd import hip

        self.hip, self.nq, self.width = hip, nq, width
        self.buf = {}
        for name, (dtype, wide) in self.KINDS.items():
            self.buf[name] = hip.Buffer(nq * (width if wide else 1) * np.dtype(dtype).itemsize)

    def ptrs(self, mask):
        """(d_labels, d_dists, d_slots, d_counts, d_D, d_E) as the device forms take them; NULL outside `mask`"""
        for b in self.buf.values():
            b.upload(np.full(b.nbytes, 0xA5, dtype=np.uint8))
        return tuple(self.buf[name].ptr if name in mask else None for name in ("labels", "dists", "slots", "counts", "D", "E"))

    def check(self, mask, want, what):
        self.hip.synchronize()
        for name, w in zip(NAMES, want):
            dtype, wide = self.KINDS[name]
            got = self.buf[name].download((self.nq, self.width) if wide else self.nq, dtype)
            if name not in mask:
                assert np.all(got.view(np.uint8) == 0xA5), f"{what}: {name} was written though its pointer was NULL"
                continue
            a, b = (got.view(np.uint32), np.asarray(w, dtype=np.float32).view(np.uint32)) if name == "dists" else (got, np.asarray(w, dtype=dtype))
            assert np.array_equal(a, b), f"{what}: {name} differ (given: {sorted(mask)})"


# ------------------------------------------------------------------------------------------------
# the unfiltered families: classic walk, 3 + 8 wave walk, ADC
# ------------------------------------------------------------------------------------------------
# family -> (environment that selects it, rows, the (k, ef, skip) triples: a full row, a partial row with a tail, skip >= count)
SEARCH = {
    "classic": ({"LANTERN_GPU_SPEC": "0"}, 400, [(10, 0, 0), (300, 0, 200), (10, 0, 400)]),
    # (the wave walk keeps its list in registers: expansion = k + skip <= 128, so its tail needs an index of fewer rows)
    "waves_3_8": ({"LANTERN_GPU_SPEC": "2"}, 100, [(10, 0, 0), (60, 0, 50), (10, 0, 100)]),
    "adc": ({"LANTERN_GPU_PQ_ADC": "1"}, 600, [(10, 0, 0), (300, 0, 400), (10, 0, 600)]),
}


def oracle_graph(oracle, n, d, M, efc, ef):
    """base rows, NQ queries, the oracle's own graph over the rows and the oracle that built it"""
    rng = np.random.default_rng(n + d)
    base, queries = rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((NQ, d), dtype=np.float32)
    ora = oracle.OracleIndex("l2sq", d, M=M, ef_construction=efc, ef=ef, seed=9, sum_mode=oracle.SUM_WAVE64)
    ora.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    return base, queries, ora.export_graph(), ora


def import_index(capi, base, g, d, M, efc, ef):
    gpu = capi.GpuIndex("l2sq", d, M=M, ef_construction=efc, ef=ef, seed=9)
    gpu.import_graph(base, g)
    gpu.set_search_shape(0, 2)  # two workgroups: three of the five queries come by ticket
    return gpu


def search_cases(capi, oracle, family, n, monkeypatch, both=True):
    """The family's index with tickets and (both) the same index made under LANTERN_GPU_TICKETS=0 (read when an index is made).
    Classic and wave walk: n x 24, M = 8, efc = 32, the ORACLE's graph imported into both indexes.  ADC: 600 x 32 in 8 subvectors x
    16 centroids, built on the device (a pq index cannot be imported), twice -- builds are deterministic, as
    test_gpu_search_params.py::test_switches_do_not_change_an_answer relies on -- and walked by the oracle in ADC's own summation
    order, whose distance bits the decoding walk does not produce: equality with it says the table walk ran."""
    made = []
    graph = None if family == "adc" else oracle_graph(oracle, n, 24, 8, 32, 32)
    for tickets in ((None, "0") if both else (None,)):
        if tickets is None:
            monkeypatch.delenv("LANTERN_GPU_TICKETS", raising=False)
        else:
            monkeypatch.setenv("LANTERN_GPU_TICKETS", tickets)
        if family == "adc":
            case, cb, codes = _pq_case(capi, oracle, "l2sq", n, 32, 8, 16, 8, 40, NQ)
            case.ora.set_pq_view(cb, codes)
            case.gpu.set_search_shape(0, 2)
        else:
            base, queries, g, ora = graph
            case = Case.__new__(Case)
            case.capi, case.metric, case.n, case.ef, case.nq, case.queries, case.oq = capi, "l2sq", n, 32, NQ, queries, queries
            case.gpu, case.ora, case.labels = import_index(capi, base, g, 24, 8, 32, 32), ora, g["labels"]
            case._dev()
        made.append(case)
    monkeypatch.delenv("LANTERN_GPU_TICKETS", raising=False)
    return made


def run_search(case, form, params, outs, mask):
    lab, dist, slot, cnt, D, E = outs.ptrs(mask)
    stride = case.rows.strides[0]
    if form == "each":
        case.gpu.search_batch_params_device(case.dq.ptr, stride, case.nq, params, outs.width, lab, dist, slot, cnt, D, E)
    else:
        k, ef, skip = params[0]
        case.gpu.search_batch_device(case.dq.ptr, case.nq, k, ef, skip, lab, dist, slot, cnt, D, E, query_stride=stride)


def search_calls(form, triples):
    """The calls that put every triple through `form`: one uniform call per triple, or ONE per-query call that mixes them (rows as wide
    as the largest k: the narrower queries' rows end in a tail beyond their k as well)."""
    if form == "uniform":
        return [([t] * NQ, t[0]) for t in triples]
    return [([triples[q % len(triples)] for q in range(NQ)], max(t[0] for t in triples))]


@pytest.mark.parametrize("form", ["uniform", "each"])
@pytest.mark.parametrize("family", list(SEARCH))
def test_tail_skip_tickets_and_null_outputs(capi, oracle, family, form, monkeypatch):
    env, n, triples = SEARCH[family]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    case, strided = search_cases(capi, oracle, family, n, monkeypatch)
    for params, width in search_calls(form, triples):
        want = case.want(params, width)
        counts = want[2]
        for q, (k, _, skip) in enumerate(params):  # the cases are what they claim to be: a full row, (a) a tail, (b) skip >= count
            assert counts[q] == k if k + skip <= 10 else 0 < counts[q] < k if skip < n else counts[q] == 0
        outs = Outs(NQ, width)
        for mask in MASKS:
            run_search(case, form, params, outs, mask)
            outs.check(mask, want, f"{family} {form} {params[0]}")
        run_search(strided, form, params, outs, ALL)
        outs.check(ALL, want, f"{family} {form} {params[0]} LANTERN_GPU_TICKETS=0")
    if form == "each" and family != "adc":
        assert case.gpu.last_params_launch()["spec"] == (family == "waves_3_8")


@pytest.mark.parametrize("form", ["uniform", "each"])
@pytest.mark.parametrize("family", list(SEARCH))
def test_done_words_hand_every_query_on_once_with_its_rows(capi, oracle, family, form, monkeypatch):
    env, n, _ = SEARCH[family]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    case, = search_cases(capi, oracle, family, n, monkeypatch, both=False)
    k = 10
    params = [(k, 0, 0)] * NQ if form == "uniform" else [(k, 0, 0), (3, 0, 2), (k, 20, 0), (1, 0, 0), (k, 0, 5)]
    want = case.want(params, k)
    if form == "uniform":
        lab, dist, cnt, calls, snaps = case.gpu.search_batch_lane_notify(2, case.queries, k)
    else:
        lab, dist, cnt, calls, snaps = case.gpu.search_batch_params_lane_notify(2, case.queries, params, k_stride=k)
    assert sorted(j for c in calls for j in c) == list(range(NQ)), "every query is handed on exactly once"
    for j in range(NQ):  # ... with its final rows in place when its callback runs
        assert np.array_equal(snaps[j][0], want[5][j]) and np.array_equal(snaps[j][1].view(np.uint32), want[1][j].view(np.uint32)) and snaps[j][2] == want[2][j]
    assert np.array_equal(lab, want[5]) and np.array_equal(dist.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(cnt, want[2])


# ------------------------------------------------------------------------------------------------
# the filtered families: the walk and the exact path, one filter for the launch and a filter per query
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["uniform", "each"])
@pytest.mark.parametrize("path", ["walk", "exact"])
def test_filtered_tail_skip_tickets_and_null_outputs(capi, oracle, path, form, monkeypatch):
    n, d, M, efc, ef, k = 400, 24, 8, 32, 32, 10
    base, queries, g, _ = oracle_graph(oracle, n, d, M, efc, ef)
    monkeypatch.delenv("LANTERN_GPU_TICKETS", raising=False)
    gpu = import_index(capi, base, g, d, M, efc, ef)
    monkeypatch.setenv("LANTERN_GPU_TICKETS", "0")  # (read when an index is made)
    strided = import_index(capi, base, g, d, M, efc, ef)
    monkeypatch.delenv("LANTERN_GPU_TICKETS")
    dist = ref.distance_matrix(oracle, base, queries, "l2sq", oracle.SUM_WAVE64)
    allowed = np.zeros(n, dtype=bool)
    allowed[np.random.default_rng(3).choice(n, size=7, replace=False)] = True  # seven allowed rows: skip 0, 5, 9 give 7, 2, 0 of k = 10
    from lantern_amd import hip

    outs = Outs(NQ, k)
    for ix in (gpu, strided):
        ix.set_filter_policy(path)
        rows = ix.device_query_rows(queries)
        dq = hip.Buffer.from_numpy(rows)
        f = ix.filter_from_bitmap(allowed)
        for skip, count in ((0, 7), (5, 2), (9, 0)):
            s, dd, c, D, E = ref.search(g, dist, allowed, M, k, ef, skip=skip, path=path)
            assert np.all(c == count)
            labels = np.where(s == EMPTY, 0, g["labels"][np.where(s == EMPTY, 0, s)]).astype(np.uint64)
            want = (s, dd, c, D, E, labels)
            for mask in (MASKS if ix is gpu else (ALL,)):
                lab, dst, slot, cnt, pD, pE = outs.ptrs(mask)
                if form == "each":
                    ix.search_batch_filtered_each_device([f] * NQ, dq.ptr, rows.strides[0], NQ, k, 0, skip, lab, dst, slot, cnt, pD, pE)
                else:
                    ix.search_batch_filtered_device(f, dq.ptr, rows.strides[0], NQ, k, 0, skip, lab, dst, slot, cnt, pD, pE)
                outs.check(mask, want, f"filtered {path} {form} skip={skip}" + ("" if ix is gpu else " LANTERN_GPU_TICKETS=0"))
                if form == "uniform":
                    shape = ix.last_filtered_launch()
                    assert shape["path"] == path and shape["grid"] == 2, shape
        if form == "each":
            got = ix.last_filtered_each()
            assert got[path] == NQ and got["walk" if path == "exact" else "exact"] == 0, got
