"""lantern_gpu_unlink_deleted and lantern_gpu_compact_deleted on a COMPACT pq index under lantern_gpu_set_delete_compact (include/lantern_gpu.h
"Deleting rows"; DESIGN.md 4.11, 4.12 "Compact pq indexes"): served from the code rows, the index stays compact.  Needs an MI355X.
The arbiter is tests/unlink_ref.py's restatement over the DECODED rows (then tests/compact_ref.py's renumbering), edge for edge.  The
expanded twin that went through the same removal and calls is a second equality, never the arbiter.  Search distances are held to
float64 over the decoded rows at the numerics contract: 1e-5 max(1, |ref|).
"""
import numpy as np
import pytest

from tests import compact_ref, unlink_ref
from tests.filtered_adc_ref import make_codebook
from tests.test_gpu_delete import graphs_equal

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
# name -> metric, n, d, num_subvectors, num_centroids, M, ef_construction, bytes of a padded code row
SHAPES = {
    "cps1_eight_codes_a_step": ("l2sq", 700, 64, 16, 64, 4, 16, 16),
    "cps5_straddles_steps": ("l2sq", 1200, 120, 6, 16, 8, 16, 16),  # 30 chunks: a subvector across two steps, a partial last step
    "cps6_one_code_chunk": ("l2sq", 300, 96, 4, 200, 4, 16, 16),
    "cos_768_at_size": ("cos", 600, 768, 96, 64, 4, 16, 128),   # 96-byte code rows at the 128-byte stride; the norms move
    "two_code_blocks": ("l2sq", 1500, 64, 16, 64, 17, 64, 16),  # cut(0) = 8 x 34 = 272 offers: more than one LDS block of 256 code rows
}
CASES = [(s, p) for s in SHAPES for p in ("random", "neighbourhoods") if (s, p) != ("two_code_blocks", "random")]


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def check(ix, twin, want, rows, metric, queries, S16):
    """(a) the restatement's graph, (b) the twin's graph, checksum and answers, (c) float64 over the decoded rows, (d) still compact"""
    got = ix.export_graph()
    graphs_equal(got, want)
    graphs_equal(got, twin.export_graph())
    assert ix.checksum() == twin.checksum()
    lab, dist, cnt = ix.search_batch(queries, 10)
    tlab, tdist, tcnt = twin.search_batch(queries, 10)
    assert np.array_equal(lab, tlab) and np.array_equal(dist.view(np.uint32), tdist.view(np.uint32)) and np.array_equal(cnt, tcnt)
    assert (lab != 0).all()  # no tombstone is reachable
    slot_of = {int(l): s for s, l in enumerate(got["labels"])}
    r = rows[np.vectorize(slot_of.get)(lab)].astype(np.float64)  # [nq][k][d]: the decoded rows behind the answers
    q = queries.astype(np.float64)[:, None, :]
    if metric == "l2sq":
        ref = ((q - r) ** 2).sum(-1)
    else:
        ref = 1 - (q * r).sum(-1) / np.sqrt((q * q).sum(-1) * (r * r).sum(-1))
    assert (np.abs(dist.astype(np.float64) - ref) <= 1e-5 * np.maximum(1, np.abs(ref))).all()
    assert ix.memory_usage()[0] == len(got["labels"]) * S16 and ix.delete_compact() == 2 and ix.deleted_count == twin.deleted_count


@pytest.mark.parametrize("name,pattern", CASES)
def test_unlink_and_compaction_on_the_code_rows(capi, oracle, name, pattern):
    metric, n, d, S, C, M, efc, S16 = SHAPES[name]
    rng = np.random.default_rng(n + d + S)
    base = rng.standard_normal((n, d), dtype=np.float32)
    queries = rng.standard_normal((32, d), dtype=np.float32)
    cb = make_codebook(rng, base, S, C)
    make = lambda: capi.GpuIndex(metric, d, M=M, ef_construction=efc, ef=16, seed=5, pq_codebook=cb, num_subvectors=S)
    twin, ix = make(), make()
    twin.set_add_batch(256, 16)
    twin.add_many(np.arange(n, dtype=np.uint64) + 1, base)
    twin.flush()
    ix.load_buffer(twin.save_buffer())
    ix.pq_compact()
    g = twin.export_graph(with_vectors=True)
    rows = np.ascontiguousarray(g.pop("vectors"))  # the decodings: what the code rows stand for
    assert g["max_level"] >= 1
    if pattern == "random":
        dead = rng.choice(n, int(0.27 * n), replace=False)
    else:  # everything the three longest level-0 lists and the entry node name at any level, those four kept: their lists empty out, the
        # offers meet full lists and re-prune, upper levels included
        hubs = np.union1d(np.argsort(-(g["nbr0"] != EMPTY).sum(axis=1), kind="stable")[:3], [g["entry_slot"]])
        dead = np.setdiff1d(np.concatenate([unlink_ref.get_list(g, int(s), l, M) for s in hubs for l in range(int(g["levels"][s]) + 1)]), hubs)
    for t in (twin, ix):
        assert t.remove_labels(dead + 1) == dead.size
    # (e) the switch at 0: refused as ever
    for call, what in ((ix.unlink_deleted, "unlink"), (ix.compact_deleted, "compaction")):
        with pytest.raises(capi.LanternGpuError, match=rf"{what} does not run on a compact pq index: expand it first \(lantern_gpu_pq_expand\)"):
            call()
    ix.set_delete_compact(1)
    assert ix.delete_compact() == 2 and twin.delete_compact() == 0 and ix.memory_usage()[0] == n * S16
    before = twin.export_graph()
    want, wst = unlink_ref.unlink(before, unlink_ref.pair_matrix(oracle, rows, metric, oracle.SUM_WAVE64, 8), M)
    st, tst = ix.unlink_deleted(), twin.unlink_deleted()
    print(f"{name} {pattern}: dead {dead.size}; {st}; the restatement: reprunes {wst['reprunes']}")
    assert {k: st[k] for k in unlink_ref.STATS} == {k: wst[k] for k in unlink_ref.STATS} == {k: tst[k] for k in unlink_ref.STATS}
    if pattern == "neighbourhoods":
        assert wst["reprunes"] > 0 and st["reprune_evals"] > 0
    if name == "two_code_blocks":
        assert st["lists_cut"] > 0  # a list with 272 offers: the block loop ran twice
    check(ix, twin, want, rows, metric, queries, S16)
    # the compaction, one case in two with room kept for rows to come
    want_c, rows_c, want_map = compact_ref.compact(want, rows)
    capacity = len(rows_c) + 50 if pattern == "neighbourhoods" else 0
    (cst, cmap), (tcst, tmap) = ix.compact_deleted(capacity), twin.compact_deleted(capacity)
    assert np.array_equal(cmap, want_map) and np.array_equal(tmap, want_map)
    assert (cst["rows_after"], cst["upper_blocks_after"]) == (len(rows_c), want_c["upper_nbr"].shape[0]) and cst["bytes_after"] == sum(ix.memory_usage())
    assert all(v == 0 for v in cst["unlink"].values()) and len(ix) == len(rows_c)
    check(ix, twin, want_c, rows_c, metric, queries, S16)
    assert np.array_equal(ix.export_codes(), twin.export_codes())
    ix.pq_expand()  # only now: the rows the twin has after its own compaction
    assert ix.export_graph(with_vectors=True)["vectors"].tobytes() == twin.export_graph(with_vectors=True)["vectors"].tobytes() == rows_c.tobytes()


def test_rows_that_cannot_be_decoded_are_refused_and_stay_compact(capi):
    rng = np.random.default_rng(3)
    base = rng.standard_normal((300, 60), dtype=np.float32)
    ix = capi.GpuIndex("l2sq", 60, M=4, ef_construction=16, ef=16, seed=5, pq_codebook=make_codebook(rng, base, 6, 10), num_subvectors=6)
    ix.add_many(np.arange(300, dtype=np.uint64) + 1, base)
    ix.flush()
    ix.pq_compact()
    ix.set_delete_compact(1)
    assert ix.delete_compact() == 1 and ix.remove_labels(np.arange(1, 80)) == 79  # subvectors of 10 dimensions are not whole 16-byte chunks
    for call, what in ((ix.unlink_deleted, "unlink"), (ix.compact_deleted, "compaction")):
        with pytest.raises(capi.LanternGpuError, match=f"{what} does not run on this compact pq index from its code rows: its subvectors are not whole 16-byte chunks"):
            call()
    assert ix.memory_usage()[0] == 300 * 16 and ix.deleted_count == 79  # never expanded silently
    with pytest.raises(capi.LanternGpuError, match="delete_compact must be 0"):
        ix.set_delete_compact(2)
