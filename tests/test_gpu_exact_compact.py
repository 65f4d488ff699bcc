"""lantern_gpu_exact_search on a COMPACT pq index under lantern_gpu_set_exact_compact (include/lantern_gpu.h; DESIGN.md 4.5 "Compact pq
indexes"): answered from the code rows (k_dense_pq and the kernels around it, csrc/dense_pq.hip), the index stays compact.  Needs an MI355X.

The arbiter is a float64 brute force over the decoded rows, codebook[codes], ordered by (distance, slot), at the tolerance of the numerics
contract: 1e-5 max(1, |ref|).  The expanded twin's slots and distance bits are a second equality, never the arbiter.
"""
import numpy as np
import pytest

from tests.filtered_adc_ref import make_codebook

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFF
# name -> metric, n, d, num_subvectors, num_centroids, query counts, ks
SHAPES = {
    "cps6_one_code_chunk": ("l2sq", 300, 96, 4, 200, (1, 129, 1025), (1, 10)),  # ragged last tile, all in the seed columns; a second query tile
    "fused_past_seed_cols": ("l2sq", 4400, 128, 32, 256, (1, 129), (1, 10, 240)),
    "cps5_straddles_steps": ("l2sq", 1200, 120, 6, 16, (1, 129), (1, 10)),        # 30 chunks: a partial last K step
    "cps1_eight_codes_a_step": ("l2sq", 700, 64, 16, 64, (1, 129), (1, 10)),
    "cos_768_zero_norms": ("cos", 2000, 768, 96, 64, (1, 129), (1, 10)),          # 96-byte code rows at the 128-byte stride
    "second_row_chunk": ("l2sq", 65536 + 129, 16, 4, 32, (1, 129), (1, 10)),
    "cancelling": ("l2sq", 4000, 128, 32, 256, (129,), (10,)),                    # every certificate is lost
}
_BUILT = {}


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def code_row_bytes(S):
    s16 = (S + 15) // 16 * 16
    return 128 if 64 < s16 < 128 else s16


def built(capi, name, metric, n, d, S, C):
    """twin keeps its decodings; ix is the same saved buffer loaded again, compact, the switch on; ref: the float64 distance matrix"""
    if name not in _BUILT:
        rng = np.random.default_rng(n + d + S)
        base = rng.standard_normal((n, d), dtype=np.float32)
        queries = rng.standard_normal((1025 if name.startswith("cps6") else 129, d), dtype=np.float32)
        if name == "cancelling":
            base, queries = (10 + 0.01 * base).astype(np.float32), (10 + 0.01 * queries).astype(np.float32)
        if metric == "cos":
            base[[5, 900, 1999]] = 0
            queries[7] = 0
        cb = make_codebook(rng, base, S, C)
        if metric == "cos":
            cb[0] = 0
        make = lambda: capi.GpuIndex(metric, d, M=4, ef_construction=16, ef=16, seed=5, pq_codebook=cb, num_subvectors=S)
        twin, ix = make(), make()
        twin.set_add_batch(1024, 16)
        twin.add_many(np.arange(n, dtype=np.uint64) + 1, base)
        twin.flush()
        ix.load_buffer(twin.save_buffer())
        ix.pq_compact()
        ix.set_exact_compact(1)
        sub, codes = d // S, twin.export_codes()
        dec = np.concatenate([cb[codes[:, s], s * sub:(s + 1) * sub] for s in range(S)], axis=1).astype(np.float64)
        if metric == "cos":
            assert not dec[[5, 900, 1999]].any()
        q = queries.astype(np.float64)
        qn, bn, dot = (q * q).sum(1)[:, None], (dec * dec).sum(1)[None, :], q @ dec.T
        if metric == "l2sq":
            ref = np.maximum(qn + bn - 2 * dot, 0)  # (float64: the cancellation costs 1e-12 here even on the rows offset by 10)
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                ref = np.where((qn == 0) & (bn == 0), 0.0, np.where((qn == 0) | (bn == 0), 1.0, 1 - dot / np.sqrt(qn * bn)))
        _BUILT[name] = {"twin": twin, "ix": ix, "queries": queries, "ref": ref, "code_bytes": n * code_row_bytes(S)}
    return _BUILT[name]


def check(b, nq, k):
    ix, twin, ref = b["ix"], b["twin"], b["ref"][:nq]
    slots, dists = ix.exact_search(b["queries"][:nq], k)
    assert ix.memory_usage()[0] == b["code_bytes"] and ix.exact_compact() == 2  # still compact
    assert not (slots == EMPTY).any()  # no query is left out
    want = np.sort(ref, axis=1)[:, :k]
    tol = 1e-5 * np.maximum(1, np.abs(want))
    own = np.take_along_axis(ref, slots.astype(np.int64), axis=1)
    assert (np.abs(own - want) <= tol).all(), np.abs(own - want).max()
    assert (np.abs(dists.astype(np.float64) - own) <= 1e-5 * np.maximum(1, np.abs(own))).all()
    for row in slots:
        assert len(set(row.tolist())) == k
    tslots, tdists = twin.exact_search(b["queries"][:nq], k)
    assert np.array_equal(slots, tslots) and np.array_equal(dists.view(np.uint32), tdists.view(np.uint32))


@pytest.mark.parametrize("fused", [None, "0"])
@pytest.mark.parametrize("name", [s for s in SHAPES if s != "cancelling"])
def test_answers_from_the_code_rows_match_float64_and_the_expanded_twin(capi, monkeypatch, name, fused):
    monkeypatch.delenv("LANTERN_GPU_DENSE_FUSED", raising=False)
    if fused is not None:
        monkeypatch.setenv("LANTERN_GPU_DENSE_FUSED", fused)
    metric, n, d, S, C, nqs, ks = SHAPES[name]
    b = built(capi, name, metric, n, d, S, C)
    for nq in nqs:
        for k in ks:
            check(b, nq, k)


def test_queries_without_a_certificate_fall_back_on_decoded_chunks(capi, monkeypatch):
    monkeypatch.delenv("LANTERN_GPU_DENSE_FUSED", raising=False)
    b = built(capi, "cancelling", *SHAPES["cancelling"][:5])
    before = capi.exact_knn_stats()["fallback"]
    b["ix"].exact_search(b["queries"], 10)
    assert capi.exact_knn_stats()["fallback"] > before
    check(b, 129, 10)


def test_switch_off_and_rows_that_cannot_be_decoded_expand_as_before(capi, monkeypatch):
    monkeypatch.delenv("LANTERN_GPU_DENSE_FUSED", raising=False)
    name = "cps6_one_code_chunk"
    b = built(capi, name, *SHAPES[name][:5])
    ix, twin, q = b["ix"], b["twin"], b["queries"][:5]
    with pytest.raises(capi.LanternGpuError, match="exact_compact must be 0"):
        ix.set_exact_compact(2)
    ix.set_exact_compact(0)
    try:
        assert ix.exact_compact() == 0
        got, want = ix.exact_search(q, 10), twin.exact_search(q, 10)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert ix.memory_usage()[0] >= 300 * 96 * 4  # expanded, as ever
    finally:
        ix.pq_compact()
        ix.set_exact_compact(1)
    assert ix.exact_compact() == 2 and twin.exact_compact() == 0
    twin.set_exact_compact(1)
    assert twin.exact_compact() == 1  # not compact: stored rows
    twin.set_exact_compact(0)
    # subvectors of 10 dimensions are not whole 16-byte chunks: no decode on the fly, the call answers and expands
    rng = np.random.default_rng(3)
    base = rng.standard_normal((300, 60), dtype=np.float32)
    cb = make_codebook(rng, base, 6, 10)
    make = lambda: capi.GpuIndex("l2sq", 60, M=4, ef_construction=16, ef=16, seed=5, pq_codebook=cb, num_subvectors=6)
    t10, i10 = make(), make()
    t10.add_many(np.arange(300, dtype=np.uint64) + 1, base)
    t10.flush()
    i10.load_buffer(t10.save_buffer())
    i10.pq_compact()
    i10.set_exact_compact(1)
    assert i10.exact_compact() == 1 and i10.memory_usage()[0] == 300 * 16
    got, want = i10.exact_search(base[:5], 10), t10.exact_search(base[:5], 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert i10.memory_usage()[0] >= 300 * 60 * 4
