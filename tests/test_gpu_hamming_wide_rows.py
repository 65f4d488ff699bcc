"""Bit rows of up to 2000 words (Lantern's cap: 2000 x 32 bits, 500 chunks of 16 bytes) in every kernel that reads them.  Needs an MI355X.

The rest of the suite stops at 385 chunks for builds and walks and at 25 words for the dense popcount contraction.  Here:
  a. rows of 386 .. 500 chunks -- the eighth load step of group_dist<M_HAMMING, 64> (449 .. 500 chunks) and the eight-chunks-per-lane
     k_connect / k_revlink_pairs with their eighth register slot in use -- through builds (every reverse-link class), walks in both launch
     shapes, gathers in both, the filtered walk and exact path, and the file;
  b. k_dense_ham behind lantern_gpu_distance_matrix(exact_order = 0), on both sides of the width (1024 words) up to which sixteen query
     rows fit the 64 KB of LDS a launch may ask for, up to the cap, and at a width no query block serves;
  c. the exact k-NN of Hamming indexes at those widths;
  d. the exact k-NN of quantization = "b1" cosine indexes (k_dense_ham<true>), over more than one column chunk.

No tolerance anywhere: Hamming distances are integers below 2^24.  The referee is the oracle -- SUM_WAVE64 for Hamming indexes, "cos_b1" /
SUM_SEQ on the packed sign bits for b1 cosine -- which tests/test_hamming_wide_rows_ref.py holds to numpy popcounts and float64."""
import numpy as np
import pytest

from tests import filtered_walk_ref as ref
from tests.quant_contract import pack_bits_msb_first
from tests.test_gpu_exact_knn import empty_graph, fam_bits, index_of
from tests.test_gpu_f16_wide_rows import Answers, assert_answers, assert_same_graph, bits, gathers, staged_lds_bytes
from tests.test_gpu_filtered_search import Dev, same

pytestmark = pytest.mark.gpu

LABEL0 = 1
N, NQ, K, EF = 500, 40, 5, 24


@pytest.fixture(scope="module")
def capi():
    from lantern_amd import capi

    capi.lib()
    assert capi.device_count() > 0, "no HIP device: the gpu tests need a real MI355X"
    return capi


def fam_random(rng, n, w, nq):
    return rng.integers(0, 2 ** 32, size=(n, w), dtype=np.uint32), rng.integers(0, 2 ** 32, size=(nq, w), dtype=np.uint32)


def fam_hubs(rng, n, w, nq):
    """one centre with 5 % .. 50 % of its bits flipped, row by row: the rows with few flips are everybody's nearest neighbours, and their
    lists overflow whatever M is (uniform random rows of 500 seldom collect more than 48 links)"""
    centre = rng.integers(0, 2 ** 32, size=w, dtype=np.uint32)

    def make(m):
        p = 0.5 * 10.0 ** -rng.random(m)
        return centre[None, :] ^ np.packbits(rng.random((m, w * 32)) < p[:, None], axis=1).view(np.uint32)

    return make(n), make(nq)


FAMILIES = {"random": fam_random, "patterns": fam_bits}  # patterns: each row one of 12 -- popcount ties everywhere, the slot decides
LONG_LIST_FAMILIES = dict(FAMILIES, hubs=fam_hubs)


def revlink_class(chunks, M0):
    """which kernel launch_revlink (kernels.hip) sends a Hamming index's full lists to"""
    if 128 <= chunks <= 512 and M0 <= 32:
        return "pairs3" if chunks <= 192 else "pairs4" if chunks <= 256 else "pairs6" if chunks <= 384 else "pairs8"
    if staged_lds_bytes(chunks, M0) <= 150 * 1024 and M0 <= 256:
        return "staged"
    return "generic"


def build_pair(capi, oracle, rows, M, efc, seed=13):
    n, words = rows.shape
    labels = np.arange(n, dtype=np.uint64) + LABEL0
    ora = oracle.OracleIndex("hamming", words, M=M, ef_construction=efc, ef=EF, seed=seed, sum_mode=oracle.SUM_WAVE64)
    ora.add_planned(labels, rows, max_batch=128, min_ratio=4)
    gpu = capi.GpuIndex("hamming", words, M=M, ef_construction=efc, ef=EF, seed=seed)
    gpu.set_add_batch(128, 4)
    gpu.add_many(labels, rows)
    gpu.flush()
    assert len(gpu) == n
    return ora, gpu


def check_build_and_search(capi, oracle, monkeypatch, family, words, M, efc):
    """as test_row_widths_around_every_load_block_boundary (tests/test_gpu_parity.py) asserts: the build edge for edge, the search bit for
    bit in both launch shapes, a lone query, the gathered distances in both launch shapes; returns the pair for more"""
    rng = np.random.default_rng([words, M])
    rows, queries = LONG_LIST_FAMILIES[family](rng, N, words, NQ)
    ora, gpu = build_pair(capi, oracle, rows, M, efc)
    gg = gpu.export_graph(with_vectors=True)
    assert_same_graph(gg, ora.export_graph())
    assert np.array_equal(gg["vectors"], rows)
    want = ora.search_batch(queries, K)
    dev = Answers(gpu, queries, K)
    for waves in (0, 4):  # the automatic shape (40 queries: the latency-bound walk) and the classic kernel
        gpu.set_search_shape(waves)
        assert_answers(dev.search(NQ), want, NQ, f"waves={waves}")
    gpu.set_search_shape(0)
    l1, d1 = gpu.search(queries[0], K)
    assert len(l1) == K and np.array_equal(l1, want[0][0]) and np.array_equal(bits(d1), bits(want[1][0]))
    picks = rng.integers(0, N, 64).astype(np.uint32)
    gref = np.array([oracle.distance(queries[1], rows[s], "hamming", oracle.SUM_WAVE64) for s in picks], dtype=np.float32)
    for kernel, g in zip(("plain", "walkshape"), gathers(gpu, queries[1], picks, monkeypatch)):
        assert np.array_equal(bits(g), bits(gref)), ("distance_gather", kernel, int(np.sum(bits(g) != bits(gref))))
    return rows, queries, ora, gpu, gg


# ------------------------------------------------------------------------------------------------
# a. builds, edge for edge, and searches, bit for bit
# ------------------------------------------------------------------------------------------------
# 386: the first width whose eighth register slot holds a chunk (lanes 0 and 1); 448: seven full load steps; 449: one chunk in the eighth;
# 500: the cap.  The last chunk full, and ragged (one to three words short)
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("M", [4, 8])
@pytest.mark.parametrize("ragged", [0, 1], ids=["full", "ragged"])
@pytest.mark.parametrize("chunks", [386, 448, 449, 500])
def test_build_and_search_with_eight_chunks_per_lane(capi, oracle, monkeypatch, chunks, ragged, M, family):
    words = chunks * 4 - ragged * (1 + (chunks + M) % 3)
    assert (words + 3) // 4 == chunks and revlink_class(chunks, 2 * M) == "pairs8"
    rows, queries, ora, gpu, gg = check_build_and_search(capi, oracle, monkeypatch, family, words, M, 32)
    c = gpu.counters()
    if family == "random":
        assert c["add_reprunes"] > 0, "no full list was re-pruned: k_revlink_pairs<M_HAMMING, 8> did not run"
    gpu.close()


@pytest.mark.parametrize("family", list(LONG_LIST_FAMILIES))
@pytest.mark.parametrize("chunks,kernel", [(500, "generic"), (140, "staged")])
def test_build_with_lists_too_long_for_the_pairs_kernel(capi, oracle, monkeypatch, chunks, kernel, family):
    """M = 24 (M0 = 48 > 32: no all-pairs table): 50 staged rows of 500 chunks are 400 KB, past the 150 KB the staged kernel may take; of 140
    chunks, 112 KB"""
    M = 24
    assert revlink_class(chunks, 2 * M) == kernel
    assert staged_lds_bytes(500, 48) > 150 * 1024 > staged_lds_bytes(140, 48) > 112000
    rows, queries, ora, gpu, gg = check_build_and_search(capi, oracle, monkeypatch, family, chunks * 4, M, 64)
    c = gpu.counters()
    if family == "hubs":
        # (k_revlink_staged counts its re-prunes; the generic k_revlink counts its distance evaluations alone)
        assert c["add_revlink_evals"] > 0, "no full list was re-pruned"
        assert (c["add_reprunes"] == 0) == (kernel == "generic"), c
    gpu.close()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_filtered_search_and_the_file_at_the_cap(capi, oracle, monkeypatch, family):
    words, M, efc = 2000, 8, 32
    rows, queries, ora, gpu, g = check_build_and_search(capi, oracle, monkeypatch, family, words, M, efc)
    dist = ref.distance_matrix(oracle, rows, queries, "hamming", oracle.SUM_WAVE64)
    u = np.random.default_rng(7).random(N)
    wide, narrow = u < 0.8, u < 0.1
    # the rule (filter.hip): exact iff allowed^2 <= 5.6 ef n, i.e. up to 259 allowed rows here
    assert wide.sum() ** 2 > 5.6 * EF * N >= narrow.sum() ** 2 and narrow.sum() > K + 3
    dev = Dev(gpu, queries, K)
    try:
        gpu.set_filter_policy("auto")
        before = gpu.filter_stats()
        got = dev.filtered(gpu.filter_from_bitmap(wide))
        assert gpu.last_filtered_launch()["path"] == "walk"
        same(got, ref.search(g, dist, wide, M, K, EF))
        idx = np.flatnonzero(narrow)
        f = gpu.filter_from_bitmap(narrow)
        for skip in (0, 3):
            s, dd, c, D, E, lab = dev.filtered(f, skip=skip)
            assert gpu.last_filtered_launch()["path"] == "exact"
            t_ids, t_d = oracle.bruteforce(rows[idx], queries, K + skip, "hamming", sum_mode=oracle.SUM_WAVE64)
            assert np.array_equal(s, idx[t_ids[:, skip:]].astype(np.uint32))
            assert np.array_equal(bits(dd), bits(t_d[:, skip:]))
            assert np.all(c == K) and np.all(D == idx.size) and np.all(E == 0)
        after = gpu.filter_stats()
        assert (after["walk"] - before["walk"], after["exact"] - before["exact"]) == (1, 2)
    finally:
        gpu.set_filter_policy("auto")
    # the file: 4 x words vector bytes per node, and back
    lab, dst, cnt = gpu.search_batch(queries, K)
    want = ora.search_batch(queries, K)
    assert np.array_equal(lab, want[0]) and np.array_equal(bits(dst), bits(want[1]))
    blob = gpu.save_buffer()
    assert len(blob) == 136 + sum(10 + (4 + 2 * M * 6) + int(l) * (4 + M * 6) + 4 * words for l in g["levels"])
    again = capi.GpuIndex("hamming", words, M=M, ef_construction=efc, ef=EF, seed=13)
    again.load_buffer(blob)
    assert len(again) == N and again.checksum() == gpu.checksum()
    lab2, dst2, cnt2 = again.search_batch(queries, K)
    assert np.array_equal(lab2, lab) and np.array_equal(bits(dst2), bits(dst)) and np.array_equal(cnt2, cnt)
    gpu.close()
    again.close()


# ------------------------------------------------------------------------------------------------
# b. the dense popcount matrix
# ------------------------------------------------------------------------------------------------
_POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.int64)


def popcount_matrix(A, B):
    """[na][nb] int64 popcounts of the XOR, a byte at a time"""
    return np.stack([_POP8[(a[None, :] ^ B).view(np.uint8)].sum(axis=1) for a in A])


# query blocks and column blocks ragged on both sides of 16 and 256; the widths: one word, an odd count of words, the last width at which
# sixteen query rows fit 64 KB (1024), the first chunk past it (1028: eight rows), the cap (2000: eight rows)
@pytest.mark.parametrize("na,nb", [(1, 1), (15, 255), (17, 257), (33, 513)])
@pytest.mark.parametrize("words", [1, 25, 1024, 1028, 2000])
def test_dense_popcount_matrix(capi, words, na, nb):
    rng = np.random.default_rng([words, na, nb])
    B, A = fam_random(rng, nb, words, na)
    if nb > 2:
        B[1], B[2] = A[0], ~A[0]  # distances 0 and 32 x words
    want = popcount_matrix(A, B)
    got = capi.distance_matrix(A, B, "hamming", exact_order=False)
    assert got.shape == (na, nb) and np.array_equal(got.astype(np.int64), want) and np.array_equal(got, np.floor(got)), np.argwhere(got != want)[:4].tolist()
    exact = capi.distance_matrix(A, B, "hamming", exact_order=True)
    assert np.array_equal(bits(got), bits(exact))


def test_dense_popcount_matrix_past_the_widest_query_block(capi):
    """one query row of 16384 words is the 64 KB block; 16388 words (4097 chunks) fit no block: the call answers right or refuses, and the
    library goes on answering.  8192 / 16384 words: the blocks of two rows and of one"""
    rng = np.random.default_rng(16388)
    for words in (4096, 8192, 16384):  # four rows, two, one
        B, A = fam_random(rng, 5, words, 3)
        assert np.array_equal(capi.distance_matrix(A, B, "hamming", exact_order=False).astype(np.int64), popcount_matrix(A, B)), words
    B, A = fam_random(rng, 5, 16388, 3)
    try:
        got = capi.distance_matrix(A, B, "hamming", exact_order=False)
    except capi.LanternGpuError as err:
        assert "distance_matrix" in str(err)
    else:
        assert np.array_equal(got.astype(np.int64), popcount_matrix(A, B))
    B, A = fam_random(rng, 5, 25, 3)
    assert np.array_equal(capi.distance_matrix(A, B, "hamming", exact_order=False).astype(np.int64), popcount_matrix(A, B))


# ------------------------------------------------------------------------------------------------
# c. the exact k-NN of Hamming indexes
# ------------------------------------------------------------------------------------------------
def exact_search_is(capi, ix, queries, k, ids, dists):
    """ids and distance bits; every query certified, none recomputed: popcount keys are exact"""
    nq = queries.shape[0]
    before = capi.exact_knn_stats()
    slots, got = ix.exact_search(queries, k)
    after = capi.exact_knn_stats()
    bad = np.nonzero(np.any(slots != ids, axis=1) | np.any(bits(got) != bits(dists), axis=1))[0]
    assert bad.size == 0, (f"{bad.size} of {nq} queries differ from the brute force", bad[:8].tolist(), slots[bad[0]][:12].tolist(), ids[bad[0]][:12].tolist())
    st = {key: after[key] - before[key] for key in after}
    assert st == {"queries": nq, "certified": nq, "fallback": 0}, st


KNN_CASES = [  # n, words, nq, k
    (300, 1024, 17, 10),   # the last width with sixteen query rows per workgroup
    (300, 1028, 33, 10),   # the first with eight
    (257, 2000, 16, 240),  # kk = 256 survivors out of 257 rows
    (4097, 1500, 5, 10),   # 4097 columns: one past the seed-column count
    (65537, 260, 3, 1),    # two column chunks; k_select's c_base at a wide stride
]


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("n,words,nq,k", KNN_CASES, ids=[f"n{c[0]}-w{c[1]}-q{c[2]}-k{c[3]}" for c in KNN_CASES])
def test_exact_search_on_wide_bit_rows_is_the_brute_force(capi, oracle, cores, n, words, nq, k, family):
    rng = np.random.default_rng([n, words, nq, k])
    rows, queries = FAMILIES[family](rng, n, words, nq)
    ids, dists = oracle.bruteforce(rows, queries, k, "hamming", oracle.SUM_WAVE64, cores)
    ix = index_of(capi, "hamming", "f32", rows, rows)
    exact_search_is(capi, ix, queries, k, ids, dists)
    ix.close()


# ------------------------------------------------------------------------------------------------
# d. the exact k-NN of b1 cosine indexes: k_dense_ham<true>
# ------------------------------------------------------------------------------------------------
def signed_rows(rng, n, d):
    """values in {-1, 0, 1} (only the strictly positive ones set a bit), every fiftieth row all non-positive: a zero norm"""
    x = rng.integers(-1, 2, size=(n, d), dtype=np.int8)
    x[::50] = -np.abs(x[::50])
    return x


B1_CASES = [  # d, n, nq, k
    (2000, 65537, 17, 10),  # 63 words in 16 chunks; two column chunks
    (33, 300, 16, 10),      # a ragged last word
    (1, 50, 7, 5),          # one bit: every distance is 0 or 1
]


@pytest.mark.parametrize("d,n,nq,k", B1_CASES, ids=[f"d{c[0]}-n{c[1]}" for c in B1_CASES])
def test_exact_search_on_b1_cosine_indexes_is_the_brute_force(capi, oracle, cores, d, n, nq, k):
    rng = np.random.default_rng([d, n, nq, k])
    rows, queries = signed_rows(rng, n, d), signed_rows(rng, nq, d).astype(np.float32)
    queries[1] = -1.0
    words, qwords = pack_bits_msb_first(rows), pack_bits_msb_first(queries)
    assert not words[0].any() and not qwords[0].any() and not qwords[1].any() and words[1:50].any(axis=1).sum() >= 10
    ids, dists = oracle.bruteforce(words, qwords, k, "cos_b1", oracle.SUM_SEQ, cores)
    ix = capi.GpuIndex("cos", d, M=4, ef_construction=8, seed=1, quantization="b1")
    if n > 1000:
        # rows only, as the index stores them (the importer copies storage words: the f32 view hands the packed bits over untouched)
        ix.import_graph(words.view(np.float32), empty_graph(n))
    else:  # through the device's own quantisation
        ix.set_add_batch(128, 4)
        ix.add_many(np.arange(n, dtype=np.uint64) + LABEL0, rows.astype(np.float32))
        ix.flush()
    assert np.array_equal(ix.export_graph(with_vectors=True)["vectors"], words)
    exact_search_is(capi, ix, queries, k, ids, dists)
    ix.close()
