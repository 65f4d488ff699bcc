// dense.cpp -- the dense path's host side: distance matrices and the SQL-callable distances, and the exact k-NN (exact search, PQ
// encoding, assign_to_clusters) as a pure plan (plan_exact_knn: lantern_gpu_plan_exact_knn shows it without a device) and one run of it;
// the same run over a filter's slot list is the filtered exact path's dense route (plan_filtered_dense, filtered_dense_device), and over
// the concatenated lists of a per-query-filter call's groups, segment by segment, that call's (plan_filtered_each_dense,
// filtered_each_dense_device).
// The kernels: bruteforce.hip, dense_native.hip; the two launchers this unit calls them through: kernels.hpp.
#include "dense.hpp"
#include "index.hpp"
#include "abi_guard.hpp"
#include "dense_tile.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>

namespace lgpu {

DenseEnv dense_env()
{
    DenseEnv e;
    if(const char *nv = std::getenv("LANTERN_GPU_DENSE_NATIVE")) e.native = std::atoi(nv);
    if(const char *fu = std::getenv("LANTERN_GPU_DENSE_FUSED")) e.fused = std::atoi(fu) != 0;
    return e;
}

namespace {
std::atomic<uint64_t> g_dense_kind[ 3 ];  // MFMA contraction launches of the process by operand kind: f32, f16, i8 (lantern_gpu_dense_kind_stats)
// lantern_gpu_exact_knn_stats: queries of every exact k-NN of the process, how many the certificate passed, how many took the
// exact-order fallback
std::atomic<uint64_t> g_knn_queries{ 0 }, g_knn_certified{ 0 }, g_knn_fallback{ 0 };

// lantern_gpu_dense_profile: HIP events around every launch of the fp32-MFMA contraction inside the exact k-NN (bench.py's
// c3_dense_exact_knn leg: the duration of steady full-chunk launches apart from the cold first ones and the partial last chunk).
// Off unless asked for; a process-wide diagnostic, not part of any index's state.
struct DenseLaunch { hipEvent_t a = nullptr, b = nullptr; uint32_t rows = 0, cols = 0, fused = 0; };
struct DenseProfile
{
    std::mutex               mu;
    bool                     on = false;
    std::vector<DenseLaunch> launches;
} g_dense_profile;
struct DenseTimer  // records event `a` now and `b` on destruction, on the launch stream
{
    DenseLaunch l;
    hipStream_t st;
    bool        armed = false;
    DenseTimer(hipStream_t s, uint32_t rows, uint32_t cols, uint32_t fused) : st(s)
    {
        if(!g_dense_profile.on) return;
        if(hipEventCreate(&l.a) != hipSuccess || hipEventCreate(&l.b) != hipSuccess) { (void)hipGetLastError(); return; }
        l.rows = rows; l.cols = cols; l.fused = fused;
        armed = hipEventRecord(l.a, st) == hipSuccess;
    }
    ~DenseTimer()
    {
        if(!armed) return;
        (void)hipEventRecord(l.b, st);
        std::lock_guard<std::mutex> g(g_dense_profile.mu);
        g_dense_profile.launches.push_back(l);
    }
};

// The exact k-NN's device temporaries (norms + best lists, the seed-column matrix, the candidate lists) come from a small grow-only pool
// per device instead of hipMalloc / hipFree per call -- a free synchronises the device, and a 1024 x 1M x 768 call made five of them:
// about a millisecond of a 13.6 ms call.  Blocks above 64 MB (the whole-chunk matrix of the unfused path) and the f32 copies of
// quantised rows are still allocated per call.  One exact k-NN at a time per device holds the pool (the calls are bandwidth- or
// MFMA-bound on the whole chip: nothing is lost by not overlapping them).
struct KnnPool
{
    std::mutex mu;
    void      *p[ 4 ] = { nullptr, nullptr, nullptr, nullptr };  // (3: a gathered chunk of a run over a slot list, pooled up to kGatherPoolMax)
    size_t     bytes[ 4 ] = { 0, 0, 0, 0 };
};
KnnPool g_knn_pool[ 16 ];
constexpr size_t kKnnPoolMax = (size_t)64 << 20;
// The gathered chunk of a run over a slot list is pooled up to a full chunk of 4096-dimensional f32 rows (201 MB at 768-d): the dense
// route of the filtered exact path answers a call in a fraction of a millisecond at small batches, and a hipMalloc / hipFree of the
// chunk per call -- the free synchronises the device -- would be a large share of it.  The block stays with the process, as the pool's others.
constexpr size_t kGatherPoolMax = (size_t)1 << 30;

// every device allocation of this unit: block `which` of a pool if one is given and the block is small, allocated for the call
// otherwise; released by the destructor
struct DeviceBlock
{
    void *ptr = nullptr;
    bool  own = false;
    DeviceBlock() = default;
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
    bool get(size_t need, KnnPool *pool = nullptr, int which = 0, size_t pool_max = kKnnPoolMax)
    {
        if(need == 0) need = 16;
        if(pool && need <= pool_max) {
            if(pool->bytes[ which ] < need) {
                if(pool->p[ which ]) (void)hipFree(pool->p[ which ]);
                pool->p[ which ] = nullptr;
                pool->bytes[ which ] = 0;
                if(hipMalloc(&pool->p[ which ], need) != hipSuccess) { (void)hipGetLastError(); return false; }
                pool->bytes[ which ] = need;
            }
            ptr = pool->p[ which ];
            return true;
        }
        own = hipMalloc(&ptr, need) == hipSuccess;
        if(!own) { (void)hipGetLastError(); ptr = nullptr; }
        return own;
    }
    template <class T> T *as() const { return (T *)ptr; }
    ~DeviceBlock() { if(own && ptr) (void)hipFree(ptr); }
};

bool metric_ok(usearch_metric_kind_t m) { return m == usearch_metric_cos_k || m == usearch_metric_l2sq_k || m == usearch_metric_hamming_k; }
}  // namespace

// ---- the plan of an exact k-NN: host arithmetic, run by exact_knn_run and read by the tests ---------------------------------------------
// Rows stored as f16 / i8 are contracted as they are stored (dense_native.hip) unless LANTERN_GPU_DENSE_NATIVE says otherwise;
// kDenseNativeDefault is what an unset switch means (set by the measurement rule recorded there).
static const int    kDenseNativeDefault = 1;
// column chunk.  [r3] 65536 columns x 1024 queries are 4096 tiles = 5.33 rounds of the 768 workgroups the contraction keeps
// resident (three per CU): the last round runs a third full.  98304 columns (6144 tiles = 8 rounds) were tried: l2sq 14.9 -> 14.5 ms
// per 1024 x 1M x 768 call, but cosine 15.4 -> 20.1 ms (the fused call repeated itself unfused), so the chunk stays.
static const size_t kDenseChunkRows = 65536, kDenseQueryTile = 1024;
// `fused`: the contractions (l2sq / cos) keep their distance matrix to themselves -- the tile epilogue appends what can still
// enter a query's top-kk to a candidate list, folded in after every launch -- once the first kSeedCols columns have given every
// query a radius the ordinary way.
static const size_t kSeedCols = 4096, kCandCap = 4096;
static const char  *kBadPlan = "lantern_gpu: bad plan input";

// which contraction runs, on what, and what the certificate is told: the part of the plan lantern_gpu_plan_dense shows
static const char *plan_operands(int64_t mcode_in, int64_t chunks_in, int64_t nb, int64_t native, ExactKnnPlan &p)
{
    if(mcode_in < 0 || mcode_in > 0x7FFFFFFF || chunks_in <= 0 || chunks_in > (int64_t)1 << 20 || nb < 0) return kBadPlan;
    p.mcode = (int)mcode_in;
    p.chunks = (uint32_t)chunks_in;
    const int  base = mcode_base(p.mcode);
    const bool f16 = mcode_is_f16(p.mcode), i8 = mcode_is_i8(p.mcode);
    p.bits = base == M_HAMMING || base == M_COS_B1;
    const bool native_on = (f16 || i8) && !p.bits && (native < 0 ? kDenseNativeDefault : (int)native) != 0;
    p.kind = !native_on ? 0 : f16 ? 1 : 2;
    p.copy = native_on ? 0 : f16 ? 1 : i8 ? 2 : 0;
    p.fchunks = native_on ? p.chunks : i8 ? p.chunks * 4 : f16 ? p.chunks * 2 : p.chunks;
    const uint64_t copy_bytes = p.copy ? (uint64_t)std::min<int64_t>(nb, (int64_t)kDenseChunkRows) * p.fchunks * 16 : 0;
    if(copy_bytes > 0xFFFFFFFFull) return "lantern_gpu: the f32 copy of a chunk of rows does not fit the plan";
    p.fb_bytes = (size_t)copy_bytes;
    // the certificate's dims: f32 scalars contracted; native f16 -- twice the halves contracted; 0 -- keys are exact
    p.dims = p.bits || (native_on && i8) ? 0u : native_on ? p.chunks * 16 : p.fchunks * 4;
    p.exact_keys = p.dims == 0;
    p.k_steps = p.bits ? 0u : (p.fchunks * 4 + 31) / 32;
    return nullptr;
}

const char *plan_exact_knn(int64_t mcode, int64_t chunks, int64_t nb_in, int64_t nq_in, int64_t k, int native, int fused, ExactKnnPlan &p)
{
    p = ExactKnnPlan();
    if(const char *why = plan_operands(mcode, chunks, nb_in, native, p)) return why;
    if(nq_in < 0 || k < 1 || k > 240) return kBadPlan;
    // rows and columns travel as 32-bit launch arguments and step fields; below that bound no size here leaves 64 bits
    if(nq_in > 0xFFFFFFFFll || nb_in > 0xFFFFFFFFll) return "lantern_gpu: the rows of an exact k-NN do not fit the plan";
    const size_t nq = (size_t)nq_in, nb = (size_t)nb_in;
    p.nq = nq; p.nb = nb; p.k = (uint32_t)k;
    // kk = k plus a margin: the MFMA distances (|q|^2 + |b|^2 - 2 q.b) differ from the exact-order ones in the
    // last bits, so the survivors are re-ranked exactly and only then cut to k
    p.kk = p.k + 16;
    p.chunk_rows = (uint32_t)std::min(nb, kDenseChunkRows);
    p.qtile = (uint32_t)kDenseQueryTile;
    p.seed_cols = (uint32_t)kSeedCols;
    p.cand_cap = (uint32_t)kCandCap;
    p.fused = fused != 0 && !p.bits && nb > kSeedCols;
    // the distance matrix of the unfused launches: a whole chunk, or only the seed columns
    p.ldd = p.fused ? p.seed_cols : p.chunk_rows;
    const size_t nqt_max = std::min(nq, kDenseQueryTile);
    p.qn_off = 0;
    p.bn_off = nq * 4;
    p.best_off = (nq + nb) * 4 + ((nq + nb) % 2) * 4;
    p.flag_off = p.best_off + nq * p.kk * 8;
    p.aux_bytes = (nq + nb) * 4 + 8 + nq * p.kk * 8 + (nq + 1) * 4;
    p.dd_bytes = nqt_max * p.ldd * 4;
    if(p.fused) {  // [nqt_max][cand_cap] keys, then the counters and the overflow flag
        p.cnt_off = nqt_max * kCandCap * 8;
        p.over_off = p.cnt_off + nqt_max * 4;
        p.cand_bytes = p.over_off + 16;
    }
    if(p.copy) p.fq_bytes = nq * p.fchunks * 16;
    // every chunk of base rows by every query tile; fused, the first chunk's tiles take two steps each: its seed columns plain, the rest fused
    const size_t tiles = (nq + kDenseQueryTile - 1) / kDenseQueryTile, nchunks = nb ? (nb + p.chunk_rows - 1) / p.chunk_rows : 0;
    p.n_steps = tiles * nchunks + (p.fused ? tiles : 0);
    return nullptr;
}

KnnStep ExactKnnPlan::step(size_t i) const
{
    const size_t tiles = (nq + qtile - 1) / qtile;
    size_t       chunk = 0, tile = 0, first = 0, cols = 0;  // first, cols: the step's columns inside its chunk (cols 0: all of them)
    if(!fused) {
        chunk = i / tiles, tile = i % tiles;
    } else if(i < 2 * tiles) {  // the first chunk (more than seed_cols rows, or the call would not be fused)
        tile = i / 2;
        if(i % 2 == 0) cols = seed_cols;
        else first = seed_cols;
    } else {
        chunk = 1 + (i - 2 * tiles) / tiles, tile = (i - 2 * tiles) % tiles;
    }
    const size_t c0 = chunk * chunk_rows, q0 = tile * qtile, nc = std::min<size_t>(chunk_rows, nb - c0);
    return { (uint32_t)q0, (uint32_t)std::min<size_t>(qtile, nq - q0), (uint32_t)(c0 + first), (uint32_t)(cols ? cols : nc - first), fused && !cols ? 1u : 0u };
}

// the steps of a plan that contracts every query with every row, as the list a run executes
static std::vector<KnnStep> plan_steps(const ExactKnnPlan &p)
{
    std::vector<KnnStep> steps(p.n_steps);
    for(size_t i = 0; i < p.n_steps; ++i) steps[ i ] = p.step(i);
    return steps;
}

// One run of a plan.  certified: one flag per query (1: the certificate of DESIGN.md 4.5 holds -- the result is the exact answer; 0: the
// caller recomputes the query in exact order, exact_knn_fallback).  *overflowed: a candidate list ran out of room (adversarially
// ordered rows): the caller repeats the search unfused.
// d_list == NULL: the base rows are d_base[0, nb).  Otherwise they are d_base[d_list[0, nb)], d_list ascending (a filter's slot list):
// every chunk is gathered into a contiguous block with its norms (k_gather_rows_norms) where the plain run points into d_base, the
// keys hold positions in the list, and the re-rank reads and emits through it.
// steps: the contraction launches, chunk-major, none across a chunk of p.chunk_rows rows -- plan_steps(p) for the two plans that
// contract every query with every row, EachDensePlan::steps for the segmented run (a query's keys then come from its own segment of
// the list only; everything behind the contractions is per query and runs unchanged).
// queued: NULL, or what the caller queues behind the certificate and in front of the wait, given the device flags (NULL: exact keys).
static bool exact_knn_run(const ExactKnnPlan &p, const std::vector<KnnStep> &steps, const uint4 *d_base, const uint32_t *d_list, const uint4 *d_q,
                          uint32_t *d_slots, float *d_dists, hipStream_t st, bool *overflowed, std::vector<uint32_t> &certified,
                          const EachDenseAnswers *queued = nullptr)
try {
    int dev = 0;
    (void)hipGetDevice(&dev);
    KnnPool *const               pool = (dev >= 0 && dev < 16) ? &g_knn_pool[ dev ] : nullptr;
    std::unique_lock<std::mutex> pool_lock;
    if(pool) pool_lock = std::unique_lock<std::mutex>(pool->mu);
    // An exception (bad_alloc in a host vector) behind queued launches unwinds through here: destroyed before the lock and the blocks,
    // this waits for the stream first, so that nothing queued names a pooled or freed block when the next run takes the pool.
    struct SyncOnUnwind
    {
        hipStream_t st;
        int         live = std::uncaught_exceptions();
        ~SyncOnUnwind() { if(std::uncaught_exceptions() > live) (void)hipStreamSynchronize(st); }
    };
    DeviceBlock b_aux, b_dd, b_cand, b_fq, b_fb, b_gb;  // (fq, fb: f32 copies of quantised rows -- the queries; one chunk of base rows.  gb: a gathered chunk)
    const SyncOnUnwind sync_on_unwind{ st };  // (declared last: destroyed first)
    const uint32_t nq = (uint32_t)p.nq, nb = (uint32_t)p.nb, kk = p.kk, chunks = p.chunks, fchunks = p.fchunks;
    const int      base_metric = mcode_base(p.mcode);
    auto dequant = [&](const uint4 *src, size_t nchunks, uint4 *dst) { return p.copy == 2 ? launch_dequant_i8(src, nchunks, dst, st) : launch_dequant_f16(src, nchunks, dst, st); };
    bool ok = b_aux.get(p.aux_bytes, pool, 0) && b_dd.get(p.dd_bytes, pool, 1);
    if(ok && p.fused) ok = b_cand.get(p.cand_bytes, pool, 2) && hipMemsetAsync(b_cand.as<char>() + p.cnt_off, 0, p.cand_bytes - p.cnt_off, st) == hipSuccess;
    if(ok && p.copy) ok = b_fq.get(p.fq_bytes) && b_fb.get(p.fb_bytes) && dequant(d_q, p.nq * chunks, b_fq.as<uint4>()) == hipSuccess;
    if(ok && d_list) ok = p.gb_bytes >= (size_t)p.chunk_rows * chunks * 16 && b_gb.get(p.gb_bytes, pool, 3, kGatherPoolMax);
    if(ok) {
        char *const     aux = b_aux.as<char>();
        float *const    dd = b_dd.as<float>(), *qn = (float *)(aux + p.qn_off), *bn = (float *)(aux + p.bn_off);
        uint64_t *const best = (uint64_t *)(aux + p.best_off), *cand = b_cand.as<uint64_t>();
        uint32_t *const flag = (uint32_t *)(aux + p.flag_off);
        uint32_t *const ccnt = p.fused ? (uint32_t *)(b_cand.as<char>() + p.cnt_off) : nullptr, *cover = p.fused ? (uint32_t *)(b_cand.as<char>() + p.over_off) : nullptr;
        uint4 *const    fb = b_fb.as<uint4>(), *gb = b_gb.as<uint4>();
        // the norms a gathered chunk gets in its own pass: the contraction's, unless it reads none or takes them from the f32 copy
        const int       gather_kind = p.bits || p.copy ? 3 : p.kind;
        const uint4    *qv = p.copy ? b_fq.as<uint4>() : d_q;
        ok = ok && hipMemsetAsync(best, 0xFF, p.nq * kk * 8, st) == hipSuccess;
        if(!p.bits) ok = ok && launch_norms(p.kind, base_metric, qv, nq, fchunks, qn, st) == hipSuccess;
        if(!p.bits && !p.copy && !d_list) ok = ok && launch_norms(p.kind, base_metric, d_base, nb, fchunks, bn, st) == hipSuccess;
        size_t si = 0;
        for(size_t c0 = 0; ok && c0 < p.nb; c0 += p.chunk_rows) {
            const size_t nc = std::min<size_t>(p.chunk_rows, p.nb - c0);
            const uint4 *bv = d_base + c0 * chunks;
            if(d_list) {
                DenseTimer t(st, 0, (uint32_t)nc, 2u);  // (lantern_gpu_dense_profile: fused = 2 marks a gather, rows = 0)
                ok = ok && launch_gather_rows_norms(gather_kind, base_metric, d_base, chunks, d_list + c0, (uint32_t)nc, gb, bn + c0, st) == hipSuccess;
                bv = gb;
            }
            if(p.copy) {
                ok = ok && dequant(bv, nc * chunks, fb) == hipSuccess;
                ok = ok && launch_norms(p.kind, base_metric, fb, (uint32_t)nc, fchunks, bn + c0, st) == hipSuccess;
                bv = fb;
            }
            for(; ok && si < steps.size() && steps[ si ].col0 < c0 + nc; ++si) {
                const KnnStep       s = steps[ si ];
                uint64_t *const     mine = best + (size_t)s.q0 * kk;
                const DenseOperands o = { p.kind, base_metric, qv + (size_t)s.q0 * fchunks, s.nqt, bv + (s.col0 - c0) * fchunks, s.cols, fchunks, qn + s.q0, bn + s.col0 };
                const DenseTopk     tk = { mine, kk, cand, ccnt, p.cand_cap, s.col0 };
                {
                    DenseTimer t(st, s.nqt, s.cols, s.fused != 0 ? 1u : 0u);
                    ok = ok && launch_contraction(o, dd, p.ldd, s.fused ? &tk : nullptr, st) == hipSuccess;
                    if(!p.bits) ++g_dense_kind[ p.kind ];
                }
                if(s.fused) ok = ok && launch_select_candidates(s.nqt, mine, kk, cand, ccnt, p.cand_cap, cover, st) == hipSuccess;
                else ok = ok && launch_select(dd, p.ldd, s.nqt, s.cols, s.col0, mine, kk, st) == hipSuccess;
            }
        }
        ok = ok && launch_rerank(p.mcode, d_q, nq, d_base, chunks, best, kk, p.k, d_slots, d_dists, d_list, st) == hipSuccess;
        // the certificate: 4 bytes per query to the host, behind the synchronisation the call makes anyway.  The popcount metrics
        // rank on the exact-order distance itself (the same integer arithmetic): their pre-selection is exact by construction.
        certified.assign(p.nq + 1, p.exact_keys ? 1u : 0u);
        certified[ p.nq ] = 0;
        if(!p.exact_keys) {
            ok = ok && hipMemsetAsync(flag + nq, 0, 4, st) == hipSuccess;
            ok = ok && launch_certify(base_metric, best, kk, d_dists, p.k, qn, nq, bn, nb, p.dims, flag, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(certified.data(), flag, (p.nq + 1) * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
        }
        uint32_t over = 0;
        if(p.fused) ok = ok && hipMemcpyAsync(&over, cover, 4, hipMemcpyDeviceToHost, st) == hipSuccess;
        if(queued) ok = ok && (*queued)(p.exact_keys ? nullptr : flag);
        ok = ok && hipStreamSynchronize(st) == hipSuccess;
        if(overflowed) *overflowed = over != 0;
        if(ok && certified[ p.nq ])  // a cosine row norm outside the bound's range: nothing is certified
            std::fill(certified.begin(), certified.end() - 1, 0u);
        certified.resize(p.nq);
    }
    if(!ok) (void)hipStreamSynchronize(st);  // nothing queued may still name the pooled blocks when the pool's lock is released
    return ok;
}
LANTERN_ABI_CATCH(nullptr)

// The queries the certificate refused, recomputed in the pair kernel's exact order over every base row: their rows gathered,
// k_pairs + k_select (top-k by (exact distance, slot)) per block of kFallbackQ queries and chunk of base rows, the keys written
// over their rows of the result.  nf x nb exact-order evaluations: rare (adversarial data), not fast.
static bool exact_knn_fallback(int mcode, uint32_t chunks, const uint4 *d_base, size_t nb, const uint4 *d_q, size_t k, const std::vector<uint32_t> &qidx,
                               uint32_t *d_slots, float *d_dists, hipStream_t st)
{
    const size_t nf = qidx.size(), CH = std::min(nb, kDenseChunkRows), kFallbackQ = 256, nfb = std::min(nf, kFallbackQ);
    DeviceBlock  b_idx, b_rows, b_best, b_dd;
    bool         ok = b_idx.get(nf * 4) && b_rows.get(nf * (size_t)chunks * 16) && b_best.get(nf * k * 8) && b_dd.get(nfb * CH * 4);
    uint32_t *const d_idx = b_idx.as<uint32_t>();
    uint4 *const    d_rows = b_rows.as<uint4>();
    uint64_t *const d_best = b_best.as<uint64_t>();
    float *const    d_dd = b_dd.as<float>();
    ok = ok && hipMemcpyAsync(d_idx, qidx.data(), nf * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemsetAsync(d_best, 0xFF, nf * k * 8, st) == hipSuccess;
    ok = ok && launch_gather_rows(d_q, chunks, d_idx, (uint32_t)nf, d_rows, st) == hipSuccess;
    for(size_t c0 = 0; ok && c0 < nb; c0 += CH) {
        const size_t nc = std::min(CH, nb - c0);
        for(size_t f0 = 0; ok && f0 < nf; f0 += kFallbackQ) {
            const size_t nft = std::min(kFallbackQ, nf - f0);
            ok = ok && launch_pairs(mcode, d_rows + f0 * chunks, (uint32_t)nft, d_base + c0 * chunks, (uint32_t)nc, chunks, d_dd, st) == hipSuccess;
            ok = ok && launch_select(d_dd, (uint32_t)nc, (uint32_t)nft, (uint32_t)nc, (uint32_t)c0, d_best + f0 * k, (uint32_t)k, st) == hipSuccess;
        }
    }
    ok = ok && launch_emit_topk(d_best, (uint32_t)k, d_idx, (uint32_t)nf, d_slots, d_dists, st) == hipSuccess;
    ok = ok && hipStreamSynchronize(st) == hipSuccess;
    if(!ok) (void)hipStreamSynchronize(st);
    return ok;
}

// A plan run to its certificate: once, and once more unfused (planned anew from the plan's own numbers) when a candidate list
// overflowed.  certified: the flag of every query; refused: the queries without one, which the caller recomputes.
static bool exact_knn_certified(const ExactKnnPlan &first, int native, const uint4 *d_base, const uint32_t *d_list, const uint4 *d_q, uint32_t *d_slots,
                                float *d_dists, hipStream_t st, std::vector<uint32_t> &certified, std::vector<uint32_t> &refused)
{
    bool over = false;
    if(!exact_knn_run(first, plan_steps(first), d_base, d_list, d_q, d_slots, d_dists, st, &over, certified)) return false;
    if(over) {  // the same call, unfused
        ExactKnnPlan plan;
        if(plan_exact_knn(first.mcode, first.chunks, (int64_t)first.nb, (int64_t)first.nq, (int64_t)first.k, native, 0, plan) != nullptr) return false;
        plan.gb_bytes = first.gb_bytes;
        if(!exact_knn_run(plan, plan_steps(plan), d_base, d_list, d_q, d_slots, d_dists, st, nullptr, certified)) return false;
    }
    refused.clear();
    for(size_t q = 0; q < first.nq; ++q)
        if(!certified[ q ]) refused.push_back((uint32_t)q);
    return true;
}

// ---- the filtered exact path's dense route (filter.hip filtered_search_locked branches on this plan) ----------------------------------
const char *plan_filtered_dense(int64_t mcode, int64_t chunks, int64_t allowed, int64_t nq, int64_t k, int64_t skip, int64_t min_queries, bool exact,
                                bool compact, int native, int fused, FilteredDensePlan &p)
{
    p = FilteredDensePlan();
    if(allowed < 0 || nq < 0 || k < 0 || skip < 0 || min_queries < 0 || k > 0xFFFFFFFFll || skip > 0xFFFFFFFFll) return kBadPlan;
    // the order of the reasons is the order the call meets them in: nothing to do, the switch, the batch, the path, the width, the index
    if(allowed == 0 || nq == 0 || k == 0) p.why = kDenseEmpty;
    else if(min_queries == 0) p.why = kDenseOff;
    else if(nq < min_queries) p.why = kDenseFewQueries;
    else if(!exact) p.why = kDenseWalkPath;
    else if(k + skip > 240) p.why = kDenseWide;
    else if(compact) p.why = kDenseCompact;
    else p.why = kDenseTaken;
    if(p.why != kDenseTaken) {  // (the operands are still checked: a bad metric code or row is refused on either side of the decision)
        ExactKnnPlan o;
        return plan_operands(mcode, chunks, allowed, native, o);
    }
    if(const char *why = plan_exact_knn(mcode, chunks, allowed, nq, k + skip, native, fused, p.knn)) return why;
    p.gather_rows = p.knn.chunk_rows;
    p.knn.gb_bytes = (size_t)p.knn.chunk_rows * p.knn.chunks * 16;
    p.norm_bytes = p.knn.bits ? 0 : p.knn.nb * 4;
    return nullptr;
}

bool filtered_dense_device(const FilteredDensePlan &p, int native, const uint4 *d_base, const uint32_t *d_list, const uint4 *d_q, uint32_t *d_slots,
                           float *d_dists, uint32_t *d_flags, hipStream_t st, std::vector<uint32_t> &refused)
try {
    if(p.why != kDenseTaken || !d_list) return false;
    std::vector<uint32_t> certified;
    if(!exact_knn_certified(p.knn, native, d_base, d_list, d_q, d_slots, d_dists, st, certified, refused)) return false;
    // the flags as the host settled them (a cosine norm out of range refuses every query) back to the device, for the answer kernel
    return hipMemcpyAsync(d_flags, certified.data(), p.knn.nq * 4, hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}
LANTERN_ABI_CATCH(nullptr)

// ---- the same route for a per-query-filter call: the groups of queries sharing a filter handle, one segmented run -------------------
const char *plan_filtered_each_dense(int64_t mcode, int64_t chunks, int64_t k, int64_t skip, int64_t min_group, bool compact, int native, const int64_t *ids,
                                     const int64_t *counts, const uint8_t *exact, size_t nq, EachDensePlan &p)
{
    p = EachDensePlan();
    if(k < 0 || skip < 0 || min_group < 0 || k > 0xFFFFFFFFll || skip > 0xFFFFFFFFll || nq > 0xFFFFFFFFull || (nq && (!ids || !counts || !exact))) return kBadPlan;
    for(size_t i = 0; i < nq; ++i)
        if(ids[ i ] < -1 || counts[ i ] < 0 || counts[ i ] > 0xFFFFFFFFll) return kBadPlan;
    {  // (the operands are checked on either side of the decision, as plan_filtered_dense does)
        ExactKnnPlan o;
        if(const char *why = plan_operands(mcode, chunks, 0, native, o)) return why;
    }
    p.group.assign(nq, 0xFFFFFFFFu);
    // the call-level reasons in the order the call meets them: the switch, the width, the index
    if(min_group == 0) return p.why = kEachDenseOff, nullptr;
    if(k + skip > 240) return p.why = kEachDenseWide, nullptr;
    if(compact) return p.why = kEachDenseCompact, nullptr;
    p.why = kEachDenseNoGroup;
    if(k == 0) return nullptr;
    // the exact-path queries behind a non-empty filter by (id, call order): a run of one id of at least min_group queries is a group
    std::vector<uint32_t> cand;
    for(size_t i = 0; i < nq; ++i)
        if(exact[ i ] && ids[ i ] >= 0 && counts[ i ] > 0) cand.push_back((uint32_t)i);
    std::stable_sort(cand.begin(), cand.end(), [&](uint32_t x, uint32_t y) { return ids[ x ] < ids[ y ]; });
    std::vector<std::pair<uint32_t, uint32_t>> runs;  // (first position in cand, length), then ordered by the first query: cand[first]
    for(size_t a = 0, b; a < cand.size(); a = b) {
        for(b = a + 1; b < cand.size() && ids[ cand[ b ] ] == ids[ cand[ a ] ]; ++b) {}
        if((int64_t)(b - a) >= min_group) runs.push_back({ (uint32_t)a, (uint32_t)(b - a) });
    }
    if(runs.empty()) return nullptr;
    std::sort(runs.begin(), runs.end(), [&](const auto &x, const auto &y) { return cand[ x.first ] < cand[ y.first ]; });
    uint64_t rows = 0;
    for(const auto &r : runs) rows += (uint64_t)counts[ cand[ r.first ] ];
    if(rows > 0xFFFFFFFFull) return p.why = kEachDenseTooMany, nullptr;
    p.qoff.push_back(0);
    p.seg.push_back(0);
    for(size_t g = 0; g < runs.size(); ++g) {
        for(uint32_t j = 0; j < runs[ g ].second; ++j) {
            const uint32_t q = cand[ runs[ g ].first + j ];
            p.group[ q ] = (uint32_t)g;
            p.order.push_back(q);
        }
        p.qoff.push_back((uint32_t)p.order.size());
        p.seg.push_back(p.seg.back() + (uint32_t)counts[ cand[ runs[ g ].first ] ]);
    }
    if(const char *why = plan_exact_knn(mcode, chunks, (int64_t)rows, (int64_t)p.order.size(), k + skip, native, 0, p.knn)) {
        p = EachDensePlan();
        return why;
    }
    p.why = kEachDenseTaken;
    p.gather_rows = p.knn.chunk_rows;
    p.knn.gb_bytes = (size_t)p.knn.chunk_rows * p.knn.chunks * 16;
    size_t g_lo = 0;  // the first group that reaches into the chunk
    for(uint64_t c0 = 0; c0 < rows; c0 += p.knn.chunk_rows) {
        const uint64_t c1 = std::min<uint64_t>(rows, c0 + p.knn.chunk_rows);
        while(p.seg[ g_lo + 1 ] <= c0) ++g_lo;
        for(size_t g = g_lo; g < runs.size() && p.seg[ g ] < c1; ++g) {
            const uint32_t col0 = (uint32_t)std::max<uint64_t>(p.seg[ g ], c0), cols = (uint32_t)std::min<uint64_t>(p.seg[ g + 1 ], c1) - col0;
            for(uint32_t q0 = p.qoff[ g ]; q0 < p.qoff[ g + 1 ]; q0 += p.knn.qtile)
                p.steps.push_back({ q0, std::min(p.knn.qtile, p.qoff[ g + 1 ] - q0), col0, cols, 0u });
        }
    }
    return nullptr;
}

bool filtered_each_dense_device(const EachDensePlan &p, const uint4 *d_base, const uint32_t *d_list, const uint4 *d_q, uint32_t *d_slots, float *d_dists,
                                hipStream_t st, const EachDenseAnswers &answers, std::vector<uint32_t> &refused)
try {
    if(p.why != kEachDenseTaken || !d_list) return false;
    std::vector<uint32_t> certified;
    if(!exact_knn_run(p.knn, p.steps, d_base, d_list, d_q, d_slots, d_dists, st, nullptr, certified, &answers)) return false;
    refused.clear();
    for(size_t q = 0; q < certified.size(); ++q)
        if(!certified[ q ]) refused.push_back((uint32_t)q);
    return true;
}
LANTERN_ABI_CATCH(nullptr)

// fp32- or native-MFMA contraction in chunks of 64k base rows + running top-(k+16) + exact-order re-rank, then per query the certificate
// that the top-(k+16) held the exact answer; the refused queries are recomputed in exact order.
bool exact_knn_device(int mcode, uint32_t chunks, const uint4 *d_base, size_t nb, const uint4 *d_q, size_t nq, size_t k, uint32_t *d_slots,
                      float *d_dists, hipStream_t st)
try {
    const DenseEnv        env = dense_env();
    ExactKnnPlan          plan;
    std::vector<uint32_t> certified, refused;
    if(plan_exact_knn(mcode, chunks, (int64_t)nb, (int64_t)nq, (int64_t)k, env.native, env.fused, plan) != nullptr) return false;
    if(!exact_knn_certified(plan, env.native, d_base, nullptr, d_q, d_slots, d_dists, st, certified, refused)) return false;
    g_knn_queries += nq;
    g_knn_certified += nq - refused.size();
    g_knn_fallback += refused.size();
    return refused.empty() || exact_knn_fallback(mcode, chunks, d_base, nb, d_q, k, refused, d_slots, d_dists, st);
}
LANTERN_ABI_CATCH(nullptr)

}  // namespace lgpu

// =====================================================================================================
// C ABI
// =====================================================================================================
using namespace lgpu;

extern "C" {

void lantern_gpu_distance_matrix(const void *a, size_t na, const void *b, size_t nb, usearch_scalar_kind_t kind, size_t dims,
                                 usearch_metric_kind_t metric, int exact_order, float *out, usearch_error_t *e)
try {
    CLEAR(e);
    if(!metric_ok(metric)) { FAIL(e, "lantern_gpu: unsupported metric kind (expected cos, l2sq or hamming)"); return; }
    const bool ham = metric == usearch_metric_hamming_k;
    // f16 / i8: rows of IEEE halves / int8 as an index of that storage holds them, under cos / l2sq (upstream usearch_distance takes them)
    const bool h16 = kind == usearch_scalar_f16_k, s8 = kind == usearch_scalar_i8_k;
    if(ham != (kind == usearch_scalar_b1_k) || (!ham && kind != usearch_scalar_f32_k && !h16 && !s8)) { FAIL(e, "lantern_gpu: scalar kind does not fit the metric"); return; }
    if(!a || !b || !out || dims == 0) { FAIL(e, "lantern_gpu: bad arguments"); return; }
    if(lantern_gpu_device_count() <= 0) { FAIL(e, kNoDevice); return; }
    if(na == 0 || nb == 0) return;
    const size_t in_bytes = ham ? (dims + 7) / 8 : h16 ? dims * 2 : s8 ? dims : dims * 4;
    const size_t chunks = (in_bytes + 15) / 16, row = chunks * 16;
    const int    mcode = (int)metric + (h16 ? M_F16 : s8 ? M_I8 : 0), dkind = h16 ? 1 : s8 ? 2 : 0;
    std::vector<char> ha(na * row, 0), hb(nb * row, 0);
    for(size_t i = 0; i < na; ++i) std::memcpy(&ha[ i * row ], (const char *)a + i * in_bytes, in_bytes);
    for(size_t i = 0; i < nb; ++i) std::memcpy(&hb[ i * row ], (const char *)b + i * in_bytes, in_bytes);
    DeviceBlock da, db, dout, dn;
    bool        ok = da.get(na * row) && db.get(nb * row) && dout.get(na * nb * 4) && dn.get((na + nb) * 4);
    ok = ok && hipMemcpy(da.ptr, ha.data(), na * row, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(db.ptr, hb.data(), nb * row, hipMemcpyHostToDevice) == hipSuccess;
    if(exact_order) {
        ok = ok && launch_pairs(mcode, da.as<uint4>(), (uint32_t)na, db.as<uint4>(), (uint32_t)nb, (uint32_t)chunks, dout.as<float>(), nullptr) == hipSuccess;
    } else {  // the dense contraction: the MFMA of the operand type for l2sq / cos, popcounts for hamming (which reads no norms)
        void *const         an = dn.ptr, *bnn = dn.as<char>() + na * 4;
        const DenseOperands o = { dkind, (int)metric, da.as<uint4>(), (uint32_t)na, db.as<uint4>(), (uint32_t)nb, (uint32_t)chunks, an, bnn };
        if(!ham) {
            ok = ok && launch_norms(dkind, (int)metric, o.Q, o.nq, o.chunks, an, nullptr) == hipSuccess;
            ok = ok && launch_norms(dkind, (int)metric, o.B, o.nb, o.chunks, bnn, nullptr) == hipSuccess;
            ++g_dense_kind[ dkind ];
        }
        ok = ok && launch_contraction(o, dout.as<float>(), (uint32_t)nb, nullptr, nullptr) == hipSuccess;
    }
    ok = ok && hipMemcpy(out, dout.ptr, na * nb * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if(!ok) FAIL(e, "lantern_gpu: HIP failure in distance_matrix");
}
LANTERN_ABI_CATCH_VOID(e)

float usearch_distance(const void *a, const void *b, usearch_scalar_kind_t kind, size_t dims, usearch_metric_kind_t metric,
                       usearch_error_t *e)
try {
    float out = 0.f;
    lantern_gpu_distance_matrix(a, 1, b, 1, kind, dims, metric, 1, &out, e);
    return out;
}
LANTERN_ABI_CATCH(e)

// ---- SQL-callable semantics (hnsw.c:296-405) ---------------------------------------------------------

static thread_local char g_dim_msg[ 160 ];

static bool same_dims(int a_dim, int b_dim, usearch_error_t *e)
try {
    if(a_dim == b_dim) return true;
    // hnsw.c:301-303
    std::snprintf(g_dim_msg, sizeof(g_dim_msg), "expected equally sized arrays but got arrays with dimensions %d and %d", a_dim, b_dim);
    FAIL(e, g_dim_msg);
    return false;
}
LANTERN_ABI_CATCH(e)

float lantern_l2sq_dist(const float *a, int a_dim, const float *b, int b_dim, usearch_error_t *e)
try {
    CLEAR(e);
    if(!same_dims(a_dim, b_dim, e)) return 0.f;
    return usearch_distance(a, b, usearch_scalar_f32_k, (size_t)a_dim, usearch_metric_l2sq_k, e);
}
LANTERN_ABI_CATCH(e)

float lantern_cos_dist(const float *a, int a_dim, const float *b, int b_dim, usearch_error_t *e)
try {
    CLEAR(e);
    if(!same_dims(a_dim, b_dim, e)) return 0.f;
    return usearch_distance(a, b, usearch_scalar_f32_k, (size_t)a_dim, usearch_metric_cos_k, e);
}
LANTERN_ABI_CATCH(e)

int32_t lantern_hamming_dist(const int32_t *a, int a_dim, const int32_t *b, int b_dim, usearch_error_t *e)
try {
    CLEAR(e);
    if(!same_dims(a_dim, b_dim, e)) return 0;
    // hnsw.c:317-319: dims = a_dim * sizeof(int32) * CHAR_BIT bits; result cast to int32 (hnsw.c:375)
    return (int32_t)usearch_distance(a, b, usearch_scalar_b1_k, (size_t)a_dim * 32, usearch_metric_hamming_k, e);
}
LANTERN_ABI_CATCH(e)

// ---- the exact k-NN's plan and counters ---------------------------------------------------------------------------------------------

const char *lantern_gpu_plan_dense(const int64_t in[ 4 ], uint32_t out[ 4 ])
{
    if(!in || !out) return "lantern_gpu: null plan array";
    ExactKnnPlan p;
    if(const char *why = plan_operands(in[ 0 ], in[ 1 ], in[ 2 ], in[ 3 ], p)) return why;
    out[ 0 ] = (uint32_t)p.kind;
    out[ 1 ] = (uint32_t)p.fb_bytes;
    out[ 2 ] = p.dims;
    out[ 3 ] = p.k_steps;
    return nullptr;
}

const char *lantern_gpu_plan_exact_knn(const int64_t in[ 7 ], uint32_t out[ 34 ], uint32_t steps[][ 4 ], size_t cap, size_t *n_steps)
try {
    if(!in || !out || !n_steps || (cap && !steps)) return "lantern_gpu: null plan array";
    ExactKnnPlan p;
    if(const char *why = plan_exact_knn(in[ 0 ], in[ 1 ], in[ 2 ], in[ 3 ], in[ 4 ], in[ 5 ] < 0 ? -1 : in[ 5 ] != 0, in[ 6 ] < 0 ? -1 : in[ 6 ] != 0, p)) return why;
    const uint32_t words[ 14 ] = { (uint32_t)p.kind, (uint32_t)p.copy, p.fchunks, p.bits, p.exact_keys, p.dims, p.k_steps, p.kk, p.chunk_rows, p.qtile, p.seed_cols,
                                   p.cand_cap, p.fused, p.ldd };
    const uint64_t sizes[ 10 ] = { p.aux_bytes, p.dd_bytes, p.cand_bytes, p.fq_bytes, p.fb_bytes, p.qn_off, p.bn_off, p.best_off, p.flag_off, p.cnt_off };
    std::copy(words, words + 14, out);
    for(int i = 0; i < 10; ++i) { out[ 14 + 2 * i ] = (uint32_t)sizes[ i ]; out[ 15 + 2 * i ] = (uint32_t)(sizes[ i ] >> 32); }
    for(size_t i = 0; i < p.n_steps && i < cap; ++i) {
        const KnnStep s = p.step(i);
        steps[ i ][ 0 ] = s.nqt; steps[ i ][ 1 ] = s.cols; steps[ i ][ 2 ] = s.fused; steps[ i ][ 3 ] = s.col0;
    }
    *n_steps = p.n_steps;
    return nullptr;
}
catch(...) {
    return kAbiException;  // (NULL is this function's "accepted")
}

const char *lantern_gpu_plan_filtered_dense(const int64_t in[ 11 ], uint32_t out[ 8 ], uint32_t steps[][ 4 ], size_t cap, size_t *n_steps)
try {
    if(!in || !out || !n_steps || (cap && !steps)) return "lantern_gpu: null plan array";
    FilteredDensePlan p;
    if(const char *why = plan_filtered_dense(in[ 0 ], in[ 1 ], in[ 2 ], in[ 3 ], in[ 4 ], in[ 5 ], in[ 6 ], in[ 7 ] != 0, in[ 8 ] != 0,
                                             in[ 9 ] < 0 ? -1 : in[ 9 ] != 0, in[ 10 ] < 0 ? -1 : in[ 10 ] != 0, p))
        return why;
    const bool     taken = p.why == kDenseTaken;
    const uint64_t sizes[ 2 ] = { p.knn.gb_bytes, p.norm_bytes };
    out[ 0 ] = taken ? 1u : 0u;
    out[ 1 ] = (uint32_t)p.why;
    out[ 2 ] = p.knn.kk;
    out[ 3 ] = p.gather_rows;
    for(int i = 0; i < 2; ++i) { out[ 4 + 2 * i ] = (uint32_t)sizes[ i ]; out[ 5 + 2 * i ] = (uint32_t)(sizes[ i ] >> 32); }
    for(size_t i = 0; i < p.knn.n_steps && i < cap; ++i) {
        const KnnStep s = p.knn.step(i);
        steps[ i ][ 0 ] = s.nqt; steps[ i ][ 1 ] = s.cols; steps[ i ][ 2 ] = s.fused; steps[ i ][ 3 ] = s.col0;
    }
    *n_steps = p.knn.n_steps;
    return nullptr;
}
catch(...) {
    return kAbiException;
}

const char *lantern_gpu_plan_filtered_each_dense(const int64_t in[ 7 ], const int64_t queries[][ 3 ], size_t nq, uint32_t out[ 6 ], uint32_t group[],
                                                 uint32_t order[], uint32_t seg[], uint32_t steps[][ 4 ], size_t cap, size_t *n_steps)
try {
    if(!in || !out || !n_steps || (cap && !steps) || (nq && (!queries || !group || !order || !seg))) return "lantern_gpu: null plan array";
    std::vector<int64_t> ids(nq), counts(nq);
    std::vector<uint8_t> exact(nq);
    for(size_t i = 0; i < nq; ++i) { ids[ i ] = queries[ i ][ 0 ]; counts[ i ] = queries[ i ][ 1 ]; exact[ i ] = queries[ i ][ 2 ] != 0; }
    EachDensePlan p;
    if(const char *why = plan_filtered_each_dense(in[ 0 ], in[ 1 ], in[ 2 ], in[ 3 ], in[ 4 ], in[ 5 ] != 0, in[ 6 ] < 0 ? -1 : in[ 6 ] != 0, ids.data(),
                                                  counts.data(), exact.data(), nq, p))
        return why;
    const bool taken = p.why == kEachDenseTaken;
    out[ 0 ] = (uint32_t)p.groups();
    out[ 1 ] = (uint32_t)p.order.size();
    out[ 2 ] = (uint32_t)p.why;
    out[ 3 ] = taken ? p.knn.kk : 0u;
    out[ 4 ] = p.gather_rows;
    out[ 5 ] = taken ? p.seg.back() : 0u;
    std::copy(p.group.begin(), p.group.end(), group);
    std::copy(p.order.begin(), p.order.end(), order);
    std::copy(p.seg.begin(), p.seg.end(), seg);
    for(size_t i = 0; i < p.steps.size() && i < cap; ++i) {
        const KnnStep &s = p.steps[ i ];
        steps[ i ][ 0 ] = s.q0; steps[ i ][ 1 ] = s.nqt; steps[ i ][ 2 ] = s.col0; steps[ i ][ 3 ] = s.cols;
    }
    *n_steps = p.steps.size();
    return nullptr;
}
catch(...) {
    return kAbiException;
}

void lantern_gpu_dense_kind_stats(uint64_t launches[ 3 ])
{
    if(!launches) return;
    for(int i = 0; i < 3; ++i) launches[ i ] = g_dense_kind[ i ].load();
}

void lantern_gpu_exact_knn_stats(uint64_t *queries, uint64_t *certified, uint64_t *fallback)
{
    if(queries) *queries = g_knn_queries.load();
    if(certified) *certified = g_knn_certified.load();
    if(fallback) *fallback = g_knn_fallback.load();
}

// on != 0: start recording (forgets earlier records).  on == 0: stop, wait for the recorded launches and write up to `cap` of them:
// ms[i] = duration of launch i (HIP events on its stream), rows[i] x cols[i] = its queries x base rows, fused[i] = 1 for the
// launch with the fused top-k epilogue, 2 for the gather of a chunk of a slot list (rows[i] = 0, cols[i] its rows).  Returns the number of
// recorded launches.
size_t lantern_gpu_dense_profile(int on, float *ms, uint32_t *rows, uint32_t *cols, uint32_t *fused, size_t cap)
try {
    std::vector<DenseLaunch> got;
    {
        std::lock_guard<std::mutex> g(g_dense_profile.mu);
        if(on) {
            for(auto &l : g_dense_profile.launches) { (void)hipEventDestroy(l.a); (void)hipEventDestroy(l.b); }
            g_dense_profile.launches.clear();
            g_dense_profile.on = true;
            return 0;
        }
        g_dense_profile.on = false;
        got.swap(g_dense_profile.launches);
    }
    for(size_t i = 0; i < got.size(); ++i) {
        float t = 0.0f;
        if(hipEventSynchronize(got[ i ].b) != hipSuccess || hipEventElapsedTime(&t, got[ i ].a, got[ i ].b) != hipSuccess) { (void)hipGetLastError(); t = -1.0f; }
        if(i < cap) {
            if(ms) ms[ i ] = t;
            if(rows) rows[ i ] = got[ i ].rows;
            if(cols) cols[ i ] = got[ i ].cols;
            if(fused) fused[ i ] = got[ i ].fused;
        }
        (void)hipEventDestroy(got[ i ].a);
        (void)hipEventDestroy(got[ i ].b);
    }
    return got.size();
}
LANTERN_ABI_CATCH(nullptr)

// ---- the exact k-NN's entry points ----------------------------------------------------------------------------------------------------

void lantern_gpu_exact_search(usearch_index_t h, const void *queries, size_t nq, size_t k, uint32_t *slots, float *distances,
                              usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix || nq == 0 || k == 0) return;
    if(k > 240) { FAIL(e, "lantern_gpu: exact_search supports k <= 240"); return; }
    std::lock_guard<std::mutex> g(ix->mu);
    if(!flush_locked(ix) || !pq_expand_locked(ix)) { FAIL(e, ix->err.c_str()); return; }
    const size_t n = ix->n, row_words = (size_t)ix->chunks * 4;
    if(n == 0) {
        for(size_t i = 0; i < nq * k; ++i) { slots[ i ] = EMPTY; distances[ i ] = INFINITY; }
        return;
    }
    const int    qkind = (ix->scalar == usearch_scalar_b1_k && !ix->b1_from_f32) ? usearch_scalar_b1_k : usearch_scalar_f32_k;  // queries arrive as f32 / bits
    const size_t in_bytes = input_bytes(ix, qkind);
    std::vector<uint32_t> padded(nq * row_words);
    for(size_t i = 0; i < nq; ++i) pad_row(ix, (const char *)queries + i * in_bytes, qkind, &padded[ i * row_words ]);
    uint4 *dq = (uint4 *)scratch(ix, kScratchCallIn, nq * row_words * 4);
    char  *dout = (char *)scratch(ix, kScratchCallOut, nq * k * 8 + 64);
    if(!dq || !dout) { FAIL(e, ix->err.c_str()); return; }
    uint32_t *d_slots = (uint32_t *)dout;
    float    *d_dists = (float *)(d_slots + nq * k);
    hipStream_t st = ix->stream;
    bool ok = hipMemcpyAsync(dq, padded.data(), nq * row_words * 4, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && exact_knn_device(ix->mcode, ix->chunks, ix->d_vec, n, dq, nq, k, d_slots, d_dists, st);
    ok = ok && hipMemcpy(slots, d_slots, nq * k * 4, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(distances, d_dists, nq * k * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if(!ok) FAIL(e, "lantern_gpu: HIP failure in exact_search");
}
LANTERN_ABI_CATCH_VOID(e)

// PQ k-means assignment (product_quantization.c:80-124 assign_to_clusters): the one dense N x k contraction in
// Lantern's C code -- N x k usearch_distance calls there, one fp32-MFMA pass + exact re-rank here.
void lantern_gpu_assign_to_clusters(const float *dataset, size_t n, size_t row_dims, size_t subvector_start, size_t subvector_dim,
                                    const float *centers, size_t k, usearch_metric_kind_t metric, uint32_t *out_cluster,
                                    float *out_distance, usearch_error_t *e)
try {
    CLEAR(e);
    if(metric != usearch_metric_cos_k && metric != usearch_metric_l2sq_k) { FAIL(e, "lantern_gpu: assign_to_clusters needs cos or l2sq"); return; }
    if(!dataset || !centers || !out_cluster || subvector_dim == 0 || subvector_start + subvector_dim > row_dims || k == 0) {
        FAIL(e, "lantern_gpu: bad arguments");
        return;
    }
    if(lantern_gpu_device_count() <= 0) { FAIL(e, kNoDevice); return; }
    if(n == 0) return;
    const size_t chunks = (subvector_dim + 3) / 4, rw = chunks * 4;
    std::vector<float> hp(n * rw, 0.f), hc(k * rw, 0.f);
    for(size_t i = 0; i < n; ++i) std::memcpy(&hp[ i * rw ], dataset + i * row_dims + subvector_start, subvector_dim * 4);
    for(size_t j = 0; j < k; ++j) std::memcpy(&hc[ j * rw ], centers + j * subvector_dim, subvector_dim * 4);
    DeviceBlock dp, dc, dout;
    bool        ok = dp.get(hp.size() * 4) && dc.get(hc.size() * 4) && dout.get(n * 8);
    ok = ok && hipMemcpy(dp.ptr, hp.data(), hp.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(dc.ptr, hc.data(), hc.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    // first minimum wins (strict `<` in the reference loop) == smallest (distance, index)
    uint32_t *const near = dout.as<uint32_t>();
    ok = ok && exact_knn_device((int)metric, (uint32_t)chunks, dc.as<uint4>(), k, dp.as<uint4>(), n, 1, near, (float *)(near + n), nullptr);
    ok = ok && hipMemcpy(out_cluster, near, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if(out_distance) ok = ok && hipMemcpy(out_distance, near + n, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if(!ok) FAIL(e, "lantern_gpu: HIP failure in assign_to_clusters");
}
LANTERN_ABI_CATCH_VOID(e)

}  // extern "C"
