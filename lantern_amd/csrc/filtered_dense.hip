// filtered_dense.hip -- the dense routes of the filtered exact path (DESIGN.md 4.9 "Dense exact path"): a single-filter call's, and the
// groups of a per-query-filter call that share a filter handle.  Both hand the allowed rows to the exact k-NN (dense.hpp), write the
// certified queries' answers with one kernel and leave the refused ones to k_search_exact_allowed.  Plans: dense.cpp.
#include <algorithm>
#include <iterator>
#include <vector>

#include "filtered_search.hpp"
#include "dense_seg.hpp"

namespace lgpu {

// The dense answers: the exact k-NN's re-ranked rows -- kk = k + skip (slot, distance) entries per dense query, ascending by (distance,
// slot) -- into a filtered call's outputs, as k_search_exact_allowed closes a query (frame_answer_rows, frame_close): rows [skip, skip
// + k) as label, distance, slot; tails label 0, +inf, EMPTY; count, D = allowed, E = 0; D added to totals[0].  One thread per answer
// cell.  flags == NULL: every query is certified; else flags[q] says so, and the refused queries' rows are left alone: the per-query
// launch behind this one answers them.  Every output pointer may be NULL.
// EACH (the segmented run of a per-query-filter call): dense query q is the call's query orig[q] and stands behind a filter of
// allowed[q] rows, and flags[nq] != 0 (a cosine row norm out of the certificate's range, in any segment) refuses them all.  Without
// it (a single-filter call) q is the call's query q, every query's filter has allowed_all rows, and neither array nor flags[nq] (the
// single-filter run writes nq flags) is read.
template <bool EACH>
__device__ __forceinline__ void dense_answers(const uint32_t *slots, const float *dists, const uint32_t *flags, const uint32_t *orig, const uint32_t *allowed,
                                              uint32_t allowed_all, uint32_t nq, uint32_t kk, uint32_t k, uint32_t skip, const uint64_t *labels, uint32_t n,
                                              uint64_t *out_labels, float *out_dists, uint32_t *out_slots, uint32_t *out_counts, uint64_t *out_D, uint64_t *out_E,
                                              unsigned long long *totals)
{
    if(EACH && flags && flags[ nq ]) return;
    const size_t cells = (size_t)nq * k;
    for(size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (size_t)gridDim.x * blockDim.x) {
        const uint32_t q = (uint32_t)(c / k), i = (uint32_t)(c % k);
        if(flags && !flags[ q ]) continue;
        const uint32_t al = EACH ? allowed[ q ] : allowed_all, have = al < kk ? al : kk, got = have <= skip ? 0u : (have - skip < k ? have - skip : k);
        const uint32_t oq = EACH ? orig[ q ] : q;
        const size_t   o = (size_t)oq * k + i;
        if(i < got) {
            const size_t   at = (size_t)q * kk + skip + i;
            const uint32_t slot = slots[ at ];
            if(out_labels) out_labels[ o ] = slot < n ? labels[ slot ] : 0;  // (every slot of the first `have` entries is a row's)
            if(out_dists) out_dists[ o ] = dists[ at ];
            if(out_slots) out_slots[ o ] = slot;
        } else {
            if(out_labels) out_labels[ o ] = 0;  // INVALID_ELEMENT_LABEL (hnsw.h:40)
            if(out_dists) out_dists[ o ] = __builtin_inff();
            if(out_slots) out_slots[ o ] = EMPTY;
        }
        if(i == 0) {
            if(out_counts) out_counts[ oq ] = got;
            if(out_D) out_D[ oq ] = al;
            if(out_E) out_E[ oq ] = 0;
            if(totals) atomicAdd(&totals[ 0 ], (unsigned long long)al);
        }
    }
}
__global__ void __launch_bounds__(256) k_dense_answers(const uint32_t *slots, const float *dists, const uint32_t *flags, uint32_t nq, uint32_t kk, uint32_t k,
                                                       uint32_t skip, uint32_t allowed, const uint64_t *labels, uint32_t n, uint64_t *out_labels, float *out_dists,
                                                       uint32_t *out_slots, uint32_t *out_counts, uint64_t *out_D, uint64_t *out_E, unsigned long long *totals)
{
    dense_answers<false>(slots, dists, flags, nullptr, nullptr, allowed, nq, kk, k, skip, labels, n, out_labels, out_dists, out_slots, out_counts, out_D, out_E, totals);
}
__global__ void __launch_bounds__(256) k_dense_each_answers(const uint32_t *slots, const float *dists, const uint32_t *flags, const uint32_t *orig,
                                                            const uint32_t *allowed, uint32_t nq, uint32_t kk, uint32_t k, uint32_t skip, const uint64_t *labels,
                                                            uint32_t n, uint64_t *out_labels, float *out_dists, uint32_t *out_slots, uint32_t *out_counts,
                                                            uint64_t *out_D, uint64_t *out_E, unsigned long long *totals)
{
    dense_answers<true>(slots, dists, flags, orig, allowed, 0u, nq, kk, k, skip, labels, n, out_labels, out_dists, out_slots, out_counts, out_D, out_E, totals);
}

bool filtered_dense_locked(Index *ix, const Filter *f, const FilteredDensePlan &plan, int native, const uint4 *d_q, size_t nq, size_t k, size_t skip,
                           const SearchOut &out, FilteredArgs &a, size_t lds, hipStream_t stream)
{
    static const char *kDenseFailed = "lantern_gpu: HIP failure on the dense route of the filtered exact path";
    const size_t kk = k + skip, dist_at = nq * kk * 4, flag_at = 2 * dist_at;
    char *const  blk = (char *)scratch(ix, kScratchDenseAnswers, flag_at + nq * 4);
    if(!blk) return false;
    uint32_t *const d_slots = (uint32_t *)blk, *d_flags = (uint32_t *)(blk + flag_at);
    float *const    d_dists = (float *)(blk + dist_at);
    if(!order_after_inserts(ix, stream)) return false;
    std::vector<uint32_t> refused;
    if(!filtered_dense_device(plan, native, ix->d_vec, f->d_slots, d_q, d_slots, d_dists, d_flags, stream, refused)) return set_err(ix, kDenseFailed), false;
    if(refused.size() < nq) {
        const size_t blocks = std::min<size_t>((nq * k + 255) / 256, 16384);
        hipLaunchKernelGGL(k_dense_answers, dim3((uint32_t)blocks), dim3(256), 0, stream, (const uint32_t *)d_slots, (const float *)d_dists,
                           (const uint32_t *)d_flags, (uint32_t)nq, (uint32_t)kk, (uint32_t)k, (uint32_t)skip, (uint32_t)f->count, (const uint64_t *)ix->d_labels, (uint32_t)ix->n,
                           out.labels, out.dists, out.slots, out.counts, out.D, out.E, (unsigned long long *)(ix->d_totals + kTotSearch));
        if(hipGetLastError() != hipSuccess) return set_err(ix, kDenseFailed), false;
    }
    if(!refused.empty()) {
        // the queries the certificate refused, by k_search_exact_allowed in its per-query form over a selection list of just those: today's
        // answers by construction.  (The launch counts as an exact launch of lantern_gpu_filter_stats: it is one.)
        std::vector<char> tbl(each_table_bytes(nq));
        const EachTables  t = each_tables(ix, tbl.data(), nq, nullptr, f, {}, refused, nullptr);
        a.frame.nq = (uint32_t)refused.size();
        if(filtered_launch(ix, true, a, lds, stream, &t.exact) < 0) return false;  // (pageable staging: the copy completes before this returns)
    }
    if(hipStreamSynchronize(stream) != hipSuccess) return set_err(ix, kDenseFailed), false;
    ix->c_filter_dense[ 0 ] += 1;
    ix->c_filter_dense[ 1 ] += nq;
    ix->c_filter_dense[ 2 ] += nq - refused.size();
    ix->c_filter_dense[ 3 ] += refused.size();
    const uint32_t shape[ 6 ] = { 3u, 0u, (uint32_t)kk, 0u, 0u, 0u };
    std::copy(std::begin(shape), std::end(shape), ix->last_filtered);
    ix->c_search_queries += nq;
    return true;
}

// ---- the dense route of a per-query-filter call (DESIGN.md 4.9 "Dense exact path, per-query filters") -----------------------------
// k_concat_slot_lists: the dense groups' slot lists, each a filter's own, into the call's one list L -- group g at positions
// [seg[g], seg[g + 1]).  One thread per position: its group by binary search over seg (strictly ascending: no group is empty), its
// slot from that group's list.
__global__ void __launch_bounds__(256) k_concat_slot_lists(const uint32_t *const *lists, const uint32_t *seg, uint32_t groups, uint32_t *out)
{
    const uint32_t total = seg[ groups ];
    for(size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = groups;  // seg[lo] <= p < seg[hi]
        while(hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if(seg[ mid ] <= p) lo = mid; else hi = mid;
        }
        out[ p ] = lists[ lo ][ p - seg[ lo ] ];
    }
}

bool filtered_each_dense_locked(Index *ix, const Filter *const *filters, const EachDensePlan &plan, const uint4 *d_q, size_t k, size_t skip,
                                const SearchOut &out, hipStream_t stream, std::vector<uint32_t> &refused)
{
    static const char *kDenseFailed = "lantern_gpu: HIP failure on the dense route of a per-query filtered call";
    const size_t nqd = plan.order.size(), groups = plan.groups(), total = plan.seg.back(), kk = k + skip, row = (size_t)ix->chunks * 16;
    auto         up = [](size_t x, size_t a) { return (x + a - 1) / a * a; };
    // lantern_gpu_set_filter_dense_each_batched: the run's batches (not taken -- f16 / i8 rows, popcount metrics: the per-step run)
    EachDenseBatches batches;
    if(ix->filter_dense_each_batched && plan_each_dense_batches(plan, 0, batches) != nullptr) return set_err(ix, kDenseFailed), false;
    const bool   batched = batches.why == kEachBatchTaken;
    const size_t n_tiles = batched ? batches.tiles() : 0, n_sel = batched ? batches.queries() : 0;
    // host tables, one copy: orig[nqd] | allowed[nqd] | seg[groups + 1] | lists[groups] (8-byte aligned) | batched: the tile table (32
    // bytes per tile) | the selection table (16 per step and query)
    const size_t t_orig = 0, t_allowed = nqd * 4, t_seg = 2 * nqd * 4, t_lists = up(t_seg + (groups + 1) * 4, 8), t_tiles = up(t_lists + groups * 8, 16);
    const size_t t_sel = t_tiles + n_tiles * sizeof(SegTile), t_bytes = t_sel + n_sel * sizeof(SegQuery);
    std::vector<uint64_t> tbl(t_bytes / 8);
    char *const           ht = (char *)tbl.data();
    uint32_t *const       h_orig = (uint32_t *)(ht + t_orig), *h_allowed = (uint32_t *)(ht + t_allowed);
    const uint32_t      **h_lists = (const uint32_t **)(ht + t_lists);
    std::copy(plan.order.begin(), plan.order.end(), h_orig);
    std::copy(plan.seg.begin(), plan.seg.end(), (uint32_t *)(ht + t_seg));
    if(batched) each_dense_seg_tables(plan, batches, (SegTile *)(ht + t_tiles), (SegQuery *)(ht + t_sel));
    for(size_t g = 0; g < groups; ++g) {
        const Filter *f = filters[ plan.order[ plan.qoff[ g ] ] ];
        h_lists[ g ] = f->d_slots;
        for(uint32_t j = plan.qoff[ g ]; j < plan.qoff[ g + 1 ]; ++j) h_allowed[ j ] = (uint32_t)f->count;
    }
    // the device block: tables | L | gathered queries | slots | dists
    const size_t b_list = up(t_bytes, 16), b_q = up(b_list + total * 4, 16), b_slots = b_q + nqd * row, b_dists = b_slots + nqd * kk * 4;
    char *const  blk = (char *)scratch(ix, kScratchDenseAnswers, b_dists + nqd * kk * 4);
    if(!blk) return false;
    uint32_t *const d_orig = (uint32_t *)(blk + t_orig), *d_allowed = (uint32_t *)(blk + t_allowed), *d_seg = (uint32_t *)(blk + t_seg);
    uint32_t *const d_list = (uint32_t *)(blk + b_list), *d_slots = (uint32_t *)(blk + b_slots);
    float *const    d_dists = (float *)(blk + b_dists);
    uint4 *const    d_gq = (uint4 *)(blk + b_q);
    if(!order_after_inserts(ix, stream)) return false;
    bool ok = hipMemcpyAsync(blk, ht, t_bytes, hipMemcpyHostToDevice, stream) == hipSuccess;
    if(ok) {
        const size_t blocks = std::min<size_t>((total + 255) / 256, 16384);
        hipLaunchKernelGGL(k_concat_slot_lists, dim3((uint32_t)blocks), dim3(256), 0, stream, (const uint32_t *const *)(blk + t_lists), (const uint32_t *)d_seg,
                           (uint32_t)groups, d_list);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && launch_gather_rows(d_q, ix->chunks, d_orig, (uint32_t)nqd, d_gq, stream) == hipSuccess;
    const EachDenseAnswers answers = [ & ](const uint32_t *d_flags) {
        const size_t blocks = std::min<size_t>((nqd * k + 255) / 256, 16384);
        hipLaunchKernelGGL(k_dense_each_answers, dim3((uint32_t)blocks), dim3(256), 0, stream, (const uint32_t *)d_slots, (const float *)d_dists, d_flags,
                           (const uint32_t *)d_orig, (const uint32_t *)d_allowed, (uint32_t)nqd, (uint32_t)kk, (uint32_t)k, (uint32_t)skip,
                           (const uint64_t *)ix->d_labels, (uint32_t)ix->n, out.labels, out.dists, out.slots, out.counts, out.D, out.E,
                           (unsigned long long *)(ix->d_totals + kTotSearch));
        return hipGetLastError() == hipSuccess;
    };
    std::vector<uint32_t> refused_at;
    EachDenseRun run;
    if(batched) {
        run.batches = &batches;
        run.d_tiles = (const SegTile *)(blk + t_tiles);
        run.d_queries = (const SegQuery *)(blk + t_sel);
    }
    ok = ok && filtered_each_dense_device(plan, ix->d_vec, d_list, d_gq, d_slots, d_dists, stream, answers, refused_at, &run);
    if(!ok) {
        (void)hipStreamSynchronize(stream);  // (nothing queued may still read the host tables or the block)
        return set_err(ix, kDenseFailed), false;
    }
    refused.clear();
    for(uint32_t at : refused_at) refused.push_back(plan.order[ at ]);
    ix->c_filter_dense[ 0 ] += 1;
    ix->c_filter_dense[ 1 ] += nqd;
    ix->c_filter_dense[ 2 ] += nqd - refused.size();
    ix->c_filter_dense[ 3 ] += refused.size();
    const uint32_t shape[ 6 ] = { (uint32_t)groups, (uint32_t)nqd, (uint32_t)(nqd - refused.size()), (uint32_t)refused.size(), (uint32_t)total, (uint32_t)plan.steps.size() };
    std::copy(std::begin(shape), std::end(shape), ix->last_each_dense);
    std::copy(std::begin(run.launches), std::end(run.launches), ix->last_each_dense_launches);
    return true;
}

}  // namespace lgpu
