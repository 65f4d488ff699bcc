// filter.hip -- filtered k-NN search: building an allow-set over an index's slots, choosing between the filtered walk and the exact
// pass over the allowed rows, and the C entry points (include/lantern_gpu.h "Filtered search"; semantics: DESIGN.md 4.9).
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <iterator>
#include <mutex>
#include <string>
#include <vector>

#include "abi_guard.hpp"
#include "dense.hpp"
#include "filter.hpp"
#include "filter_ops.hpp"
#include "host_trip.hpp"
#include "index.hpp"

namespace lgpu {

// ---- building the bitmap on the device ----------------------------------------------------------------------------------
// one thread per 32 slots: the word of slots [32 w, 32 w + 32).  A slot is allowed iff its label is among the sorted labels
// (binary search), and -- SKIP_DELETED -- its label is not 0 (INVALID_ELEMENT_LABEL, hnsw.h:40).
__global__ void k_filter_from_labels(const uint64_t *slot_labels, size_t n, const uint64_t *sorted, size_t m, int skip_deleted, uint32_t *bits,
                                     size_t words)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(w >= words) return;
    uint32_t word = 0;
    for(uint32_t b = 0; b < 32; ++b) {
        const size_t slot = w * 32 + b;
        if(slot >= n) break;
        const uint64_t l = slot_labels[ slot ];
        if(skip_deleted && l == 0) continue;
        if(label_in_sorted(sorted, m, l)) word |= 1u << b;
    }
    bits[ w ] = word;
}
// a caller's slot bitmap, uploaded: bits at or past n cleared, SKIP_DELETED applied
__global__ void k_filter_mask(const uint64_t *slot_labels, size_t n, int skip_deleted, uint32_t *bits, size_t words)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(w >= words) return;
    uint32_t word = bits[ w ];
    for(uint32_t b = 0; b < 32; ++b) {
        const size_t slot = w * 32 + b;
        if(slot >= n || (skip_deleted && slot_labels[ slot ] == 0)) word &= ~(1u << b);
    }
    bits[ w ] = word;
}

static const char *kFilteredBatchFailed = "lantern_gpu: HIP failure during filtered batched search";
static const char *kFilterFlags = "lantern_gpu: unknown filter flags (only LANTERN_GPU_FILTER_SKIP_DELETED is defined)";

static void filter_release(Filter *f)
{
    if(!f) return;
    (void)hipSetDevice(f->device);
    if(f->d_bits) (void)hipFree(f->d_bits);
    if(f->d_slots) (void)hipFree(f->d_slots);
    f->magic = 0;
    delete f;
}

// the bitmap is in f->d_bits: its popcount and the allowed slots in ascending order (the exact path's work list), by the list pass of
// filter_ops.hip on the index stream -- only the count crosses to the host, to size the list.  The pass's scratch is the block of one
// call on the index stream (index.hpp kScratchCallIn): the caller holds ix->mu, and the stream has been waited for on return.
static bool filter_finish(Index *ix, Filter *f)
{
    static const char *kFailed = "lantern_gpu: HIP failure building a filter";
    FilterListPlan plan;
    if(filter_list_plan(f->words, plan) != hipSuccess) return set_err(ix, kFailed), false;
    void *const blk = scratch(ix, kScratchCallIn, plan.bytes);
    if(!blk) return false;
    if(filter_list_count(f->d_bits, f->words, plan, blk, &f->count, ix->stream) != hipSuccess) return set_err(ix, kFailed), false;
    if(f->count) {
        if(hipMalloc((void **)&f->d_slots, f->count * 4) != hipSuccess) return set_err(ix, "lantern_gpu: out of device memory (filter slot list)"), false;
        if(filter_list_write(f->d_bits, f->words, plan, blk, f->d_slots, f->count, ix->stream) != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess)
            return set_err(ix, kFailed), false;
    }
    return true;
}

static Filter *filter_new(Index *ix)
{
    Filter *f = new Filter();
    f->ix = ix;
    f->device = ix->device;
    f->n = ix->n;
    f->epoch = ix->epoch;
    f->words = ((std::max<size_t>(ix->n, 1) + 31) / 32 + 3) / 4 * 4;
    if(hipMalloc((void **)&f->d_bits, f->words * 4) != hipSuccess || hipMemset(f->d_bits, 0, f->words * 4) != hipSuccess) {
        set_err(ix, "lantern_gpu: out of device memory (filter bitmap)");
        filter_release(f);
        return nullptr;
    }
    return f;
}

// a caller's labels sorted on the device (rocPRIM radix sort, as grouping.hip) for the kernels that binary-search them.  The sort is
// queued on `stream`; whoever holds one waits for the stream before it goes out of scope.
struct SortedLabels
{
    uint64_t *d_in = nullptr, *d_sorted = nullptr;
    void     *temp = nullptr;
    bool sort(const uint64_t *labels, size_t m, hipStream_t stream)
    {
        size_t temp_bytes = 0;
        return hipMalloc((void **)&d_in, m * 8) == hipSuccess && hipMalloc((void **)&d_sorted, m * 8) == hipSuccess &&
               hipMemcpy(d_in, labels, m * 8, hipMemcpyHostToDevice) == hipSuccess &&
               rocprim::radix_sort_keys(nullptr, temp_bytes, (const uint64_t *)d_in, d_sorted, m, 0u, 64u, stream) == hipSuccess &&
               hipMalloc(&temp, std::max<size_t>(temp_bytes, 16)) == hipSuccess &&
               rocprim::radix_sort_keys(temp, temp_bytes, (const uint64_t *)d_in, d_sorted, m, 0u, 64u, stream) == hipSuccess;
    }
    ~SortedLabels()
    {
        if(d_in) (void)hipFree(d_in);
        if(d_sorted) (void)hipFree(d_sorted);
        if(temp) (void)hipFree(temp);
    }
};

static Filter *filter_from_labels_locked(Index *ix, const uint64_t *labels, size_t m, int skip_deleted)
{
    Filter *f = filter_new(ix);
    if(!f) return nullptr;
    bool ok = true;
    if(m > 0 && ix->n > 0) {
        // the labels sorted on the device, then one thread per word binary-searches them
        SortedLabels s;
        ok = s.sort(labels, m, ix->stream);
        if(ok) {
            const int blocks = (int)((f->words + 255) / 256);
            hipLaunchKernelGGL(k_filter_from_labels, dim3(blocks), dim3(256), 0, ix->stream, (const uint64_t *)ix->d_labels, ix->n,
                               (const uint64_t *)s.d_sorted, m, skip_deleted, f->d_bits, f->words);
            ok = hipGetLastError() == hipSuccess;
        }
        ok = (hipStreamSynchronize(ix->stream) == hipSuccess) && ok;
        if(!ok) set_err(ix, "lantern_gpu: HIP failure building a filter from labels");
    }
    if(!ok || !filter_finish(ix, f)) {
        filter_release(f);
        return nullptr;
    }
    return f;
}

// `old` brought to the index's present size (lantern_gpu_filter_extend): the caller has checked that it is this index's, of this epoch
// and no larger than the index.  A fresh handle; `old` is only read.
static Filter *filter_extend_locked(Index *ix, const Filter *old, const uint64_t *labels, size_t m, int all_new, int skip_deleted)
{
    Filter *f = filter_new(ix);
    if(!f) return nullptr;
    SortedLabels s;
    bool         ok = !(m > 0 && ix->n > old->n) || s.sort(labels, m, ix->stream);
    ok = ok && launch_filter_extend((const uint64_t *)ix->d_labels, old->n, ix->n, (const uint64_t *)s.d_sorted, s.d_sorted ? m : 0, all_new, skip_deleted,
                                    old->d_bits, old->words, f->d_bits, f->words, ix->stream) == hipSuccess;
    ok = (hipStreamSynchronize(ix->stream) == hipSuccess) && ok;
    if(!ok) set_err(ix, "lantern_gpu: HIP failure extending a filter");
    if(!ok || !filter_finish(ix, f)) {
        filter_release(f);
        return nullptr;
    }
    return f;
}

// a op b (lantern_gpu_filter_combine): the caller has checked both against the index as it stands.  A fresh handle.
static Filter *filter_combine_locked(Index *ix, const Filter *a, const Filter *b, int op)
{
    Filter *f = filter_new(ix);
    if(!f) return nullptr;
    const bool ok = launch_filter_combine(a->d_bits, b->d_bits, op, ix->n, f->d_bits, f->words, ix->stream) == hipSuccess &&
                    hipStreamSynchronize(ix->stream) == hipSuccess;
    if(!ok) set_err(ix, "lantern_gpu: HIP failure combining two filters");
    if(!ok || !filter_finish(ix, f)) {
        filter_release(f);
        return nullptr;
    }
    return f;
}

static Filter *filter_from_bitmap_locked(Index *ix, const uint32_t *words, size_t n_words, int skip_deleted)
{
    Filter *f = filter_new(ix);
    if(!f) return nullptr;
    bool ok = n_words == 0 || hipMemcpy(f->d_bits, words, n_words * 4, hipMemcpyHostToDevice) == hipSuccess;
    if(ok) {
        const int blocks = (int)((f->words + 255) / 256);
        hipLaunchKernelGGL(k_filter_mask, dim3(blocks), dim3(256), 0, ix->stream, (const uint64_t *)ix->d_labels, ix->n, skip_deleted, f->d_bits,
                           f->words);
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ix->stream) == hipSuccess;
    }
    if(!ok) set_err(ix, "lantern_gpu: HIP failure building a filter from a slot bitmap");
    if(!ok || !filter_finish(ix, f)) {
        filter_release(f);
        return nullptr;
    }
    return f;
}

// ---- the search ------------------------------------------------------------------------------------------------------------
constexpr size_t kFilteredLds = 160 * 1024;  // a workgroup's LDS
constexpr size_t kFilteredLdsTarget = 64 * 1024;  // what the visited set may grow the walk's LDS to (two workgroups per CU)
constexpr int    kFilteredWaves = 4;
constexpr size_t kFilterSeedsMax = 4096;  // lantern_gpu_set_filter_seeds refuses more

// What the shape and the path of a filtered launch are computed from: the index's fields and its filter policy, nothing else -- so
// that the plan is a pure function (lantern_gpu_plan_filtered_params) of what the launch really reads.
struct FilterPlanIn
{
    uint32_t chunks, M0;
    size_t   n, ef_default;
    int      path;  // lantern_gpu_set_filter_policy
    size_t   cand_cap;
    double   exact_factor;
    size_t   seeds;  // lantern_gpu_set_filter_seeds (changes no shape: a round of seeds is at most M0 rows, a hop's)
    // a compact pq index served by ADC (search_filtered_pq_kernel.hip): 16-byte chunks of a code row, 1..8; `chunks` is then the raw query
    // row's.  0: rows of `chunks` chunks, stored -- or decoded on the fly, whose shape is the expanded index's
    uint32_t adc_code_chunks = 0;
};
// a compact pq index's row routine, by plan_search's own condition (search_plan.cpp): decoded on the fly, else ADC
static bool compact_adc(const Index *ix) { return ix->pq_compact && (search_env().pq_adc || ix->pqd_inv == 0); }
static FilterPlanIn filter_plan_in(const Index *ix)
{
    FilterPlanIn p{ ix->chunks, ix->M0, ix->n, ix->ef, ix->filter_path, ix->filter_cand_cap, ix->filter_exact_factor, ix->filter_seeds };
    if(compact_adc(ix)) p.adc_code_chunks = ix->pq_S16 / 16;
    return p;
}
// What lies in front of the lists in a launch's LDS, in chunks: the query row -- ADC: the table first (code_chunks x 16 KiB:
// RowAcc<M_*_ADC> reads it from the first LDS bytes), the raw query row behind it
static uint32_t plan_lds_chunks(const FilterPlanIn &p) { return p.adc_code_chunks ? filtered_adc_lds_chunks(p.adc_code_chunks, p.chunks) : p.chunks; }
static size_t   plan_table_bytes(const FilterPlanIn &p) { return (size_t)filtered_adc_lds_chunks(p.adc_code_chunks, 0) * 16; }
// lanes per row: a code row has at most 8 chunks
static int plan_lanes(const FilterPlanIn &p) { return p.adc_code_chunks ? 8 : group_lanes_for(p.chunks); }

// exp, cand_cap, vis_slots / rows_per_round and the LDS bytes of one launch
struct FilteredShape
{
    uint32_t exp = 0, cand_cap = 0, vis_slots = 0, rows_per_round = 0;
    size_t   lds = 0;
};
static const char *kWalkOverBudget = "lantern_gpu: ef/k exceed the 160 KiB LDS budget of the filtered search kernel";
static const char *kExactOverBudget = "lantern_gpu: k + skip exceed the 160 KiB LDS budget of the exact filtered search kernel";
static const char *kJointOverBudget =
    "lantern_gpu: the queries fit the 160 KiB LDS budget of the filtered search kernel one by one, but the largest expansion and the largest "
    "candidate cap of the batch do not fit together: split the batch";

// the exact launch's carve for a list of kk keys
static void exact_carve(const FilterPlanIn &p, size_t kk, FilteredShape &s)
{
    s.exp = (uint32_t)kk;
    s.rows_per_round = (uint32_t)(2 * 64 * kFilteredWaves / plan_lanes(p));
    s.lds = filtered_exact_lds_bytes(plan_lds_chunks(p), s.exp, s.rows_per_round);
}
// the walk launch's carve for `exp` keys of top and `cap` of next: the visited set takes what is left of the LDS target -- beside an
// ADC table, which alone may exceed that target, what is left of the workgroup's LDS (at most 2048 slots either way)
static void walk_carve(const FilterPlanIn &p, size_t exp, size_t cap, FilteredShape &s)
{
    s.exp = (uint32_t)exp;
    s.cand_cap = (uint32_t)cap;
    const uint32_t chunks = plan_lds_chunks(p);
    const size_t   target = p.adc_code_chunks ? kFilteredLds : kFilteredLdsTarget;
    uint32_t vis_slots = 2048;
    while(vis_slots && filtered_walk_lds_bytes(chunks, s.exp, s.cand_cap, p.M0, vis_slots) > target)
        vis_slots = vis_slots > 256 ? vis_slots - 256 : 0;
    if(vis_slots && vis_slots < 4 * p.M0) vis_slots = 0;
    s.vis_slots = vis_slots;
    s.lds = filtered_walk_lds_bytes(chunks, s.exp, s.cand_cap, p.M0, vis_slots);
}
// The part of a filtered launch's shape that depends on (k, ef, skip, index) only -- not on the filter.  NULL, or the refusal.
static const char *filtered_shape_of(const FilterPlanIn &p, bool exact, size_t k, size_t skip, size_t exp, FilteredShape &s)
{
    if(exact) {
        exact_carve(p, k + skip, s);
        if(s.lds > kFilteredLds) return kExactOverBudget;
    } else {
        const size_t base = filtered_walk_lds_bytes(plan_lds_chunks(p), (uint32_t)exp, 0, p.M0, 0);
        if(base + exp * 16 > kFilteredLds) return kWalkOverBudget;
        size_t cap = p.cand_cap ? std::max(p.cand_cap, exp) : std::max<size_t>(4 * exp, 256);
        cap = std::min(cap, (kFilteredLds - base) / 16);
        if(p.cand_cap && cap < std::max(p.cand_cap, exp)) return "lantern_gpu: the candidate cap exceeds the 160 KiB LDS budget of the filtered search kernel";
        walk_carve(p, exp, cap, s);
    }
    return nullptr;
}
static void shape_into(const FilteredShape &s, FilteredArgs &a, size_t &lds)
{
    a.exp = s.exp, a.cand_cap = s.cand_cap, a.rows_per_round = s.rows_per_round, a.frame.vis_slots = s.vis_slots;
    lds = s.lds;
}
// ... into the launch's arguments.  false -> ix->err.
static bool filtered_shape(Index *ix, bool exact, size_t k, size_t skip, size_t exp, FilteredArgs &a, size_t &lds)
{
    FilteredShape s;
    if(const char *why = filtered_shape_of(filter_plan_in(ix), exact, k, skip, exp, s)) return set_err(ix, why), false;
    shape_into(s, a, lds);
    return true;
}

static const char *kNotAFilter = "lantern_gpu: not a filter handle (stale, freed or foreign pointer)";

// Why `f` cannot serve a search of `ix` as it stands now; empty: it can.
static std::string filter_mismatch(const Index *ix, const Filter *f)
{
    if(f->ix != ix)
        return "lantern_gpu: the filter belongs to another index (built over " + std::to_string(f->n) + " rows; this index holds " + std::to_string(ix->n) + ")";
    if(f->epoch != ix->epoch)  // (before the size: a delete / compact / add sequence may bring the size back)
        return "lantern_gpu: stale filter: the index was compacted since the filter was built (its slots name other rows now; build the filter again)";
    if(f->n != ix->n)
        return "lantern_gpu: stale filter: built when the index held " + std::to_string(f->n) + " rows, it now holds " + std::to_string(ix->n) +
               " (build the filter again)";
    return {};
}
// (checked after the filters)  A compact pq index is served once lantern_gpu_set_filter_compact has said so.
static bool filtered_index_ok(Index *ix)
{
    const bool refused = ix->pq_compact && !ix->filter_compact;
    if(refused) set_err(ix, "lantern_gpu: filtered search does not run on a compact pq index: expand it first (lantern_gpu_pq_expand)");
    return !refused;
}

// the path of a query under `f`: forced, or the rule of DESIGN.md 4.9 -- a walk under selectivity s evaluates about D / s rows, the
// exact pass `allowed`
static bool count_takes_exact(const FilterPlanIn &p, size_t count, size_t ef_sel)
{
    if(p.path) return p.path == 2;
    return (double)count * (double)count <= p.exact_factor * (double)ef_sel * (double)p.n;
}
static bool filter_takes_exact(const Index *ix, const Filter *f, size_t ef_sel) { return count_takes_exact(filter_plan_in(ix), f->count, ef_sel); }

// the kernel arguments that depend neither on the filter nor on the path
static FilteredArgs filtered_args(const Index *ix, const uint4 *d_q, size_t k, size_t skip, const SearchOut &out)
{
    FilteredArgs a{};
    a.view = ix->view();
    a.frame.queries = d_q;
    a.k = (uint32_t)k;
    a.skip = (uint32_t)skip;
    a.frame.labels = ix->d_labels;
    a.frame.out_labels = out.labels, a.frame.out_dists = out.dists, a.frame.out_slots = out.slots;
    a.frame.out_counts = out.counts, a.frame.out_D = out.D, a.frame.out_E = out.E;
    a.frame.totals = ix->d_totals + kTotSearch;
    if(ix->pq_compact) {  // the code rows, with what their row routine reads (as search_plan.cpp search_launch fills SearchArgs)
        a.view.vec = (const uint4 *)ix->d_codes16;
        if(compact_adc(ix)) {
            a.view.chunks = ix->pq_S16 / 16;
            a.adc_centers = ix->d_centers;
            a.adc_S = ix->pq_S, a.adc_C = ix->pq_C, a.adc_subdim = ix->pq_subdim, a.adc_qchunks = ix->chunks;
        } else {
            a.view.pq_centers = (const uint4 *)ix->d_centers;
            a.view.pq_cps = ix->pq_subdim / 4;
            a.view.pq_C = ix->pq_C;
            a.view.pq_inv = ix->pqd_inv;
            a.view.pq_row_bytes = ix->pq_S16;
        }
    }
    return a;
}

// the per-query form's table of one launch: host bytes that go into the scratch of the launch's slot, and where in them the launch's
// descriptors and selection list lie
constexpr size_t kNoTable = ~(size_t)0;
struct EachTable
{
    const char *host;
    size_t      bytes, descs_at, select_at;
    size_t      params_at = kNoTable;  // the per-query-parameter form: where the launch's rows {k, expansion, skip, C} lie
};

// workgroups of a filtered launch that a CU holds
static int filtered_per_cu(size_t lds) { return (int)std::max<size_t>(1, std::min<size_t>(4, kFilteredLds / std::max<size_t>(lds, 1))); }

// the empty answer in every row of a call, kw wide, with no launch
static bool empty_answers(Index *ix, const SearchOut &out, size_t nq, size_t kw, hipStream_t stream)
{
    if(out.labels && kw && hipMemsetAsync(out.labels, 0, nq * kw * 8, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    if(out.dists && kw && hipMemsetD32Async((hipDeviceptr_t)out.dists, 0x7F800000, nq * kw, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    if(out.slots && kw && hipMemsetAsync(out.slots, 0xFF, nq * kw * 4, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    if(out.counts && hipMemsetAsync(out.counts, 0, nq * 4, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    if(out.D && hipMemsetAsync(out.D, 0, nq * 8, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    if(out.E && hipMemsetAsync(out.E, 0, nq * 8, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    return true;
}

// ONE launch of either kernel over a.frame.nq queries, `a` shaped by filtered_shape: the grid, the launch slot (which orders the launch
// after inserts and holds the walk's visited bitmaps), the per-query table if there is one, the ticket, the launch and its count.
// Returns the grid; < 0 -> ix->err.
static int filtered_launch(Index *ix, bool exact, FilteredArgs &a, size_t lds, hipStream_t stream, const EachTable *tbl = nullptr)
{
    const int per_cu = filtered_per_cu(lds);
    const int grid = search_grid(ix, a.frame.nq, kFilteredWaves, kFilteredWaves * per_cu);
    const int slot = acquire_search_slot(ix, stream, (size_t)grid);
    if(slot < 0) return -1;
    if(tbl) {
        char *const d_tbl = (char *)scratch(ix, launch_table_scratch(slot), tbl->bytes);
        if(!d_tbl) return -1;
        if(hipMemcpyAsync(d_tbl, tbl->host, tbl->bytes, hipMemcpyHostToDevice, stream) != hipSuccess) {
            set_err(ix, "lantern_gpu: HIP failure (per-query filter table)");
            return -1;
        }
        a.descs = (const FilterDesc *)(d_tbl + tbl->descs_at);
        a.frame.qlist = (const uint32_t *)(d_tbl + tbl->select_at);
        if(tbl->params_at != kNoTable) a.qparams = (const uint4 *)(d_tbl + tbl->params_at);
    }
    a.frame.bitmaps = ix->slot_bitmaps[ slot ];
    a.frame.bm_words = (uint32_t)ix->slot_words[ slot ];
    a.frame.undo_cap = vis_undo_cap();
    a.frame.ticket = next_ticket(ix, a.frame.nq, grid, stream);
    hipError_t e;
    if(ix->pq_compact) {
        const int metric = ix->metric + (a.adc_centers ? M_ADC : M_PQD);
        e = exact ? launch_search_exact_allowed_pq(metric, a, kFilteredWaves, grid, stream) : launch_search_filtered_pq(metric, a, kFilteredWaves, grid, stream);
    } else {
        e = exact ? launch_search_exact_allowed(ix->mcode, a, kFilteredWaves, grid, stream) : launch_search_filtered(ix->mcode, a, kFilteredWaves, grid, stream);
    }
    if(e != hipSuccess) {
        set_err(ix, std::string("lantern_gpu: HIP error launching the filtered search: ") + hipGetErrorString(e));
        return -1;
    }
    if(!release_search_slot(ix, slot, stream)) return -1;
    (exact ? ix->c_filter_exact : ix->c_filter_walk) += 1;
    return grid;
}

// ---- the exact path's dense route (DESIGN.md 4.9 "Dense exact path") ---------------------------------------------------------------
// k_dense_answers: the exact k-NN's re-ranked rows -- kk = k + skip (slot, distance) entries per query, ascending by (distance, slot) --
// into a filtered call's outputs, as k_search_exact_allowed closes a query (frame_answer_rows, frame_close): rows [skip, skip + k) as
// label, distance, slot; tails label 0, +inf, EMPTY; count, D = allowed, E = 0; D added to totals[0].  One thread per answer cell.
// Queries without a flag are left alone: the per-query launch behind this one answers them.  Every output pointer may be NULL.
__global__ void __launch_bounds__(256) k_dense_answers(const uint32_t *slots, const float *dists, const uint32_t *flags, uint32_t nq, uint32_t kk, uint32_t k,
                                                       uint32_t skip, uint32_t allowed, const uint64_t *labels, uint32_t n, uint64_t *out_labels, float *out_dists,
                                                       uint32_t *out_slots, uint32_t *out_counts, uint64_t *out_D, uint64_t *out_E, unsigned long long *totals)
{
    const uint32_t have = allowed < kk ? allowed : kk, got = have <= skip ? 0u : (have - skip < k ? have - skip : k);
    const size_t   cells = (size_t)nq * k;
    for(size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (size_t)gridDim.x * blockDim.x) {
        const uint32_t q = (uint32_t)(c / k), i = (uint32_t)(c % k);
        if(!flags[ q ]) continue;
        if(i < got) {
            const size_t   at = (size_t)q * kk + skip + i;
            const uint32_t slot = slots[ at ];
            if(out_labels) out_labels[ c ] = slot < n ? labels[ slot ] : 0;  // (every slot of the first `have` entries is a row's)
            if(out_dists) out_dists[ c ] = dists[ at ];
            if(out_slots) out_slots[ c ] = slot;
        } else {
            if(out_labels) out_labels[ c ] = 0;  // INVALID_ELEMENT_LABEL (hnsw.h:40)
            if(out_dists) out_dists[ c ] = __builtin_inff();
            if(out_slots) out_slots[ c ] = EMPTY;
        }
        if(i == 0) {
            if(out_counts) out_counts[ q ] = got;
            if(out_D) out_D[ q ] = allowed;
            if(out_E) out_E[ q ] = 0;
            if(totals) atomicAdd(&totals[ 0 ], (unsigned long long)allowed);
        }
    }
}

// One single-filter call on the dense route, planned by `plan` (taken).  `a`, `lds`: the exact launch's arguments and carve, which the
// recomputed queries run with.  Waits for the stream (the certificate's flags cross to the host).
static bool filtered_dense_locked(Index *ix, const Filter *f, const FilteredDensePlan &plan, int native, const uint4 *d_q, size_t nq, size_t k, size_t skip,
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
        const size_t      nr = refused.size(), off_desc = (nr * 4 + 7) & ~(size_t)7;
        std::vector<char> tbl(off_desc + nq * sizeof(FilterDesc));
        std::copy(refused.begin(), refused.end(), (uint32_t *)tbl.data());
        FilterDesc *const hd = (FilterDesc *)(tbl.data() + off_desc);
        for(size_t i = 0; i < nq; ++i) hd[ i ] = FilterDesc{ f->d_bits, f->d_slots, (uint32_t)f->count, 0u };
        a.frame.nq = (uint32_t)nr;
        const EachTable t{ tbl.data(), tbl.size(), off_desc, 0 };
        if(filtered_launch(ix, true, a, lds, stream, &t) < 0) return false;  // (pageable staging: the copy completes before this returns)
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

// The caller holds ix->mu and has flushed.  false -> ix->err.  batch_call: one of the two single-filter batch entry points, which alone
// may take the exact path's dense route (lantern_gpu_set_filter_dense); a cursor's search never does.
static bool filtered_search_locked(Index *ix, const Filter *f, const uint4 *d_q, size_t nq, size_t k, size_t ef, size_t skip, const SearchOut &out,
                                   hipStream_t stream, bool batch_call = false)
{
    const std::string why = filter_mismatch(ix, f);
    if(!why.empty()) return set_err(ix, why), false;
    if(!filtered_index_ok(ix)) return false;
    if(nq == 0 || k == 0) return true;
    const size_t ef_sel = ef ? ef : ix->ef;
    const size_t exp = std::max(ef_sel, k + skip);
    std::fill(std::begin(ix->last_seeds), std::end(ix->last_seeds), 0u);
    if(f->count == 0 || ix->n == 0) {  // nothing allowed: the empty answer, no launch
        std::fill(std::begin(ix->last_filtered), std::end(ix->last_filtered), 0u);
        return empty_answers(ix, out, nq, k, stream);
    }
    const bool   exact = filter_takes_exact(ix, f, ef_sel);
    FilteredArgs a = filtered_args(ix, d_q, k, skip, out);
    a.frame.nq = (uint32_t)nq;
    a.allow_bits = f->d_bits;
    a.allow_slots = f->d_slots;
    a.allow_count = (uint32_t)f->count;
    size_t lds = 0;
    if(!filtered_shape(ix, exact, k, skip, exp, a, lds)) return false;
    if(batch_call && ix->filter_dense_min) {  // the exact path's second implementation: the same answers from the contraction
        const DenseEnv    env = dense_env();
        FilteredDensePlan dense;
        const char *const bad = plan_filtered_dense(ix->mcode, ix->chunks, (int64_t)f->count, (int64_t)nq, (int64_t)k, (int64_t)skip,
                                                    (int64_t)ix->filter_dense_min, exact, ix->pq_compact, env.native, env.fused, dense);
        if(!bad && dense.why == kDenseTaken) return filtered_dense_locked(ix, f, dense, env.native, d_q, nq, k, skip, out, a, lds, stream);
    }
    int grid;
    if(!exact && ix->filter_seeds) {
        // the seeded walk exists in the per-query form only: every query's descriptor is this filter, the selection list the identity
        const size_t      off_desc = (nq * 4 + 7) & ~(size_t)7;
        std::vector<char> tbl(off_desc + nq * sizeof(FilterDesc));
        uint32_t *const   sel = (uint32_t *)tbl.data();
        FilterDesc *const hd = (FilterDesc *)(tbl.data() + off_desc);
        for(size_t i = 0; i < nq; ++i) {
            sel[ i ] = (uint32_t)i;
            hd[ i ] = FilterDesc{ f->d_bits, f->d_slots, (uint32_t)f->count, 0u };
        }
        a.seeds = (uint32_t)ix->filter_seeds;
        const EachTable t{ tbl.data(), tbl.size(), off_desc, 0 };
        grid = filtered_launch(ix, false, a, lds, stream, &t);  // (pageable staging: the copy completes before this returns)
        ix->last_seeds[ 1 ] = (uint32_t)std::min(ix->filter_seeds, f->count);
        ix->last_seeds[ 2 ] = (uint32_t)nq;
    } else {
        grid = filtered_launch(ix, exact, a, lds, stream);
        if(!exact) ix->last_seeds[ 3 ] = (uint32_t)nq;
    }
    if(grid < 0) return false;
    const uint32_t shape[ 6 ] = { exact ? 2u : 1u, (uint32_t)grid, a.exp, a.cand_cap, a.frame.vis_slots, (uint32_t)lds };
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

// k_dense_each_answers: k_dense_answers for the segmented run -- dense query q (its re-ranked row: kk = k + skip entries) is the
// call's query orig[q] and stands behind a filter of allowed[q] rows: its cells go to the row of orig[q], D = allowed[q].  flags ==
// NULL: every query is certified; else flags[q] says so, and flags[nq] != 0 (a cosine row norm out of the certificate's range, in any
// segment) refuses them all.  The refused queries' rows are left alone: the per-query launch behind this one answers them.
__global__ void __launch_bounds__(256) k_dense_each_answers(const uint32_t *slots, const float *dists, const uint32_t *flags, const uint32_t *orig,
                                                            const uint32_t *allowed, uint32_t nq, uint32_t kk, uint32_t k, uint32_t skip, const uint64_t *labels,
                                                            uint32_t n, uint64_t *out_labels, float *out_dists, uint32_t *out_slots, uint32_t *out_counts,
                                                            uint64_t *out_D, uint64_t *out_E, unsigned long long *totals)
{
    if(flags && flags[ nq ]) return;
    const size_t cells = (size_t)nq * k;
    for(size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < cells; c += (size_t)gridDim.x * blockDim.x) {
        const uint32_t q = (uint32_t)(c / k), i = (uint32_t)(c % k);
        if(flags && !flags[ q ]) continue;
        const uint32_t al = allowed[ q ], have = al < kk ? al : kk, got = have <= skip ? 0u : (have - skip < k ? have - skip : k);
        const uint32_t oq = orig[ q ];
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

// The dense groups of one per-query-filter call, planned by `plan` (taken): L, the tables and the gathered queries into the dense
// scratch block, the segmented run with the answer kernel queued in front of its wait.  refused: the call's queries (original
// indices) the certificate refused, which the call's exact launch answers.  Waits for the stream, once.
static bool filtered_each_dense_locked(Index *ix, const Filter *const *filters, const EachDensePlan &plan, const uint4 *d_q, size_t k, size_t skip,
                                       const SearchOut &out, hipStream_t stream, std::vector<uint32_t> &refused)
{
    static const char *kDenseFailed = "lantern_gpu: HIP failure on the dense route of a per-query filtered call";
    const size_t nqd = plan.order.size(), groups = plan.groups(), total = plan.seg.back(), kk = k + skip, row = (size_t)ix->chunks * 16;
    auto         up = [](size_t x, size_t a) { return (x + a - 1) / a * a; };
    // host tables, one copy: orig[nqd] | allowed[nqd] | seg[groups + 1] | lists[groups] (8-byte aligned)
    const size_t          t_orig = 0, t_allowed = nqd * 4, t_seg = 2 * nqd * 4, t_lists = up(t_seg + (groups + 1) * 4, 8), t_bytes = t_lists + groups * 8;
    std::vector<uint64_t> tbl(t_bytes / 8);
    char *const           ht = (char *)tbl.data();
    uint32_t *const       h_orig = (uint32_t *)(ht + t_orig), *h_allowed = (uint32_t *)(ht + t_allowed);
    const uint32_t      **h_lists = (const uint32_t **)(ht + t_lists);
    std::copy(plan.order.begin(), plan.order.end(), h_orig);
    std::copy(plan.seg.begin(), plan.seg.end(), (uint32_t *)(ht + t_seg));
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
    ok = ok && filtered_each_dense_device(plan, ix->d_vec, d_list, d_gq, d_slots, d_dists, stream, answers, refused_at);
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
    return true;
}

// ---- the per-query form: filters[i] is query i's filter ------------------------------------------------------------------------
// bytes of the host block filtered_each_locked stages its selection lists and descriptor table in
// (`params`: with the per-query-parameter form's rows)
static size_t each_table_bytes(size_t nq, bool params = false) { return nq * (sizeof(FilterDesc) + 4) + 16 + (params ? nq * 16 + 16 : 0); }

// Every entry of filters[] is NULL or a live filter of this index at its present size; else ix->err names the first offender.
static bool each_filters_ok(Index *ix, const Filter *const *filters, size_t nq)
{
    for(size_t i = 0; i < nq; ++i) {
        const Filter *f = filters[ i ];
        if(!f) continue;
        const std::string why = f->magic != kFilterMagic ? std::string(kNotAFilter) : filter_mismatch(ix, f);
        if(why.empty()) continue;
        set_err(ix, why + " (filters[" + std::to_string(i) + "])");
        return false;
    }
    return filtered_index_ok(ix);
}

// the queries of a per-query call by what becomes of them (lantern_gpu_last_filtered_each [0..4))
struct EachCounts { uint32_t walk, exact, unfiltered, empty; };

// The launches of a per-query call whose queries are split already: `walk` and `exact` are the two selection lists (what rides in a
// launch without a path behind the queries of its list), aw / ae the launches' shaped arguments.  `rows`: NULL, or the call's
// parameter table [nq][4] (the per-query-parameter form).  `h_tbl`: a page-locked block of each_table_bytes(nq, rows) or NULL, as
// filtered_each_locked's.  false -> ix->err.
static bool each_launches(Index *ix, const Filter *const *filters, size_t nq, const std::vector<uint32_t> &walk, const std::vector<uint32_t> &exact,
                          FilteredArgs &aw, size_t lds_w, FilteredArgs &ae, size_t lds_e, const uint32_t *rows, const EachCounts &c, hipStream_t stream,
                          char *h_tbl)
{
    std::vector<const Filter *> distinct;
    for(size_t i = 0; i < nq; ++i)
        if(filters[ i ]) distinct.push_back(filters[ i ]);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());

    // the host block: walk selection list | parameter rows (by query; the per-query-parameter form) | descriptor table (by query) |
    // exact selection list -- each launch copies its list and the tables in one piece into the scratch of its own launch slot
    const size_t off_par = rows ? ((size_t)walk.size() * 4 + 15) & ~(size_t)15 : ((size_t)walk.size() * 4 + 7) & ~(size_t)7;
    const size_t off_desc = off_par + (rows ? nq * 16 : 0), off_sel_e = off_desc + nq * sizeof(FilterDesc);
    const size_t tbl_bytes = off_sel_e + exact.size() * 4;
    std::vector<char> pageable;
    if(!h_tbl) { pageable.resize(tbl_bytes); h_tbl = pageable.data(); }
    if(!walk.empty()) std::memcpy(h_tbl, walk.data(), walk.size() * 4);
    if(rows) std::memcpy(h_tbl + off_par, rows, nq * 16);
    if(!exact.empty()) std::memcpy(h_tbl + off_sel_e, exact.data(), exact.size() * 4);
    FilterDesc *const hd = (FilterDesc *)(h_tbl + off_desc);
    for(size_t i = 0; i < nq; ++i) {
        const Filter *f = filters[ i ];
        hd[ i ] = f ? FilterDesc{ f->d_bits, f->d_slots, (uint32_t)f->count, 0u } : FilterDesc{ nullptr, nullptr, 0u, ix->n ? 1u : 0u };
    }

    uint32_t launches = 0;
    for(int pass = 0; pass < 2; ++pass) {
        const bool ex = pass == 1;
        if((ex ? exact : walk).empty()) continue;
        FilteredArgs &a = ex ? ae : aw;
        a.frame.nq = (uint32_t)(ex ? exact : walk).size();
        const EachTable t = ex ? EachTable{ h_tbl + off_par, tbl_bytes - off_par, off_desc - off_par, off_sel_e - off_par, rows ? 0 : kNoTable }
                               : EachTable{ h_tbl, off_sel_e, off_desc, 0, rows ? off_par : kNoTable };
        if(filtered_launch(ix, ex, a, ex ? lds_e : lds_w, stream, &t) < 0) return false;
        launches += 1;
    }
    const uint32_t shape[ 6 ] = { c.walk, c.exact, c.unfiltered, c.empty, (uint32_t)distinct.size(), launches };
    std::copy(std::begin(shape), std::end(shape), ix->last_each);
    const uint32_t n_seeded = ix->filter_seeds ? c.walk - c.unfiltered : 0u;
    ix->last_seeds[ 2 ] = n_seeded;
    ix->last_seeds[ 3 ] = c.walk - n_seeded;
    ix->c_search_queries += nq;
    return true;
}

// The caller holds ix->mu and has flushed.  The queries split into a walk group and an exact group by the path rule, evaluated per
// query from its own filter's count; each group is ONE launch over its own selection list, and every answer lands in the caller's
// row of its query.  Empty filters have no path: they ride in the exact launch (or, when nothing else takes the exact path, in the
// walk launch), where a descriptor with count 0 gives the empty answer without touching a row.
// `h_tbl`: a page-locked block of each_table_bytes(nq) that stays untouched until the stream work is done, or NULL (pageable
// staging: the copies then complete before this returns).  false -> ix->err; nothing has been launched unless the failure is HIP's.
// dense_call: one of the two entry points that may send groups of exact-path queries sharing a filter handle through the dense route
// (lantern_gpu_set_filter_dense_each): those queries leave the exact list, the dense run answers them in front of the launches, and
// the ones its certificate refuses come back into the exact list.  The lane form never does.  With a dense group the sentence above
// holds up to the dense run only: when a launch behind it is then refused for a reason that is not HIP's (a scratch block, a launch
// slot), the call fails with the certified dense queries' rows already written and their D already in the cumulative counter.
static bool filtered_each_locked(Index *ix, const Filter *const *filters, const uint4 *d_q, size_t nq, size_t k, size_t ef, size_t skip,
                                 const SearchOut &out, hipStream_t stream, char *h_tbl, bool dense_call = false)
{
    if(!each_filters_ok(ix, filters, nq)) return false;
    std::fill(std::begin(ix->last_each_dense), std::end(ix->last_each_dense), 0u);
    if(nq == 0 || k == 0) return true;
    const size_t ef_sel = ef ? ef : ix->ef;
    const size_t exp = std::max(ef_sel, k + skip);
    std::vector<uint32_t> walk, exact, empty;
    uint32_t              n_unfiltered = 0;
    for(size_t i = 0; i < nq; ++i) {
        const Filter *f = filters[ i ];
        if(ix->n == 0 || (f && f->count == 0)) { empty.push_back((uint32_t)i); continue; }
        if(!f) { n_unfiltered += 1; walk.push_back((uint32_t)i); continue; }
        (filter_takes_exact(ix, f, ef_sel) ? exact : walk).push_back((uint32_t)i);
    }
    const uint32_t n_walk = (uint32_t)walk.size(), n_exact = (uint32_t)exact.size(), n_empty = (uint32_t)empty.size();

    // the launches' carves, and their refusals, by the lists as the path rule left them: the dense route below changes neither
    const FilteredArgs base = filtered_args(ix, d_q, k, skip, out);
    FilteredArgs aw = base, ae = base;
    aw.seeds = (uint32_t)ix->filter_seeds;  // (an unfiltered entry has no slot list: it runs the unseeded walk in the same launch)
    size_t       lds_w = 0, lds_e = 0;
    if(!walk.empty() && !filtered_shape(ix, false, k, skip, exp, aw, lds_w)) return false;
    if((!exact.empty() || (walk.empty() && !empty.empty())) && !filtered_shape(ix, true, k, skip, exp, ae, lds_e)) return false;

    if(dense_call && ix->filter_dense_each_min && !exact.empty()) {
        const DenseEnv       env = dense_env();
        std::vector<int64_t> ids(nq), counts(nq);
        std::vector<uint8_t> is_exact(nq, 0);
        for(size_t i = 0; i < nq; ++i) {
            ids[ i ] = filters[ i ] ? (int64_t)(uintptr_t)filters[ i ] : -1;  // (a handle's address is a user-space one: never negative)
            counts[ i ] = filters[ i ] ? (int64_t)filters[ i ]->count : 0;
        }
        for(uint32_t q : exact) is_exact[ q ] = 1;
        EachDensePlan     dense;
        const char *const bad = plan_filtered_each_dense(ix->mcode, ix->chunks, (int64_t)k, (int64_t)skip, (int64_t)ix->filter_dense_each_min, ix->pq_compact,
                                                         env.native, ids.data(), counts.data(), is_exact.data(), nq, dense);
        if(!bad && dense.why == kEachDenseTaken) {
            std::vector<uint32_t> refused;
            if(!filtered_each_dense_locked(ix, filters, dense, d_q, k, skip, out, stream, refused)) return false;
            exact.erase(std::remove_if(exact.begin(), exact.end(), [&](uint32_t q) { return dense.group[ q ] != 0xFFFFFFFFu; }), exact.end());
            exact.insert(exact.end(), refused.begin(), refused.end());
        }
    }
    // the exact group's queries differ in length by orders of magnitude: longest first, so that the launch's tail is a short one
    std::stable_sort(exact.begin(), exact.end(), [&](uint32_t x, uint32_t y) { return filters[ x ]->count > filters[ y ]->count; });
    std::vector<uint32_t> &host = (exact.empty() && !walk.empty()) ? walk : exact;
    host.insert(host.end(), empty.begin(), empty.end());

    const EachCounts c{ n_walk, n_exact, n_unfiltered, n_empty };
    return each_launches(ix, filters, nq, walk, exact, aw, lds_w, ae, lds_e, nullptr, c, stream, h_tbl);
}

// ---- per-query filters AND per-query (k, ef, skip): lantern_gpu_search_batch_filtered_each_params* -------------------------------
// The plan of such a call: every query's path, expansion and C by the uniform call's own rules, the two selection lists, the
// parameter table and the two launches' carves.  A pure function of FilterPlanIn, the filters' counts and the parameters.
struct EachParamsPlan
{
    std::vector<uint32_t> walk, exact;  // the selection lists, in launch order, the riders (no path: an empty filter, k == 0, an empty
                                        // index) behind the queries of the list they ride in
    std::vector<uint32_t> rows;         // [nq][4] {k, expansion (exact: k + skip), skip, C}
    std::vector<uint8_t>  path;         // [nq] 0 none, 1 walk, 2 exact
    EachCounts            counts{};     // (`empty`: every rider)
    uint32_t              n_k0 = 0;     // queries with k == 0
    FilteredShape         sw, se;       // the launches' carves: the largest expansion with the largest C; the largest k + skip
};

// "" or the refusal.  counts[i]: the allowed count of query i's filter, -1 for a NULL entry.
static std::string plan_filtered_params(const FilterPlanIn &p, const int64_t *counts, const lantern_gpu_query_params *params, size_t nq, EachParamsPlan &out)
{
    out = EachParamsPlan{};
    out.rows.assign(nq * 4, 0u);
    out.path.assign(nq, 0);
    std::vector<uint32_t> riders;
    size_t                max_exp = 0, max_cap = 0, max_kk = 0;
    for(size_t i = 0; i < nq; ++i) {
        const size_t k = params[ i ].k, skip = params[ i ].skip;
        uint32_t *const row = &out.rows[ 4 * i ];
        row[ 0 ] = (uint32_t)k, row[ 2 ] = (uint32_t)skip;
        out.n_k0 += k == 0;
        if(k == 0 || p.n == 0 || counts[ i ] == 0) { riders.push_back((uint32_t)i); continue; }
        const size_t ef_sel = params[ i ].ef ? params[ i ].ef : p.ef_default;
        const bool   exact = counts[ i ] >= 0 && count_takes_exact(p, (size_t)counts[ i ], ef_sel);
        // (far past the LDS budget already: refused below, and it fits the table's word)
        const size_t  exp = std::min<size_t>(std::max(ef_sel, k + skip), (size_t)1 << 20), kk = std::min<size_t>(k + skip, (size_t)1 << 20);
        FilteredShape s;
        if(const char *why = filtered_shape_of(p, exact, kk, 0, exp, s)) return std::string(why) + " (params[" + std::to_string(i) + "])";
        row[ 1 ] = s.exp, row[ 3 ] = s.cand_cap;
        out.path[ i ] = exact ? 2 : 1;
        (exact ? out.exact : out.walk).push_back((uint32_t)i);
        if(exact) max_kk = std::max<size_t>(max_kk, s.exp);
        else max_exp = std::max<size_t>(max_exp, s.exp), max_cap = std::max<size_t>(max_cap, s.cand_cap), out.counts.unfiltered += counts[ i ] < 0;
    }
    out.counts.walk = (uint32_t)out.walk.size(), out.counts.exact = (uint32_t)out.exact.size(), out.counts.empty = (uint32_t)riders.size();
    // one carve per launch.  The exact list's is the carve of its largest k + skip, which fits because that query does; the walk's
    // joins the largest expansion with the largest C, which two different queries may have brought
    if(!out.walk.empty()) {
        if(filtered_walk_lds_bytes(plan_lds_chunks(p), (uint32_t)max_exp, (uint32_t)max_cap, p.M0, 0) > kFilteredLds) return kJointOverBudget;
        walk_carve(p, max_exp, max_cap, out.sw);
    }
    if(!out.exact.empty()) exact_carve(p, max_kk, out.se);
    // the walk list by expansion descending, the exact list by allowed count descending (both stable): the longest first, so that a
    // launch's tail is a short one
    std::stable_sort(out.walk.begin(), out.walk.end(), [&](uint32_t x, uint32_t y) { return out.rows[ 4 * x + 1 ] > out.rows[ 4 * y + 1 ]; });
    std::stable_sort(out.exact.begin(), out.exact.end(), [&](uint32_t x, uint32_t y) { return counts[ x ] > counts[ y ]; });
    std::vector<uint32_t> &host = (out.exact.empty() && !out.walk.empty()) ? out.walk : out.exact;
    if(!out.walk.empty() || !out.exact.empty()) host.insert(host.end(), riders.begin(), riders.end());
    return "";
}

// The caller holds ix->mu and has flushed: the filters checked, the call planned.  false -> ix->err; nothing is queued.
static bool each_params_plan_locked(Index *ix, const Filter *const *filters, const lantern_gpu_query_params *params, size_t nq, EachParamsPlan &plan)
{
    if(!each_filters_ok(ix, filters, nq)) return false;
    std::vector<int64_t> counts(nq);
    for(size_t i = 0; i < nq; ++i) counts[ i ] = filters[ i ] ? (int64_t)filters[ i ]->count : -1;
    const std::string why = plan_filtered_params(filter_plan_in(ix), counts.data(), params, nq, plan);
    if(!why.empty()) return set_err(ix, why), false;
    return true;
}

// The caller holds ix->mu, has flushed and has planned the call under this hold of the mutex.  `h_tbl` as filtered_each_locked's, of
// each_table_bytes(nq, true).
static bool filtered_each_params_locked(Index *ix, const EachParamsPlan &plan, const Filter *const *filters, const uint4 *d_q, size_t nq, size_t k_stride,
                                        const SearchOut &out, hipStream_t stream, char *h_tbl)
{
    std::fill(std::begin(ix->last_each_dense), std::end(ix->last_each_dense), 0u);  // (a per-query-filter call that makes no dense run)
    if(nq == 0) return true;
    const uint32_t shape[ 4 ] = { plan.sw.exp, plan.sw.cand_cap, plan.se.exp, plan.n_k0 };
    std::copy(std::begin(shape), std::end(shape), ix->last_each_params);
    if(plan.walk.empty() && plan.exact.empty()) {  // riders only: the empty answers, no launch
        const uint32_t none[ 6 ] = { 0, 0, 0, plan.counts.empty, 0, 0 };
        std::copy(std::begin(none), std::end(none), ix->last_each);
        ix->last_seeds[ 2 ] = ix->last_seeds[ 3 ] = 0;
        return empty_answers(ix, out, nq, k_stride, stream);
    }
    const FilteredArgs base = filtered_args(ix, d_q, k_stride, 0, out);  // (k: the width of an answer row)
    FilteredArgs aw = base, ae = base;
    aw.seeds = (uint32_t)ix->filter_seeds;
    size_t lds_w = 0, lds_e = 0;
    shape_into(plan.sw, aw, lds_w);
    shape_into(plan.se, ae, lds_e);
    return each_launches(ix, filters, nq, plan.walk, plan.exact, aw, lds_w, ae, lds_e, plan.rows.data(), plan.counts, stream, h_tbl);
}

// one query through `cur` (streaming: never a row twice): the first k allowed rows not handed out before
static size_t cursor_search_filtered_locked(Index *ix, const Filter *f, Cursor *cur, const void *query, int kind, size_t k, size_t ef, bool streaming,
                                            uint64_t *labels, float *distances)
{
    if(!cursor_epoch_ok(ix, cur, streaming)) return 0;
    if(ix->n == 0 || k == 0) return 0;
    const size_t want = std::max<size_t>(1, std::min(cur->seen.size() + k, std::max<size_t>(f->count, 1)));
    const size_t row = (size_t)ix->chunks * 16;
    std::vector<uint32_t> padded((size_t)ix->chunks * 4);
    pad_row(ix, query, kind, padded.data());
    char *dq = (char *)scratch(ix, kScratchCallIn, row);
    char *dout = (char *)scratch(ix, kScratchCallOut, want * 16 + 16);
    if(!dq || !dout) return 0;
    bool ok = hipMemcpyAsync(dq, padded.data(), row, hipMemcpyHostToDevice, ix->stream) == hipSuccess;
    const SearchOut out{ (uint64_t *)dout, (float *)(dout + want * 8), (uint32_t *)(dout + want * 12), (uint32_t *)(dout + want * 16), nullptr, nullptr };
    ok = ok && filtered_search_locked(ix, f, (const uint4 *)dq, 1, want, ef, 0, out, ix->stream);
    std::vector<char> h(want * 16 + 4);
    ok = ok && hipMemcpyAsync(h.data(), dout, want * 16 + 4, hipMemcpyDeviceToHost, ix->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(ix->stream) == hipSuccess;
    if(!ok) {
        if(ix->err.empty()) set_err(ix, "lantern_gpu: HIP failure during filtered search");
        return 0;
    }
    uint32_t got;
    std::memcpy(&got, h.data() + want * 16, 4);
    return take_unseen(cur, (const uint64_t *)h.data(), (const float *)(h.data() + want * 8), (const uint32_t *)(h.data() + want * 12), got, k, labels, distances);
}

}  // namespace lgpu

// =====================================================================================================
// C ABI
// =====================================================================================================
using namespace lgpu;

// (lantern_gpu_filter_t stays an incomplete type: a handle is a Filter, recognised by its magic word)
static Filter *FF(const lantern_gpu_filter_t *f, usearch_error_t *e)
{
    if(!f) { FAIL(e, "lantern_gpu: null filter handle"); return nullptr; }
    if(((const Filter *)f)->magic != kFilterMagic) { FAIL(e, kNotAFilter); return nullptr; }
    return (Filter *)f;
}

// The handles of a per-query call: the filter array, then the index.  Whether every entry belongs to the index can only be told with the
// index in hand (each_filters_ok, which names the first offender of any kind); without one, an entry that is no filter at all is
// still worth naming.
static Index *FHS(usearch_index_t h, const lantern_gpu_filter_t *const *filters, size_t nq, usearch_error_t *e)
{
    static thread_local std::string msg;
    if(nq && !filters) { FAIL(e, "lantern_gpu: null filter array"); return nullptr; }
    Index *ix = H(h, e);
    if(ix) return ix;
    for(size_t i = 0; i < nq; ++i) {
        if(!filters[ i ] || ((const Filter *)filters[ i ])->magic == kFilterMagic) continue;
        msg = std::string(kNotAFilter) + " (filters[" + std::to_string(i) + "])";
        FAIL(e, msg.c_str());
        break;
    }
    return nullptr;
}

extern "C" {

lantern_gpu_filter_t *lantern_gpu_filter_from_labels(usearch_index_t h, const usearch_label_t *labels, size_t n, uint32_t flags, usearch_error_t *e)
try {
    CLEAR(e);
    if(flags & ~(uint32_t)LANTERN_GPU_FILTER_SKIP_DELETED) { FAIL(e, kFilterFlags); return nullptr; }
    if(n && !labels) { FAIL(e, "lantern_gpu: null label array"); return nullptr; }
    Index *ix = H(h, e);
    if(!ix) return nullptr;
    std::lock_guard<std::mutex> g(ix->mu);
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return nullptr; }
    ix->err.clear();
    Filter *f = filter_from_labels_locked(ix, labels, n, (flags & LANTERN_GPU_FILTER_SKIP_DELETED) ? 1 : 0);
    if(!f) { FAIL(e, ix->err.c_str()); return nullptr; }
    return (lantern_gpu_filter_t *)f;
}
LANTERN_ABI_CATCH(e)

lantern_gpu_filter_t *lantern_gpu_filter_from_slot_bitmap(usearch_index_t h, const uint32_t *words, size_t n_words, uint32_t flags, usearch_error_t *e)
try {
    CLEAR(e);
    if(flags & ~(uint32_t)LANTERN_GPU_FILTER_SKIP_DELETED) { FAIL(e, kFilterFlags); return nullptr; }
    if(n_words && !words) { FAIL(e, "lantern_gpu: null bitmap"); return nullptr; }
    Index *ix = H(h, e);
    if(!ix) return nullptr;
    std::lock_guard<std::mutex> g(ix->mu);
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return nullptr; }
    ix->err.clear();
    const size_t need = (ix->n + 31) / 32;
    if(n_words != need) {
        set_err(ix, "lantern_gpu: the slot bitmap has " + std::to_string(n_words) + " words; an index of " + std::to_string(ix->n) + " rows needs " +
                        std::to_string(need));
        FAIL(e, ix->err.c_str());
        return nullptr;
    }
    Filter *f = filter_from_bitmap_locked(ix, words, n_words, (flags & LANTERN_GPU_FILTER_SKIP_DELETED) ? 1 : 0);
    if(!f) { FAIL(e, ix->err.c_str()); return nullptr; }
    return (lantern_gpu_filter_t *)f;
}
LANTERN_ABI_CATCH(e)

size_t lantern_gpu_filter_count(const lantern_gpu_filter_t *f, usearch_error_t *e)
try {
    CLEAR(e);
    const Filter *ff = FF(f, e);
    return ff ? ff->count : 0;
}
LANTERN_ABI_CATCH(e)

size_t lantern_gpu_filter_resident_bytes(const lantern_gpu_filter_t *f, usearch_error_t *e)
try {
    CLEAR(e);
    const Filter *ff = FF(f, e);
    return ff ? ff->words * 4 + ff->count * 4 : 0;
}
LANTERN_ABI_CATCH(e)

// ---- a filter's life cycle: extended to the index's new size, combined with another, read back (DESIGN.md 4.9 "Filter life cycle").
// The argument checks come first, the handles behind them; the device is first used under ix->mu, after the flush.
lantern_gpu_filter_t *lantern_gpu_filter_extend(usearch_index_t h, const lantern_gpu_filter_t *filter, const usearch_label_t *labels, size_t n, uint32_t flags,
                                                usearch_error_t *e)
try {
    CLEAR(e);
    if(flags & ~(uint32_t)(LANTERN_GPU_FILTER_SKIP_DELETED | LANTERN_GPU_FILTER_EXTEND_ALL)) {
        FAIL(e, "lantern_gpu: unknown filter flags (an extension takes LANTERN_GPU_FILTER_SKIP_DELETED and LANTERN_GPU_FILTER_EXTEND_ALL)");
        return nullptr;
    }
    if(n && !labels) { FAIL(e, "lantern_gpu: null label array"); return nullptr; }
    if((flags & LANTERN_GPU_FILTER_EXTEND_ALL) && (n || labels)) {
        FAIL(e, "lantern_gpu: LANTERN_GPU_FILTER_EXTEND_ALL allows every new slot: it takes no labels (labels NULL, n 0)");
        return nullptr;
    }
    const Filter *old = FF(filter, e);
    if(!old) return nullptr;
    Index *ix = H(h, e);
    if(!ix) return nullptr;
    std::lock_guard<std::mutex> g(ix->mu);
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return nullptr; }
    ix->err.clear();
    // another index's filter and one from before a compaction: the messages a search gives.  (Within an epoch an index only grows.)
    if(old->ix != ix || old->epoch != ix->epoch) set_err(ix, filter_mismatch(ix, old));
    else if(old->n > ix->n) set_err(ix, "lantern_gpu: the filter was built over " + std::to_string(old->n) + " rows; the index holds " + std::to_string(ix->n));
    if(!ix->err.empty()) { FAIL(e, ix->err.c_str()); return nullptr; }
    Filter *f = filter_extend_locked(ix, old, labels, n, (flags & LANTERN_GPU_FILTER_EXTEND_ALL) ? 1 : 0, (flags & LANTERN_GPU_FILTER_SKIP_DELETED) ? 1 : 0);
    if(!f) { FAIL(e, ix->err.c_str()); return nullptr; }
    return (lantern_gpu_filter_t *)f;
}
LANTERN_ABI_CATCH(e)

lantern_gpu_filter_t *lantern_gpu_filter_combine(usearch_index_t h, const lantern_gpu_filter_t *a, const lantern_gpu_filter_t *b, int op, usearch_error_t *e)
try {
    CLEAR(e);
    if(op != LANTERN_GPU_FILTER_AND && op != LANTERN_GPU_FILTER_OR && op != LANTERN_GPU_FILTER_ANDNOT) {
        FAIL(e, "lantern_gpu: filter op must be LANTERN_GPU_FILTER_AND (0), LANTERN_GPU_FILTER_OR (1) or LANTERN_GPU_FILTER_ANDNOT (2)");
        return nullptr;
    }
    const Filter *fa = FF(a, e);
    if(!fa) return nullptr;
    const Filter *fb = FF(b, e);
    if(!fb) return nullptr;
    Index *ix = H(h, e);
    if(!ix) return nullptr;
    std::lock_guard<std::mutex> g(ix->mu);
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return nullptr; }
    ix->err.clear();
    for(const Filter *f : { fa, fb }) {
        const std::string why = filter_mismatch(ix, f);
        if(why.empty()) continue;
        set_err(ix, why + (f == fa ? " (operand a)" : " (operand b)"));
        FAIL(e, ix->err.c_str());
        return nullptr;
    }
    Filter *f = filter_combine_locked(ix, fa, fb, op);
    if(!f) { FAIL(e, ix->err.c_str()); return nullptr; }
    return (lantern_gpu_filter_t *)f;
}
LANTERN_ABI_CATCH(e)

size_t lantern_gpu_filter_rows(const lantern_gpu_filter_t *f, usearch_error_t *e)
try {
    CLEAR(e);
    const Filter *ff = FF(f, e);
    return ff ? ff->n : 0;
}
LANTERN_ABI_CATCH(e)

size_t lantern_gpu_filter_export(const lantern_gpu_filter_t *filter, uint32_t *words, size_t n_words, uint32_t *slots, size_t cap, usearch_error_t *e)
try {
    CLEAR(e);
    const Filter *f = FF(filter, e);
    if(!f) return 0;
    if(words && n_words < (f->n + 31) / 32) { FAIL(e, "lantern_gpu: the word array is shorter than the filter's bitmap (ceil(rows / 32) words)"); return 0; }
    // the handle's own device memory, which nothing writes after the filter is built: no index is needed, a stale filter reads as well
    const size_t nw = std::min(n_words, f->words), ns = std::min(cap, f->count);
    bool         ok = hipSetDevice(f->device) == hipSuccess;
    if(words) {
        ok = ok && (nw == 0 || hipMemcpy(words, f->d_bits, nw * 4, hipMemcpyDeviceToHost) == hipSuccess);
        if(ok && n_words > nw) std::memset(words + nw, 0, (n_words - nw) * 4);
    }
    if(slots && ns) ok = ok && hipMemcpy(slots, f->d_slots, ns * 4, hipMemcpyDeviceToHost) == hipSuccess;
    if(!ok) { FAIL(e, "lantern_gpu: HIP failure reading a filter back"); return 0; }
    return f->count;
}
LANTERN_ABI_CATCH(e)

void lantern_gpu_filter_free(lantern_gpu_filter_t *f)
try {
    if(!f || ((const Filter *)f)->magic != kFilterMagic) return;
    filter_release((Filter *)f);
}
LANTERN_ABI_CATCH_VOID(nullptr)

void lantern_gpu_set_filter_policy(usearch_index_t h, int path, size_t cand_cap, double exact_factor, usearch_error_t *e)
try {
    CLEAR(e);
    if(path < 0 || path > 2) { FAIL(e, "lantern_gpu: filter path must be 0 (auto), 1 (walk) or 2 (exact)"); return; }
    if(!(exact_factor >= 0) || std::isinf(exact_factor)) { FAIL(e, "lantern_gpu: exact_factor must be a finite number >= 0"); return; }
    Index *ix = H(h, e);
    if(!ix) return;
    std::lock_guard<std::mutex> g(ix->mu);
    ix->filter_path = path;
    ix->filter_cand_cap = cand_cap;
    ix->filter_exact_factor = exact_factor;
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_set_filter_seeds(usearch_index_t h, size_t seeds, usearch_error_t *e)
try {
    CLEAR(e);
    if(seeds > kFilterSeedsMax) { FAIL(e, "lantern_gpu: filter seeds must be at most 4096 (0 = off)"); return; }
    Index *ix = H(h, e);
    if(!ix) return;
    std::lock_guard<std::mutex> g(ix->mu);
    ix->filter_seeds = seeds;
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_set_filter_compact(usearch_index_t h, int on, usearch_error_t *e)
try {
    CLEAR(e);
    if(on != 0 && on != 1) { FAIL(e, "lantern_gpu: filter_compact must be 0 (compact pq indexes refused) or 1 (served)"); return; }
    Index *ix = H(h, e);
    if(!ix) return;
    std::lock_guard<std::mutex> g(ix->mu);
    ix->filter_compact = on != 0;
}
LANTERN_ABI_CATCH_VOID(e)

int lantern_gpu_filter_compact(usearch_index_t h, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return 0;
    std::lock_guard<std::mutex> g(ix->mu);
    if(!ix->filter_compact) return 0;
    return !ix->pq_compact ? 1 : compact_adc(ix) ? 3 : 2;
}
LANTERN_ABI_CATCH(e)

void lantern_gpu_set_filter_dense(usearch_index_t h, size_t min_queries, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return;
    std::lock_guard<std::mutex> g(ix->mu);
    ix->filter_dense_min = min_queries;
}
LANTERN_ABI_CATCH_VOID(e)

size_t lantern_gpu_filter_dense(usearch_index_t h, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return 0;
    std::lock_guard<std::mutex> g(ix->mu);
    return ix->filter_dense_min;
}
LANTERN_ABI_CATCH(e)

void lantern_gpu_filter_dense_stats(usearch_index_t h, uint64_t out[ 4 ], usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return;
    if(!out) { FAIL(e, "lantern_gpu: null output array"); return; }
    std::lock_guard<std::mutex> g(ix->mu);
    std::copy(std::begin(ix->c_filter_dense), std::end(ix->c_filter_dense), out);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_set_filter_dense_each(usearch_index_t h, size_t min_group, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return;
    std::lock_guard<std::mutex> g(ix->mu);
    ix->filter_dense_each_min = min_group;
}
LANTERN_ABI_CATCH_VOID(e)

size_t lantern_gpu_filter_dense_each(usearch_index_t h, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return 0;
    std::lock_guard<std::mutex> g(ix->mu);
    return ix->filter_dense_each_min;
}
LANTERN_ABI_CATCH(e)

void lantern_gpu_last_filtered_each_dense(usearch_index_t h, uint32_t out[ 6 ], usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return;
    if(!out) { FAIL(e, "lantern_gpu: null output array"); return; }
    std::lock_guard<std::mutex> g(ix->mu);
    std::copy(std::begin(ix->last_each_dense), std::end(ix->last_each_dense), out);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_last_filtered_seeds(usearch_index_t h, uint32_t out[ 4 ], usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return;
    if(!out) { FAIL(e, "lantern_gpu: null output array"); return; }
    std::lock_guard<std::mutex> g(ix->mu);
    out[ 0 ] = (uint32_t)ix->filter_seeds;
    std::copy(ix->last_seeds + 1, ix->last_seeds + 4, out + 1);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_filter_stats(usearch_index_t h, uint64_t *walk_launches, uint64_t *exact_launches, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return;
    std::lock_guard<std::mutex> g(ix->mu);
    if(walk_launches) *walk_launches = ix->c_filter_walk;
    if(exact_launches) *exact_launches = ix->c_filter_exact;
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_last_filtered_launch(usearch_index_t h, uint32_t out[ 6 ], usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return;
    if(!out) { FAIL(e, "lantern_gpu: null output array"); return; }
    std::lock_guard<std::mutex> g(ix->mu);
    std::copy(std::begin(ix->last_filtered), std::end(ix->last_filtered), out);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_search_batch_filtered_device(usearch_index_t h, const lantern_gpu_filter_t *filter, const void *d_queries, size_t query_stride_bytes,
                                              size_t nq, size_t k, size_t ef, size_t skip, uint64_t *d_labels, float *d_distances, uint32_t *d_slots,
                                              uint32_t *d_counts, uint64_t *d_D, uint64_t *d_E, void *stream, usearch_error_t *e)
try {
    CLEAR(e);
    const Filter *f = FF(filter, e);
    if(!f) return;
    Index *ix = H(h, e);
    if(!ix) return;
    const SearchOut out{ d_labels, d_distances, d_slots, d_counts, d_D, d_E };
    device_trip(ix, stride_is(query_stride_bytes),
                [ & ] { return filtered_search_locked(ix, f, (const uint4 *)d_queries, nq, k, ef, skip, out, (hipStream_t)stream, true); }, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_search_batch_filtered(usearch_index_t h, const lantern_gpu_filter_t *filter, const void *queries, size_t nq, usearch_scalar_kind_t kind,
                                       size_t k, size_t ef, usearch_label_t *labels, float *distances, uint32_t *counts, usearch_error_t *e)
try {
    CLEAR(e);
    const Filter *f = FF(filter, e);
    if(!f) return;
    Index *ix = H(h, e);
    if(!ix) return;
    if(!kind_accepted(ix, (int)kind)) { FAIL(e, kKindMismatch); return; }
    if(nq == 0 || k == 0) return;
    if(!queries || !labels || !distances) { FAIL(e, "lantern_gpu: null query or result pointer"); return; }
    host_trip_sync(ix, nq, k, 0, queries, (int)kind, kFilteredBatchFailed, nullptr,
                   [ = ](const HostBatch &b) { return filtered_search_locked(ix, f, (const uint4 *)b.d_q, nq, k, ef, 0, b.out(b.d_out), b.stream, true); }, labels,
                   distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_last_filtered_each(usearch_index_t h, uint32_t out[ 6 ], usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return;
    if(!out) { FAIL(e, "lantern_gpu: null output array"); return; }
    std::lock_guard<std::mutex> g(ix->mu);
    std::copy(std::begin(ix->last_each), std::end(ix->last_each), out);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_search_batch_filtered_each_device(usearch_index_t h, const lantern_gpu_filter_t *const *filters, const void *d_queries,
                                                   size_t query_stride_bytes, size_t nq, size_t k, size_t ef, size_t skip, uint64_t *d_labels,
                                                   float *d_distances, uint32_t *d_slots, uint32_t *d_counts, uint64_t *d_D, uint64_t *d_E,
                                                   void *stream, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = FHS(h, filters, nq, e);
    if(!ix) return;
    const SearchOut out{ d_labels, d_distances, d_slots, d_counts, d_D, d_E };
    device_trip(ix, stride_is(query_stride_bytes), [ & ] {
        return filtered_each_locked(ix, (const Filter *const *)filters, (const uint4 *)d_queries, nq, k, ef, skip, out, (hipStream_t)stream, nullptr, true);
    }, e);
}
LANTERN_ABI_CATCH_VOID(e)

// the filter check and the launch of the per-query host forms, of either host trip (the tables go into the staging block's extra area)
static auto each_validate(const lantern_gpu_filter_t *const *filters, size_t nq)
{
    return [ = ](Index *ix) { return each_filters_ok(ix, (const Filter *const *)filters, nq); };
}
static auto each_launch(Index *ix, const lantern_gpu_filter_t *const *filters, size_t nq, size_t k, size_t ef, bool dense_call)
{
    return [ = ](const HostBatch &b) {
        return filtered_each_locked(ix, (const Filter *const *)filters, (const uint4 *)b.d_q, nq, k, ef, 0, b.out(b.d_out), b.stream, b.h_extra(), dense_call);
    };
}

void lantern_gpu_search_batch_filtered_each(usearch_index_t h, const lantern_gpu_filter_t *const *filters, const void *queries, size_t nq,
                                            usearch_scalar_kind_t kind, size_t k, size_t ef, usearch_label_t *labels, float *distances,
                                            uint32_t *counts, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = FHS(h, filters, nq, e);
    if(!ix) return;
    if(!kind_accepted(ix, (int)kind)) { FAIL(e, kKindMismatch); return; }
    if(nq && k && (!queries || !labels || !distances)) { FAIL(e, "lantern_gpu: null query or result pointer"); return; }
    host_trip_sync(ix, nq, k, each_table_bytes(nq), queries, (int)kind, kFilteredBatchFailed, each_validate(filters, nq),
                   each_launch(ix, filters, nq, k, ef, true), labels, distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

// lantern_gpu_search_batch_lane with a filter per query: the lane trip, the selection lists and descriptor table in the block's extra area
void lantern_gpu_search_batch_filtered_each_lane(usearch_index_t h, int lane, const lantern_gpu_filter_t *const *filters, const void *queries,
                                                 size_t nq, usearch_scalar_kind_t kind, size_t k, size_t ef, usearch_label_t *labels,
                                                 float *distances, uint32_t *counts, usearch_error_t *e)
try {
    CLEAR(e);
    if(!lane_ok(lane, e)) return;
    Index *ix = FHS(h, filters, nq, e);
    if(!ix) return;
    if(!kind_accepted(ix, (int)kind)) { FAIL(e, kKindMismatch); return; }
    if(nq && k && (!queries || !labels || !distances)) { FAIL(e, "lantern_gpu: null buffer"); return; }
    host_trip_lane(ix, lane, nq, k, each_table_bytes(nq), queries, (int)kind, kFilteredBatchFailed, each_validate(filters, nq),
                   each_launch(ix, filters, nq, k, ef, false), labels, distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

// ---- per-query filters with per-query (k, ef, skip): the entry points (include/lantern_gpu.h has the contract and the order of the refusals)
void lantern_gpu_last_filtered_each_params(usearch_index_t h, uint32_t out[ 4 ], usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return;
    if(!out) { FAIL(e, "lantern_gpu: null output array"); return; }
    std::lock_guard<std::mutex> g(ix->mu);
    std::copy(std::begin(ix->last_each_params), std::end(ix->last_each_params), out);
}
LANTERN_ABI_CATCH_VOID(e)

// refusals 1 and 2: the handles, as FHS; then the parameter array
static Index *FPH(usearch_index_t h, const lantern_gpu_filter_t *const *filters, const lantern_gpu_query_params *params, size_t nq, size_t k_stride,
                  usearch_error_t *e)
{
    static thread_local std::string msg;
    Index *ix = FHS(h, filters, nq, e);
    if(!ix) return nullptr;
    msg = params_check(params, nq, k_stride);
    if(msg.empty()) return ix;
    FAIL(e, msg.c_str());
    return nullptr;
}

// refusals 3 to 6 of the host forms, of either host trip: the filters, then the plan, which the launch of the same trip reads
struct EachParamsValidate
{
    static constexpr bool              zero_width_rows = true;  // (host_trip.hpp: k_stride == 0 is a batch of k_i == 0, whose counts are written)
    const lantern_gpu_filter_t *const *filters;
    const lantern_gpu_query_params    *params;
    size_t                             nq;
    EachParamsPlan                    *plan;
    bool operator()(Index *ix) const { return each_params_plan_locked(ix, (const Filter *const *)filters, params, nq, *plan); }
};
static auto each_params_launch(Index *ix, const EachParamsPlan *plan, const lantern_gpu_filter_t *const *filters, size_t nq, size_t k_stride)
{
    return [ = ](const HostBatch &b) {
        return filtered_each_params_locked(ix, *plan, (const Filter *const *)filters, (const uint4 *)b.d_q, nq, k_stride, b.out(b.d_out), b.stream, b.h_extra());
    };
}

void lantern_gpu_search_batch_filtered_each_params_device(usearch_index_t h, const lantern_gpu_filter_t *const *filters, const void *d_queries,
                                                          size_t query_stride_bytes, size_t nq, const lantern_gpu_query_params *params,
                                                          size_t k_stride, uint64_t *d_labels, float *d_distances, uint32_t *d_slots,
                                                          uint32_t *d_counts, uint64_t *d_D, uint64_t *d_E, void *stream, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = FPH(h, filters, params, nq, k_stride, e);
    if(!ix) return;
    const SearchOut out{ d_labels, d_distances, d_slots, d_counts, d_D, d_E };
    device_trip(ix, stride_is(query_stride_bytes), [ & ] {
        EachParamsPlan plan;
        return each_params_plan_locked(ix, (const Filter *const *)filters, params, nq, plan) &&
               filtered_each_params_locked(ix, plan, (const Filter *const *)filters, (const uint4 *)d_queries, nq, k_stride, out, (hipStream_t)stream, nullptr);
    }, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_search_batch_filtered_each_params(usearch_index_t h, const lantern_gpu_filter_t *const *filters, const void *queries, size_t nq,
                                                   usearch_scalar_kind_t kind, const lantern_gpu_query_params *params, size_t k_stride,
                                                   usearch_label_t *labels, float *distances, uint32_t *counts, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = FPH(h, filters, params, nq, k_stride, e);
    if(!ix) return;
    if(!kind_accepted(ix, (int)kind)) { FAIL(e, kKindMismatch); return; }
    if(nq && (!queries || (k_stride && (!labels || !distances)))) { FAIL(e, "lantern_gpu: null query or result pointer"); return; }
    EachParamsPlan plan;
    host_trip_sync(ix, nq, k_stride, each_table_bytes(nq, true), queries, (int)kind, kFilteredBatchFailed, EachParamsValidate{ filters, params, nq, &plan },
                   each_params_launch(ix, &plan, filters, nq, k_stride), labels, distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_search_batch_filtered_each_params_lane(usearch_index_t h, int lane, const lantern_gpu_filter_t *const *filters, const void *queries,
                                                        size_t nq, usearch_scalar_kind_t kind, const lantern_gpu_query_params *params, size_t k_stride,
                                                        usearch_label_t *labels, float *distances, uint32_t *counts, usearch_error_t *e)
try {
    CLEAR(e);
    if(!lane_ok(lane, e)) return;
    Index *ix = FPH(h, filters, params, nq, k_stride, e);
    if(!ix) return;
    if(!kind_accepted(ix, (int)kind)) { FAIL(e, kKindMismatch); return; }
    if(nq && (!queries || (k_stride && (!labels || !distances)))) { FAIL(e, "lantern_gpu: null buffer"); return; }
    EachParamsPlan plan;
    host_trip_lane(ix, lane, nq, k_stride, each_table_bytes(nq, true), queries, (int)kind, kFilteredBatchFailed,
                   EachParamsValidate{ filters, params, nq, &plan }, each_params_launch(ix, &plan, filters, nq, k_stride), labels, distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

// the plan without a device (include/lantern_gpu.h has the field order): `cols` words of a launch's row are written
static const char *plan_flat(const FilterPlanIn &p, const int64_t counts[], const lantern_gpu_query_params params[], size_t nq, uint32_t per_query[][ 4 ],
                             uint32_t *launch, int cols)
{
    static thread_local std::string msg;
    EachParamsPlan plan;
    msg = plan_filtered_params(p, counts, params, nq, plan);
    if(!msg.empty()) return msg.c_str();
    for(size_t i = 0; i < nq; ++i) {
        per_query[ i ][ 0 ] = plan.path[ i ], per_query[ i ][ 1 ] = plan.rows[ 4 * i + 1 ], per_query[ i ][ 2 ] = plan.rows[ 4 * i + 3 ], per_query[ i ][ 3 ] = 0;
    }
    for(int l = 0; l < 2; ++l) {
        const std::vector<uint32_t> &list = l ? plan.exact : plan.walk;
        const FilteredShape         &s = l ? plan.se : plan.sw;
        for(size_t at = 0; at < list.size(); ++at) per_query[ list[ at ] ][ 3 ] = (uint32_t)at;
        const uint32_t row[ 7 ] = { (uint32_t)list.size(), s.exp, s.cand_cap, l ? s.rows_per_round : s.vis_slots, (uint32_t)s.lds,
                                    list.empty() ? 0u : (uint32_t)filtered_per_cu(s.lds), list.empty() ? 0u : (uint32_t)plan_table_bytes(p) };
        std::copy(row, row + cols, launch + l * cols);
    }
    return nullptr;
}
static FilterPlanIn plan_in_flat(const int64_t in[ 8 ])
{
    double factor;
    std::memcpy(&factor, &in[ 6 ], 8);
    return FilterPlanIn{ (uint32_t)in[ 0 ], (uint32_t)in[ 1 ], (size_t)in[ 2 ], (size_t)in[ 3 ], (int)in[ 4 ], (size_t)in[ 5 ], factor, (size_t)in[ 7 ] };
}

const char *lantern_gpu_plan_filtered_params(const int64_t in[ 8 ], const int64_t counts[], const lantern_gpu_query_params params[], size_t nq,
                                             uint32_t per_query[][ 4 ], uint32_t launch[ 2 ][ 6 ])
try {
    if(!in || !launch || (nq && (!counts || !params || !per_query))) return "lantern_gpu: null array";
    return plan_flat(plan_in_flat(in), counts, params, nq, per_query, &launch[ 0 ][ 0 ], 6);
}
catch(...) {
    return "lantern_gpu: out of memory planning a filtered search";
}

const char *lantern_gpu_plan_filtered_compact(const int64_t in[ 9 ], const int64_t counts[], const lantern_gpu_query_params params[], size_t nq,
                                              uint32_t per_query[][ 4 ], uint32_t launch[ 2 ][ 7 ])
try {
    if(!in || !launch || (nq && (!counts || !params || !per_query))) return "lantern_gpu: null array";
    if(in[ 8 ] < 0 || in[ 8 ] > 8) return "lantern_gpu: a code row has 1 to 8 chunks (0: rows decoded on the fly)";
    FilterPlanIn p = plan_in_flat(in);
    p.adc_code_chunks = (uint32_t)in[ 8 ];
    return plan_flat(p, counts, params, nq, per_query, &launch[ 0 ][ 0 ], 7);
}
catch(...) {
    return "lantern_gpu: out of memory planning a filtered search";
}

size_t lantern_gpu_cursor_search_filtered(lantern_gpu_cursor_t *c, const lantern_gpu_filter_t *filter, const void *query, usearch_scalar_kind_t kind,
                                          size_t k, size_t ef, bool streaming, usearch_label_t *labels, float *distances, usearch_error_t *e)
try {
    CLEAR(e);
    if(!c) { FAIL(e, "lantern_gpu: null cursor"); return 0; }
    const Filter *f = FF(filter, e);
    if(!f) return 0;
    Index *ix = H(c->ix, e);
    if(!ix) return 0;
    if(!kind_accepted(ix, (int)kind)) { FAIL(e, "lantern_gpu: scalar kind of the query does not match the index"); return 0; }
    if(k == 0) return 0;
    if(!query || !labels || !distances) { FAIL(e, "lantern_gpu: null query or result pointer"); return 0; }
    std::lock_guard<std::mutex> g(ix->mu);
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return 0; }
    ix->err.clear();
    const size_t out = cursor_search_filtered_locked(ix, f, &c->cur, query, (int)kind, k, ef, streaming, labels, distances);
    if(!ix->err.empty()) FAIL(e, ix->err.c_str());
    return out;
}
LANTERN_ABI_CATCH(e)

}  // extern "C"
