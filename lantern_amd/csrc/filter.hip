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
#include "filter.hpp"
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
        size_t lo = 0, hi = m;
        while(lo < hi) {
            const size_t mid = (lo + hi) >> 1;
            if(sorted[ mid ] < l) lo = mid + 1; else hi = mid;
        }
        if(lo < m && sorted[ lo ] == l) word |= 1u << b;
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

// the bitmap is in f->d_bits: its popcount and the allowed slots in ascending order (the exact path's work list)
static bool filter_finish(Index *ix, Filter *f)
{
    std::vector<uint32_t> h(f->words);
    if(hipMemcpy(h.data(), f->d_bits, f->words * 4, hipMemcpyDeviceToHost) != hipSuccess) { set_err(ix, "lantern_gpu: HIP failure building a filter"); return false; }
    std::vector<uint32_t> slots;
    for(size_t w = 0; w < f->words; ++w)
        for(uint32_t x = h[ w ]; x; x &= x - 1) slots.push_back((uint32_t)(w * 32 + (size_t)__builtin_ctz(x)));
    f->count = slots.size();
    if(!slots.empty()) {
        if(hipMalloc((void **)&f->d_slots, slots.size() * 4) != hipSuccess ||
           hipMemcpy(f->d_slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
            set_err(ix, "lantern_gpu: out of device memory (filter slot list)");
            return false;
        }
    }
    return true;
}

static Filter *filter_new(Index *ix)
{
    Filter *f = new Filter();
    f->ix = ix;
    f->device = ix->device;
    f->n = ix->n;
    f->words = ((std::max<size_t>(ix->n, 1) + 31) / 32 + 3) / 4 * 4;
    if(hipMalloc((void **)&f->d_bits, f->words * 4) != hipSuccess || hipMemset(f->d_bits, 0, f->words * 4) != hipSuccess) {
        set_err(ix, "lantern_gpu: out of device memory (filter bitmap)");
        filter_release(f);
        return nullptr;
    }
    return f;
}

static Filter *filter_from_labels_locked(Index *ix, const uint64_t *labels, size_t m, int skip_deleted)
{
    Filter *f = filter_new(ix);
    if(!f) return nullptr;
    bool ok = true;
    if(m > 0 && ix->n > 0) {
        // the labels sorted on the device (rocPRIM radix sort, as grouping.hip), then one thread per word binary-searches them
        uint64_t *d_in = nullptr, *d_sorted = nullptr;
        void     *temp = nullptr;
        size_t    temp_bytes = 0;
        ok = hipMalloc((void **)&d_in, m * 8) == hipSuccess && hipMalloc((void **)&d_sorted, m * 8) == hipSuccess &&
             hipMemcpy(d_in, labels, m * 8, hipMemcpyHostToDevice) == hipSuccess &&
             rocprim::radix_sort_keys(nullptr, temp_bytes, (const uint64_t *)d_in, d_sorted, m, 0u, 64u, ix->stream) == hipSuccess &&
             hipMalloc(&temp, std::max<size_t>(temp_bytes, 16)) == hipSuccess &&
             rocprim::radix_sort_keys(temp, temp_bytes, (const uint64_t *)d_in, d_sorted, m, 0u, 64u, ix->stream) == hipSuccess;
        if(ok) {
            const int blocks = (int)((f->words + 255) / 256);
            hipLaunchKernelGGL(k_filter_from_labels, dim3(blocks), dim3(256), 0, ix->stream, (const uint64_t *)ix->d_labels, ix->n,
                               (const uint64_t *)d_sorted, m, skip_deleted, f->d_bits, f->words);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ix->stream) == hipSuccess;
        }
        if(d_in) (void)hipFree(d_in);
        if(d_sorted) (void)hipFree(d_sorted);
        if(temp) (void)hipFree(temp);
        if(!ok) set_err(ix, "lantern_gpu: HIP failure building a filter from labels");
    }
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

// The part of a filtered launch's shape that depends on (k, ef, skip, index) only -- not on the filter: exp, cand_cap, vis_slots /
// rows_per_round and the LDS bytes.  false -> ix->err.
static bool filtered_shape(Index *ix, bool exact, size_t k, size_t skip, size_t exp, FilteredArgs &a, size_t &lds)
{
    const int G = group_lanes_for(ix->chunks);
    if(exact) {
        a.exp = (uint32_t)(k + skip);
        a.rows_per_round = (uint32_t)(2 * 64 * kFilteredWaves / G);
        lds = filtered_exact_lds_bytes(ix->chunks, a.exp, a.rows_per_round);
        if(lds > kFilteredLds) {
            set_err(ix, "lantern_gpu: k + skip exceed the 160 KiB LDS budget of the exact filtered search kernel");
            return false;
        }
    } else {
        a.exp = (uint32_t)exp;
        const size_t base = filtered_walk_lds_bytes(ix->chunks, a.exp, 0, ix->M0, 0);
        if(base + exp * 16 > kFilteredLds) {
            set_err(ix, "lantern_gpu: ef/k exceed the 160 KiB LDS budget of the filtered search kernel");
            return false;
        }
        size_t cap = ix->filter_cand_cap ? std::max(ix->filter_cand_cap, exp) : std::max<size_t>(4 * exp, 256);
        cap = std::min(cap, (kFilteredLds - base) / 16);
        if(ix->filter_cand_cap && cap < std::max(ix->filter_cand_cap, exp)) {
            set_err(ix, "lantern_gpu: the candidate cap exceeds the 160 KiB LDS budget of the filtered search kernel");
            return false;
        }
        a.cand_cap = (uint32_t)cap;
        uint32_t vis_slots = 2048;
        while(vis_slots && filtered_walk_lds_bytes(ix->chunks, a.exp, a.cand_cap, ix->M0, vis_slots) > kFilteredLdsTarget)
            vis_slots = vis_slots > 256 ? vis_slots - 256 : 0;
        if(vis_slots && vis_slots < 4 * ix->M0) vis_slots = 0;
        a.frame.vis_slots = vis_slots;
        lds = filtered_walk_lds_bytes(ix->chunks, a.exp, a.cand_cap, ix->M0, vis_slots);
    }
    return true;
}

static const char *kNotAFilter = "lantern_gpu: not a filter handle (stale, freed or foreign pointer)";

// Why `f` cannot serve a search of `ix` as it stands now; empty: it can.
static std::string filter_mismatch(const Index *ix, const Filter *f)
{
    if(f->ix != ix)
        return "lantern_gpu: the filter belongs to another index (built over " + std::to_string(f->n) + " rows; this index holds " + std::to_string(ix->n) + ")";
    if(f->n != ix->n)
        return "lantern_gpu: stale filter: built when the index held " + std::to_string(f->n) + " rows, it now holds " + std::to_string(ix->n) +
               " (build the filter again)";
    return {};
}
// (checked after the filters)
static bool filtered_index_ok(Index *ix)
{
    if(ix->pq_compact) set_err(ix, "lantern_gpu: filtered search does not run on a compact pq index: expand it first (lantern_gpu_pq_expand)");
    return !ix->pq_compact;
}

// the path of a query under `f`: forced, or the rule of DESIGN.md 4.9 -- a walk under selectivity s evaluates about D / s rows, the
// exact pass `allowed`
static bool filter_takes_exact(const Index *ix, const Filter *f, size_t ef_sel)
{
    if(ix->filter_path) return ix->filter_path == 2;
    return (double)f->count * (double)f->count <= ix->filter_exact_factor * (double)ef_sel * (double)ix->n;
}

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
    return a;
}

// the per-query form's table of one launch: host bytes that go into the scratch of the launch's slot, and where in them the launch's
// descriptors and selection list lie
struct EachTable
{
    const char *host;
    size_t      bytes, descs_at, select_at;
};

// ONE launch of either kernel over a.frame.nq queries, `a` shaped by filtered_shape: the grid, the launch slot (which orders the launch
// after inserts and holds the walk's visited bitmaps), the per-query table if there is one, the ticket, the launch and its count.
// Returns the grid; < 0 -> ix->err.
static int filtered_launch(Index *ix, bool exact, FilteredArgs &a, size_t lds, hipStream_t stream, const EachTable *tbl = nullptr)
{
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, kFilteredLds / std::max<size_t>(lds, 1)));
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
    }
    a.frame.bitmaps = ix->slot_bitmaps[ slot ];
    a.frame.bm_words = (uint32_t)ix->slot_words[ slot ];
    a.frame.undo_cap = vis_undo_cap();
    a.frame.ticket = next_ticket(ix, a.frame.nq, grid, stream);
    const hipError_t e = exact ? launch_search_exact_allowed(ix->mcode, a, kFilteredWaves, grid, stream)
                               : launch_search_filtered(ix->mcode, a, kFilteredWaves, grid, stream);
    if(e != hipSuccess) {
        set_err(ix, std::string("lantern_gpu: HIP error launching the filtered search: ") + hipGetErrorString(e));
        return -1;
    }
    if(!release_search_slot(ix, slot, stream)) return -1;
    (exact ? ix->c_filter_exact : ix->c_filter_walk) += 1;
    return grid;
}

// The caller holds ix->mu and has flushed.  false -> ix->err.
static bool filtered_search_locked(Index *ix, const Filter *f, const uint4 *d_q, size_t nq, size_t k, size_t ef, size_t skip, const SearchOut &out,
                                   hipStream_t stream)
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
        if(out.labels && hipMemsetAsync(out.labels, 0, nq * k * 8, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
        if(out.dists && hipMemsetD32Async((hipDeviceptr_t)out.dists, 0x7F800000, nq * k, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
        if(out.slots && hipMemsetAsync(out.slots, 0xFF, nq * k * 4, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
        if(out.counts && hipMemsetAsync(out.counts, 0, nq * 4, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
        if(out.D && hipMemsetAsync(out.D, 0, nq * 8, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
        if(out.E && hipMemsetAsync(out.E, 0, nq * 8, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
        return true;
    }
    const bool   exact = filter_takes_exact(ix, f, ef_sel);
    FilteredArgs a = filtered_args(ix, d_q, k, skip, out);
    a.frame.nq = (uint32_t)nq;
    a.allow_bits = f->d_bits;
    a.allow_slots = f->d_slots;
    a.allow_count = (uint32_t)f->count;
    size_t lds = 0;
    if(!filtered_shape(ix, exact, k, skip, exp, a, lds)) return false;
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

// ---- the per-query form: filters[i] is query i's filter ------------------------------------------------------------------------
// bytes of the host block filtered_each_locked stages its selection lists and descriptor table in
static size_t each_table_bytes(size_t nq) { return nq * (sizeof(FilterDesc) + 4) + 16; }

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

// The caller holds ix->mu and has flushed.  The queries split into a walk group and an exact group by the path rule, evaluated per
// query from its own filter's count; each group is ONE launch over its own selection list, and every answer lands in the caller's
// row of its query.  Empty filters have no path: they ride in the exact launch (or, when nothing else takes the exact path, in the
// walk launch), where a descriptor with count 0 gives the empty answer without touching a row.
// `h_tbl`: a page-locked block of each_table_bytes(nq) that stays untouched until the stream work is done, or NULL (pageable
// staging: the copies then complete before this returns).  false -> ix->err; nothing has been launched unless the failure is HIP's.
static bool filtered_each_locked(Index *ix, const Filter *const *filters, const uint4 *d_q, size_t nq, size_t k, size_t ef, size_t skip,
                                 const SearchOut &out, hipStream_t stream, char *h_tbl)
{
    if(!each_filters_ok(ix, filters, nq)) return false;
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
    // the exact group's queries differ in length by orders of magnitude: longest first, so that the launch's tail is a short one
    std::stable_sort(exact.begin(), exact.end(), [&](uint32_t x, uint32_t y) { return filters[ x ]->count > filters[ y ]->count; });
    std::vector<uint32_t> &host = (exact.empty() && !walk.empty()) ? walk : exact;
    host.insert(host.end(), empty.begin(), empty.end());
    std::vector<const Filter *> distinct;
    for(size_t i = 0; i < nq; ++i)
        if(filters[ i ]) distinct.push_back(filters[ i ]);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());

    const FilteredArgs base = filtered_args(ix, d_q, k, skip, out);
    FilteredArgs aw = base, ae = base;
    aw.seeds = (uint32_t)ix->filter_seeds;  // (an unfiltered entry has no slot list: it runs the unseeded walk in the same launch)
    size_t       lds_w = 0, lds_e = 0;
    if(!walk.empty() && !filtered_shape(ix, false, k, skip, exp, aw, lds_w)) return false;
    if(!exact.empty() && !filtered_shape(ix, true, k, skip, exp, ae, lds_e)) return false;

    // the host block: walk selection list | descriptor table (by query) | exact selection list -- each launch copies its list and
    // the table in one piece into the scratch of its own launch slot
    const size_t off_desc = ((size_t)walk.size() * 4 + 7) & ~(size_t)7, off_sel_e = off_desc + nq * sizeof(FilterDesc);
    const size_t tbl_bytes = off_sel_e + exact.size() * 4;
    std::vector<char> pageable;
    if(!h_tbl) { pageable.resize(tbl_bytes); h_tbl = pageable.data(); }
    if(!walk.empty()) std::memcpy(h_tbl, walk.data(), walk.size() * 4);
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
        const EachTable t = ex ? EachTable{ h_tbl + off_desc, tbl_bytes - off_desc, 0, nq * sizeof(FilterDesc) } : EachTable{ h_tbl, off_sel_e, off_desc, 0 };
        if(filtered_launch(ix, ex, a, ex ? lds_e : lds_w, stream, &t) < 0) return false;
        launches += 1;
    }
    const uint32_t shape[ 6 ] = { n_walk, n_exact, n_unfiltered, n_empty, (uint32_t)distinct.size(), launches };
    std::copy(std::begin(shape), std::end(shape), ix->last_each);
    const uint32_t n_seeded = ix->filter_seeds ? n_walk - n_unfiltered : 0u;
    ix->last_seeds[ 2 ] = n_seeded;
    ix->last_seeds[ 3 ] = n_walk - n_seeded;
    ix->c_search_queries += nq;
    return true;
}

// one query through `cur` (streaming: never a row twice): the first k allowed rows not handed out before
static size_t cursor_search_filtered_locked(Index *ix, const Filter *f, Cursor *cur, const void *query, int kind, size_t k, size_t ef, bool streaming,
                                            uint64_t *labels, float *distances)
{
    if(!streaming) cur->seen.clear();
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
                [ & ] { return filtered_search_locked(ix, f, (const uint4 *)d_queries, nq, k, ef, skip, out, (hipStream_t)stream); }, e);
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
                   [ = ](const HostBatch &b) { return filtered_search_locked(ix, f, (const uint4 *)b.d_q, nq, k, ef, 0, b.out(b.d_out), b.stream); }, labels,
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
        return filtered_each_locked(ix, (const Filter *const *)filters, (const uint4 *)d_queries, nq, k, ef, skip, out, (hipStream_t)stream, nullptr);
    }, e);
}
LANTERN_ABI_CATCH_VOID(e)

// the filter check and the launch of the per-query host forms, of either host trip (the tables go into the staging block's extra area)
static auto each_validate(const lantern_gpu_filter_t *const *filters, size_t nq)
{
    return [ = ](Index *ix) { return each_filters_ok(ix, (const Filter *const *)filters, nq); };
}
static auto each_launch(Index *ix, const lantern_gpu_filter_t *const *filters, size_t nq, size_t k, size_t ef)
{
    return [ = ](const HostBatch &b) {
        return filtered_each_locked(ix, (const Filter *const *)filters, (const uint4 *)b.d_q, nq, k, ef, 0, b.out(b.d_out), b.stream, b.h_extra());
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
    host_trip_sync(ix, nq, k, each_table_bytes(nq), queries, (int)kind, kFilteredBatchFailed, each_validate(filters, nq), each_launch(ix, filters, nq, k, ef),
                   labels, distances, counts, e);
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
                   each_launch(ix, filters, nq, k, ef), labels, distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

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
