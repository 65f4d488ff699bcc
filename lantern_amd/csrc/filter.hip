// filter.hip -- the filter objects of filtered k-NN search: building an allow-set over an index's slots, extending and combining one,
// the handle checks every filtered entry point makes, and the life-cycle entry points (include/lantern_gpu.h "Filtered search";
// semantics: DESIGN.md 4.9).  The plan of a filtered call is filtered_plan.cpp's, its launches filtered_search.cpp's.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "abi_guard.hpp"
#include "filter_ops.hpp"
#include "filtered_search.hpp"

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

// ---- the handle checks -------------------------------------------------------------------------------------------------------------
const char *const kNotAFilter = "lantern_gpu: not a filter handle (stale, freed or foreign pointer)";

std::string filter_mismatch(const Index *ix, const Filter *f)
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

Filter *FF(const lantern_gpu_filter_t *f, usearch_error_t *e)
{
    if(!f) { FAIL(e, "lantern_gpu: null filter handle"); return nullptr; }
    if(((const Filter *)f)->magic != kFilterMagic) { FAIL(e, kNotAFilter); return nullptr; }
    return (Filter *)f;
}

}  // namespace lgpu

// =====================================================================================================
// C ABI
// =====================================================================================================
using namespace lgpu;

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

}  // extern "C"
