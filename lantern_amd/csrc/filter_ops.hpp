// filter_ops.hpp -- a filter's life cycle on the device (filter_ops.hip): the ascending slot list of a bitmap, the word-wise combination
// of two bitmaps, and a bitmap extended to the index's new size.  filter.hip owns the handles and the entry points; semantics:
// include/lantern_gpu.h "Filtered search" and DESIGN.md 4.9 "Filter life cycle".
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace lgpu {

// Is `l` among sorted[0 .. m) (ascending)?  The membership test of every kernel that builds a bitmap from labels.
__device__ inline bool label_in_sorted(const uint64_t *sorted, size_t m, uint64_t l)
{
    size_t lo = 0, hi = m;
    while(lo < hi) {
        const size_t mid = (lo + hi) >> 1;
        if(sorted[ mid ] < l) lo = mid + 1; else hi = mid;
    }
    return lo < m && sorted[ lo ] == l;
}

constexpr int    kFilterListThreads = 256;                      // a workgroup of the list kernels: one bitmap word per thread
constexpr size_t kFilterListSpan = kFilterListThreads * 32;     // ... so it covers this many slots

// ---- bitmap -> ascending slot list, in two steps around the one allocation whose size only the count gives -----------------------
// where the steps keep their intermediate results in ONE block of device scratch: counts[groups] | offsets[groups] | total (8 bytes) |
// the scan's temporary storage.  Computed once per build (filter_list_plan) and handed to both steps.
struct FilterListPlan
{
    size_t groups = 0;  // workgroups of the list kernels: ceil(words / kFilterListThreads)
    size_t offsets_at = 0, total_at = 0, temp_at = 0, temp_bytes = 0;
    size_t bytes = 0;  // of the block
};
hipError_t filter_list_plan(size_t words, FilterListPlan &plan);
// Step 1: the workgroups' popcounts, their exclusive scan and the total, queued on `stream`; the total crosses to *count (one
// 8-byte copy) and the stream has been waited for when this returns.  d_scratch: plan.bytes.
hipError_t filter_list_count(const uint32_t *d_bits, size_t words, const FilterListPlan &plan, void *d_scratch, size_t *count, hipStream_t stream);
// Step 2: d_slots[0 .. count) = the set bits' slots, ascending (queued; `d_scratch` as step 1 left it).
hipError_t filter_list_write(const uint32_t *d_bits, size_t words, const FilterListPlan &plan, const void *d_scratch, uint32_t *d_slots, size_t count,
                             hipStream_t stream);

// out[w] = a[w] op b[w] for w < words, bits at or past n cleared.  op: LANTERN_GPU_FILTER_AND / _OR / _ANDNOT.
hipError_t launch_filter_combine(const uint32_t *a, const uint32_t *b, int op, size_t n, uint32_t *out, size_t words, hipStream_t stream);

// bits[0 .. words): the old bitmap (old_words words over n_old slots) below n_old; a slot in [n_old, n_new) is set iff (all_new or its
// label is in sorted[0 .. m)) and not (skip_deleted and its label is 0); zero from n_new on.
hipError_t launch_filter_extend(const uint64_t *slot_labels, size_t n_old, size_t n_new, const uint64_t *sorted, size_t m, int all_new, int skip_deleted,
                                const uint32_t *old_bits, size_t old_words, uint32_t *bits, size_t words, hipStream_t stream);

}  // namespace lgpu
