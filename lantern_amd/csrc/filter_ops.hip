// filter_ops.hip -- the device passes of a filter's life cycle (filter_ops.hpp; DESIGN.md 4.9 "Filter life cycle"): the ascending slot
// list of a bitmap (k_filter_list_count, one exclusive scan, k_filter_list_write), two bitmaps combined word by word
// (k_filter_combine), and a bitmap extended to the index's new size (k_filter_extend).  64-lane waves; every store is a vector store.
#include <rocprim/device/device_scan.hpp>

#include "../../include/lantern_gpu.h"
#include "filter_ops.hpp"

namespace lgpu {

constexpr int kListWaves = kFilterListThreads / 64;

// the inclusive sum of v over the lanes [0, lane] of a 64-lane wave (every lane of the wave calls it)
__device__ inline uint32_t wave_inclusive_sum(uint32_t v, int lane)
{
    for(int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if(lane >= d) v += up;
    }
    return v;
}

// Pass 1: counts[g] = the set bits of workgroup g's words (one word per thread), and their sum over the grid added to *total
__global__ void __launch_bounds__(kFilterListThreads) k_filter_list_count(const uint32_t *bits, size_t words, uint32_t *counts, unsigned long long *total)
{
    __shared__ uint32_t wave_sum[ kListWaves ];
    const size_t   w = (size_t)blockIdx.x * kFilterListThreads + threadIdx.x;
    const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_sum(w < words ? (uint32_t)__popc(bits[ w ]) : 0u, lane);
    if(lane == 63) wave_sum[ wave ] = incl;
    __syncthreads();
    if(threadIdx.x == 0) {
        uint32_t c = 0;
        for(int i = 0; i < kListWaves; ++i) c += wave_sum[ i ];
        counts[ blockIdx.x ] = c;
        if(c) atomicAdd(total, (unsigned long long)c);
    }
}

// Pass 2: the slots of every thread's word, ascending, at offsets[workgroup] + the set bits of the workgroup's words in front of it
// (the waves in front through LDS, the lanes in front by the wave's prefix).  Nothing is written at or past `count`.
__global__ void __launch_bounds__(kFilterListThreads) k_filter_list_write(const uint32_t *bits, size_t words, const uint32_t *offsets, uint32_t *slots, size_t count)
{
    __shared__ uint32_t wave_sum[ kListWaves ];
    const size_t   w = (size_t)blockIdx.x * kFilterListThreads + threadIdx.x;
    const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t word = w < words ? bits[ w ] : 0u, mine = (uint32_t)__popc(word);
    const uint32_t incl = wave_inclusive_sum(mine, lane);
    if(lane == 63) wave_sum[ wave ] = incl;
    __syncthreads();
    size_t at = (size_t)offsets[ blockIdx.x ] + (incl - mine);
    for(int i = 0; i < wave; ++i) at += wave_sum[ i ];
    for(uint32_t x = word; x && at < count; x &= x - 1, ++at) slots[ at ] = (uint32_t)(w * 32 + (size_t)__builtin_ctz(x));
}

// the bits of word w that lie below n
__device__ inline uint32_t bits_below(size_t w, size_t n)
{
    const size_t first = w * 32;
    return first + 32 <= n ? 0xFFFFFFFFu : first >= n ? 0u : (1u << (uint32_t)(n - first)) - 1u;
}

__global__ void __launch_bounds__(256) k_filter_combine(const uint32_t *a, const uint32_t *b, int op, size_t n, uint32_t *out, size_t words)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(w >= words) return;
    const uint32_t x = a[ w ], y = b[ w ];
    const uint32_t r = op == LANTERN_GPU_FILTER_AND ? x & y : op == LANTERN_GPU_FILTER_OR ? x | y : x & ~y;
    out[ w ] = r & bits_below(w, n);
}

// one thread per word of the new bitmap: a word wholly below n_old is the old one; the others keep the old word's bits below n_old
// and take the slots [n_old, n_new) by the rule of k_filter_from_labels (filter.hip)
__global__ void __launch_bounds__(256) k_filter_extend(const uint64_t *slot_labels, size_t n_old, size_t n_new, const uint64_t *sorted, size_t m, int all_new,
                                                       int skip_deleted, const uint32_t *old_bits, size_t old_words, uint32_t *bits, size_t words)
{
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(w >= words) return;
    uint32_t word = w < old_words ? old_bits[ w ] & bits_below(w, n_old) : 0u;
    if(w * 32 + 32 <= n_old) { bits[ w ] = word; return; }
    for(uint32_t b = 0; b < 32; ++b) {
        const size_t slot = w * 32 + b;
        if(slot < n_old) continue;
        if(slot >= n_new) break;
        const uint64_t l = slot_labels[ slot ];
        if(skip_deleted && l == 0) continue;
        if(all_new || label_in_sorted(sorted, m, l)) word |= 1u << b;
    }
    bits[ w ] = word;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
static size_t list_groups(size_t words) { return (words + kFilterListThreads - 1) / kFilterListThreads; }
static size_t up(size_t x, size_t a) { return (x + a - 1) / a * a; }

hipError_t filter_list_plan(size_t words, FilterListPlan &s)
{
    s = FilterListPlan{};
    s.groups = list_groups(words);
    if(!s.groups) return hipSuccess;
    s.offsets_at = s.groups * 4;
    s.total_at = up(2 * s.groups * 4, 8);
    s.temp_at = up(s.total_at + 8, 256);
    const hipError_t e = rocprim::exclusive_scan(nullptr, s.temp_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, s.groups, rocprim::plus<uint32_t>(), (hipStream_t)0);
    s.bytes = s.temp_at + (s.temp_bytes > 16 ? s.temp_bytes : 16);
    return e;
}

hipError_t filter_list_count(const uint32_t *d_bits, size_t words, const FilterListPlan &s, void *d_scratch, size_t *count, hipStream_t stream)
{
    *count = 0;
    if(!s.groups) return hipSuccess;
    char *const               blk = (char *)d_scratch;
    uint32_t *const           counts = (uint32_t *)blk, *offsets = (uint32_t *)(blk + s.offsets_at);
    unsigned long long *const total = (unsigned long long *)(blk + s.total_at);
    hipError_t                e;
    if((e = hipMemsetAsync(total, 0, 8, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_filter_list_count, dim3((uint32_t)s.groups), dim3(kFilterListThreads), 0, stream, d_bits, words, counts, total);
    if((e = hipGetLastError()) != hipSuccess) return e;
    size_t temp_bytes = s.temp_bytes;
    if((e = rocprim::exclusive_scan((void *)(blk + s.temp_at), temp_bytes, (const uint32_t *)counts, offsets, 0u, s.groups, rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
    unsigned long long h_total = 0;
    if((e = hipMemcpyAsync(&h_total, total, 8, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    *count = (size_t)h_total;
    return hipSuccess;
}

hipError_t filter_list_write(const uint32_t *d_bits, size_t words, const FilterListPlan &s, const void *d_scratch, uint32_t *d_slots, size_t count, hipStream_t stream)
{
    if(!s.groups || !count) return hipSuccess;
    const uint32_t *offsets = (const uint32_t *)((const char *)d_scratch + s.offsets_at);
    hipLaunchKernelGGL(k_filter_list_write, dim3((uint32_t)s.groups), dim3(kFilterListThreads), 0, stream, d_bits, words, offsets, d_slots, count);
    return hipGetLastError();
}

hipError_t launch_filter_combine(const uint32_t *a, const uint32_t *b, int op, size_t n, uint32_t *out, size_t words, hipStream_t stream)
{
    if(!words) return hipSuccess;
    hipLaunchKernelGGL(k_filter_combine, dim3((uint32_t)((words + 255) / 256)), dim3(256), 0, stream, a, b, op, n, out, words);
    return hipGetLastError();
}

hipError_t launch_filter_extend(const uint64_t *slot_labels, size_t n_old, size_t n_new, const uint64_t *sorted, size_t m, int all_new, int skip_deleted,
                                const uint32_t *old_bits, size_t old_words, uint32_t *bits, size_t words, hipStream_t stream)
{
    if(!words) return hipSuccess;
    hipLaunchKernelGGL(k_filter_extend, dim3((uint32_t)((words + 255) / 256)), dim3(256), 0, stream, slot_labels, n_old, n_new, sorted, m, all_new, skip_deleted,
                       old_bits, old_words, bits, words);
    return hipGetLastError();
}

}  // namespace lgpu
