// query_frame.hpp -- what a persistent search workgroup does AROUND one query, once: take a ticket position and turn it into a query
// (frame_query), stage the query row and its norm in LDS (frame_stage), bind the workgroup's visited bitmap and undo log (frame_bind),
// write the answer rows (frame_answer_rows), and close the query: count, D, E, the totals, the next ticket, the host-visible done
// words (frame_close).  The walk between them is the kernel's own: k_search (search_kernel.hpp), k_search_adc
// (search_adc_kernel.hip), k_search_filtered and k_search_exact_allowed (search_filtered_kernel.hip) call the pieces in this order;
// k_screen_probe (screen_probe_kernel.hip) stages its query with frame_stage.  The fields the pieces read are FrameArgs
// (kernels.hpp), embedded as `frame` in SearchArgs and FilteredArgs: a piece is written against `ARGS::frame` and reads it where
// the kernel's argument struct has it.
#pragma once
#include <cstddef>
#include <type_traits>

#include "kernels.hpp"
#include "walk.hpp"

namespace lgpu {

// ---------------------------------------------------------------------------------------------------
// Kernel arguments are RE-READ from the kernarg segment at the two points of a query that need them (before the walk: the
// view, the query pointer, ef; after it: the output pointers) through a pointer the compiler cannot see through.  Left to
// itself it loads all ~45 argument dwords once and keeps them live across the persistent loop -- over the hop loop, which
// already needs ~60 scalars -- and pays with ~60 scalar-register spill reloads per hop; a dozen scalar loads per QUERY are free.
// So every piece below takes the kernarg pointer its caller made AT THAT POINT (kernarg_opaque(), never hoisted above the walk)
// and loads what it needs from it there.  The pieces that loop over the workgroup's threads take the kernel's own tid = threadIdx.x
// and T = blockDim.x: read again inside a piece, they cost k_search<M_L2SQ_F16, 64> three more spilled VGPRs
// (profiles/query_frame_kernel_resources.md).
typedef const __attribute__((address_space(4))) unsigned char *KernargBytes;
__device__ __forceinline__ KernargBytes kernarg_opaque()
{
    KernargBytes p = (KernargBytes)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
#define LGPU_KARG(base, T, ...) (*(const __attribute__((address_space(4))) T *)((base) + (__VA_ARGS__)))
#define LGPU_FRAME_ARG(base, ARGS, field) LGPU_KARG(base, decltype(FrameArgs::field), offsetof(ARGS, frame) + offsetof(FrameArgs, field))

typedef const __attribute__((address_space(4))) uint32_t *ConstWords;

// Pick: the query a workgroup serves at ticket position `pos`: pos itself, or -- LIST, the launches that serve a list of queries --
// the entry of FrameArgs::qlist (pos comes out of LDS: made wave-uniform, the list entry is a scalar load).  Rows are written by
// the query, the next position is drawn after pos.
template <class ARGS, bool LIST> __device__ __forceinline__ uint32_t frame_query(KernargBytes ka, uint32_t pos)
{
    if constexpr(LIST) {
        const uint32_t upos = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos);
        return ((ConstWords)(uintptr_t)LGPU_FRAME_ARG(ka, ARGS, qlist))[ upos ];
    } else {
        return pos;
    }
}

// Stage: the query row into s.q, and ||query||^2 once per query for the metrics that cache norms, by the chain Acc<M_COS> would
// run for every row
template <int METRIC, int G> __device__ __forceinline__ void frame_stage(const int tid, const int T, WalkLds &s, const uint4 *queries, uint32_t q, uint32_t chunks)
{
    for(uint32_t i = tid; i < chunks; i += T) s.q[ i ] = queries[ (size_t)q * chunks + i ];
    __syncthreads();
    if(kCachedNorms<METRIC>) {
        if(tid < G) {
            const float qn = group_norm<METRIC, G>(s.q, (int)chunks, tid);
            if(tid == G - 1) s.scal[ S_QN2 ] = __float_as_int(qn);
        }
        __syncthreads();
    }
}

// Bind: the workgroup's slab of FrameArgs::bitmaps -- its visited bitmap (returned; bm_words words) and, behind it, its undo log
template <class ARGS> __device__ __forceinline__ uint32_t *frame_bind(KernargBytes ka, WalkLds &s, uint32_t &bm_words)
{
    bm_words = LGPU_FRAME_ARG(ka, ARGS, bm_words);
    uint32_t *bitmap = vis_slab(LGPU_FRAME_ARG(ka, ARGS, bitmaps), bm_words);
    s.undo = bitmap + bm_words;
    s.undo_cap = LGPU_FRAME_ARG(ka, ARGS, undo_cap);
    return bitmap;
}

// Answer rows: keys[skip, skip + k) of the cnt keys in s.keys into query q's rows, kw wide, the unused tail label 0 / +inf / EMPTY.
// Returns how many rows the query got.
template <class ARGS> __device__ __forceinline__ int frame_answer_rows(const int tid, const int T, KernargBytes kb, const WalkLds &s, uint32_t q, int cnt, uint32_t k, uint32_t skip, uint32_t kw)
{
    const uint64_t *labels = LGPU_FRAME_ARG(kb, ARGS, labels);
    uint64_t       *out_labels = LGPU_FRAME_ARG(kb, ARGS, out_labels);
    float          *out_dists = LGPU_FRAME_ARG(kb, ARGS, out_dists);
    uint32_t       *out_slots = LGPU_FRAME_ARG(kb, ARGS, out_slots);
    int             got = cnt - (int)skip;
    got = got < 0 ? 0 : (got > (int)k ? (int)k : got);
    for(uint32_t i = tid; i < kw; i += T) {
        const size_t o = (size_t)q * kw + i;
        if((int)i < got) {
            const uint64_t key = s.keys[ skip + i ];
            const uint32_t slot = key_slot(key);
            if(out_labels) out_labels[ o ] = labels[ slot ];
            if(out_dists) out_dists[ o ] = key_dist(key);
            if(out_slots) out_slots[ o ] = slot;
        } else {
            if(out_labels) out_labels[ o ] = 0;  // INVALID_ELEMENT_LABEL (hnsw.h:40)
            if(out_dists) out_dists[ o ] = __builtin_inff();
            if(out_slots) out_slots[ o ] = EMPTY;
        }
    }
    return got;
}

// the host-visible done words exist where the argument struct has them: members `done` and `done_flags` (SearchArgs)
template <class ARGS, class = void> struct HasDoneWords : std::false_type {};
template <class ARGS> struct HasDoneWords<ARGS, std::void_t<decltype(ARGS::done), decltype(ARGS::done_flags)>> : std::true_type {};
template <class ARGS> constexpr bool kHasDoneWords = HasDoneWords<ARGS>::value;

// Close: query q's count, D and E, the launch's totals, the next ticket position (returned to every thread through S_POS), the done
// words.  SCREEN_TOTALS (k_search's screened instantiations): ARGS::screen_totals takes D and the rows the screen let through.
template <class ARGS, bool SCREEN_TOTALS = false>
__device__ __forceinline__ uint32_t frame_close(const int tid, KernargBytes kb, WalkLds &s, uint32_t q, uint32_t pos, int got, uint32_t D, uint32_t E)
{
    if(tid == 0) {
        uint32_t *const           out_counts = LGPU_FRAME_ARG(kb, ARGS, out_counts);
        uint64_t *const           out_D = LGPU_FRAME_ARG(kb, ARGS, out_D), *const out_E = LGPU_FRAME_ARG(kb, ARGS, out_E);
        unsigned long long *const totals = LGPU_FRAME_ARG(kb, ARGS, totals);
        uint32_t *const           ticket = LGPU_FRAME_ARG(kb, ARGS, ticket);
        if(out_counts) out_counts[ q ] = (uint32_t)got;
        if(out_D) out_D[ q ] = D;
        if(out_E) out_E[ q ] = E;
        if(totals) { atomicAdd(&totals[ 0 ], (unsigned long long)D); atomicAdd(&totals[ 1 ], (unsigned long long)E); }
        if constexpr(SCREEN_TOTALS) {
            unsigned long long *const st = LGPU_KARG(kb, decltype(ARGS::screen_totals), offsetof(ARGS, screen_totals));
            if(st) { atomicAdd(&st[ 0 ], (unsigned long long)D); atomicAdd(&st[ 1 ], (unsigned long long)(D - (uint32_t)s.scal[ S_NREJ ])); }
        }
        // next query: a ticket (walks differ in length by 2x; static striding leaves workgroups idle at the end)
        s.scal[ S_POS ] = ticket ? (int)(gridDim.x + atomicAdd(ticket, 1u)) : (int)(pos + gridDim.x);
    }
    __syncthreads();
    if constexpr(kHasDoneWords<ARGS>) {
        if(tid == 0) {
            // a host that waits on this counter instead of on the stream (the lone-query path: index.cpp search_one_locked)
            // sees this query's answers first: they were written before the barrier above, and the fence orders them
            uint32_t *const done = LGPU_KARG(kb, decltype(ARGS::done), offsetof(ARGS, done));
            uint32_t *const done_flags = LGPU_KARG(kb, decltype(ARGS::done_flags), offsetof(ARGS, done_flags));
            if(done || done_flags) __threadfence_system();
            if(done) __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            if(done_flags) __hip_atomic_store(&done_flags[ q ], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    pos = (uint32_t)s.scal[ S_POS ];
    __syncthreads();
    return pos;
}

}  // namespace lgpu
