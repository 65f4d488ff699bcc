// insert_frame.hpp -- what a persistent insertion workgroup does AROUND one new vector's walk, once: bind the workgroup's visited
// bitmap and undo log (insert_bind), stage the stored row as the "query" and empty the node's levels (insert_stage), publish a
// level's result and pick the next level's start (insert_publish_level), and close the vector: the totals and the next batch
// member (insert_close).  The walk between them is the kernel's own: k_insert (insert_kernel.hip) and k_insert_spec
// (insert_spec_kernel.hip) call the pieces in this order and keep their carve_* calls, their descent, only_upper and their choice
// of level walk.  Two parts of the build's determinism contract live here and nowhere else: the tie rule for the next level's
// start, and which levels stay empty.
// As in query_frame.hpp, the pieces that loop over the workgroup's threads take the kernel's own tid = threadIdx.x and
// T = blockDim.x.  The register tables of both units are the ones the kernels had with the frame written out in each
// (profiles/insert_frame_kernel_resources.md).
#pragma once
#include "kernels.hpp"
#include "walk.hpp"

namespace lgpu {

// Bind: the workgroup's slab of InsertArgs::bitmaps -- its visited bitmap (returned; a.bm_words words) and, behind it, its undo log
__device__ __forceinline__ uint32_t *insert_bind(const InsertArgs &a, WalkLds &s)
{
    uint32_t *bitmap = vis_slab(a.bitmaps, a.bm_words);
    s.undo = bitmap + a.bm_words;
    s.undo_cap = a.undo_cap;
    return bitmap;
}

// Stage: the stored row `me` into s.q with its cached norm, and the node's levels [0, target] emptied.  SCREEN (k_insert's screened
// instantiations; walk.hpp S_SCREEN): the screen's tables, and this vector's counts, live in LDS.  The caller's barrier follows.
template <int METRIC, bool SCREEN = false>
__device__ __forceinline__ void insert_stage(const int tid, const int T, const InsertArgs &a, WalkLds &s, uint32_t me, uint32_t item0, int target, uint32_t chunks)
{
    const uint4 *own = row_of(a.view, me);
    for(uint32_t i = tid; i < chunks; i += T) s.q[ i ] = own[ i ];
    for(uint32_t i = tid; i <= (uint32_t)target; i += T) a.top_count[ item0 + i ] = 0;  // levels above max_level stay empty
    if(tid == 0) s.scal[ S_QN2 ] = __float_as_int(row_norm<METRIC>(a.view, me));     // the "query" is a stored row
    if constexpr(SCREEN) {
        if(tid == 0) {
            uint64_t *const sp = (uint64_t *)&s.scal[ S_SCREEN ];
            sp[ 0 ] = (uint64_t)a.view.screen;
            sp[ 1 ] = (uint64_t)a.view.screen_meta;
            s.scal[ S_NREJ ] = 0;
            s.scal[ S_NTEST ] = 0;
        }
    }
}

// Publish level: the cnt sorted keys of s.keys into the item's row of a.tops, its count, and the start of the next lower level --
// connect_new_node_'s first pick, the closest result under (distance, tie_mix) -- returned to every thread through S_CUR
__device__ __forceinline__ uint32_t insert_publish_level(const int tid, const int T, const InsertArgs &a, WalkLds &s, uint32_t me, uint32_t item, int cnt)
{
    uint64_t *top = a.tops + (size_t)item * a.efc;
    for(int i = tid; i < cnt; i += T) top[ i ] = s.keys[ i ] & ~1ull;  // drop the "expanded" bit
    if(tid == 0) {
        a.top_count[ item ] = (uint32_t)cnt;
        // sel[0] of the heuristic = minimum by (distance, tie_mix(slot, me)): only an exact tie at the
        // smallest distance can differ from keys[0]
        const uint32_t d0 = (uint32_t)(s.keys[ 0 ] >> 32);
        uint32_t       best = key_slot(s.keys[ 0 ]);
        for(int i = 1; i < cnt && (uint32_t)(s.keys[ i ] >> 32) == d0; ++i) {
            const uint32_t id = key_slot(s.keys[ i ]);
            if(tie_mix(id, me) < tie_mix(best, me)) best = id;
        }
        s.scal[ S_CUR ] = (int)best;
    }
    __syncthreads();
    const uint32_t cur = (uint32_t)s.scal[ S_CUR ];
    __syncthreads();
    return cur;
}

// Close: D and E into the totals (SCREEN: and the rows tested and rejected, kInsertScreenTotals on), then the batch member after b,
// by ticket or by stride, returned to every thread through S_POS
template <bool SCREEN = false>
__device__ __forceinline__ uint32_t insert_close(const int tid, const InsertArgs &a, WalkLds &s, uint32_t b, uint32_t D, uint32_t E)
{
    if(tid == 0) {
        if(a.totals) {
            atomicAdd(&a.totals[ 0 ], (unsigned long long)D);
            atomicAdd(&a.totals[ 1 ], (unsigned long long)E);
            if constexpr(SCREEN) {
                atomicAdd(&a.totals[ kInsertScreenTotals ], (unsigned long long)(uint32_t)s.scal[ S_NTEST ]);
                atomicAdd(&a.totals[ kInsertScreenTotals + 1 ], (unsigned long long)(uint32_t)s.scal[ S_NREJ ]);
            }
        }
        s.scal[ S_POS ] = a.ticket ? (int)(a.b_begin + gridDim.x + atomicAdd(a.ticket, 1u)) : (int)(b + gridDim.x);
    }
    __syncthreads();
    b = (uint32_t)s.scal[ S_POS ];
    __syncthreads();
    return b;
}

}  // namespace lgpu
