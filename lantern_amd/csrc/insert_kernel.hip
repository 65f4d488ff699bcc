// insert_kernel.hip -- k_insert: the walk of usearch_add (build.c:128; server.rs:349 add_raw).  Per new vector: descent + a
// per-level ef_construction-wide walk (walk.hpp); the sorted results go to k_connect (kernels.hip).
#include <algorithm>
#include <cstdlib>

#ifndef LGPU_LIST_PREFETCH  // the insertion walks do not fetch the front's list ahead: measured -2 % on builds (profiles/r06_list_prefetch_ab.md)
#define LGPU_LIST_PREFETCH 0
#endif
#ifdef LGPU_INSERT_ROW_BLOCK_COS  // this translation unit's own block for the cosine row pairs (device_common.hpp LGPU_ROW_BLOCK_COS)
#define LGPU_ROW_BLOCK_COS LGPU_INSERT_ROW_BLOCK_COS
#endif
#include "kernels.hpp"
#include "walk.hpp"
#include "insert_frame.hpp"
#include "dispatch.hpp"

namespace lgpu {

// ---------------------------------------------------------------------------------------------------
// k_insert: the WALK half of an insertion.  Per new vector: descent to its level, then per level an
// ef_construction-wide search_level whose sorted result (<= efc keys) goes to HBM for k_connect.  What surrounds
// the walk -- staging, publishing a level, the next level's start, the totals, the next member -- is insert_frame.hpp.
// SCREEN (f32 l2sq / cosine rows of >= 128 chunks, the register list: launch_insert below): level 0 tests its candidates on the int8
// row copy first, as k_search does (walk.hpp hop_distances_screened); the launch has the planes' block behind its visited set.
template <int METRIC, int G, int KPL = 2, bool SCREEN = false>  // KPL: as k_search (keys per lane of wave 0's register list; 0 = LDS list)
#ifndef LGPU_INSERT_MIN_BLOCKS
#define LGPU_INSERT_MIN_BLOCKS 6  // (measured: 5 and 4 -- 81 / 90 registers, no spills -- build at the same speed; DESIGN_HISTORY.md H.2 item 1)
#endif
// [r6] the cosine walks are compiled for the FIVE workgroups per CU that k_insert's LDS lets run anyway (<= 96 VGPRs): with the blocked row
// loads they spill at 80 (48 bytes of scratch, reloads inside a hop) -- same-box A/B at 1M x 768: walk 742 -> 691 ms, 949 -> 993 k vectors/s;
// the other metrics measure the same or slower at five (profiles/r06_row_block_ab.jsonl, second table)
// The screened walks are compiled for five whatever the metric: k_insert's LDS (31 KB: insert_batch.cpp plan_insert) lets five workgroups share a
// CU anyway, and at six the l2sq form spills 21 / 24 VGPRs (80 / 92 bytes of scratch) against 3 / 8 (16 / 36 bytes) at five
#ifndef LGPU_INSERT_SCREEN_MIN_BLOCKS
#define LGPU_INSERT_SCREEN_MIN_BLOCKS 5
#endif
__global__ void __launch_bounds__(512, SCREEN ? LGPU_INSERT_SCREEN_MIN_BLOCKS : (METRIC % 100 == M_COS) ? 5 : LGPU_INSERT_MIN_BLOCKS) k_insert(InsertArgs a)
{
    static_assert(!SCREEN || ((METRIC == M_L2SQ || METRIC == M_COS) && G == 64 && KPL > 0), "the screen serves the f32 l2sq and cosine walks over rows of >= 128 chunks, list in registers");
    const int tid = threadIdx.x, T = blockDim.x;
    WalkLds   s;
    carve_walk(lgpu_smem, s, a.view.chunks, a.efc, a.view.M0, a.vis_slots);
    uint32_t *bitmap = insert_bind(a, s);
    const uint32_t chunks = a.view.chunks, M = a.view.M;
    for(uint32_t b = a.b_begin + blockIdx.x; b < a.count;) {
        const uint32_t me = a.first_slot + b;
        const int      target = a.view.levels[ me ];
        const uint32_t item0 = a.link_off[ b ] / M;  // one item per (node, level)
        insert_stage<METRIC, SCREEN>(tid, T, a, s, me, item0, target, chunks);
        __syncthreads();
        if constexpr(SCREEN) screen_stage_query<METRIC>(tid, s, chunks, __int_as_float(s.scal[ S_QN2 ]));  // (ends in a barrier)
        uint32_t D = 0, E = 0;
        const int lowest = a.only_upper ? 1 : 0;  // (block-uniform: a node of level 0 has nothing to walk then)
        uint32_t cur = target >= lowest ? greedy_descent<METRIC, G>(a.view, s, a.view.entry, a.view.max_level, target, D) : 0u;
        for(int level = target < a.view.max_level ? target : a.view.max_level; level >= lowest; --level) {
            int cnt;
            if constexpr(SCREEN) cnt = search_level_reg<METRIC, G, KPL, false, 2, true, true>(a.view, s, bitmap, a.bm_words, cur, level, (int)a.efc, D, E);
            else if constexpr(KPL > 0) cnt = search_level_reg<METRIC, G, KPL>(a.view, s, bitmap, a.bm_words, cur, level, (int)a.efc, D, E);
            else cnt = search_level<METRIC, G>(a.view, s, bitmap, a.bm_words, cur, level, (int)a.efc, D, E);
            cur = insert_publish_level(tid, T, a, s, me, item0 + (uint32_t)level, cnt);
        }
        b = insert_close<SCREEN>(tid, a, s, b, D, E);
    }
}

size_t insert_lds_bytes(uint32_t chunks, uint32_t efc, uint32_t M0, uint32_t vis_slots) { return walk_lds_bytes(chunks, efc, M0, vis_slots); }

hipError_t launch_insert(int metric, const InsertArgs &a, int waves, int grid, hipStream_t stream)
{
    // (a view with a screen: the launch screens -- insert_batch.cpp passes the screen only where plan_insert planned the planes' block)
    const bool   screened = a.view.screen != nullptr;
    const size_t lds = insert_lds_bytes(a.view.chunks, a.efc, a.view.M0, a.vis_slots) + (screened ? screen_query_lds_bytes(a.view.chunks) : 0);
    const int    kpl = a.lds_list ? 0 : a.efc <= 64 ? 1 : a.efc <= 128 ? 2 : 0;
#define LGPU_LAUNCH_INSERT(...) LGPU_LAUNCH_LDS((k_insert<__VA_ARGS__>), grid, 64 * waves, lds, stream, a)
#define CALL(MM, GG)                               \
    {                                              \
        if(kpl == 1) LGPU_LAUNCH_INSERT(MM, GG, 1) \
        else if(kpl == 2) LGPU_LAUNCH_INSERT(MM, GG, 2) \
        else LGPU_LAUNCH_INSERT(MM, GG, 0)         \
    }
    if(screened) {  // the four screened instantiations: f32 l2sq / cosine, 64 lanes per row, the register list, a split walk
        if(kpl == 0 || group_lanes_for(a.view.chunks) != 64 || waves < 2 || !a.view.screen_meta || a.only_upper) return hipErrorInvalidValue;
        if(metric == M_L2SQ && kpl == 1) LGPU_LAUNCH_INSERT(M_L2SQ, 64, 1, true)
        else if(metric == M_L2SQ) LGPU_LAUNCH_INSERT(M_L2SQ, 64, 2, true)
        else if(metric == M_COS && kpl == 1) LGPU_LAUNCH_INSERT(M_COS, 64, 1, true)
        else if(metric == M_COS) LGPU_LAUNCH_INSERT(M_COS, 64, 2, true)
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
    LGPU_DISPATCH(metric, a.view.chunks, CALL);
#undef CALL
#undef LGPU_LAUNCH_INSERT
    return hipGetLastError();
}

}  // namespace lgpu
