// search_kernel.hpp -- the k_search template (usearch_search_ef, lantern_hnsw/src/hnsw/scan.c:220-228, 273-281): one workgroup per
// query, persistent over the batch (work handed out by ticket); greedy descent + ef-bounded base-layer walk (walk.hpp,
// walk_spec.hpp).  Instantiated in two translation units that compile side by side: search_kernel.hip (the bandwidth-bound
// shapes) and search_spec_kernel.hip (the latency-bound ones).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>

#include "kernels.hpp"
#include "walk.hpp"
#include "walk_spec.hpp"
#include "dispatch.hpp"
#include "query_frame.hpp"

namespace lgpu {

// ---------------------------------------------------------------------------------------------------
// ROWS = 4 is the SMALL-BATCH shape: when the batch cannot fill six workgroups per CU anyway (<= four 4-wave workgroups per
// CU), every workgroup keeps four rows per group in flight instead of two and may use 128 VGPRs (four waves per SIMD): a
// CU's fetch rate is set by the bytes it has in flight, and at 1024 queries x 768-d the two-row shape left it at ~60 %.
// (Kernel arguments are re-read from the kernarg segment at the points of a query that need them: query_frame.hpp says why.)
#define LGPU_SEARCH_ARG(base, field) LGPU_KARG(base, decltype(SearchArgs::field), offsetof(SearchArgs, field))
#define LGPU_VIEW_ARG(base, STRUCT, field) LGPU_KARG(base, decltype(View::field), offsetof(STRUCT, view) + offsetof(View, field))
#define LGPU_LOAD_VIEW(v, base, STRUCT)             \
    {                                               \
        v.vec = LGPU_VIEW_ARG(base, STRUCT, vec);   \
        v.chunks = LGPU_VIEW_ARG(base, STRUCT, chunks); \
        v.M = LGPU_VIEW_ARG(base, STRUCT, M);       \
        v.M0 = LGPU_VIEW_ARG(base, STRUCT, M0);     \
        v.nbr0 = LGPU_VIEW_ARG(base, STRUCT, nbr0); \
        v.upper_off = LGPU_VIEW_ARG(base, STRUCT, upper_off); \
        v.upper_nbr = LGPU_VIEW_ARG(base, STRUCT, upper_nbr); \
        v.levels = LGPU_VIEW_ARG(base, STRUCT, levels); \
        v.norm2 = LGPU_VIEW_ARG(base, STRUCT, norm2); \
        v.n = LGPU_VIEW_ARG(base, STRUCT, n);       \
        v.entry = LGPU_VIEW_ARG(base, STRUCT, entry); \
        v.max_level = LGPU_VIEW_ARG(base, STRUCT, max_level); \
    }
// ... and the fields only the decode-on-the-fly metrics read
#define LGPU_LOAD_VIEW_PQD(v, base, STRUCT)                   \
    {                                                         \
        v.pq_centers = LGPU_VIEW_ARG(base, STRUCT, pq_centers); \
        v.pq_cps = LGPU_VIEW_ARG(base, STRUCT, pq_cps);       \
        v.pq_C = LGPU_VIEW_ARG(base, STRUCT, pq_C);           \
        v.pq_inv = LGPU_VIEW_ARG(base, STRUCT, pq_inv);       \
        v.pq_row_bytes = LGPU_VIEW_ARG(base, STRUCT, pq_row_bytes); \
    }

// a query's row of SearchArgs::qparams (wave-uniform: q came through the scalar cache, and so does the row)
struct QueryParams { uint32_t k, ef, skip; };
__device__ __forceinline__ QueryParams query_params(KernargBytes ka, uint32_t q)
{
    const ConstWords row = (ConstWords)(uintptr_t)LGPU_SEARCH_ARG(ka, qparams) + (size_t)q * 4;
    return QueryParams{ row[ 0 ], row[ 1 ], row[ 2 ] };
}

// SPEC: the latency-bound walk of walk_spec.hpp -- 1: every wave evaluates rows and waves 0..2 carry the roles on top (the
// small-batch shape, four waves); 2: three dedicated role waves + row waves (the lone-query shape, 3 + 8 waves).
// EACH: the per-query-parameter form (search_each_kernel.hip, search_each_spec_kernel.hip).  The launch serves the queries of a list
// (FrameArgs::qlist: the ticket hands out list positions, the answers land in the row of the query a position names) and every query
// brings its own k, expansion and skip in a 16-byte row {k, expansion, skip, 0} of SearchArgs::qparams, read through the scalar cache
// once the workgroup has its query.  The LDS carve is the launch's (SearchArgs::ef = the largest expansion of the list); the walk runs
// with the query's own expansion, the answer rows are k_stride wide.  k = 0: no walk, the empty answer.
template <int METRIC, int G, bool PROF = false, int ROWS = 2, int KPL = 1, int SPEC = 0, bool EACH = false>
#ifndef LGPU_SEARCH_MIN_BLOCKS_COS
#define LGPU_SEARCH_MIN_BLOCKS_COS 6
#endif
__global__ void __launch_bounds__(SPEC >= 2 ? 704 : 512, SPEC >= 2 ? 3 : (SPEC == 1 || ROWS != 2) ? 4 : (METRIC % 100 == M_COS) ? LGPU_SEARCH_MIN_BLOCKS_COS : 6)  // SPEC 0, ROWS 2: <= 80 VGPRs, six 4-wave workgroups per CU
k_search(SearchArgs)
{
    static_assert(!EACH || (!PROF && (SPEC == 0 || SPEC == 2)), "the per-query form exists for the classic shapes and the 3 + 8 wave shape");
    const int tid = threadIdx.x, T = blockDim.x;
    WalkLds   s;
    SpecLds   sc;
    {
        const KernargBytes ka = kernarg_opaque();
        unsigned char     *end = carve_walk(lgpu_smem, s, LGPU_VIEW_ARG(ka, SearchArgs, chunks), LGPU_SEARCH_ARG(ka, ef), LGPU_VIEW_ARG(ka, SearchArgs, M0),
                                            LGPU_FRAME_ARG(ka, SearchArgs, vis_slots));
        if constexpr(SPEC != 0) carve_spec(end, sc, LGPU_VIEW_ARG(ka, SearchArgs, M0), LGPU_SEARCH_ARG(ka, spec_prefetch), LGPU_SEARCH_ARG(ka, spec_cache));
        else (void)end;
    }
    // the int8 screen of the f32 l2sq and cosine walks over rows of >= 128 chunks (walk.hpp hop_distances_screened); used iff the view
    // has one
    constexpr bool SCREEN = LGPU_SCREEN && (METRIC == M_L2SQ || METRIC == M_COS) && G == 64 && !PROF && SPEC == 0 && KPL > 0;
    for(uint32_t pos = blockIdx.x; pos < LGPU_FRAME_ARG(kernarg_opaque(), SearchArgs, nq);) {
        uint32_t    q = pos;
        QueryParams each{};
        if constexpr(EACH) {
            const KernargBytes ka = kernarg_opaque();
            q = frame_query<SearchArgs, true>(ka, pos);
            each = query_params(ka, q);
        }
        uint32_t D = 0, E = 0;
        int      cnt = 0;
        unsigned long long pc[ 8 ] = { 0, 0, 0, 0, 0, 0, 0, 0 }, t_q = 0;
        {
            const KernargBytes ka = kernarg_opaque();
            View               v;
            LGPU_LOAD_VIEW(v, ka, SearchArgs)
            if constexpr(METRIC >= M_PQD) LGPU_LOAD_VIEW_PQD(v, ka, SearchArgs)
            if constexpr(SCREEN) {  // (walk.hpp S_SCREEN: the screen's tables, and the count of rows it rejects, live in LDS)
                if(tid == 0) {
                    uint64_t *const sp = (uint64_t *)&s.scal[ S_SCREEN ];
                    sp[ 0 ] = (uint64_t)LGPU_VIEW_ARG(ka, SearchArgs, screen);
                    sp[ 1 ] = (uint64_t)LGPU_VIEW_ARG(ka, SearchArgs, screen_meta);
                    s.scal[ S_NREJ ] = 0;
                }
            }
            uint32_t        bm_words;
            uint32_t *const bitmap = frame_bind<SearchArgs>(ka, s, bm_words);
            const int       ef = EACH ? (int)each.ef : (int)LGPU_SEARCH_ARG(ka, ef);
            frame_stage<METRIC, G>(tid, T, s, LGPU_FRAME_ARG(ka, SearchArgs, queries), q, v.chunks);
            if constexpr(SCREEN) {  // the query's int8 planes, where the launch carved their block: iff its view has a screen (search_plan.cpp)
                if(LGPU_VIEW_ARG(ka, SearchArgs, screen)) screen_stage_query<METRIC>(tid, s, v.chunks, __int_as_float(s.scal[ S_QN2 ]));
            }
            if constexpr(PROF) {
                t_q = (unsigned long long)clock64();
                s.touched = LGPU_SEARCH_ARG(ka, touched);
                s.trace_cap = LGPU_SEARCH_ARG(ka, trace_cap);
                uint32_t *const tr = LGPU_SEARCH_ARG(ka, trace);
                s.trace = tr ? tr + (size_t)q * s.trace_cap : nullptr;
                s.trace_count = tr ? LGPU_SEARCH_ARG(ka, trace_count) + q : nullptr;
            }
            if(v.n != 0 && (!EACH || each.k != 0)) {
                uint32_t start;
                if constexpr(SPEC != 0) start = greedy_descent_spec<METRIC, G>(v, s, v.entry, v.max_level, 0, D);
                else start = greedy_descent<METRIC, G, PROF, SCREEN>(v, s, v.entry, v.max_level, 0, D, SCREEN ? LGPU_SEARCH_ARG(ka, screen_descent) : 0u);
                if constexpr(PROF) pc[ 6 ] = (unsigned long long)clock64() - t_q;
                // KPL keys per lane of wave 0 hold the candidate list (ef <= 64 KPL); KPL = 0: the list lives in LDS
                if constexpr(SPEC != 0)
                    cnt = search_level_spec<METRIC, G, KPL, ROWS, (G == 64 && SPEC == 2 ? 3 : 2), SPEC == 2, PROF>(v, s, sc, bitmap, bm_words, start, ef, D, E,
                                                                                                                     PROF ? LGPU_SEARCH_ARG(ka, phase_cycles) : nullptr);
                else if constexpr(KPL > 0) cnt = search_level_reg<METRIC, G, KPL, PROF, ROWS, SCREEN>(v, s, bitmap, bm_words, start, 0, ef, D, E, pc, SCREEN ? LGPU_SEARCH_ARG(ka, list_prefetch) : 0u);
                else cnt = search_level<METRIC, G, PROF, ROWS>(v, s, bitmap, bm_words, start, 0, ef, D, E, pc);
            }
        }
        const KernargBytes kb = kernarg_opaque();
        if constexpr(PROF && SPEC == 0) {
            unsigned long long *const phase_cycles = LGPU_SEARCH_ARG(kb, phase_cycles);
            if(tid == 0) pc[ 7 ] = (unsigned long long)clock64() - t_q;
            if((tid & 63) == 0 && phase_cycles) {  // thread 0, and the list wave's first lane (slot 4 of the split walk)
                for(int i = 0; i < 8; ++i)
                    if(tid == 0 ? (i != 4 || pc[ 4 ] != 0) : (i == 4 && pc[ 4 ] != 0)) atomicAdd(&phase_cycles[ i ], pc[ i ]);
            }
        }
        const uint32_t k = EACH ? each.k : LGPU_SEARCH_ARG(kb, k), skip = EACH ? each.skip : LGPU_SEARCH_ARG(kb, skip);
        const uint32_t kw = EACH ? LGPU_SEARCH_ARG(kb, k_stride) : k;  // the width of an answer row
        const int      got = frame_answer_rows<SearchArgs>(tid, T, kb, s, q, cnt, k, skip, kw);
        pos = frame_close<SearchArgs, SCREEN>(tid, kb, s, q, pos, got, D, E);
    }
}

}  // namespace lgpu
