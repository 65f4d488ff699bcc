// search_launch.hpp -- the two launcher bodies of k_search (search_kernel.hpp), each a template on EACH (the per-query-parameter
// form): the bandwidth-bound shapes and the latency-bound ones.  A body is instantiated where it is called: search_kernel.hip and
// search_spec_kernel.hip take EACH = false, search_each_kernel.hip and search_each_spec_kernel.hip EACH = true, so the kernels stay
// spread over four translation units that compile side by side.  The instrumented (PROF) instantiations exist for EACH = false only.
#pragma once
#include "search_kernel.hpp"

namespace lgpu {

// the record of an instantiation (lantern_gpu_last_search_cells): k_search's own parameter list with its defaults, so that the launch
// macro hands the recorder and the kernel the same arguments
template <int METRIC, int G, bool PROF = false, int ROWS = 2, int KPL = 1, int SPEC = 0, bool EACH = false> static inline void note_search(const SearchArgs &a)
{
    note_search_cell(1, METRIC, G, PROF, ROWS, KPL, SPEC, EACH, a);
}
// one instantiation: note it, opt the kernel in to its dynamic LDS size, then launch
#define LGPU_LAUNCH_SEARCH(...)                                                                \
    {                                                                                          \
        note_search<__VA_ARGS__>(a);                                                           \
        LGPU_LAUNCH_LDS((k_search<__VA_ARGS__>), grid, 64 * waves, lds, stream, a)             \
    }
// ... for the list placement of this launch (walk.hpp search_level_reg): one key per lane of wave 0 up to ef = 64, two up to
// 128, the LDS list beyond (or when LANTERN_GPU_LDS_LIST asks for it)
#define LGPU_LAUNCH_SEARCH_KPL(MM, GG, PP, RR)                           \
    {                                                                    \
        if(kpl == 1) LGPU_LAUNCH_SEARCH(MM, GG, PP, RR, 1, 0, EACH)      \
        else if(kpl == 2) LGPU_LAUNCH_SEARCH(MM, GG, PP, RR, 2, 0, EACH) \
        else LGPU_LAUNCH_SEARCH(MM, GG, PP, RR, 0, 0, EACH)              \
    }

// the bandwidth-bound shapes: a.spec == 0; EACH: by the launch's largest expansion (a.ef), a.qparams and a.frame.qlist set
template <bool EACH> static hipError_t launch_search_classic(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream)
{
    if(EACH && a.phase_cycles) return hipErrorInvalidValue;
    // (a view with a screen: the launch screens -- search_plan.cpp passes the screen only where it planned the planes' block)
    const size_t lds = search_lds_bytes(a.view.chunks, a.ef, a.view.M0, a.frame.vis_slots) + (a.view.screen ? screen_query_lds_bytes(a.view.chunks) : 0);
    const int    kpl = a.lds_list ? 0 : a.ef <= 64 ? 1 : a.ef <= 128 ? 2 : 0;
    const int    G_ = group_lanes_for(a.view.chunks);
    if(a.wide_rows && !a.phase_cycles && G_ == 64) {  // the small-batch shape (rows of >= 128 chunks)
        bool launched = true;
        switch(metric) {
            case M_L2SQ: LGPU_LAUNCH_SEARCH_KPL(M_L2SQ, 64, false, 4); break;
            case M_COS: LGPU_LAUNCH_SEARCH_KPL(M_COS, 64, false, 4); break;
            case M_HAMMING: LGPU_LAUNCH_SEARCH_KPL(M_HAMMING, 64, false, 4); break;
            case M_L2SQ_F16: LGPU_LAUNCH_SEARCH_KPL(M_L2SQ_F16, 64, false, 4); break;
            case M_COS_F16: LGPU_LAUNCH_SEARCH_KPL(M_COS_F16, 64, false, 4); break;
            case M_L2SQ_PQD: LGPU_LAUNCH_SEARCH_KPL(M_L2SQ_PQD, 64, false, 4); break;
            case M_COS_PQD: LGPU_LAUNCH_SEARCH_KPL(M_COS_PQD, 64, false, 4); break;
            default: launched = false;  // i8 storage (rows of >= 2033 dims) has no four-row instantiation: the two-row shape below
        }
        if(launched) return hipGetLastError();
    }
    if constexpr(!EACH) {
        if(a.phase_cycles) {  // diagnostic instantiations: the f32 metrics at the two common row shapes
            if(metric == M_L2SQ && G_ == 64) LGPU_LAUNCH_SEARCH_KPL(M_L2SQ, 64, true, 2)
            else if(metric == M_L2SQ && G_ == 16) LGPU_LAUNCH_SEARCH_KPL(M_L2SQ, 16, true, 2)
            else if(metric == M_COS && G_ == 64) LGPU_LAUNCH_SEARCH_KPL(M_COS, 64, true, 2)
            else return hipErrorInvalidValue;
            return hipGetLastError();
        }
    }
#define CALL(MM, GG) LGPU_LAUNCH_SEARCH_KPL(MM, GG, false, 2)
    if(mcode_is_pqd(metric)) PQD_G(metric, a.view.chunks, CALL);
    else LGPU_DISPATCH(metric, a.view.chunks, CALL);
#undef CALL
    return hipGetLastError();
}

// rows in flight per G-lane group, so that eight row waves cover a 32-entry list in one pass (the four-wave shape takes two)
#define LGPU_SPEC_ROWS(GG) ((GG) == 64 ? 4 : (GG) == 32 ? 2 : 1)
// (the four-wave shape, spec 1, has no per-query form)
#define LGPU_LAUNCH_SPEC(MM, GG)                                                              \
    {                                                                                         \
        if(EACH || a.spec == 2) {                                                             \
            if(kpl == 1) LGPU_LAUNCH_SEARCH(MM, GG, false, LGPU_SPEC_ROWS(GG), 1, 2, EACH)    \
            else LGPU_LAUNCH_SEARCH(MM, GG, false, LGPU_SPEC_ROWS(GG), 2, 2, EACH)            \
        } else if constexpr(!EACH) {                                                          \
            if(kpl == 1) LGPU_LAUNCH_SEARCH(MM, GG, false, LGPU_SPEC_ROWS(GG), 1, 1)          \
            else LGPU_LAUNCH_SEARCH(MM, GG, false, LGPU_SPEC_ROWS(GG), 2, 1)                  \
        }                                                                                     \
    }

// the latency-bound shapes: a.spec != 0; EACH: a.spec == 2 only
template <bool EACH> static hipError_t launch_search_latency(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream)
{
    if(EACH && (a.phase_cycles || a.spec != 2)) return hipErrorInvalidValue;
    if(a.ef > 128 || a.view.M0 > 64 || a.view.M0 < 2 || waves < 2 || (a.spec >= 2 && waves < 4)) return hipErrorInvalidValue;
    const size_t lds = search_lds_bytes(a.view.chunks, a.ef, a.view.M0, a.frame.vis_slots) + spec_lds_bytes(a.view.M0, a.spec_prefetch, a.spec_cache);
    const int    kpl = a.ef <= 64 ? 1 : 2;
    if constexpr(!EACH) {
        if(a.phase_cycles) {  // diagnostic instantiations (lantern_gpu_spec_profile): f32 l2sq / cos rows of 32..63 and of >= 128 chunks, ef <= 64
            const int G_ = group_lanes_for(a.view.chunks);
#define LGPU_PROF_SPEC(MM, GG, RR) { if(a.spec == 2) LGPU_LAUNCH_SEARCH(MM, GG, true, RR, 1, 2) else LGPU_LAUNCH_SEARCH(MM, GG, true, RR, 1, 1) }
            if(kpl == 1 && metric == M_L2SQ && G_ == 16) LGPU_PROF_SPEC(M_L2SQ, 16, 1)
            else if(kpl == 1 && metric == M_L2SQ && G_ == 64) LGPU_PROF_SPEC(M_L2SQ, 64, 4)
            else if(kpl == 1 && metric == M_COS && G_ == 64) LGPU_PROF_SPEC(M_COS, 64, 4)
#undef LGPU_PROF_SPEC
            else return hipErrorInvalidValue;
            return hipGetLastError();
        }
    }
    if(a.spec >= 3) return hipErrorInvalidValue;  // (search_plan.cpp never asks: LANTERN_GPU_SPEC=3 / 4 mean 2)
    if(mcode_is_pqd(metric)) PQD_G(metric, a.view.chunks, LGPU_LAUNCH_SPEC);
    else LGPU_DISPATCH(metric, a.view.chunks, LGPU_LAUNCH_SPEC);
    return hipGetLastError();
}

}  // namespace lgpu
