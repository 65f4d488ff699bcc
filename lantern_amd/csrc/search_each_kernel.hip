// search_each_kernel.hip -- k_search in its per-query-parameter form (search_kernel.hpp, EACH) for the bandwidth-bound shapes: the
// classic two-row shape for every metric, lanes per row and list placement, and the four-row small-batch shape where the uniform
// kernel has one.  Its own translation unit: it compiles beside search_kernel.hip, whose instantiations it leaves untouched.  The
// instrumented (PROF) instantiations have no per-query form: a per-query call in profiling mode runs these.
#include "search_kernel.hpp"

namespace lgpu {

#define LGPU_LAUNCH_EACH_KPL(MM, GG, RR)                                   \
    {                                                                      \
        if(kpl == 1) LGPU_LAUNCH_SEARCH(MM, GG, false, RR, 1, 0, true)     \
        else if(kpl == 2) LGPU_LAUNCH_SEARCH(MM, GG, false, RR, 2, 0, true) \
        else LGPU_LAUNCH_SEARCH(MM, GG, false, RR, 0, 0, true)             \
    }

hipError_t launch_search_each(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream)
{
    if(!a.qparams || !a.qlist || a.phase_cycles) return hipErrorInvalidValue;
    if(a.spec) return launch_search_each_spec(metric, a, waves, grid, stream);
    const size_t lds = search_lds_bytes(a.view.chunks, a.ef, a.view.M0, a.vis_slots);
    const int    kpl = a.lds_list ? 0 : a.ef <= 64 ? 1 : a.ef <= 128 ? 2 : 0;  // (as launch_search: by the launch's largest expansion)
    const int    G_ = group_lanes_for(a.view.chunks);
    if(a.wide_rows && G_ == 64) {  // the small-batch shape (rows of >= 128 chunks)
        bool launched = true;
        switch(metric) {
            case M_L2SQ: LGPU_LAUNCH_EACH_KPL(M_L2SQ, 64, 4); break;
            case M_COS: LGPU_LAUNCH_EACH_KPL(M_COS, 64, 4); break;
            case M_HAMMING: LGPU_LAUNCH_EACH_KPL(M_HAMMING, 64, 4); break;
            case M_L2SQ_F16: LGPU_LAUNCH_EACH_KPL(M_L2SQ_F16, 64, 4); break;
            case M_COS_F16: LGPU_LAUNCH_EACH_KPL(M_COS_F16, 64, 4); break;
            case M_L2SQ_PQD: LGPU_LAUNCH_EACH_KPL(M_L2SQ_PQD, 64, 4); break;
            case M_COS_PQD: LGPU_LAUNCH_EACH_KPL(M_COS_PQD, 64, 4); break;
            default: launched = false;  // (i8 storage: the two-row shape below, as launch_search)
        }
        if(launched) return hipGetLastError();
    }
#define CALL(MM, GG) LGPU_LAUNCH_EACH_KPL(MM, GG, 2)
    if(mcode_is_pqd(metric)) {  // a compact pq index, rows decoded on the fly; G by the DECODED row
#define PQD_G(MM)                                                                    \
    switch(G_) { case 64: CALL(MM, 64); break; case 32: CALL(MM, 32); break; case 16: CALL(MM, 16); break; default: CALL(MM, 8); }
        if(metric == M_L2SQ_PQD) PQD_G(M_L2SQ_PQD)
        else if(metric == M_COS_PQD) PQD_G(M_COS_PQD)
        else return hipErrorInvalidValue;
#undef PQD_G
        return hipGetLastError();
    }
    LGPU_DISPATCH(metric, a.view.chunks, CALL);
#undef CALL
    return hipGetLastError();
}

}  // namespace lgpu
