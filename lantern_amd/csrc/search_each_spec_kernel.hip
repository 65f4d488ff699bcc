// search_each_spec_kernel.hip -- k_search in its per-query-parameter form (search_kernel.hpp, EACH) for the latency-bound shape a
// per-query call can take: three role waves + eight row waves (spec 2), which is what service-sized batches run.  The four-wave
// shape (spec 1, on request only) and the experimental walks have no per-query form: index.cpp falls back to the classic shape.
#include "search_kernel.hpp"

namespace lgpu {

#define LGPU_SPEC_ROWS(GG) ((GG) == 64 ? 4 : (GG) == 32 ? 2 : 1)  // (as search_spec_kernel.hip)
#define LGPU_LAUNCH_EACH_SPEC(MM, GG)                                                     \
    {                                                                                     \
        if(kpl == 1) LGPU_LAUNCH_SEARCH(MM, GG, false, LGPU_SPEC_ROWS(GG), 1, 2, true)    \
        else LGPU_LAUNCH_SEARCH(MM, GG, false, LGPU_SPEC_ROWS(GG), 2, 2, true)            \
    }

hipError_t launch_search_each_spec(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream)
{
    if(!a.qparams || !a.qlist || a.phase_cycles || a.spec != 2) return hipErrorInvalidValue;
    if(a.ef > 128 || a.view.M0 > 64 || a.view.M0 < 2 || waves < 4) return hipErrorInvalidValue;
    const size_t lds = search_lds_bytes(a.view.chunks, a.ef, a.view.M0, a.vis_slots) + spec_lds_bytes(a.view.M0, a.spec_prefetch, a.spec_cache, 0);
    const int    kpl = a.ef <= 64 ? 1 : 2;
    if(mcode_is_pqd(metric)) {  // a compact pq index, rows decoded on the fly
        const int G_ = group_lanes_for(a.view.chunks);
#define PQD_G(MM)                                                                                                                   \
    switch(G_) { case 64: LGPU_LAUNCH_EACH_SPEC(MM, 64); break; case 32: LGPU_LAUNCH_EACH_SPEC(MM, 32); break; case 16: LGPU_LAUNCH_EACH_SPEC(MM, 16); break; \
                 default: LGPU_LAUNCH_EACH_SPEC(MM, 8); }
        if(metric == M_L2SQ_PQD) PQD_G(M_L2SQ_PQD)
        else if(metric == M_COS_PQD) PQD_G(M_COS_PQD)
        else return hipErrorInvalidValue;
#undef PQD_G
        return hipGetLastError();
    }
    LGPU_DISPATCH(metric, a.view.chunks, LGPU_LAUNCH_EACH_SPEC);
    return hipGetLastError();
}

}  // namespace lgpu
