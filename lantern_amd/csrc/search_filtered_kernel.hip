// search_filtered_kernel.hip -- the filtered k-NN search's two kernels (search_filtered_kernel.hpp: k_search_filtered and
// k_search_exact_allowed) over rows stored in HBM: every metric code of LGPU_DISPATCH, in every form.  The instantiations over a compact
// pq index are search_filtered_pq_kernel.hip's.
#include "dispatch.hpp"
#include "search_filtered_kernel.hpp"

namespace lgpu {

size_t filtered_walk_lds_bytes(uint32_t chunks, uint32_t exp, uint32_t cand_cap, uint32_t M0, uint32_t vis_slots)
{
    return walk_lds_bytes(chunks, exp, M0, vis_slots) + 16 + (size_t)cand_cap * 16;
}
size_t filtered_exact_lds_bytes(uint32_t chunks, uint32_t kk, uint32_t rows_per_round) { return walk_lds_bytes(chunks, kk, rows_per_round, 0); }

hipError_t launch_search_filtered(int metric, const FilteredArgs &a, int waves, int grid, hipStream_t stream)
{
    const size_t lds = filtered_walk_lds_bytes(a.view.chunks, a.exp, a.cand_cap, a.view.M0, a.frame.vis_slots);
    if((a.seeds || a.qparams) && !a.descs) return hipErrorInvalidValue;  // the seeded walk and the per-query parameters exist in the per-query form only (filter.hip builds the table)
    LGPU_DISPATCH(metric, a.view.chunks, LGPU_FILTERED_WALK_FORMS);
    return hipGetLastError();
}

hipError_t launch_search_exact_allowed(int metric, const FilteredArgs &a, int waves, int grid, hipStream_t stream)
{
    const size_t lds = filtered_exact_lds_bytes(a.view.chunks, a.exp, a.rows_per_round);
    if(a.qparams && !a.descs) return hipErrorInvalidValue;
    LGPU_DISPATCH(metric, a.view.chunks, LGPU_FILTERED_EXACT_FORMS);
    return hipGetLastError();
}

}  // namespace lgpu
