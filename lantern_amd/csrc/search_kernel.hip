// search_kernel.hip -- k_search launcher for the bandwidth-bound shapes (search_kernel.hpp has the kernel, search_launch.hpp the
// launcher body; the latency-bound instantiations live in search_spec_kernel.hip).  Its own translation unit: the instantiations
// (metric x lanes per row x list placement x rows in flight) compile in parallel with the build-side kernels.
#include "search_launch.hpp"

namespace lgpu {

size_t search_lds_bytes(uint32_t chunks, uint32_t ef_cap, uint32_t M0, uint32_t vis_slots) { return walk_lds_bytes(chunks, ef_cap, M0, vis_slots); }

hipError_t launch_search(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream)
{
    if(a.qparams) return launch_search_each(metric, a, waves, grid, stream);  // the per-query-parameter form (search_each_kernel.hip)
    if(a.spec) return launch_search_spec(metric, a, waves, grid, stream);
    return launch_search_classic<false>(metric, a, waves, grid, stream);
}

}  // namespace lgpu
