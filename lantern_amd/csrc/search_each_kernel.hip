// search_each_kernel.hip -- k_search in its per-query-parameter form (search_kernel.hpp, EACH) for the bandwidth-bound shapes: the
// classic two-row shape for every metric, lanes per row and list placement, and the four-row small-batch shape where the uniform
// kernel has one (search_launch.hpp, the same launcher body).  Its own translation unit: it compiles beside search_kernel.hip, whose
// instantiations it leaves untouched.  The instrumented (PROF) instantiations have no per-query form: a per-query call in profiling
// mode runs these.
#include "search_launch.hpp"

namespace lgpu {

hipError_t launch_search_each(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream)
{
    if(!a.qparams || !a.frame.qlist) return hipErrorInvalidValue;
    if(a.spec) return launch_search_each_spec(metric, a, waves, grid, stream);
    return launch_search_classic<true>(metric, a, waves, grid, stream);
}

}  // namespace lgpu
