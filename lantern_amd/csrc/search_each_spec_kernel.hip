// search_each_spec_kernel.hip -- k_search in its per-query-parameter form (search_kernel.hpp, EACH) for the latency-bound shape a
// per-query call can take: three role waves + eight row waves (spec 2), which is what service-sized batches run (search_launch.hpp,
// the same launcher body).  The four-wave shape (spec 1, on request only) has no per-query form:
// search_plan.cpp falls back to the classic shape.
#include "search_launch.hpp"

namespace lgpu {

hipError_t launch_search_each_spec(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream)
{
    if(!a.qparams || !a.frame.qlist) return hipErrorInvalidValue;
    return launch_search_latency<true>(metric, a, waves, grid, stream);
}

}  // namespace lgpu
