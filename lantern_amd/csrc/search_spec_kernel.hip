// search_spec_kernel.hip -- k_search in its latency-bound forms (walk_spec.hpp): a lone query (three role waves + eight row
// waves) and batches that cannot fill the chip (four waves).  Same template as search_kernel.hip, its own translation unit; the
// launcher body is search_launch.hpp's.
#include "search_launch.hpp"

namespace lgpu {

size_t search_spec_lds_bytes(uint32_t M0, uint32_t prefetch, uint32_t cache_entries) { return spec_lds_bytes(M0, prefetch, cache_entries); }

hipError_t launch_search_spec(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream)
{
    return launch_search_latency<false>(metric, a, waves, grid, stream);
}

}  // namespace lgpu
