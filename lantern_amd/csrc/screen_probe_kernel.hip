// screen_probe_kernel.hip -- diagnostics: the int8 screen's reject decision, made by walk.hpp's own
// hop_distances_screened and exported (lantern_gpu_screen_probe).  One workgroup plays one hop of a walk whose list is full: it stages
// the query with the search kernels' own pieces (query_frame.hpp frame_stage: the cached norm of a cosine query included; walk.hpp
// screen_stage_query: its int8 planes), takes the caller's slots as the hop's new neighbours and the
// caller's radius as the key `worst`, and reports which keys the screen set to ~0.  Nothing here decides anything: the tests compare
// the verdicts with tests/test_screen_bound*.py on the host.
#include "query_frame.hpp"

namespace lgpu {

constexpr uint32_t kProbeSlots = 64;  // the hop's new neighbours: at most this many (the carve's cap_max; the survivors fit s.sorted)

template <int METRIC>
__global__ void __launch_bounds__(512) k_screen_probe(View v, const uint4 *query, const uint32_t *slots, uint32_t n, float radius, uint8_t *out)
{
    constexpr int G = 64;
    const int     tid = threadIdx.x, T = blockDim.x;
    WalkLds       s;
    (void)carve_walk(lgpu_smem, s, v.chunks, kProbeSlots, kProbeSlots);
    if(tid == 0) {
        uint64_t *const sp = (uint64_t *)&s.scal[ S_SCREEN ];
        sp[ 0 ] = (uint64_t)v.screen;
        sp[ 1 ] = (uint64_t)v.screen_meta;
        s.scal[ S_NREJ ] = 0;
        s.scal[ S_NSURV ] = 0;
        s.scal[ S_QN2 ] = 0;
    }
    for(uint32_t i = tid; i < n; i += T) {
        s.newids[ i ] = slots[ i ];
        s.newkeys[ i ] = 0;  // a survivor's key is left alone by the screen
    }
    frame_stage<METRIC, G>(tid, T, s, query, 0, v.chunks);  // (its barriers cover the writes above)
    const float qn2 = __int_as_float(s.scal[ S_QN2 ]);
    screen_stage_query<METRIC>(tid, s, v.chunks, qn2);  // the planes block: behind the (empty) visited set
    (void)hop_distances_screened<METRIC, G, 2>(v, s, (int)n, make_key(radius, 0u), qn2);  // (ends in a barrier)
    for(uint32_t i = tid; i < n; i += T) out[ i ] = s.newkeys[ i ] == ~0ull ? 1 : 0;
}

hipError_t launch_screen_probe(int metric, const View &v, const uint4 *query, const uint32_t *slots, uint32_t n, float radius, int threads,
                               uint8_t *out, hipStream_t stream)
{
    if(n == 0) return hipSuccess;
    if(n > kProbeSlots || (threads != 256 && threads != 512) || !v.screen || !v.screen_meta || !screen_rows_for(v.chunks)) return hipErrorInvalidValue;
    const size_t lds = walk_lds_bytes(v.chunks, kProbeSlots, kProbeSlots) + screen_query_lds_bytes(v.chunks);
    if(metric == M_L2SQ) hipLaunchKernelGGL(k_screen_probe<M_L2SQ>, dim3(1), dim3(threads), lds, stream, v, query, slots, n, radius, out);
    else if(metric == M_COS) hipLaunchKernelGGL(k_screen_probe<M_COS>, dim3(1), dim3(threads), lds, stream, v, query, slots, n, radius, out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace lgpu
