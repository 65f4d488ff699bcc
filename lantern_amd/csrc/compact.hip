// compact.hip -- the kernels of lantern_gpu_compact_deleted (include/lantern_gpu.h "Deleting rows"; the host side is
// in unlink.hip, behind the unlink it performs first).
//
//   k_compact_flags    one thread per old slot: live flag and live level, the inputs of two rocPRIM exclusive scans (as filter.hip and
//                      the unlink use rocPRIM).  The scans give map (live slots below s) and uoff (their levels: the new upper_off).
//   k_compact_finish   map[s] = EMPTY for a tombstone; src_of[map[s]] = s for a live slot
//   k_compact_rows     THE BANDWIDTH PATH: new row j = old row src_of[j].  The new block is written as ONE contiguous stream of 16-byte
//                      units; the old block is read in runs, a live run being contiguous.  The same template moves the f32 / f16 / i8 /
//                      bit rows, the int8 screen rows and (in bytes where a code row is no multiple of 16) the pq code rows.
//   k_compact_lists    nbr0 and the upper blocks through the map (a random 4-byte gather over n * 4 bytes: cache resident), padding kept,
//                      entries that are neither padding nor mapped counted
//   k_compact_meta     labels, levels, norms, screen metadata, upper_off of the new slots
//
// No kernel writes an old array: a failure at any point leaves the index as the unlink left it.
#include <rocprim/device/device_scan.hpp>

#include "device_common.hpp"
#include "kernels.hpp"

namespace lgpu {

__global__ void __launch_bounds__(256) k_compact_flags(const uint64_t *labels, const uint8_t *levels, size_t n, uint32_t *flags, uint32_t *lv)
{
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(s > n) return;  // (word n: the scans' totals land there)
    const bool live = s < n && labels[ s ] != 0;
    flags[ s ] = live ? 1u : 0u;
    lv[ s ] = live ? (uint32_t)levels[ s ] : 0u;
}

__global__ void __launch_bounds__(256) k_compact_finish(const uint32_t *flags, size_t n, uint32_t *map, uint32_t *src_of)
{
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(s >= n) return;
    if(flags[ s ]) src_of[ map[ s ] ] = (uint32_t)s;
    else map[ s ] = EMPTY;
}

// Unit `local` (< 2^20) of the tile that starts at unit `base` of a block of rows of `units` units each: its row and its place in the
// row.  The 64-bit division is the tile's (uniform: scalar), the lane's is 32-bit.
struct TileOrigin
{
    size_t   row0;
    uint32_t rem0;
};
__device__ __forceinline__ TileOrigin tile_origin(size_t base, uint32_t units)
{
    TileOrigin t;
    t.row0 = base / units;
    t.rem0 = (uint32_t)(base - t.row0 * units);
    return t;
}

// Persistent workgroups; a tile is 256 * U consecutive units of the NEW block, U per lane, 256 apart: a wave's store instruction writes
// 64 consecutive units (1 KiB of uint4) and its load reads them from one old row, or from a few where rows are short or a row ends.
// All U loads of a lane (each behind its own 4-byte src_of read, which is sequential: cache lines shared by the whole tile) are issued
// before the first store, so 256 * U units per workgroup are in flight.  Offsets are size_t: 10M x 3 KiB is past 4 GiB.
template <typename T, int U>
__global__ void __launch_bounds__(256) k_compact_rows(const T *__restrict__ src, T *__restrict__ dst, const uint32_t *__restrict__ src_of, size_t live,
                                                      uint32_t units)
{
    constexpr uint32_t kTile = 256u * U;
    const size_t       total = live * (size_t)units, tiles = (total + kTile - 1) / kTile;
    for(size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t     base = t * kTile;
        const TileOrigin o = tile_origin(base, units);
        const uint32_t   last = (uint32_t)std::min<size_t>(total - base, kTile) - 1;  // the tile's last unit inside the block
        T                v[ U ];
#pragma unroll
        for(int u = 0; u < U; ++u) {  // (a lane past the end reads the last unit again: no branch around the loads)
            const uint32_t local = std::min(threadIdx.x + 256u * (uint32_t)u, last);
            const uint32_t at = o.rem0 + local, q = at / units, w = at - q * units;
            v[ u ] = src[ (size_t)src_of[ o.row0 + q ] * units + w ];
        }
#pragma unroll
        for(int u = 0; u < U; ++u) {
            const uint32_t local = threadIdx.x + 256u * (uint32_t)u;
            if(base + local < total) dst[ base + local ] = v[ u ];
        }
    }
}

// One thread per entry of the new array.  UPPER = false: entry i of the level-0 list of new slot j.  UPPER = true: entry i of every upper
// block of new slot j (most slots have none: one byte read).
template <bool UPPER>
__global__ void __launch_bounds__(256) k_compact_lists(const uint32_t *__restrict__ old_nbr, uint32_t *__restrict__ new_nbr, const uint32_t *__restrict__ src_of,
                                                       const uint32_t *__restrict__ map, const uint32_t *__restrict__ new_uoff, uint32_t n_old, size_t live,
                                                       uint32_t W, const uint8_t *__restrict__ old_levels, const uint32_t *__restrict__ old_uoff,
                                                       unsigned long long *dangling)
{
    const size_t total = live * (size_t)W, tiles = (total + 255) / 256;
    uint32_t     bad = 0;
    for(size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t     base = t * 256;
        const TileOrigin o = tile_origin(base, W);
        if(base + threadIdx.x >= total) continue;
        const uint32_t at = o.rem0 + threadIdx.x, q = at / W, i = at - q * W;
        const size_t   j = o.row0 + q;
        const uint32_t s = src_of[ j ];
        const int      blocks = UPPER ? (int)old_levels[ s ] : 1;
        const size_t   from = UPPER ? (size_t)old_uoff[ s ] * W : (size_t)s * W, to = UPPER ? (size_t)new_uoff[ s ] * W : j * (size_t)W;
        for(int b = 0; b < blocks; ++b) {
            const uint32_t e = old_nbr[ from + (size_t)b * W + i ];
            uint32_t       r = EMPTY;
            if(e != EMPTY) {
                r = e < n_old ? map[ e ] : EMPTY;
                bad += r == EMPTY;
            }
            new_nbr[ to + (size_t)b * W + i ] = r;
        }
    }
    if(bad) atomicAdd(dangling, (unsigned long long)bad);
}

__global__ void __launch_bounds__(256) k_compact_meta(CompactMeta a, const uint32_t *src_of, const uint32_t *uoff, size_t live)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(j >= live) return;
    const uint32_t s = src_of[ j ];
    a.new_labels[ j ] = a.labels[ s ];
    a.new_levels[ j ] = a.levels[ s ];
    a.new_upper_off[ j ] = uoff[ s ];
    if(a.new_norm2) a.new_norm2[ j ] = a.norm2[ s ];
    if(a.new_screen_meta) a.new_screen_meta[ j ] = a.screen_meta[ s ];
}

size_t compact_temp_bytes(size_t n)
{
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u, n + 1, rocprim::plus<uint32_t>());
    return bytes;
}

hipError_t launch_compact_map(const uint64_t *labels, const uint8_t *levels, size_t n, const CompactMap &m, hipStream_t stream)
{
    if(n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n + 1 + 255) / 256);
    hipLaunchKernelGGL(k_compact_flags, dim3(blocks), dim3(256), 0, stream, labels, levels, n, m.flags, m.lv);
    hipError_t e = hipGetLastError();
    size_t     bytes = m.temp_bytes;
    if(e == hipSuccess) e = rocprim::exclusive_scan(m.temp, bytes, (const uint32_t *)m.flags, m.map, 0u, n + 1, rocprim::plus<uint32_t>(), stream);
    bytes = m.temp_bytes;
    if(e == hipSuccess) e = rocprim::exclusive_scan(m.temp, bytes, (const uint32_t *)m.lv, m.uoff, 0u, n + 1, rocprim::plus<uint32_t>(), stream);
    if(e != hipSuccess) return e;
    hipLaunchKernelGGL(k_compact_finish, dim3(blocks), dim3(256), 0, stream, (const uint32_t *)m.flags, n, m.map, m.src_of);
    return hipGetLastError();
}

// workgroups of a persistent copy launch: eight per CU (2048 threads: the CU's full complement of waves at <= 64 VGPRs)
static unsigned copy_grid(size_t tiles, int num_cus) { return (unsigned)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)std::max(num_cus, 1) * 8)); }

hipError_t launch_compact_rows(const void *src, void *dst, const uint32_t *src_of, size_t live, size_t row_bytes, int num_cus, hipStream_t stream)
{
    if(live == 0 || row_bytes == 0) return hipSuccess;
    if(row_bytes % 16 == 0) {
        constexpr int  U = 8;  // 32 KiB per workgroup in flight
        const uint32_t units = (uint32_t)(row_bytes / 16);
        const size_t   tiles = (live * units + 256 * U - 1) / (256 * U);
        hipLaunchKernelGGL((k_compact_rows<uint4, U>), dim3(copy_grid(tiles, num_cus)), dim3(256), 0, stream, (const uint4 *)src, (uint4 *)dst, src_of, live, units);
    } else {
        constexpr int U = 4;
        const size_t  tiles = (live * row_bytes + 256 * U - 1) / (256 * U);
        hipLaunchKernelGGL((k_compact_rows<uint8_t, U>), dim3(copy_grid(tiles, num_cus)), dim3(256), 0, stream, (const uint8_t *)src, (uint8_t *)dst, src_of, live,
                           (uint32_t)row_bytes);
    }
    return hipGetLastError();
}

hipError_t launch_compact_lists(const uint32_t *old_nbr, uint32_t *new_nbr, const CompactMap &m, uint32_t n_old, size_t live, uint32_t W,
                                const uint8_t *old_levels, const uint32_t *old_uoff, unsigned long long *dangling, int num_cus, hipStream_t stream)
{
    if(live == 0 || W == 0) return hipSuccess;
    const size_t   tiles = (live * W + 255) / 256;
    const unsigned grid = copy_grid(tiles, num_cus);
    if(old_levels)
        hipLaunchKernelGGL((k_compact_lists<true>), dim3(grid), dim3(256), 0, stream, old_nbr, new_nbr, (const uint32_t *)m.src_of, (const uint32_t *)m.map,
                           (const uint32_t *)m.uoff, n_old, live, W, old_levels, old_uoff, dangling);
    else
        hipLaunchKernelGGL((k_compact_lists<false>), dim3(grid), dim3(256), 0, stream, old_nbr, new_nbr, (const uint32_t *)m.src_of, (const uint32_t *)m.map,
                           (const uint32_t *)m.uoff, n_old, live, W, old_levels, old_uoff, dangling);
    return hipGetLastError();
}

hipError_t launch_compact_meta(const CompactMeta &a, const CompactMap &m, size_t live, hipStream_t stream)
{
    if(live == 0) return hipSuccess;
    hipLaunchKernelGGL(k_compact_meta, dim3((unsigned)((live + 255) / 256)), dim3(256), 0, stream, a, (const uint32_t *)m.src_of, (const uint32_t *)m.uoff, live);
    return hipGetLastError();
}

}  // namespace lgpu
