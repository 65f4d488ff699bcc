// dense_tile.hpp -- what the two dense contractions share: the output tile, the fused epilogue's argument block and the
// persistent grid.  bruteforce.hip (k_dense_f32: f32 rows) and dense_native.hip (k_dense_native: f16 / i8 rows) include it.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace lgpu {

// 128 x 128 output tile per 256-thread workgroup; 4 waves as 2 x 2, each wave 2 x 2 MFMA tiles of 32 x 32 (64 accumulator
// registers per lane); K staged through LDS 32 words (128 bytes per row) at a time: 32 floats, 64 halves or 128 int8.
constexpr int BM = 128, BN = 128, BK = 32;

// FUSED: the tile does not write its distances; an output that can still enter its query's running top-kk -- ordered distance
// <= the kk-th best so far, read once per tile -- is appended to that query's candidate list (cand[q][CAP], cnt[q]), which
// k_select folds into `best` after the launch.  Once a few thousand columns have been seen that is a handful of appends per
// query and launch instead of a 268 MB matrix written here and read back there.
struct DenseTopk
{
    const uint64_t *best;  // [nq][kk] running top-kk keys (ordered distance << 32 | column), ascending
    uint32_t        kk;
    uint64_t       *cand;  // [nq][cap]
    uint32_t       *cnt;   // [nq] appended so far (may exceed cap: k_select reports the overflow)
    uint32_t        cap;
    uint32_t        c_base;  // column id of this launch's first base row
};

constexpr int DENSE_WGS_PER_CU = 2;  // 67 KB of LDS each

// persistent grid of the contractions: DENSE_WGS_PER_CU workgroups per CU of the current device (fewer if there are fewer tiles)
uint32_t dense_grid(uint32_t tiles);

// dense_native.hip's half of launch_contraction / launch_norms (kernels.hpp; bruteforce.hip hands it every kind but 0)
struct DenseOperands;
hipError_t launch_contraction_native(const DenseOperands &o, float *out, uint32_t ldo, const DenseTopk *topk, hipStream_t stream);
hipError_t launch_norms_native(int kind, int metric, const uint4 *rows, uint32_t n, uint32_t chunks, uint32_t *out, hipStream_t stream);

}  // namespace lgpu
