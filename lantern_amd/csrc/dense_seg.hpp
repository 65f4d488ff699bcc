// dense_seg.hpp -- the segmented contraction and selection of a per-query-filter call's batched dense run (dense_seg.hip; DESIGN.md 4.9
// "Dense exact path, per-query filters: batched"): the two device tables a batch is launched from, and the two launchers.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace lgpu {

// the two tile shapes of k_dense_seg: a step of at most kSegSkinnyQ queries is cut into skinny tiles (32 queries x 256 rows), a larger
// one into 128 x 128 tiles
constexpr uint32_t kSegSkinnyQ = 32, kSegSkinnyCols = 256, kSegBigQ = 128, kSegBigCols = 128;

// one output tile of one step: queries [q0, q0 + nq) of the run's query block against rows [col0, col0 + cols) of the gathered chunk;
// its cells go to dd[out + i * ld + j].  shape: 0 skinny (nq <= 32, cols <= 256), 1 the 128 x 128 tile
struct SegTile
{
    uint32_t q0, nq, col0, cols, out, ld, shape, pad;
};
// one query of one step, as k_select_seg folds it: its row of the step's block (dd[off .. off + cols)), the list position of the
// block's first column, and its row of the best lists
struct SegQuery
{
    uint32_t off, cols, c_base, row;
};

// one launch: every tile of a batch.  Q / B: the query block and the gathered chunk, `stride` floats per row; qn / bn: their norm
// words (bn: the chunk's).  metric: M_L2SQ or M_COS
hipError_t launch_dense_seg(int metric, const float *Q, const float *B, uint32_t stride, const float *qn, const float *bn, float *dd, const SegTile *tiles,
                            uint32_t n_tiles, hipStream_t stream);
// one launch: every (step, query) of a batch folded into best[row][kk]
hipError_t launch_select_seg(const float *dd, const SegQuery *queries, uint32_t n, uint64_t *best, uint32_t kk, hipStream_t stream);

}  // namespace lgpu
