// dense_seg.hip -- the batched dense run of a per-query-filter call (DESIGN.md 4.9 "Dense exact path, per-query filters: batched"):
// k_dense_seg contracts the tiles of MANY steps -- a step is a tile of one group's queries against that group's rows inside one gathered
// chunk -- in one launch, from a device-resident tile table; k_select_seg folds every step's block of the packed matrix into its
// queries' best lists in one more.  f32 rows under l2sq / cos only; the plan (dense.cpp plan_each_dense_batches) sends everything else
// down the per-step run.  The tile constants, the metric epilogue and the persistent grid are dense_tile.hpp's.
#include "kernels.hpp"
#include "dense_tile.hpp"
#include "dense_seg.hpp"

namespace lgpu {

typedef float    floatx16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One LDS buffer is 288 rows of one K step (BK floats = 128 bytes each), unpadded: a skinny tile holds its 32 query rows in rows
// [0, 32) and its 256 base rows behind them; a 128 x 128 tile its query rows in [0, 128) and its base rows in [128, 256).  Two
// buffers are 72 KB: two workgroups per CU.
constexpr int SEG_ROWS = 288, SEG_BUF = SEG_ROWS * BK;

// Persistent workgroups over a table of tiles.  Workgroup b runs on XCD b % 8; every XCD takes a contiguous range of the table and
// its workgroups consecutive entries of it (k_dense_f32's order), so the tiles of one step -- adjacent in the table -- read that
// step's base rows through one L2.
// The K steps of ALL of a workgroup's tiles form one software pipeline over the two buffers with one barrier per K step: while step
// s is on the matrix cores, step s + 1 -- the next tile's first step, when s is a tile's last -- is landing in the other buffer
// (`buffer_load_dwordx4 ... lds`: global memory to LDS without a register in between, 16 bytes per lane).  A workgroup that draws
// forty 4 x 488 tiles fills the pipeline once.
// Loads are branch-free: a tile's two descriptors start at its first query / base row and end behind its last one, so the rows of
// the LDS tile past its counts land as zeros, and so does a k past the end of the row (offset pushed out of range).  A load
// instruction of a wave lands as 8 rows of 8 16-byte units; unit u of row r holds k-quad u ^ ((r >> 1) & 7) of that row, r counted
// inside its matrix -- the XOR swizzle that makes the 16-byte fragment reads of 16 consecutive rows hit 16 different bank groups.
// Fragments and the contraction index's permutation are k_dense_f32's: per round j, half h = lane / 32 reads k-quad 2 j + h, and MFMA
// e contracts the pair {8 j + e, 8 j + 4 + e}.
// A skinny tile: wave w owns base rows [64 w, 64 w + 64) as two 32 x 32 blocks (32 accumulator registers).  A 128 x 128 tile: the
// waves as 2 x 2, each 2 x 2 blocks (64).
// The epilogue writes the live nq x cols cells of the tile only.
template <int METRIC>
__global__ void __launch_bounds__(256, 2) k_dense_seg(const float *Q, const float *B, uint32_t stride /* floats per row */, const float *qn, const float *bn,
                                                     float *dd, const SegTile *tiles, uint32_t T)
{
    __shared__ float S[ 2 ][ SEG_BUF ];
    const int        tid = threadIdx.x, lane = tid & 63;
    const uint32_t   wu = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t   x = blockIdx.x & 7, j = blockIdx.x >> 3;
    const uint32_t   wx = (gridDim.x - x + 7) >> 3;  // workgroups on this XCD
    const uint32_t   cnt = (T >> 3) + (x < (T & 7) ? 1u : 0u), start = x * (T >> 3) + (x < (T & 7) ? x : (T & 7));  // its entries
    const uint32_t   my_n = cnt > j ? (cnt - j + wx - 1) / wx : 0u;
    if(my_n == 0) return;
    auto entry = [&](uint32_t i) {  // (uniform: every field through readfirstlane, so that what depends on it stays scalar)
        const SegTile &t = tiles[ start + j + i * wx ];
        SegTile        r;
        r.q0 = __builtin_amdgcn_readfirstlane(t.q0);
        r.nq = __builtin_amdgcn_readfirstlane(t.nq);
        r.col0 = __builtin_amdgcn_readfirstlane(t.col0);
        r.cols = __builtin_amdgcn_readfirstlane(t.cols);
        r.out = __builtin_amdgcn_readfirstlane(t.out);
        r.ld = __builtin_amdgcn_readfirstlane(t.ld);
        r.shape = __builtin_amdgcn_readfirstlane(t.shape);
        r.pad = 0;
        return r;
    };

    // ---- the load side: (tile li, k position lk), one step ahead of the MFMAs
    uint32_t li = 0, lk = 0, l_big = 0;
    u32x4    rq, rb;  // buffer descriptors as words: base, base_hi (stride 0), bytes, flags
    auto     make_desc = [](const float *base, uint32_t bytes) {
        const uint64_t a = (uint64_t)(uintptr_t)base;
        u32x4          d;
        d.x = (uint32_t)a;
        d.y = (uint32_t)(a >> 32) & 0xFFFFu;
        d.z = bytes;
        d.w = 0x00020000u;
        return d;
    };
    auto set_load_tile = [&](uint32_t i) {
        if(i < my_n) {
            const SegTile  t = entry(i);
            l_big = t.shape;
            // (the table is the host's; the counts are cut to the shape here, so that no entry can reach past its LDS rows' sources)
            const uint32_t ra = l_big ? kSegBigQ : kSegSkinnyQ, cb = l_big ? kSegBigCols : kSegSkinnyCols;
            rq = make_desc(Q + (size_t)t.q0 * stride, (t.nq < ra ? t.nq : ra) * stride * 4u);
            rb = make_desc(B + (size_t)t.col0 * stride, (t.cols < cb ? t.cols : cb) * stride * 4u);
        } else {
            l_big = 0;
            rq = make_desc(Q, 0);
            rb = make_desc(B, 0);
        }
    };
    auto lds_addr = [](const float *p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const float *)p; };
    // step (li, lk) into buffer Sp: row group g = 4 it + wave is LDS rows [8 g, 8 g + 8); the first ga groups are query rows.  (M0, the
    // LDS base of such a load, is written and used inside one statement; nothing else in this kernel touches it.)
    auto dma_step = [&](const float *Sp) {
        const uint32_t ga = l_big ? kSegBigQ / 8 : kSegSkinnyQ / 8, groups = l_big ? (kSegBigQ + kSegBigCols) / 8 : (kSegSkinnyQ + kSegSkinnyCols) / 8;
#pragma unroll
        for(uint32_t it = 0; it < SEG_ROWS / 32; ++it) {
            const uint32_t g = it * 4u + wu;
            if(g >= groups) continue;
            const bool     a = g < ga;
            const uint32_t row = (a ? g : g - ga) * 8u + ((uint32_t)lane >> 3);        // inside its matrix
            const uint32_t kq = (((uint32_t)lane & 7u) ^ ((row >> 1) & 7u)) * 4u;    // the k-quad this lane fetches
            const uint32_t off = lk + kq < stride ? (row * stride + lk + kq) * 4u : 0x80000000u;
            if(a) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds_addr(Sp + g * 256u)), "v"(off), "s"(rq) : "memory");
            else asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds_addr(Sp + g * 256u)), "v"(off), "s"(rb) : "memory");
        }
    };
    auto dma_wait = []() { asm volatile("s_waitcnt vmcnt(0)" : : : "memory"); };
    auto advance = [&]() {
        lk += BK;
        if(lk >= stride) {
            lk = 0;
            set_load_tile(++li);
        }
    };

    // ---- the compute side
    floatx16 acc[ 4 ];  // skinny: [column block]; 128 x 128: [2 row block + column block]
    auto     zero_acc = [&]() {
#pragma unroll
        for(int i = 0; i < 4; ++i)
#pragma unroll
            for(int r = 0; r < 16; ++r) acc[ i ][ r ] = 0.f;
    };
    zero_acc();
    uint32_t foff[ 4 ];
#pragma unroll
    for(int jq = 0; jq < 4; ++jq) foff[ jq ] = (((uint32_t)(2 * jq) + ((uint32_t)lane >> 5)) ^ (((uint32_t)lane >> 1) & 7u)) * 4u;
    const uint32_t wm = wu >> 1, wn = wu & 1;
    auto           step_skinny = [&](const float *Sp) {
        const float *Ap = Sp + (uint32_t)(lane & 31) * BK, *Bp = Sp + (kSegSkinnyQ + wu * 64u + (uint32_t)(lane & 31)) * BK;
#pragma unroll
        for(int jq = 0; jq < 4; ++jq) {
            const float4 a = *(const float4 *)(Ap + foff[ jq ]), b0 = *(const float4 *)(Bp + foff[ jq ]), b1 = *(const float4 *)(Bp + 32 * BK + foff[ jq ]);
            acc[ 0 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc[ 0 ], 0, 0, 0);
            acc[ 1 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc[ 1 ], 0, 0, 0);
            acc[ 0 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc[ 0 ], 0, 0, 0);
            acc[ 1 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc[ 1 ], 0, 0, 0);
            acc[ 0 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc[ 0 ], 0, 0, 0);
            acc[ 1 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc[ 1 ], 0, 0, 0);
            acc[ 0 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc[ 0 ], 0, 0, 0);
            acc[ 1 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc[ 1 ], 0, 0, 0);
        }
    };
    auto step_big = [&](const float *Sp) {
        const float *Ap = Sp + (wm * 64u + (uint32_t)(lane & 31)) * BK, *Bp = Sp + (kSegBigQ + wn * 64u + (uint32_t)(lane & 31)) * BK;
#pragma unroll
        for(int jq = 0; jq < 4; ++jq) {
            const float4 a0 = *(const float4 *)(Ap + foff[ jq ]), a1 = *(const float4 *)(Ap + 32 * BK + foff[ jq ]);
            const float4 b0 = *(const float4 *)(Bp + foff[ jq ]), b1 = *(const float4 *)(Bp + 32 * BK + foff[ jq ]);
#define LGPU_SEG_MFMA4(E)                                                                     \
    acc[ 0 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.E, b0.E, acc[ 0 ], 0, 0, 0);           \
    acc[ 1 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.E, b1.E, acc[ 1 ], 0, 0, 0);           \
    acc[ 2 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.E, b0.E, acc[ 2 ], 0, 0, 0);           \
    acc[ 3 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.E, b1.E, acc[ 3 ], 0, 0, 0);
            LGPU_SEG_MFMA4(x)
            LGPU_SEG_MFMA4(y)
            LGPU_SEG_MFMA4(z)
            LGPU_SEG_MFMA4(w)
#undef LGPU_SEG_MFMA4
        }
    };
    // ---- a tile's epilogue.  C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).  Block
    // (rows r0 + [0, 32), columns c0 + [0, 32)) of the tile: the query norms of its 32 rows sit one per lane and reach their rows by
    // a cross-lane read; only cells below the tile's counts are stored.
    auto block_out = [&](const SegTile &t, const floatx16 &v, uint32_t r0, uint32_t c0) {
        const uint32_t ql = r0 + (uint32_t)(lane & 31), c = c0 + (uint32_t)(lane & 31);
        const float    nqv = dense_tile_norm<METRIC == M_L2SQ>(ql < t.nq ? qn[ t.q0 + ql ] : 0.f);
        const float    nb2 = dense_tile_norm<METRIC == M_L2SQ>(c < t.cols ? bn[ t.col0 + c ] : 0.f);
        float *const   o = dd + t.out + c;
#pragma unroll
        for(int r = 0; r < 16; ++r) {
            const uint32_t rl = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * ((uint32_t)lane >> 5);
            const float    nq2 = __shfl(nqv, (int)rl, 64);
            const float    d = dense_tile_dist<METRIC == M_L2SQ>(v[ r ], nq2, nb2);
            if(r0 + rl < t.nq && c < t.cols) o[ (size_t)(r0 + rl) * t.ld ] = d;
        }
    };
    auto epilogue = [&](const SegTile &t) {
        if(t.shape == 0) {
            block_out(t, acc[ 0 ], 0u, wu * 64u);
            block_out(t, acc[ 1 ], 0u, wu * 64u + 32u);
        } else {
            block_out(t, acc[ 0 ], wm * 64u, wn * 64u);
            block_out(t, acc[ 1 ], wm * 64u, wn * 64u + 32u);
            block_out(t, acc[ 2 ], wm * 64u + 32u, wn * 64u);
            block_out(t, acc[ 3 ], wm * 64u + 32u, wn * 64u + 32u);
        }
    };

    // ---- fill the pipeline: the first step into buffer 0
    set_load_tile(0);
    dma_step(S[ 0 ]);
    advance();
    dma_wait();
    __syncthreads();
    const uint32_t KS = (stride + BK - 1) / BK;
    uint32_t       ti = 0, ks = 0, par = 0;
    SegTile        ct = entry(0);
    for(;;) {
        // the next step's loads go out first: the other buffer's last readers passed the barrier below a step ago.  (Nothing is issued
        // behind the workgroup's last step: no load is in flight when it ends.)
        if(li < my_n) {
            dma_step(S[ par ^ 1 ]);
            advance();
        }
        if(ct.shape == 0) step_skinny(S[ par ]);
        else step_big(S[ par ]);
        if(++ks == KS) {  // (the next tile's first step is already on its way)
            epilogue(ct);
            zero_acc();
            ks = 0;
            if(++ti == my_n) break;
            ct = entry(ti);
        }
        dma_wait();
        __syncthreads();  // the step's one barrier: the other buffer is complete for everyone, and this one has no reader left
        par ^= 1;
    }
}

// ---------------------------------------------------------------------------------------------------
// k_select_seg: k_select's per-query body (bruteforce.hip: the same (ordered distance << 32 | position) keys, the same kk survivors
// -- restated, so that k_select's code object stays as it was measured), one workgroup per (step, query) entry of a batch's
// selection table.  Entries that name the same best-list row cannot meet in one launch: a batch holds a query in one step only.
constexpr int SEG_SEL_BUF = 2048;

static __device__ void seg_bitonic_sort_lds(uint64_t *a, int n /* power of two */)
{
    for(int size = 2; size <= n; size <<= 1)
        for(int stride = size >> 1; stride > 0; stride >>= 1) {
            for(int i = threadIdx.x; i < n / 2; i += blockDim.x) {
                const int      lo = (i / stride) * stride * 2 + (i % stride), hi = lo + stride;
                const bool     up = ((lo / size) & 1) == 0;
                const uint64_t x = a[ lo ], y = a[ hi ];
                if((x > y) == up) { a[ lo ] = y; a[ hi ] = x; }
            }
            __syncthreads();
        }
}

__global__ void __launch_bounds__(256) k_select_seg(const float *dd, const SegQuery *queries, uint64_t *best, uint32_t kk)
{
    __shared__ uint64_t buf[ SEG_SEL_BUF ];
    __shared__ int      cnt;
    __shared__ uint64_t tau;
    const SegQuery  e = queries[ blockIdx.x ];
    const float    *row = dd + e.off;
    const uint32_t  ncols = e.cols, c_base = e.c_base;
    uint64_t       *mine = best + (size_t)e.row * kk;
    for(int i = threadIdx.x; i < SEG_SEL_BUF; i += blockDim.x) buf[ i ] = i < (int)kk ? mine[ i ] : ~0ull;
    if(threadIdx.x == 0) { cnt = (int)kk; tau = mine[ kk - 1 ]; }
    __syncthreads();
    for(uint32_t base = 0; base < ncols; base += blockDim.x * 4) {
        // 4 columns per thread per round; anything below the current k-th best goes to the buffer
        for(int u = 0; u < 4; ++u) {
            const uint32_t c = base + u * blockDim.x + threadIdx.x;
            if(c < ncols) {
                const uint64_t key = ((uint64_t)f2ord(row[ c ]) << 32) | (uint64_t)(c_base + c);
                if(key < tau) {
                    const int p = atomicAdd(&cnt, 1);
                    if(p < SEG_SEL_BUF) buf[ p ] = key;
                }
            }
        }
        __syncthreads();
        // at most 1024 new entries per round, so sorting whenever the buffer is more than half full guarantees the next round fits
        if(cnt > SEG_SEL_BUF / 2 || base + blockDim.x * 4 >= ncols) {
            int n2 = 64;  // the buffer holds cnt keys, ~0 beyond: sort the smallest power of two that covers them
            while(n2 < cnt && n2 < SEG_SEL_BUF) n2 <<= 1;
            seg_bitonic_sort_lds(buf, n2);
            for(int i = (int)kk + threadIdx.x; i < SEG_SEL_BUF; i += blockDim.x) buf[ i ] = ~0ull;
            if(threadIdx.x == 0) { cnt = (int)kk; tau = buf[ kk - 1 ]; }
            __syncthreads();
        }
    }
    for(int i = threadIdx.x; i < (int)kk; i += blockDim.x) mine[ i ] = buf[ i ];
}

// ---------------------------------------------------------------------------------------------------
hipError_t launch_dense_seg(int metric, const float *Q, const float *B, uint32_t stride, const float *qn, const float *bn, float *dd, const SegTile *tiles,
                            uint32_t n_tiles, hipStream_t stream)
{
    if(n_tiles == 0) return hipSuccess;
    // a lane's byte offset inside a tile's rows is 32 bits, and 0x80000000 has to stay out of every descriptor's range
    if(stride == 0 || stride % 4 != 0 || (uint64_t)stride * 4 * kSegSkinnyCols >= 0x80000000ull) return hipErrorInvalidValue;
    if(metric == M_L2SQ) hipLaunchKernelGGL((k_dense_seg<M_L2SQ>), dim3(dense_grid(n_tiles)), dim3(256), 0, stream, Q, B, stride, qn, bn, dd, tiles, n_tiles);
    else if(metric == M_COS) hipLaunchKernelGGL((k_dense_seg<M_COS>), dim3(dense_grid(n_tiles)), dim3(256), 0, stream, Q, B, stride, qn, bn, dd, tiles, n_tiles);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_select_seg(const float *dd, const SegQuery *queries, uint32_t n, uint64_t *best, uint32_t kk, hipStream_t stream)
{
    if(n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_select_seg, dim3(n), dim3(256), 0, stream, dd, queries, best, kk);
    return hipGetLastError();
}

}  // namespace lgpu
