// dense_pq.hip -- the exact k-NN's kernels on the CODE rows of a compact pq index (lantern_gpu_set_exact_compact):
// the index keeps num_subvectors code bytes per row in HBM and nothing here writes a decoded copy of them.
//
//   k_dense_pq         k_dense_f32's contraction (bruteforce.hip: the 128 x 128 tile, BK = 32, the persistent grid, the XCD-aware tile
//                      order, one barrier per K step, the fused top-k epilogue) with a B tile that is GATHERED: a 16-byte slot of the
//                      tile is chunk `off` of centroid codes[row][sv] of subvector sv, fetched from the L2-resident centroid tables by
//                      the same LDS-direct load, whose per-lane offset now carries the gather as well as the XOR swizzle.  The values
//                      that land in LDS are PqdRow's (device_common.hpp), so the matrix is k_dense_f32's over the decoded rows bit for bit.
//   k_row_norms_pq     k_row_norms over PqdRow: the expanded index's norm words
//   k_rerank_pq        k_rerank for M_L2SQ_PQD / M_COS_PQD: the survivors' exact-order distances over PqdRow, as the walk forms them
//   k_pq_decode_rows   a chunk of code rows decoded for the exact-order fallback (k_pairs + k_select run on it unchanged)
#include "kernels.hpp"
#include "walk.hpp"
#include "dense_tile.hpp"
#include "row_norms.hpp"

namespace lgpu {

typedef float floatx16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ PqdRow pq_row(const uint8_t *codes, const DensePqRows &pq, size_t row)
{
    return PqdRow{ codes + row * pq.row_bytes, pq.centers, pq.cps, pq.C, pq.inv };
}

// ---------------------------------------------------------------------------------------------------
// The pipeline is k_dense_f32's, step for step (its comment explains the half-rounds); what differs is the load side of B.
//
// A lane owns the same four slots of the B slab in every K step: rows lrow + 32 it (it = 0..3) at chunk-in-step cq -- the k-quad the
// swizzle gives it.  At the step whose first chunk is k0 that is decoded chunk ch = k0 + cq of each of the four rows: subvector
// sv = (ch * inv) >> 16, chunk off = ch - sv * cps inside it -- ONE subvector and offset for all four rows, worked out once per step
// (`cb`: the byte offset of chunk `off` of centroid 0 of sv; pushed out of the descriptor's range when ch is past the row).  A
// subvector narrower than a step (cps = 1: the row's eight lanes read eight code bytes) or one that straddles two steps (cps = 5)
// is nothing special: every slot does its own arithmetic.
//
// The code byte is a dependent load in front of the centroid load.  It runs ONE STEP AHEAD of it, in registers: the loads of step
// s + 2 are issued in step s behind the barrier; right behind them the load cursor advances to step s + 3 and the lane reads ITS four
// code bytes of that step (code_fetch: four global_load_ubyte, L1 / L2 hits -- the 256 lanes share the tile's code rows, at most
// 16 KB) into cbyte[].  They are first touched a whole step later, behind step s + 1's wait for its loads, where the four centroid
// offsets cb + code * cps * 16 are formed and the loads of step s + 3 issued.  Six registers (four bytes, cb, the row mask), no LDS:
// two workgroups per CU as k_dense_f32.
// Branch-free as k_dense_f32: the centroid descriptor spans the tables and nothing else; a row past the tile's last (the code byte
// is then read from the tile's last row, inside the block) and a chunk past the row push the offset out of its range and land as zeros.
template <int METRIC, bool FUSED = false>
__global__ void __launch_bounds__(256, 2) k_dense_pq(const float *Q, uint32_t nq, const uint8_t *codes, uint32_t nb, uint32_t stride /* floats per decoded row */,
                                                  DensePqRows pq, const float *qn, const float *bn, float *out, uint32_t ldo, DenseTopk tk)
{
    constexpr bool L2 = METRIC == M_L2SQ;
    __shared__ float A_0[ BM * BK ], A_1[ BM * BK ], B_0[ BN * BK ], B_1[ BN * BK ];
    __shared__ float Ns[ 2 ][ 3 * 128 ];  // per tile parity: 128 query norms, 128 base norms (cosine: inverse roots), 128 query radii
    const int        tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int        wm = wave >> 1, wn = wave & 1;
    const uint32_t   tiles_m = (nq + BM - 1) / BM, T = tiles_m * ((nb + BN - 1) / BN);
    const uint32_t   x = blockIdx.x & 7, j = blockIdx.x >> 3;
    const uint32_t   wx = (gridDim.x - x + 7) >> 3;  // workgroups on this XCD
    const uint32_t   cnt = (T >> 3) + (x < (T & 7) ? 1u : 0u), start = x * (T >> 3) + (x < (T & 7) ? x : (T & 7));  // its tiles
    const uint32_t   my_n = cnt > j ? (cnt - j + wx - 1) / wx : 0u;
    if(my_n == 0) return;
    auto tile_origin = [&](uint32_t i, uint32_t &q0, uint32_t &c0) {
        const uint32_t lin = start + j + i * wx;
        q0 = (lin % tiles_m) * BM;
        c0 = (lin / tiles_m) * BN;
    };

    floatx16 acc[ 2 ][ 2 ];
    auto     zero_acc = [&]() {
#pragma unroll
        for(int i = 0; i < 2; ++i)
#pragma unroll
            for(int jj = 0; jj < 2; ++jj)
#pragma unroll
                for(int r = 0; r < 16; ++r) acc[ i ][ jj ][ r ] = 0.f;
    };
    zero_acc();

    // ---- the load side of the pipeline: (tile li, k position lk), up to two steps ahead of the MFMAs; the code bytes a third
    const int      wu = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t cq = ((uint32_t)lane & 7u) ^ (((uint32_t)wu * 4u + ((uint32_t)lane >> 4)) & 7u);  // the chunk of a step this lane fetches
    const uint32_t kq = cq * 4u, lrow = (uint32_t)(wu * 8 + (lane >> 3));
    const uint32_t voff = (lrow * stride + kq) * 4u, vstep = 32u * stride * 4u;
    const uint32_t chunks = stride >> 2, cpsb = pq.cps * 16u;
    uint32_t       li = 0, lk = 0;
    uint32_t       lc0 = 0, lrows = 0;  // the load tile's first base row and how many it has (0: past this workgroup's last tile)
    uint32_t       cbyte[ 4 ] = { 0, 0, 0, 0 }, cb = 0x80000000u, rmask = 0;  // of step (li, lk): the lane's code bytes, its centroid-0 offset, its rows that exist
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 rq;  // buffer descriptors as words: base, base_hi (stride 0), bytes, flags
    auto  make_desc = [](const void *base, uint32_t bytes) {
        const uint64_t a = (uint64_t)(uintptr_t)base;
        u32x4          d;
        d.x = (uint32_t)a;
        d.y = (uint32_t)(a >> 32) & 0xFFFFu;
        d.z = bytes;
        d.w = 0x00020000u;
        return d;
    };
    const u32x4 rb = make_desc(pq.centers, chunks * pq.C * 16u);  // [S][C][cps] chunks: S cps = the row's chunks (host-checked below 2^31 bytes)
    auto        set_load_tile = [&](uint32_t i) {
        if(i < my_n) {
            uint32_t q0, c0;
            tile_origin(i, q0, c0);
            const uint32_t rows_q = nq - q0 < (uint32_t)BM ? nq - q0 : (uint32_t)BM;
            rq = make_desc(Q + (size_t)q0 * stride, rows_q * stride * 4u);
            lc0 = c0;
            lrows = nb - c0 < (uint32_t)BN ? nb - c0 : (uint32_t)BN;
        } else {  // past this workgroup's last tile: an empty descriptor and no rows, every load returns zeros
            rq = make_desc(Q, 0);
            lrows = 0;
        }
    };
    auto code_fetch = [&]() {
        const uint32_t ch = (lk >> 2) + cq;
        const bool     kin = ch < chunks;
        const uint32_t sv = kin ? (ch * pq.inv) >> 16 : 0u, off = ch - sv * pq.cps;
        cb = kin ? (sv * pq.C * pq.cps + off) * 16u : 0x80000000u;
        rmask = 0;
        if(lrows != 0) {  // (uniform)
#pragma unroll
            for(int it = 0; it < 4; ++it) {
                const uint32_t r = lrow + 32u * (uint32_t)it;
                const bool     in = r < lrows;
                cbyte[ it ] = codes[ (size_t)(lc0 + (in ? r : lrows - 1u)) * pq.row_bytes + sv ];
                rmask |= (in ? 1u : 0u) << it;
            }
        }
    };
    auto lds_addr = [](const float *p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const float *)p; };
    // (as k_dense_f32: inline assembly, M0 written and used inside one statement.  The compiler does not count these loads; the code
    // bytes' plain loads it does count, and a wait it places for them can only wait for more than they need)
    auto dma1 = [&](int it, const float *Ap, const float *Bp) {
        const uint32_t off = lk + kq < stride ? voff + (uint32_t)it * vstep + lk * 4u : 0x80000000u;
        const uint32_t goff = (rmask >> it) & 1u ? cb + cbyte[ it ] * cpsb : 0x80000000u;  // (cb out of range stays out of range: + at most 2^24)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds_addr(Ap + (it * 4 + wu) * 256)), "v"(off), "s"(rq) : "memory");
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds_addr(Bp + (it * 4 + wu) * 256)), "v"(goff), "s"(rb) : "memory");
    };
    auto dma_wait = []() { asm volatile("s_waitcnt vmcnt(0)" : : : "memory"); };
    auto advance = [&]() {  // to the next step, and its code bytes on their way
        lk += BK;
        if(lk >= stride) {
            lk = 0;
            set_load_tile(++li);
        }
        code_fetch();
    };
    // ---- a tile's norms and radii: loaded a tile ahead into two registers, written to LDS in the tile's first step
    float    nreg = 0.f;
    uint32_t rreg = 0;
    auto     load_norms = [&](uint32_t i) {
        uint32_t q0, c0;
        tile_origin(i, q0, c0);
        nreg = tid < BM ? (q0 + tid < nq ? qn[ q0 + tid ] : 0.f) : (c0 + (tid - BM) < nb ? bn[ c0 + (tid - BM) ] : 0.f);
        if(FUSED && tid < BM)  // the query's current radius: the distance of its kk-th best so far (all ones while the list is short)
            rreg = q0 + tid < nq ? (uint32_t)(tk.best[ (size_t)(q0 + tid) * tk.kk + tk.kk - 1 ] >> 32) : 0u;
    };
    auto store_norms = [&](uint32_t par) {
        Ns[ par ][ tid ] = dense_tile_norm<L2>(nreg);
        if(FUSED && tid < BM) Ns[ par ][ 256 + tid ] = rreg == 0xFFFFFFFFu ? __builtin_inff() : ord2f(rreg);  // (rows past nq: ord2f(0) = NaN, nothing passes)
    };
    // ---- fragments (k_dense_f32's: one 16-byte read per lane, row block and round)
    uint32_t foff[ 4 ];
#pragma unroll
    for(int jq = 0; jq < 4; ++jq) foff[ jq ] = (((uint32_t)(2 * jq) + ((uint32_t)lane >> 5)) ^ (((uint32_t)lane >> 1) & 7u)) * 4u;
    const uint32_t rowa = (uint32_t)(wm * 64 + (lane & 31)) * BK, rowb = (uint32_t)(wn * 64 + (lane & 31)) * BK;
    float4         fa[ 2 ][ 2 ], fb[ 2 ][ 2 ];  // [fragment set][row block]
    auto           frag = [&](int set, const float *Ap, const float *Bp, int jq) {
        fa[ set ][ 0 ] = *(const float4 *)(Ap + rowa + foff[ jq ]);
        fa[ set ][ 1 ] = *(const float4 *)(Ap + rowa + 32 * BK + foff[ jq ]);
        fb[ set ][ 0 ] = *(const float4 *)(Bp + rowb + foff[ jq ]);
        fb[ set ][ 1 ] = *(const float4 *)(Bp + rowb + 32 * BK + foff[ jq ]);
    };
    auto mfma4 = [&](float a0, float a1, float b0, float b1) {
        acc[ 0 ][ 0 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[ 0 ][ 0 ], 0, 0, 0);
        acc[ 0 ][ 1 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[ 0 ][ 1 ], 0, 0, 0);
        acc[ 1 ][ 0 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[ 1 ][ 0 ], 0, 0, 0);
        acc[ 1 ][ 1 ] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[ 1 ][ 1 ], 0, 0, 0);
    };
    auto mfma8 = [&](int set, int h) {  // h = 0: e = 0, 1;  h = 1: e = 2, 3
        if(h == 0) {
            mfma4(fa[ set ][ 0 ].x, fa[ set ][ 1 ].x, fb[ set ][ 0 ].x, fb[ set ][ 1 ].x);
            mfma4(fa[ set ][ 0 ].y, fa[ set ][ 1 ].y, fb[ set ][ 0 ].y, fb[ set ][ 1 ].y);
        } else {
            mfma4(fa[ set ][ 0 ].z, fa[ set ][ 1 ].z, fb[ set ][ 0 ].z, fb[ set ][ 1 ].z);
            mfma4(fa[ set ][ 0 ].w, fa[ set ][ 1 ].w, fb[ set ][ 0 ].w, fb[ set ][ 1 ].w);
        }
    };
    // plain-output variant: the finished tile's distances leave from a register stash, one of eight parts per K step of the next tile
    // (k_dense_f32 says why)
    floatx16 stash[ 2 ][ 2 ];
    uint32_t st_q0 = 0, st_c0 = 0;
    int      st_done = 8;
    auto     flush_part = [&](auto part_c) {
        constexpr int part = decltype(part_c)::value, i = part >> 2, jj = (part >> 1) & 1, h = part & 1;
        const uint32_t c = st_c0 + (uint32_t)(wn * 64 + jj * 32 + (lane & 31));
#pragma unroll
        for(int r = 8 * h; r < 8 * h + 8; ++r) {
            const uint32_t q = st_q0 + (uint32_t)(wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5));
            out[ (size_t)q * ldo + c ] = stash[ i ][ jj ][ r ];
        }
    };
    auto flush_range = [&](int from, int to) {  // parts [from, to) that have not left yet
        const int d = __builtin_amdgcn_readfirstlane(st_done);
        if(d <= 0 && 0 >= from && 0 < to) flush_part(std::integral_constant<int, 0>{});
        if(d <= 1 && 1 >= from && 1 < to) flush_part(std::integral_constant<int, 1>{});
        if(d <= 2 && 2 >= from && 2 < to) flush_part(std::integral_constant<int, 2>{});
        if(d <= 3 && 3 >= from && 3 < to) flush_part(std::integral_constant<int, 3>{});
        if(d <= 4 && 4 >= from && 4 < to) flush_part(std::integral_constant<int, 4>{});
        if(d <= 5 && 5 >= from && 5 < to) flush_part(std::integral_constant<int, 5>{});
        if(d <= 6 && 6 >= from && 6 < to) flush_part(std::integral_constant<int, 6>{});
        if(d <= 7 && 7 >= from && 7 < to) flush_part(std::integral_constant<int, 7>{});
    };
    auto flush_next = [&]() {
        const int d = __builtin_amdgcn_readfirstlane(st_done);
        if(d >= 8) return;
        flush_range(d, d + 1);
        st_done = d + 1;
    };
    auto flush_rest = [&]() {
        flush_range(0, 8);
        st_done = 8;
    };
    auto epilogue = [&](uint32_t ti) {
        // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        uint32_t q0, c0;
        tile_origin(ti, q0, c0);
        if constexpr(!FUSED) {
            flush_rest();  // (a tile of fewer than eight K steps: the previous one's parts have not all left yet)
            st_q0 = q0;
            st_c0 = c0;
        }
        const float *Nq = Ns[ ti & 1 ], *Nb = Ns[ ti & 1 ] + 128, *Nr = Ns[ ti & 1 ] + 256;
        const bool   interior = q0 + (uint32_t)BM <= nq && c0 + (uint32_t)BN <= nb;  // (uniform)
        if constexpr(!FUSED) st_done = interior ? 0 : 8;
#pragma unroll
        for(int i = 0; i < 2; ++i)
#pragma unroll
            for(int jj = 0; jj < 2; ++jj) {
                const int      cl = wn * 64 + jj * 32 + (lane & 31);
                const uint32_t c = c0 + (uint32_t)cl;
                const float    nb2 = Nb[ cl ];
                auto           dist_of = [&](int r, float dot) {
                    return dense_tile_dist<L2>(dot, Nq[ wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) ], nb2);
                };
                if constexpr(FUSED) {
                    // which of the 16 outputs are inside their query's radius (NaN never passes; rows past nq carry a NaN radius), then
                    // the rare appends
                    uint32_t pass = 0;
#pragma unroll
                    for(int r = 0; r < 16; ++r) {
                        const int ql = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        pass |= (dist_of(r, acc[ i ][ jj ][ r ]) <= Nr[ ql ] ? 1u : 0u) << r;
                    }
                    if(c >= nb) pass = 0;
                    while(pass) {
                        const int r = __builtin_ctz(pass);
                        pass &= pass - 1;
                        float dot = 0.f;
#pragma unroll
                        for(int rr = 0; rr < 16; ++rr)
                            if(rr == r) dot = acc[ i ][ jj ][ rr ];
                        const float    d = dist_of(r, dot);
                        const uint32_t q = q0 + (uint32_t)(wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5));
                        const uint32_t p = atomicAdd(&tk.cnt[ q ], 1u);
                        if(p < tk.cap) tk.cand[ (size_t)q * tk.cap + p ] = ((uint64_t)f2ord(d) << 32) | (uint64_t)(tk.c_base + c);
                    }
                } else if(interior) {
#pragma unroll
                    for(int r = 0; r < 16; ++r) stash[ i ][ jj ][ r ] = dist_of(r, acc[ i ][ jj ][ r ]);
                } else {
#pragma unroll
                    for(int r = 0; r < 16; ++r) {
                        const uint32_t q = q0 + (uint32_t)(wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5));
                        const float    d = dist_of(r, acc[ i ][ jj ][ r ]);
                        if(q < nq && c < nb) out[ (size_t)q * ldo + c ] = d;
                    }
                }
            }
    };
    // ---- fill the pipeline: steps 0 and 1 into the two LDS buffers (their code bytes are waited for where the offsets are formed)
    set_load_tile(0);
    code_fetch();
    load_norms(0);
#pragma unroll
    for(int it = 0; it < 4; ++it) dma1(it, A_0, B_0);
    advance();
#pragma unroll
    for(int it = 0; it < 4; ++it) dma1(it, A_1, B_1);
    advance();
    dma_wait();
    __syncthreads();
    frag(0, A_0, B_0, 0);
    const uint32_t KS = (stride + BK - 1) / BK;
    uint32_t       ti = 0, ks = 0;
#define LGPU_FENCE __builtin_amdgcn_sched_barrier(0)
#define LGPU_DENSE_PQ_STEP(P)                                                       \
    {                                                                               \
        float *const Ap = (P) ? A_1 : A_0, *const Bp = (P) ? B_1 : B_0;             \
        float *const Ao = (P) ? A_0 : A_1, *const Bo = (P) ? B_0 : B_1;             \
        frag(1, Ap, Bp, 1);                                                         \
        LGPU_FENCE;                                                                 \
        mfma8(0, 0);                                                                \
        mfma8(0, 1);                                                                \
        LGPU_FENCE;                                                                 \
        frag(0, Ap, Bp, 2);                                                         \
        LGPU_FENCE;                                                                 \
        mfma8(1, 0);                                                                \
        mfma8(1, 1);                                                                \
        LGPU_FENCE;                                                                 \
        frag(1, Ap, Bp, 3);                                                         \
        LGPU_FENCE;                                                                 \
        mfma8(0, 0);                                                                \
        LGPU_FENCE;                                                                 \
        dma_wait(); /* this wave's loads of step s + 1 -- and the code bytes of step s + 2, fetched a step ago */ \
        __syncthreads();                                                            \
        if constexpr(!FUSED) flush_next();                                          \
        if(ks == 0) {                                                               \
            store_norms(ti & 1);                                                    \
            if(ti + 1 < my_n) load_norms(ti + 1);                                   \
        }                                                                           \
        mfma8(0, 1);                                                                \
        LGPU_FENCE;                                                                 \
        dma1(0, Ap, Bp);                                                            \
        dma1(1, Ap, Bp);                                                            \
        frag(0, Ao, Bo, 0);                                                         \
        LGPU_FENCE;                                                                 \
        mfma8(1, 0);                                                                \
        LGPU_FENCE;                                                                 \
        dma1(2, Ap, Bp);                                                            \
        dma1(3, Ap, Bp);                                                            \
        advance();                                                                  \
        LGPU_FENCE;                                                                 \
        mfma8(1, 1);                                                                \
        LGPU_FENCE;                                                                 \
        if(++ks == KS) {                                                            \
            if(KS == 1) __syncthreads(); /* the norms were written after this step's only barrier */ \
            epilogue(ti);                                                           \
            zero_acc();                                                             \
            ks = 0;                                                                 \
            if(++ti == my_n) break;                                                 \
        }                                                                           \
    }
    for(;;) {
        LGPU_DENSE_PQ_STEP(0)
        LGPU_DENSE_PQ_STEP(1)
    }
    if constexpr(!FUSED) flush_rest();  // the workgroup's last tile
#undef LGPU_DENSE_PQ_STEP
#undef LGPU_FENCE
}

// ---------------------------------------------------------------------------------------------------
// k_row_norms (bruteforce.hip) over decoded chunks: the same lane chain (chunks gl, gl + G, ...), the same group_sum<G>
template <int G>
__global__ void __launch_bounds__(256) k_row_norms_pq(const uint8_t *codes, uint32_t n, uint32_t chunks, DensePqRows pq, float *out)
{
    const uint32_t gid = (blockIdx.x * blockDim.x + threadIdx.x) / G, gl = threadIdx.x % G;
    const uint32_t ngroups = gridDim.x * blockDim.x / G;
    for(uint32_t i = gid; i < n; i += ngroups) {
        const PqdRow r = pq_row(codes, pq, i);
        NormAcc<0>   acc;
        for(uint32_t ch = gl; ch < chunks; ch += G) acc.add(r[ (int)ch ]);
        const uint32_t s = acc.template finish<G>(0);
        if(gl == G - 1) out[ i ] = __uint_as_float(s);
    }
}

// k_rerank over code rows: group_dist<M_*_PQD> is Acc<M_*> over PqdRow -- the walk's distance of a compact index, the expanded index's
// bits.  The kk <= 256 keys (distance, slot) are distinct, so a key's place in the order is the number of keys below it: counted,
// not sorted.
template <int METRIC, int G>
__global__ void __launch_bounds__(256) k_rerank_pq(const uint4 *Q, const uint8_t *codes, uint32_t chunks, DensePqRows pq, const uint64_t *best, uint32_t kk,
                                                   uint32_t k, uint32_t *out_slots, float *out_dists)
{
    __shared__ uint64_t keys[ 256 ];
    const uint32_t q = blockIdx.x;
    const int      tid = threadIdx.x, g = tid / G, gl = tid % G, NG = 256 / G;
    keys[ tid ] = ~0ull;
    __syncthreads();
    for(uint32_t i = g; i < kk; i += NG) {
        const uint64_t cand = best[ (size_t)q * kk + i ];
        if(cand == ~0ull) continue;
        const uint32_t slot = (uint32_t)(cand & 0xFFFFFFFFu);
        const float    d = group_dist<METRIC, G>(Q + (size_t)q * chunks, pq_row(codes, pq, slot), (int)chunks, gl);
        if(gl == G - 1) keys[ i ] = ((uint64_t)f2ord(d) << 32) | slot;
    }
    __syncthreads();
    const uint64_t key = keys[ tid ];
    const uint32_t have = (uint32_t)__syncthreads_count(key != ~0ull);
    if(key != ~0ull) {
        uint32_t rank = 0;
        for(int o = 0; o < 256; ++o) rank += keys[ o ] < key ? 1u : 0u;
        if(rank < k) {
            out_slots[ (size_t)q * k + rank ] = (uint32_t)(key & 0xFFFFFFFFu);
            out_dists[ (size_t)q * k + rank ] = ord2f((uint32_t)(key >> 32));
        }
    }
    for(uint32_t i = have + (uint32_t)tid; i < k; i += 256) {
        out_slots[ (size_t)q * k + i ] = EMPTY;
        out_dists[ (size_t)q * k + i ] = __builtin_inff();
    }
}

__global__ void __launch_bounds__(256) k_pq_decode_rows(const uint8_t *codes, uint32_t n, uint32_t chunks, DensePqRows pq, uint4 *dst)
{
    const size_t total = (size_t)n * chunks;
    for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        dst[ i ] = pq_row(codes, pq, i / chunks)[ (int)(i % chunks) ];
}

// ---------------------------------------------------------------------------------------------------
// what every launcher here checks first: PqdRow's arithmetic holds (the host verified `inv` for rows of up to 4096 chunks), the rows
// are whole subvectors, and the centroid tables fit the contraction's 32-bit byte offsets with room for the out-of-range marker
static bool pq_rows_ok(const DensePqRows &pq, uint32_t chunks)
{
    return pq.centers && pq.cps != 0 && pq.inv != 0 && pq.C != 0 && pq.C <= 256 && chunks != 0 && chunks <= 4096 && chunks % pq.cps == 0 &&
           chunks / pq.cps <= pq.row_bytes;
}

template <bool FUSED> static hipError_t launch_pq(const DenseOperands &o, float *out, uint32_t ldo, const DenseTopk &tk, hipStream_t stream)
{
    if(o.nq == 0 || o.nb == 0) return hipSuccess;
    if((o.metric != M_L2SQ && o.metric != M_COS) || !pq_rows_ok(o.pq, o.chunks)) return hipErrorInvalidValue;
    const uint32_t tiles = ((o.nq + BM - 1) / BM) * ((o.nb + BN - 1) / BN), stride = o.chunks * 4;
    if(o.metric == M_L2SQ)
        hipLaunchKernelGGL((k_dense_pq<M_L2SQ, FUSED>), dim3(dense_grid(tiles)), dim3(256), 0, stream, (const float *)o.Q, o.nq, (const uint8_t *)o.B, o.nb, stride,
                           o.pq, (const float *)o.qn, (const float *)o.bn, out, ldo, tk);
    else
        hipLaunchKernelGGL((k_dense_pq<M_COS, FUSED>), dim3(dense_grid(tiles)), dim3(256), 0, stream, (const float *)o.Q, o.nq, (const uint8_t *)o.B, o.nb, stride,
                           o.pq, (const float *)o.qn, (const float *)o.bn, out, ldo, tk);
    return hipGetLastError();
}

hipError_t launch_contraction_pq(const DenseOperands &o, float *out, uint32_t ldo, const DenseTopk *topk, hipStream_t stream)
{
    const DenseTopk none = { nullptr, 0, nullptr, nullptr, 0, 0 };
    return !topk ? launch_pq<false>(o, out, ldo, none, stream) : launch_pq<true>(o, (float *)nullptr, 0u, *topk, stream);
}

hipError_t launch_norms_pq(const DensePqRows &pq, const uint4 *rows, uint32_t n, uint32_t chunks, float *out, hipStream_t stream)
{
    if(n == 0) return hipSuccess;
    if(!pq_rows_ok(pq, chunks)) return hipErrorInvalidValue;
    const int G_ = group_lanes_for(chunks);
    uint32_t  blocks = (uint32_t)(((uint64_t)n * G_ + 255) / 256);
    if(blocks > 16384) blocks = 16384;
#define NP(GG) hipLaunchKernelGGL((k_row_norms_pq<GG>), dim3(blocks), dim3(256), 0, stream, (const uint8_t *)rows, n, chunks, pq, out)
    switch(G_) { case 64: NP(64); break; case 32: NP(32); break; case 16: NP(16); break; default: NP(8); }
#undef NP
    return hipGetLastError();
}

hipError_t launch_rerank_pq(int metric, const DensePqRows &pq, const uint4 *Q, uint32_t nq, const uint4 *B, uint32_t chunks, const uint64_t *best, uint32_t kk,
                            uint32_t k, uint32_t *out_slots, float *out_dists, hipStream_t stream)
{
    if(nq == 0) return hipSuccess;
    if(!pq_rows_ok(pq, chunks) || kk > 256 || k > kk || (metric != M_L2SQ_PQD && metric != M_COS_PQD)) return hipErrorInvalidValue;
    const int G_ = group_lanes_for(chunks);
#define RP(MM, GG) hipLaunchKernelGGL((k_rerank_pq<MM, GG>), dim3(nq), dim3(256), 0, stream, Q, (const uint8_t *)B, chunks, pq, best, kk, k, out_slots, out_dists)
#define RPG(MM) switch(G_) { case 64: RP(MM, 64); break; case 32: RP(MM, 32); break; case 16: RP(MM, 16); break; default: RP(MM, 8); }
    if(metric == M_L2SQ_PQD) RPG(M_L2SQ_PQD) else RPG(M_COS_PQD)
#undef RPG
#undef RP
    return hipGetLastError();
}

hipError_t launch_pq_decode_rows(const DensePqRows &pq, const uint4 *rows, uint32_t n, uint32_t chunks, uint4 *dst, hipStream_t stream)
{
    if(n == 0) return hipSuccess;
    if(!pq_rows_ok(pq, chunks)) return hipErrorInvalidValue;
    const size_t blocks = std::min<size_t>(((size_t)n * chunks + 255) / 256, 16384);
    hipLaunchKernelGGL(k_pq_decode_rows, dim3((uint32_t)blocks), dim3(256), 0, stream, (const uint8_t *)rows, n, chunks, pq, dst);
    return hipGetLastError();
}

}  // namespace lgpu
