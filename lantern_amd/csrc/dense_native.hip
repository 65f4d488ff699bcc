// dense_native.hip -- the dense contraction of the exact k-NN on rows that are STORED as f16 or i8, on the matrix cores' own
// operand types instead of an f32 copy:
//
//   k_row_norms_f16   ||x||^2 of f16 rows: every half unpacked exactly, one fmaf chain per lane, group_sum<G>
//   k_row_norms_i8    sum x^2 of i8 rows as an exact int32 (dot4 per word, integer group_sum); for cosine its IEEE square root,
//                     the one Acc<M_COS_I8>::finish takes
//   k_dense_native    D[q][c] for a 128 x 128 tile per workgroup, v_mfma_f32_32x32x16_f16 / v_mfma_i32_32x32x32_i8.
//                     f16: products of two halves are exact in f32, so the only error is the accumulation's -- the certificate
//                     of k_certify covers it with dims = 2 x halves contracted.  i8: the contraction is integer-exact and the
//                     epilogue repeats the pair kernel's operations, so the key IS the exact-order distance, bit for bit.
//
// The tile, the LDS image (128 rows x 128 bytes per matrix and buffer, 16-byte units XOR-swizzled), the LDS-direct buffer loads
// with their bounded descriptors, the XCD-aware tile order and the fused top-k epilogue are k_dense_f32's (bruteforce.hip, where
// each of them is explained); a K step is the same 128-byte slab per row -- 64 halves or 128 int8 -- and a 16-byte fragment
// read is exactly one A or B operand of these MFMAs, so a step is 16 MFMAs per wave where the f32 kernel has 64.
#include "kernels.hpp"
#include "walk.hpp"
#include "dense_tile.hpp"
#include "row_norms.hpp"

namespace lgpu {

typedef float    nat_f32x16 __attribute__((ext_vector_type(16)));
typedef int      nat_i32x16 __attribute__((ext_vector_type(16)));
typedef int      nat_i32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 nat_f16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------------
// (the arithmetic: NormAcc, row_norms.hpp -- shared with k_gather_rows_norms)
template <int G>
__global__ void __launch_bounds__(256) k_row_norms_f16(const uint4 *rows, uint32_t n, uint32_t chunks, float *out)
{
    const uint32_t gid = (blockIdx.x * blockDim.x + threadIdx.x) / G, gl = threadIdx.x % G;
    const uint32_t ngroups = gridDim.x * blockDim.x / G;
    for(uint32_t i = gid; i < n; i += ngroups) {
        const uint4 *r = rows + (size_t)i * chunks;
        NormAcc<1>   acc;
        for(uint32_t ch = gl; ch < chunks; ch += G) acc.add(r[ ch ]);
        const uint32_t s = acc.template finish<G>(0);
        if(gl == G - 1) out[ i ] = __uint_as_float(s);
    }
}

// out[i]: the int32 sum of squares (l2sq), or the bits of sqrtf((float)sum) (cosine)
template <int G>
__global__ void __launch_bounds__(256) k_row_norms_i8(const uint4 *rows, uint32_t n, uint32_t chunks, uint32_t *out, int cosine)
{
    const uint32_t gid = (blockIdx.x * blockDim.x + threadIdx.x) / G, gl = threadIdx.x % G;
    const uint32_t ngroups = gridDim.x * blockDim.x / G;
    for(uint32_t i = gid; i < n; i += ngroups) {
        const uint4 *r = rows + (size_t)i * chunks;
        NormAcc<2>   acc;
        for(uint32_t ch = gl; ch < chunks; ch += G) acc.add(r[ ch ]);
        const uint32_t s = acc.template finish<G>(cosine);
        if(gl == G - 1) out[ i ] = s;
    }
}

// ---------------------------------------------------------------------------------------------------
constexpr int KIND_F16 = 1, KIND_I8 = 2;  // (lantern_gpu_plan_dense's operand kinds)

template <int KIND> struct NativeMfma;
template <> struct NativeMfma<KIND_F16>
{
    typedef nat_f32x16 acc_t;
    static __device__ __forceinline__ acc_t mfma(const uint4 &a, const uint4 &b, acc_t c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(nat_f16x8, a), __builtin_bit_cast(nat_f16x8, b), c, 0, 0, 0);
    }
};
template <> struct NativeMfma<KIND_I8>
{
    typedef nat_i32x16 acc_t;
    static __device__ __forceinline__ acc_t mfma(const uint4 &a, const uint4 &b, acc_t c)
    {
        return __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(nat_i32x4, a), __builtin_bit_cast(nat_i32x4, b), c, 0, 0, 0);
    }
};

// Q, B: rows of `stride` 32-bit words (whole 16-byte chunks, zero padded); qn, bn: what the norm kernels above wrote, as words.
// The pipeline is k_dense_f32's over two LDS buffers -- loads of step s + 1 land while step s is on the matrix cores, step s + 2
// is issued into this step's buffer behind the step's one barrier -- dealt out over four rounds of 4 MFMAs:
//   round 0..2   read the next round's fragments (one 16-byte read per lane and row block), then the round's MFMAs
//   behind 2     wait for this wave's loads of step s + 1, the barrier: the other buffer is complete for everyone and this one
//                has no reader left (its last fragment reads were issued before round 2's MFMAs)
//   round 3      issue all of step s + 2's loads into this buffer, read round 0's fragments of step s + 1, the round's MFMAs
template <int KIND, int METRIC, bool FUSED>
__global__ void __launch_bounds__(256, 2) k_dense_native(const uint32_t *Q, uint32_t nq, const uint32_t *B, uint32_t nb, uint32_t stride /* words per row */,
                                                      const uint32_t *qn, const uint32_t *bn, float *out, uint32_t ldo, DenseTopk tk)
{
    typedef typename NativeMfma<KIND>::acc_t acc_t;
    __shared__ uint32_t A_0[ BM * BK ], A_1[ BM * BK ], B_0[ BN * BK ], B_1[ BN * BK ];
    __shared__ uint32_t Ns[ 2 ][ 3 * 128 ];  // per tile parity: 128 query norms, 128 base norms, 128 query radii (float bits)
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

    acc_t acc[ 2 ][ 2 ];
    auto  zero_acc = [&]() {
#pragma unroll
        for(int i = 0; i < 2; ++i)
#pragma unroll
            for(int jj = 0; jj < 2; ++jj)
#pragma unroll
                for(int r = 0; r < 16; ++r) acc[ i ][ jj ][ r ] = 0;
    };
    zero_acc();

    // ---- the load side of the pipeline: (tile li, k position lk in words), up to two steps ahead of the MFMAs
    const int      wu = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t kq = (((uint32_t)lane & 7u) ^ (((uint32_t)wu * 4u + ((uint32_t)lane >> 4)) & 7u)) * 4u;  // the 16-byte unit this lane fetches
    const uint32_t voff = ((uint32_t)(wu * 8 + (lane >> 3)) * stride + kq) * 4u, vstep = 32u * stride * 4u;
    uint32_t       li = 0, lk = 0;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 rq, rb;  // buffer descriptors as words: base, base_hi (stride 0), bytes, flags
    auto  make_desc = [](const uint32_t *base, uint32_t bytes) {
        const uint64_t a = (uint64_t)(uintptr_t)base;
        u32x4          d;
        d.x = __builtin_amdgcn_readfirstlane((uint32_t)a);  // (uniform values: said so, so that the descriptors stay scalar)
        d.y = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32) & 0xFFFFu);
        d.z = __builtin_amdgcn_readfirstlane(bytes);
        d.w = 0x00020000u;
        return d;
    };
    auto set_load_tile = [&](uint32_t i) {
        if(i < my_n) {
            uint32_t q0, c0;
            tile_origin(i, q0, c0);
            const uint32_t rows_q = nq - q0 < (uint32_t)BM ? nq - q0 : (uint32_t)BM, rows_b = nb - c0 < (uint32_t)BN ? nb - c0 : (uint32_t)BN;
            rq = make_desc(Q + (size_t)q0 * stride, rows_q * stride * 4u);
            rb = make_desc(B + (size_t)c0 * stride, rows_b * stride * 4u);
        } else {  // past this workgroup's last tile: empty descriptors, every load returns zeros
            rq = make_desc(Q, 0);
            rb = make_desc(B, 0);
        }
    };
    // (inline assembly and the explicit wait: see k_dense_f32)
    auto lds_addr = [](const uint32_t *p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const uint32_t *)p; };
    auto dma1 = [&](int it, const uint32_t *Ap, const uint32_t *Bp) {
        const uint32_t off = lk + kq < stride ? voff + (uint32_t)it * vstep + lk * 4u : 0x80000000u;
        // (the descriptors are uniform; where the compiler carries one through the loop in vector registers all the same, this
        // brings it back to the scalar ones the instruction needs -- and is nothing where it did not)
        auto scalar = [](u32x4 d) {
            d.x = __builtin_amdgcn_readfirstlane(d.x);
            d.y = __builtin_amdgcn_readfirstlane(d.y);
            d.z = __builtin_amdgcn_readfirstlane(d.z);
            d.w = __builtin_amdgcn_readfirstlane(d.w);
            return d;
        };
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds_addr(Ap + (it * 4 + wu) * 256)), "v"(off), "s"(scalar(rq)) : "memory");
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds_addr(Bp + (it * 4 + wu) * 256)), "v"(off), "s"(scalar(rb)) : "memory");
    };
    auto dma_wait = []() { asm volatile("s_waitcnt vmcnt(0)" : : : "memory"); };
    auto advance = [&]() {
        lk += BK;
        if(lk >= stride) {
            lk = 0;
            set_load_tile(++li);
        }
    };
    // ---- a tile's norms and radii: loaded a tile ahead into two registers, written to LDS in the tile's first step
    uint32_t nreg = 0, rreg = 0;
    auto     load_norms = [&](uint32_t i) {
        uint32_t q0, c0;
        tile_origin(i, q0, c0);
        nreg = tid < BM ? (q0 + tid < nq ? qn[ q0 + tid ] : 0u) : (c0 + (tid - BM) < nb ? bn[ c0 + (tid - BM) ] : 0u);
        if(FUSED && tid < BM)  // the query's current radius: the distance of its kk-th best so far (all ones while the list is short)
            rreg = q0 + tid < nq ? (uint32_t)(tk.best[ (size_t)(q0 + tid) * tk.kk + tk.kk - 1 ] >> 32) : 0u;
    };
    auto store_norms = [&](uint32_t par) {
        uint32_t nv = nreg;
        if(KIND == KIND_F16 && METRIC != M_L2SQ) {  // f16 cosine: 1 / sqrt(norm), 0 stays 0 (as k_dense_f32)
            const float f = __uint_as_float(nv);
            nv = __float_as_uint(f == 0.f ? 0.f : 1.f / __builtin_sqrtf(f));
        }
        Ns[ par ][ tid ] = nv;
        if(FUSED && tid < BM) Ns[ par ][ 256 + tid ] = __float_as_uint(rreg == 0xFFFFFFFFu ? __builtin_inff() : ord2f(rreg));  // (rows past nq: NaN, nothing passes)
    };
    // ---- fragments: one 16-byte read per lane, row block and round: half h = lane / 32 reads unit 2 j + h of its row, which is
    // the lane's whole operand of one MFMA (8 halves / 16 int8); A and B take the same units, so the contraction index is
    // permuted the same way on both sides
    uint32_t foff[ 4 ];
#pragma unroll
    for(int jq = 0; jq < 4; ++jq) foff[ jq ] = (((uint32_t)(2 * jq) + ((uint32_t)lane >> 5)) ^ (((uint32_t)lane >> 1) & 7u)) * 4u;
    const uint32_t rowa = (uint32_t)(wm * 64 + (lane & 31)) * BK, rowb = (uint32_t)(wn * 64 + (lane & 31)) * BK;
    uint4          fa[ 2 ][ 2 ], fb[ 2 ][ 2 ];  // [fragment set][row block]
    auto           frag = [&](int set, const uint32_t *Ap, const uint32_t *Bp, int jq) {
        fa[ set ][ 0 ] = *(const uint4 *)(Ap + rowa + foff[ jq ]);
        fa[ set ][ 1 ] = *(const uint4 *)(Ap + rowa + 32 * BK + foff[ jq ]);
        fb[ set ][ 0 ] = *(const uint4 *)(Bp + rowb + foff[ jq ]);
        fb[ set ][ 1 ] = *(const uint4 *)(Bp + rowb + 32 * BK + foff[ jq ]);
    };
    auto mfma4 = [&](int set) {
        acc[ 0 ][ 0 ] = NativeMfma<KIND>::mfma(fa[ set ][ 0 ], fb[ set ][ 0 ], acc[ 0 ][ 0 ]);
        acc[ 0 ][ 1 ] = NativeMfma<KIND>::mfma(fa[ set ][ 0 ], fb[ set ][ 1 ], acc[ 0 ][ 1 ]);
        acc[ 1 ][ 0 ] = NativeMfma<KIND>::mfma(fa[ set ][ 1 ], fb[ set ][ 0 ], acc[ 1 ][ 0 ]);
        acc[ 1 ][ 1 ] = NativeMfma<KIND>::mfma(fa[ set ][ 1 ], fb[ set ][ 1 ], acc[ 1 ][ 1 ]);
    };
    // plain-output variant: the finished tile's distances leave through a register stash, one part per K step of the next tile
    // (k_dense_f32 has the reason)
    nat_f32x16 stash[ 2 ][ 2 ];
    uint32_t   st_q0 = 0, st_c0 = 0;
    int        st_done = 8;
    auto       flush_part = [&](auto part_c) {
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
        // C/D layout of the 32x32 MFMAs (f32 and i32 alike): col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        uint32_t q0, c0;
        tile_origin(ti, q0, c0);
        if constexpr(!FUSED) {
            flush_rest();  // (a tile of fewer than eight K steps: the previous one's parts have not all left yet)
            st_q0 = q0;
            st_c0 = c0;
        }
        const uint32_t *Nq = Ns[ ti & 1 ], *Nb = Ns[ ti & 1 ] + 128, *Nr = Ns[ ti & 1 ] + 256;
        const bool      interior = q0 + (uint32_t)BM <= nq && c0 + (uint32_t)BN <= nb;  // (uniform)
        if constexpr(!FUSED) st_done = interior ? 0 : 8;
#pragma unroll
        for(int i = 0; i < 2; ++i)
#pragma unroll
            for(int jj = 0; jj < 2; ++jj) {
                const int      cl = wn * 64 + jj * 32 + (lane & 31);
                const uint32_t c = c0 + (uint32_t)cl;
                const uint32_t nbw = Nb[ cl ];
                auto           dist_of = [&](int r, auto dotv) {
                    const uint32_t nqw = Nq[ wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) ];
                    float          d;
                    if constexpr(KIND == KIND_I8) {
                        // the pair kernel's distance, operation for operation (Acc<M_L2SQ_I8> / Acc<M_COS_I8>::finish)
                        const int ab = (int)dotv;
                        if(METRIC == M_L2SQ) {
                            d = (float)(int)(nqw + nbw - 2u * (uint32_t)ab);
                        } else {
                            const float sa = __uint_as_float(nqw), sb = __uint_as_float(nbw);  // the stored roots: 0 exactly when the sum is 0
                            if(sa == 0.f && sb == 0.f) d = 0.f;
                            else if(sa == 0.f || sb == 0.f) d = 1.f;
                            else d = 1.f - (float)ab / (sa * sb);
                        }
                    } else {
                        const float dot = (float)dotv, nq2 = __uint_as_float(nqw), nb2 = __uint_as_float(nbw);
                        if(METRIC == M_L2SQ) {
                            d = nq2 + nb2 - 2.f * dot;
                            d = d < 0.f ? 0.f : d;
                        } else {
                            if(nq2 == 0.f && nb2 == 0.f) d = 0.f;  // (nq2 / nb2 hold the INVERSE roots here)
                            else if(nq2 == 0.f || nb2 == 0.f) d = 1.f;
                            else d = 1.f - dot * (nq2 * nb2);
                        }
                    }
                    return d;
                };
                if constexpr(FUSED) {
                    uint32_t pass = 0;
#pragma unroll
                    for(int r = 0; r < 16; ++r) {
                        const int ql = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        pass |= (dist_of(r, acc[ i ][ jj ][ r ]) <= __uint_as_float(Nr[ ql ]) ? 1u : 0u) << r;
                    }
                    if(c >= nb) pass = 0;
                    while(pass) {
                        const int r = __builtin_ctz(pass);
                        pass &= pass - 1;
                        auto dot = acc[ i ][ jj ][ 0 ];
#pragma unroll
                        for(int rr = 1; rr < 16; ++rr)
                            if(rr == r) dot = acc[ i ][ jj ][ rr ];
                        const float    d = dist_of(r, dot);
                        const uint32_t q = q0 + (uint32_t)(wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5));
                        const uint32_t p = atomicAdd(&tk.cnt[ q ], 1u);
                        if(p < tk.cap) tk.cand[ (size_t)q * tk.cap + p ] = ((uint64_t)f2ord(d) << 32) | (uint64_t)(tk.c_base + c);
                    }
                } else {
                    if(interior) {
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
            }
    };
    // ---- fill the pipeline: steps 0 and 1 into the two LDS buffers
    set_load_tile(0);
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
#define LGPU_NATIVE_STEP(P)                                                         \
    {                                                                               \
        uint32_t *const Ap = (P) ? A_1 : A_0, *const Bp = (P) ? B_1 : B_0;          \
        uint32_t *const Ao = (P) ? A_0 : A_1, *const Bo = (P) ? B_0 : B_1;          \
        frag(1, Ap, Bp, 1);                                                         \
        LGPU_FENCE;                                                                 \
        mfma4(0);                                                                   \
        LGPU_FENCE;                                                                 \
        frag(0, Ap, Bp, 2);                                                         \
        LGPU_FENCE;                                                                 \
        mfma4(1);                                                                   \
        LGPU_FENCE;                                                                 \
        frag(1, Ap, Bp, 3);                                                         \
        LGPU_FENCE;                                                                 \
        mfma4(0);                                                                   \
        LGPU_FENCE;                                                                 \
        dma_wait();                                                                 \
        __syncthreads();                                                            \
        if constexpr(!FUSED) flush_next(); /* one part of the previous tile's distances: a whole step to drain */ \
        if(ks == 0) { /* (behind the wait for the loads: the norms' own load is long done) */ \
            store_norms(ti & 1);                                                    \
            if(ti + 1 < my_n) load_norms(ti + 1);                                   \
        }                                                                           \
        dma1(0, Ap, Bp);                                                            \
        dma1(1, Ap, Bp);                                                            \
        dma1(2, Ap, Bp);                                                            \
        dma1(3, Ap, Bp);                                                            \
        advance();                                                                  \
        frag(0, Ao, Bo, 0);                                                         \
        LGPU_FENCE;                                                                 \
        mfma4(1);                                                                   \
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
        LGPU_NATIVE_STEP(0)
        LGPU_NATIVE_STEP(1)
    }
    if constexpr(!FUSED) flush_rest();  // the workgroup's last tile
#undef LGPU_NATIVE_STEP
#undef LGPU_FENCE
}

// ---------------------------------------------------------------------------------------------------
hipError_t launch_norms_native(int kind, int metric, const uint4 *rows, uint32_t n, uint32_t chunks, uint32_t *out, hipStream_t stream)
{
    if(n == 0) return hipSuccess;
    if(kind != KIND_F16 && kind != KIND_I8) return hipErrorInvalidValue;
    const int G_ = group_lanes_for(chunks);
    uint32_t  blocks = (uint32_t)(((uint64_t)n * G_ + 255) / 256);
    if(blocks > 16384) blocks = 16384;
    const int cosine = metric == M_COS ? 1 : 0;
#define NN(GG)                                                                                                                 \
    if(kind == KIND_F16) hipLaunchKernelGGL((k_row_norms_f16<GG>), dim3(blocks), dim3(256), 0, stream, rows, n, chunks, (float *)out); \
    else hipLaunchKernelGGL((k_row_norms_i8<GG>), dim3(blocks), dim3(256), 0, stream, rows, n, chunks, out, cosine)
    switch(G_) {
        case 64: NN(64); break;
        case 32: NN(32); break;
        case 16: NN(16); break;
        default: NN(8);
    }
#undef NN
    return hipGetLastError();
}

template <bool FUSED>
static hipError_t launch_native(const DenseOperands &o, float *out, uint32_t ldo, const DenseTopk &tk, hipStream_t stream)
{
    if(o.nq == 0 || o.nb == 0) return hipSuccess;
    if((o.metric != M_L2SQ && o.metric != M_COS) || (o.kind != KIND_F16 && o.kind != KIND_I8)) return hipErrorInvalidValue;
    const uint32_t stride = o.chunks * 4;
    const uint32_t tiles = ((o.nq + BM - 1) / BM) * ((o.nb + BN - 1) / BN);
#define DN(KK, MM)                                                                                                                          \
    hipLaunchKernelGGL((k_dense_native<KK, MM, FUSED>), dim3(dense_grid(tiles)), dim3(256), 0, stream, (const uint32_t *)o.Q, o.nq, (const uint32_t *)o.B, \
                       o.nb, stride, (const uint32_t *)o.qn, (const uint32_t *)o.bn, out, ldo, tk)
    if(o.kind == KIND_F16) {
        if(o.metric == M_L2SQ) DN(KIND_F16, M_L2SQ);
        else DN(KIND_F16, M_COS);
    } else {
        if(o.metric == M_L2SQ) DN(KIND_I8, M_L2SQ);
        else DN(KIND_I8, M_COS);
    }
#undef DN
    return hipGetLastError();
}

hipError_t launch_contraction_native(const DenseOperands &o, float *out, uint32_t ldo, const DenseTopk *topk, hipStream_t stream)
{
    const DenseTopk none = { nullptr, 0, nullptr, nullptr, 0, 0 };
    return !topk ? launch_native<false>(o, out, ldo, none, stream) : launch_native<true>(o, (float *)nullptr, 0u, *topk, stream);
}

}  // namespace lgpu
