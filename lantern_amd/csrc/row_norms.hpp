// row_norms.hpp -- the norm word of one row as the dense contractions read it (DenseOperands::qn / bn), written once: one lane's
// chain over the row's chunks gl, gl + G, ... in order, then group_sum<G>.  k_row_norms (bruteforce.hip), k_row_norms_f16 /
// k_row_norms_i8 (dense_native.hip) and k_gather_rows_norms (bruteforce.hip) all accumulate through NormAcc, so a norm has the same
// bits whichever kernel wrote it and the certificate's bound covers them alike.
#pragma once
#include "kernels.hpp"
#include "walk.hpp"

namespace lgpu {

// KIND: DenseOperands::kind -- 0 f32 rows, 1 f16 rows, 2 i8 rows; kNormNone: rows that carry no norm (bit rows; rows that are
// dequantised before they are contracted, whose norms are taken on the copy)
constexpr int kNormNone = 3;

template <int KIND> struct NormAcc;
template <> struct NormAcc<0>  // ||x||^2 in f32: one fmaf chain per lane
{
    float s = 0.f;
    __device__ __forceinline__ void add(const uint4 &x)
    {
        s = __builtin_fmaf(__uint_as_float(x.x), __uint_as_float(x.x), s);
        s = __builtin_fmaf(__uint_as_float(x.y), __uint_as_float(x.y), s);
        s = __builtin_fmaf(__uint_as_float(x.z), __uint_as_float(x.z), s);
        s = __builtin_fmaf(__uint_as_float(x.w), __uint_as_float(x.w), s);
    }
    template <int G> __device__ __forceinline__ uint32_t finish(int) { return __float_as_uint(group_sum<G>(s)); }
};
template <> struct NormAcc<1>  // f16 rows: every half unpacked exactly, the same chain
{
    float s = 0.f;
    __device__ __forceinline__ void add(const uint4 &x)
    {
        const uint32_t w[ 4 ] = { x.x, x.y, x.z, x.w };
#pragma unroll
        for(int j = 0; j < 4; ++j) {
            float lo, hi;
            unpack_h2(w[ j ], lo, hi);
            s = __builtin_fmaf(lo, lo, s);
            s = __builtin_fmaf(hi, hi, s);
        }
    }
    template <int G> __device__ __forceinline__ uint32_t finish(int) { return __float_as_uint(group_sum<G>(s)); }
};
template <> struct NormAcc<2>  // i8 rows: the exact int32 sum of squares (l2sq), or the bits of its IEEE root (cosine)
{
    int s = 0;
    __device__ __forceinline__ void add(const uint4 &x)
    {
        s = dot4_i8(x.x, x.x, s);
        s = dot4_i8(x.y, x.y, s);
        s = dot4_i8(x.z, x.z, s);
        s = dot4_i8(x.w, x.w, s);
    }
    template <int G> __device__ __forceinline__ uint32_t finish(int cosine)
    {
        const uint32_t a2 = group_sum<G>((uint32_t)s);
        return cosine ? __float_as_uint(__builtin_sqrtf((float)(int)a2)) : a2;
    }
};
template <> struct NormAcc<kNormNone>
{
    __device__ __forceinline__ void add(const uint4 &) {}
    template <int G> __device__ __forceinline__ uint32_t finish(int) { return 0u; }
};

}  // namespace lgpu
