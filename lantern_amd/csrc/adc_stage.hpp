// adc_stage.hpp -- what an ADC kernel stages in LDS for one query before it evaluates a row: the raw f32 query row, the per-query table
// (RowAcc<M_*_ADC>, device_common.hpp, reads it from the first LDS bytes) and, for cosine, |query|.  k_search_adc
// (search_adc_kernel.hip) and the filtered kernels over ADC rows (search_filtered_kernel.hpp) stage through this one body, so a row
// has the same distance bits in all of them.  PARITY UNPINNED BY THE REFERENCE (search_adc_kernel.hip has the definition).
#pragma once
#include "walk.hpp"

namespace lgpu {


// The per-query table: one thread per (subvector, centroid) entry, one fma chain each.  B entries per thread at a time, their
// centroid loads issued together: the table of centroids comes from L2 (786 KB per query at 96 x 256 x 8), and one chain per
// thread at a time left the loads' latency bare -- 35 round trips per query, a third of a query's time at ef = 64.
template <int METRIC, int B>
__device__ __forceinline__ void adc_build_table(float *lut, const float *centers, const float *rawq, uint32_t S, uint32_t C, uint32_t subdim, uint32_t sub_floats,
                                                uint32_t tid, uint32_t T)
{
    for(uint32_t e0 = tid; e0 < S * C; e0 += B * T) {
        const float *cent[ B ], *qs[ B ];
        float        acc[ B ];
        bool         on[ B ];
#pragma unroll
        for(int u = 0; u < B; ++u) {
            const uint32_t e = e0 + (uint32_t)u * T;
            on[ u ] = e < S * C;
            const uint32_t ee = on[ u ] ? e : 0u, sv = ee / C, c = ee % C;
            cent[ u ] = centers + ((size_t)sv * C + c) * sub_floats;
            qs[ u ] = rawq + (size_t)sv * subdim;
            acc[ u ] = 0.f;
        }
        for(uint32_t j4 = 0; j4 < sub_floats; j4 += 4) {
            float4 cv[ B ];
#pragma unroll
            for(int u = 0; u < B; ++u) cv[ u ] = *(const float4 *)(cent[ u ] + j4);  // (rows of the centroid table are padded to whole float4s)
#pragma unroll
            for(int u = 0; u < B; ++u) {
                const float cj[ 4 ] = { cv[ u ].x, cv[ u ].y, cv[ u ].z, cv[ u ].w };
#pragma unroll
                for(int jj = 0; jj < 4; ++jj) {
                    if(j4 + (uint32_t)jj < subdim) {
                        const float qv = qs[ u ][ j4 + (uint32_t)jj ];
                        if constexpr(METRIC == M_L2SQ_ADC) {
                            const float t = qv - cj[ jj ];
                            acc[ u ] = __builtin_fmaf(t, t, acc[ u ]);
                        } else {
                            acc[ u ] = __builtin_fmaf(qv, cj[ jj ], acc[ u ]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for(int u = 0; u < B; ++u) {
            const uint32_t e = e0 + (uint32_t)u * T;
            if(on[ u ]) lut[ (size_t)(e / C) * ADC_LUT_STRIDE + e % C ] = acc[ u ];
        }
    }
}

// Stage query q: its raw row (qchunks chunks) into rawq4, the table into lut (S subvectors x C centroids of `subdim` dimensions; the
// padding rows up to S16, the code row's width, get entry 0 = +0.0: a padding code is 0 and adds nothing), and for cosine |query| into
// S_QN2 by the chain and tree the f32 cosine kernels use for a row of qchunks chunks.  Every thread of the workgroup calls it; it ends
// in a barrier, and nothing of an earlier query survives it.
template <int METRIC>
__device__ __forceinline__ void adc_stage(const int tid, const int T, WalkLds &s, float *lut, uint4 *rawq4, const uint4 *queries, uint32_t q, const float *centers,
                                          uint32_t S, uint32_t C, uint32_t subdim, uint32_t qchunks, uint32_t S16)
{
    const float *const rawq = (const float *)rawq4;
    const uint32_t     sub_floats = ((subdim + 3) / 4) * 4;
    for(uint32_t i = tid; i < qchunks; i += T) rawq4[ i ] = queries[ (size_t)q * qchunks + i ];
    __syncthreads();
    adc_build_table<METRIC, 4>(lut, centers, rawq, S, C, subdim, sub_floats, (uint32_t)tid, (uint32_t)T);  // (8 and 16 at a time: no faster)
    for(uint32_t sv = S + tid; sv < S16; sv += T) lut[ (size_t)sv * ADC_LUT_STRIDE ] = 0.f;
    if constexpr(METRIC == M_COS_ADC) {
        const int Gq = group_lanes_for(qchunks);
        if(tid < Gq) {
            float qn;
            switch(Gq) {
                case 64: qn = group_norm<M_COS, 64>(rawq4, (int)qchunks, tid); break;
                case 32: qn = group_norm<M_COS, 32>(rawq4, (int)qchunks, tid); break;
                case 16: qn = group_norm<M_COS, 16>(rawq4, (int)qchunks, tid); break;
                default: qn = group_norm<M_COS, 8>(rawq4, (int)qchunks, tid); break;
            }
            if(tid == Gq - 1) s.scal[ S_QN2 ] = __float_as_int(qn);
        }
    }
    __syncthreads();
}

}  // namespace lgpu
