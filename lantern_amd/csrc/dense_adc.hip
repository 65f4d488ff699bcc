// dense_adc.hip -- the exact k-NN's pre-selection on the CODE rows of a compact pq index by table lookups (lantern_gpu_set_exact_adc;
// DESIGN.md 4.5 "Compact pq indexes: ADC pre-selection").  k_dense_pq (dense_pq.hip) pays 2 d flops per (query, row) on 128-query tiles
// however few queries there are; here a (query, row) costs S byte-indexed LDS reads and S adds, and a row is read as its code bytes.
//
//   k_adc_tables   every query's table, once per call: [nq][S16][ADC_LUT_STRIDE] f32, entry (sv, c) = adc_build_table's fma chain of
//                  (q - c)^2 (l2sq) or q.c (cos) over subvector sv -- the ADC walk's bits; padding subvectors up to S16: entry 0 = +0.0
//   k_scan_adc     the scan.  A workgroup owns T queries (their tables in LDS) and a slab of the step's code rows; a lane owns a row.
//
// The keys only PRE-SELECT: k_select / launch_select_candidates, k_rerank_pq, k_certify and the fallback run behind this launch as they
// run behind k_dense_pq, and the certificate's bound covers these keys' error.
#include "kernels.hpp"
#include "adc_stage.hpp"
#include "dense_tile.hpp"

namespace lgpu {

// One workgroup per (block of `svb` subvectors, query): a lone query still spreads over S / svb workgroups.  adc_build_table is handed
// the block as if it were the whole table: its entries depend on nothing but their own subvector.
template <int METRIC>
__global__ void __launch_bounds__(256) k_adc_tables(const float *Q, uint32_t qfloats, const float *centers, uint32_t S, uint32_t C, uint32_t subdim, uint32_t S16,
                                                    uint32_t svb, float *tables)
{
    const uint32_t q = blockIdx.y, sv0 = blockIdx.x * svb, n = S - sv0 < svb ? S - sv0 : svb;
    float *const   lut = tables + (size_t)q * S16 * ADC_LUT_STRIDE;
    adc_build_table<METRIC, 4>(lut + (size_t)sv0 * ADC_LUT_STRIDE, centers + (size_t)sv0 * C * subdim, Q + (size_t)q * qfloats + (size_t)sv0 * subdim, n, C, subdim,
                               subdim, threadIdx.x, blockDim.x);
    if(blockIdx.x == 0)
        for(uint32_t sv = S + threadIdx.x; sv < S16; sv += blockDim.x) lut[ (size_t)sv * ADC_LUT_STRIDE ] = 0.f;
}

// ---------------------------------------------------------------------------------------------------
// Grid: x = row slabs of `slab_rows` rows, y = groups of T queries.  LDS: T tables of nch * 16 subvectors, nothing else -- a query's
// radius and norm are uniform values in registers.
//
// The tables arrive by 16-byte loads, the whole workgroup striding over the T contiguous tables of its group (queries past nq: not
// loaded; their lookups read whatever the LDS holds and their keys go nowhere).  Then lane l of the workgroup takes rows
// slab + l, slab + l + blockDim, ...: the row's nch chunks of 16 code bytes are requested together (a wave reads one contiguous run of
// 64 rows), and every code byte, extracted once, indexes the T tables.  acc[t] is ONE f32 chain per (row, query) in ascending
// subvector order, from +0.0: S - 1 roundings (0 + x is exact, and so is adding a padding subvector's +0.0).
// Key: l2sq -- the sum (non-negative: no clamp, no norms); cos -- dense_tile_dist's epilogue on (dot, 1 / |q|, 1 / |b|), its zero-norm rules.
// FUSED: DenseTopk's contract as k_dense_pq keeps it -- the radius is read once per workgroup.
template <int METRIC, bool FUSED, int T>
__global__ void __launch_bounds__(kAdcScanBlock) k_scan_adc(const uint8_t *codes, uint32_t nb, uint32_t row_bytes, uint32_t nch, const float *tables, uint32_t nq,
                                                            const float *qn, const float *bn, float *out, uint32_t ldo, DenseTopk tk, uint32_t slab_rows)
{
    constexpr bool L2 = METRIC == M_L2SQ;
    float *const   lut = (float *)lgpu_smem;
    const uint32_t tid = threadIdx.x, q0 = blockIdx.y * (uint32_t)T;
    const uint32_t tq = nq - q0 < (uint32_t)T ? nq - q0 : (uint32_t)T;  // the group's queries that exist
    const uint32_t tab = nch * 16u * (uint32_t)ADC_LUT_STRIDE;          // floats of a table
    {
        const float4 *const src = (const float4 *)(tables + (size_t)q0 * tab);
        float4 *const       dst = (float4 *)lut;
        for(uint32_t i = tid; i < tq * (tab / 4u); i += blockDim.x) dst[ i ] = src[ i ];
    }
    float qinv[ T ], rad[ T ];
#pragma unroll
    for(int t = 0; t < T; ++t) {
        const bool on = (uint32_t)t < tq;
        qinv[ t ] = L2 || !on ? 0.f : dense_tile_norm<false>(qn[ q0 + t ]);
        rad[ t ] = __builtin_nanf("");  // (nothing passes a NaN radius)
        if(FUSED && on) {  // the query's current radius: the distance of its kk-th best so far (all ones while the list is short)
            const uint32_t r = (uint32_t)(tk.best[ (size_t)(q0 + t) * tk.kk + tk.kk - 1 ] >> 32);
            rad[ t ] = r == 0xFFFFFFFFu ? __builtin_inff() : ord2f(r);
        }
    }
    __syncthreads();
    const uint32_t r0 = blockIdx.x * slab_rows, r1 = nb - r0 < slab_rows ? nb : r0 + slab_rows;
    for(uint32_t r = r0 + tid; r < r1; r += blockDim.x) {
        const uint4 *const row = (const uint4 *)(codes + (size_t)r * row_bytes);
        uint4              c[ 8 ];
#pragma unroll
        for(int i = 0; i < 8; ++i)
            if((uint32_t)i < nch) c[ i ] = row[ i ];  // (nch is uniform: scalar branches)
        float binv = 0.f;
        if(!L2) binv = dense_tile_norm<false>(bn[ r ]);
        float acc[ T ];
#pragma unroll
        for(int t = 0; t < T; ++t) acc[ t ] = 0.f;
#pragma unroll
        for(int i = 0; i < 8; ++i) {
            if((uint32_t)i < nch) {
                const float   *l = lut + (size_t)i * 16 * ADC_LUT_STRIDE;
                const uint32_t w[ 4 ] = { c[ i ].x, c[ i ].y, c[ i ].z, c[ i ].w };
#pragma unroll
                for(int j = 0; j < 4; ++j)
#pragma unroll
                    for(int b = 0; b < 4; ++b) {
                        const uint32_t e = (uint32_t)(j * 4 + b) * ADC_LUT_STRIDE + ((w[ j ] >> (8 * b)) & 255u);
#pragma unroll
                        for(int t = 0; t < T; ++t) acc[ t ] = acc[ t ] + l[ (size_t)t * tab + e ];
                    }
            }
        }
#pragma unroll
        for(int t = 0; t < T; ++t) {
            if((uint32_t)t >= tq) continue;
            const uint32_t q = q0 + (uint32_t)t;
            const float    d = L2 ? acc[ t ] : dense_tile_dist<false>(acc[ t ], qinv[ t ], binv);
            if constexpr(FUSED) {
                if(d <= rad[ t ]) {
                    const uint32_t p = atomicAdd(&tk.cnt[ q ], 1u);
                    if(p < tk.cap) tk.cand[ (size_t)q * tk.cap + p ] = ((uint64_t)f2ord(d) << 32) | (uint64_t)(tk.c_base + r);
                }
            } else {
                out[ (size_t)q * ldo + r ] = d;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// what both launchers check first: the scan's view of the operands.  S: subvectors (whole subvectors of cps chunks fill a decoded
// row); S16: the table's rows -- at most the code row's stride, which the index may have padded further (96 -> 128)
struct AdcShape { uint32_t S, S16, subdim, T; };
static bool adc_shape(int metric, const DensePqRows &pq, uint32_t chunks, AdcShape &s)
{
    if((metric != M_L2SQ && metric != M_COS) || !pq.centers || pq.cps == 0 || pq.C == 0 || pq.C > (uint32_t)ADC_LUT_STRIDE || chunks == 0 || chunks % pq.cps != 0)
        return false;
    s.S = chunks / pq.cps;
    s.S16 = (s.S + 15) / 16 * 16;
    s.subdim = pq.cps * 4;
    s.T = adc_scan_T(s.S16);
    return s.S16 <= 128 && s.S16 <= pq.row_bytes && pq.row_bytes % 16 == 0 && s.T != 0;
}

static uint32_t device_cus() { return dense_grid(0xFFFFFFFFu) / (uint32_t)DENSE_WGS_PER_CU; }

hipError_t launch_adc_tables(int metric, const uint4 *Q, uint32_t nq, uint32_t chunks, const DensePqRows &pq, float *tables, hipStream_t stream)
{
    if(nq == 0) return hipSuccess;
    AdcShape s;
    if(!adc_shape(metric, pq, chunks, s) || !Q || !tables || nq > 65535) return hipErrorInvalidValue;
    // subvectors per workgroup: four (1024 entries at 256 centroids: one pass of the 256 threads, four chains each) once the queries
    // alone cover the device, one below that
    const uint32_t svb = nq * ((s.S + 3) / 4) >= device_cus() ? 4u : 1u;
    const dim3     grid((s.S + svb - 1) / svb, nq);
    if(metric == M_L2SQ)
        hipLaunchKernelGGL((k_adc_tables<M_L2SQ_ADC>), grid, dim3(256), 0, stream, (const float *)Q, chunks * 4, (const float *)pq.centers, s.S, pq.C, s.subdim, s.S16, svb, tables);
    else
        hipLaunchKernelGGL((k_adc_tables<M_COS_ADC>), grid, dim3(256), 0, stream, (const float *)Q, chunks * 4, (const float *)pq.centers, s.S, pq.C, s.subdim, s.S16, svb, tables);
    return hipGetLastError();
}

template <int METRIC, bool FUSED>
static hipError_t launch_scan(const DenseOperands &o, const AdcShape &s, const float *tables, float *out, uint32_t ldo, const DenseTopk &tk, hipStream_t stream)
{
    // the grid: (row slabs x query groups).  Fewer groups than CUs: the rows are split until the grid covers the device, down to a
    // wave of rows per slab.  (One workgroup fits a CU: the tables take 64 .. 128 KB of its LDS.)
    const uint32_t groups = (o.nq + s.T - 1) / s.T, cus = device_cus();
    const uint32_t want = groups >= cus ? 1u : (cus + groups - 1) / groups;
    const uint32_t slab_rows = ((o.nb + want - 1) / want + 63) / 64 * 64, slabs = (o.nb + slab_rows - 1) / slab_rows;
    const size_t   lds = s.T * adc_table_bytes(s.S16);
    const dim3     grid(slabs, groups);
#define LGPU_SCAN(TT)                                                                                                                                      \
    LGPU_LAUNCH_LDS((k_scan_adc<METRIC, FUSED, TT>), grid, kAdcScanBlock, lds, stream, (const uint8_t *)o.B, o.nb, o.pq.row_bytes, s.S16 / 16, tables, o.nq, \
                    (const float *)o.qn, (const float *)o.bn, out, ldo, tk, slab_rows)
    if(s.T == 4) LGPU_SCAN(4) else if(s.T == 2) LGPU_SCAN(2) else LGPU_SCAN(1)
#undef LGPU_SCAN
    return hipGetLastError();
}

hipError_t launch_contraction_adc(const DenseOperands &o, const float *tables, float *out, uint32_t ldo, const DenseTopk *topk, hipStream_t stream)
{
    AdcShape s;
    if(o.kind != kDensePq || !adc_shape(o.metric, o.pq, o.chunks, s) || !tables || (!topk && !out) || (o.metric == M_COS && (!o.qn || !o.bn)))
        return hipErrorInvalidValue;
    if(o.nq == 0 || o.nb == 0) return hipSuccess;
    if((o.nq + s.T - 1) / s.T > 65535) return hipErrorInvalidValue;  // (gridDim.y)
    const DenseTopk none = { nullptr, 0, nullptr, nullptr, 0, 0 };
    if(o.metric == M_L2SQ) return !topk ? launch_scan<M_L2SQ, false>(o, s, tables, out, ldo, none, stream) : launch_scan<M_L2SQ, true>(o, s, tables, nullptr, 0u, *topk, stream);
    return !topk ? launch_scan<M_COS, false>(o, s, tables, out, ldo, none, stream) : launch_scan<M_COS, true>(o, s, tables, nullptr, 0u, *topk, stream);
}

}  // namespace lgpu
