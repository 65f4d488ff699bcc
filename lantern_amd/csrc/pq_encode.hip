// pq_encode.hip -- product quantisation of f32 rows in ONE launch (DESIGN.md 4.7 "Encoding in one launch").
//
//   k_pq_encode<METRIC, SC>   a block of rows x a strip of subvectors -> the strip's code bytes of every row
//   plan_pq_encode            pure: is a shape served, and how the launch is cut (lantern_gpu_plan_pq_encode shows it without a device)
//   launch_pq_encode          the one launcher, dispatching on (METRIC, SC)
//   lantern_gpu_pq_encode     the stateless entry point: quantize_vector over a table of rows
//
// What a code byte is does not change: per (row, subvector) the centroid c with the smallest make_key(D, c), where D is the pair
// kernel's exact-order distance group_dist<METRIC, 8>(subvector, centroid) of the subvector zero padded to SC chunks -- what
// launch_pq_take + exact_knn_device(k = 1) + launch_pq_put find per subvector.  With SC <= 8 every lane of the pair kernel's 8-lane
// group owns AT MOST ONE chunk, so one thread can form D alone: the SC chunk partials come out of Acc<METRIC>::add itself, the lanes
// without a chunk contribute the 0.f their accumulators start from, and the butterfly with offsets 1, 2, 4 as the group's LAST lane
// sees it is the fixed tree ((p7 + p6) + (p5 + p4)) + ((p0 + p1) + (p2 + p3)).  There is no cross-lane step and no matrix instruction:
// an MFMA contraction would order the sums differently and would need the certificate and the re-rank this kernel exists to avoid.
//
// The split: a workgroup of 256 threads owns kPqEncodeRows rows x a strip of T consecutive subvectors (T from the host: the fewest
// subvectors whose floats cover whole 128-byte lines of a row, as far as S and the LDS allow).  LDS image, dynamic, <= 64 KB:
//   [ T ][ C ][ SC ] uint4    the strip's centroid tables, copied once per workgroup (contiguous in Index::d_centers)
//   [ T * subdim ][ 256 ] f32 the strip's floats of the 256 rows, COLUMN by column: float j of row r at [ j ][ (r + j) & 255 ]
// The rows are read with a wave on contiguous bytes of a row (16-byte loads where the strip is 16-byte aligned) and written to LDS
// transposed; the rotation by j spreads both the transposing writes (fixed r, consecutive j) and the later reads (fixed j, consecutive
// r) over the banks.  Each thread then pulls its own row's subvector into registers, zero padded as k_pq_take pads it, and walks
// c = 0 .. C - 1: every lane reads the SAME centroid (an LDS broadcast), forms D and keeps the smallest key.
#include <algorithm>
#include <cstring>
#include <vector>

#include "abi_guard.hpp"
#include "dense.hpp"
#include "index.hpp"

namespace lgpu {

namespace {

// the 8-lane butterfly (offsets 1, 2, 4) as lane 7 evaluates it, on partials of which only the first SC are not the initial 0.f
template <int SC> __device__ __forceinline__ float lone_group_sum(const float (&p)[ SC ])
{
    float q[ 8 ];
#pragma unroll
    for(int l = 0; l < 8; ++l) q[ l ] = l < SC ? p[ l ] : 0.f;
    return ((q[ 7 ] + q[ 6 ]) + (q[ 5 ] + q[ 4 ])) + ((q[ 0 ] + q[ 1 ]) + (q[ 2 ] + q[ 3 ]));
}

// group_dist<METRIC, 8>(x, y, SC, .) in its last lane, by one thread
template <int METRIC, int SC> __device__ __forceinline__ float lone_dist(const uint4 (&x)[ SC ], const uint4 *y)
{
    Acc<METRIC> lane[ SC ];  // lane l's accumulator: its one chunk
#pragma unroll
    for(int l = 0; l < SC; ++l) lane[ l ].add(x[ l ], y[ l ]);
    if constexpr(METRIC == M_COS) {
        float ab[ SC ], a2[ SC ], b2[ SC ];
#pragma unroll
        for(int l = 0; l < SC; ++l) ab[ l ] = lane[ l ].ab, a2[ l ] = lane[ l ].a2, b2[ l ] = lane[ l ].b2;
        return cos_finish(lone_group_sum<SC>(ab), lone_group_sum<SC>(a2), lone_group_sum<SC>(b2));  // Acc<M_COS>::finish's rules and expression
    } else {
        float s[ SC ];
#pragma unroll
        for(int l = 0; l < SC; ++l) s[ l ] = lane[ l ].s;
        return lone_group_sum<SC>(s);
    }
}

struct PqEncodeLaunch : PqEncodeArgs
{
    uint32_t T;     // subvectors of a strip (plan_pq_encode)
    uint32_t vec4;  // rows, row_floats and T * subdim allow 16-byte loads of a strip
};

template <int METRIC, int SC> __global__ void __launch_bounds__(256) k_pq_encode(const PqEncodeLaunch a)
{
    const uint32_t tid = threadIdx.x, r0 = blockIdx.x * kPqEncodeRows, sv0 = blockIdx.y * a.T;
    const uint32_t Tn = a.S - sv0 < a.T ? a.S - sv0 : a.T, W = Tn * a.subdim;  // the strip: subvectors, floats
    const uint32_t nrows = a.count - r0 < kPqEncodeRows ? a.count - r0 : kPqEncodeRows;
    uint4 *const   tab = (uint4 *)lgpu_smem;
    float *const   cols = (float *)(lgpu_smem + (size_t)a.T * a.C * SC * 16);

    const uint4 *const src = (const uint4 *)a.centers + (size_t)sv0 * a.C * SC;
    for(uint32_t i = tid; i < Tn * a.C * SC; i += 256) tab[ i ] = src[ i ];

    const float *const base = a.rows + (size_t)r0 * a.row_floats + (size_t)sv0 * a.subdim;
    if(a.vec4 && W % 4 == 0) {
        const uint32_t W4 = W / 4;
        for(uint32_t i = tid; i < nrows * W4; i += 256) {
            const uint32_t r = i / W4, j = (i - r * W4) * 4;
            const float4   v = *(const float4 *)(base + (size_t)r * a.row_floats + j);
            cols[ (j + 0) * 256 + ((r + j + 0) & 255) ] = v.x;
            cols[ (j + 1) * 256 + ((r + j + 1) & 255) ] = v.y;
            cols[ (j + 2) * 256 + ((r + j + 2) & 255) ] = v.z;
            cols[ (j + 3) * 256 + ((r + j + 3) & 255) ] = v.w;
        }
    } else {
        for(uint32_t i = tid; i < nrows * W; i += 256) {
            const uint32_t r = i / W, j = i - r * W;
            cols[ j * 256 + ((r + j) & 255) ] = base[ (size_t)r * a.row_floats + j ];
        }
    }
    __syncthreads();
    if(tid >= nrows) return;

    const size_t row = (size_t)r0 + tid;
    for(uint32_t t = 0; t < Tn; ++t) {
        uint4 x[ SC ];  // the thread's subvector, zero padded to SC chunks
#pragma unroll
        for(int l = 0; l < SC; ++l) {
            float f[ 4 ];
#pragma unroll
            for(int e = 0; e < 4; ++e) {
                const uint32_t j = (uint32_t)(l * 4 + e), col = t * a.subdim + j;
                f[ e ] = j < a.subdim ? cols[ col * 256 + ((tid + col) & 255) ] : 0.f;
            }
            x[ l ] = make_uint4(__float_as_uint(f[ 0 ]), __float_as_uint(f[ 1 ]), __float_as_uint(f[ 2 ]), __float_as_uint(f[ 3 ]));
        }
        const uint4 *const ct = tab + (size_t)t * a.C * SC;
        uint64_t           best = ~0ull;  // (no key is ~0: a slot takes bits 1 .. 8 of the low word)
#pragma unroll 2
        for(uint32_t c = 0; c < a.C; ++c) {
            const uint64_t key = make_key(lone_dist<METRIC, SC>(x, ct + (size_t)c * SC), c);
            best = key < best ? key : best;  // on the key, as k_select ranks: NaN distances order as there, the lower index wins a tie
        }
        const uint32_t sv = sv0 + t;
        const uint8_t  code = (uint8_t)key_slot(best);
        a.codes[ ((size_t)a.first + row) * a.S + sv ] = code;
        if(a.codes16) a.codes16[ ((size_t)a.first + row) * a.S16 + sv ] = code;
        if(a.out_distance) a.out_distance[ row * a.S + sv ] = key_dist(best);
    }
}

uint32_t gcd_u32(uint32_t a, uint32_t b)
{
    while(b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}

}  // namespace

PqEncodePlan plan_pq_encode(int metric, uint32_t dims, uint32_t S, uint32_t C, size_t rows, bool on)
{
    PqEncodePlan p;
    const uint32_t subdim = S ? dims / S : 0, SC = (subdim + 3) / 4;
    const size_t   table = (size_t)C * SC * 16;  // one subvector's centroids
    // the order of the reasons is the order a call meets them in: the switch, the metric, the shape
    if(!on) p.why = kPqEncodeOff;
    else if(metric != M_L2SQ && metric != M_COS) p.why = kPqEncodeMetric;
    else if(subdim == 0 || subdim > 32) p.why = kPqEncodeSubdim;
    else if(C == 0 || C > 256) p.why = kPqEncodeCentroids;
    else if(table + (size_t)64 * subdim * 4 > kPqEncodeLdsMax) p.why = kPqEncodeLds;
    else p.why = kPqEncodeServed;
    if(p.why != kPqEncodeServed) return p;
    // T: the fewest subvectors whose floats are whole 128-byte lines of the row (4 at subdim 8), no more than there are, and as many
    // of those as leave tables and rows inside the LDS a launch may ask for (T = 1 always does: 32 KB of tables + 32 KB of rows at most)
    const auto lds_for = [&](uint32_t T) { return T * table + (size_t)kPqEncodeRows * T * subdim * 4; };
    uint32_t   T = std::min(32u / gcd_u32(32u, subdim), S);
    while(T > 1 && lds_for(T) > kPqEncodeLdsMax) --T;
    p.SC = SC;
    p.T = T;
    p.grid_x = (uint32_t)((rows + kPqEncodeRows - 1) / kPqEncodeRows);
    p.grid_y = (S + T - 1) / T;
    p.lds = lds_for(T);
    p.launches = 1;
    return p;
}

hipError_t launch_pq_encode(int metric, const PqEncodeArgs &args, hipStream_t stream)
{
    if(args.count == 0) return hipSuccess;
    if(args.S == 0 || (uint64_t)args.S * args.subdim > 0xFFFFFFFFull || (args.codes16 && args.S16 < args.S)) return hipErrorInvalidValue;
    const PqEncodePlan p = plan_pq_encode(metric, args.S * args.subdim, args.S, args.C, args.count, true);
    if(p.why != kPqEncodeServed || p.grid_x > 0x7FFFFFFFu || p.grid_y > 65535u || (size_t)args.S * args.subdim > args.row_floats) return hipErrorInvalidValue;
    PqEncodeLaunch a;
    static_cast<PqEncodeArgs &>(a) = args;
    a.T = p.T;
    a.vec4 = (p.T * args.subdim) % 4 == 0 && args.row_floats % 4 == 0 && (uintptr_t)args.rows % 16 == 0 ? 1u : 0u;
    const dim3 grid(p.grid_x, p.grid_y);
#define LGPU_PQE(MM, CC) hipLaunchKernelGGL((k_pq_encode<MM, CC>), grid, dim3(256), p.lds, stream, a)
#define LGPU_PQE_SC(MM)                                                                                          \
    switch(p.SC) {                                                                                               \
    case 1: LGPU_PQE(MM, 1); break;                                                                              \
    case 2: LGPU_PQE(MM, 2); break;                                                                              \
    case 3: LGPU_PQE(MM, 3); break;                                                                              \
    case 4: LGPU_PQE(MM, 4); break;                                                                              \
    case 5: LGPU_PQE(MM, 5); break;                                                                              \
    case 6: LGPU_PQE(MM, 6); break;                                                                              \
    case 7: LGPU_PQE(MM, 7); break;                                                                              \
    default: LGPU_PQE(MM, 8); break;                                                                             \
    }
    if(metric == M_COS) { LGPU_PQE_SC(M_COS) }
    else { LGPU_PQE_SC(M_L2SQ) }
#undef LGPU_PQE_SC
#undef LGPU_PQE
    return hipGetLastError();
}

PqEncodeRecord &last_pq_encode()
{
    static thread_local PqEncodeRecord rec;
    return rec;
}

}  // namespace lgpu

// =====================================================================================================
// C ABI
// =====================================================================================================
using namespace lgpu;

extern "C" {

const char *lantern_gpu_plan_pq_encode(const int64_t in[ 8 ], uint32_t out[ 8 ])
try {
    if(!in || !out) return "lantern_gpu: null plan array";
    // metric, dimensions, subvectors (they divide the dimensions: usearch_init's rule), centroids, rows
    if(in[ 0 ] < 0 || in[ 0 ] > 0x7FFFFFFF || in[ 1 ] < 1 || in[ 1 ] > (int64_t)1 << 20 || in[ 2 ] < 1 || in[ 2 ] > in[ 1 ] || in[ 1 ] % in[ 2 ] != 0 || in[ 3 ] < 1 ||
       in[ 3 ] > 0xFFFFFFFFll || in[ 4 ] < 0 || in[ 4 ] > (int64_t)1 << 38)
        return "lantern_gpu: bad plan input";
    const PqEncodePlan p = plan_pq_encode((int)in[ 0 ], (uint32_t)in[ 1 ], (uint32_t)in[ 2 ], (uint32_t)in[ 3 ], (size_t)in[ 4 ], in[ 5 ] != 0);
    out[ 0 ] = p.why == kPqEncodeServed ? 1u : 0u;
    out[ 1 ] = (uint32_t)p.why;
    out[ 2 ] = p.T;
    out[ 3 ] = p.grid_x;
    out[ 4 ] = p.grid_y;
    out[ 5 ] = (uint32_t)p.lds;
    out[ 6 ] = p.launches;
    out[ 7 ] = p.SC;
    return nullptr;
}
catch(...) {
    return kAbiException;
}

void lantern_gpu_last_pq_encode(uint32_t out[ 4 ])
{
    if(!out) return;
    const PqEncodeRecord &r = last_pq_encode();
    out[ 0 ] = r.pieces, out[ 1 ] = r.fused, out[ 2 ] = r.passes, out[ 3 ] = r.rows;
}

// quantize_table / quantize_vector (lantern.sql:256-395, product_quantization.c:207-240) over a table of rows: every subvector of every
// row in one call.  Rows pass through staging pieces of at most kAddCompactStageRows rows; a piece is one k_pq_encode launch where
// plan_pq_encode serves the shape, the per-subvector passes (launch_pq_take + exact_knn_device) elsewhere -- the same bytes.
void lantern_gpu_pq_encode(const float *rows, size_t n, size_t dimensions, const float *codebook, size_t num_subvectors, size_t num_centroids,
                           usearch_metric_kind_t metric, uint8_t *codes, float *out_distance, usearch_error_t *e)
try {
    CLEAR(e);
    if(metric != usearch_metric_cos_k && metric != usearch_metric_l2sq_k) { FAIL(e, "lantern_gpu: pq_encode needs cos or l2sq"); return; }
    if(!rows || !codebook || !codes || dimensions == 0 || dimensions > (size_t)1 << 20 || num_subvectors == 0 || num_subvectors > dimensions ||
       dimensions % num_subvectors != 0 || num_centroids == 0 || num_centroids > 256 || n > 0x7FFFFFFFull) {
        FAIL(e, "lantern_gpu: bad arguments");
        return;
    }
    if(lantern_gpu_device_count() <= 0) { FAIL(e, kNoDevice); return; }
    PqEncodeRecord &rec = last_pq_encode();
    rec = PqEncodeRecord();
    if(n == 0) return;
    const uint32_t d = (uint32_t)dimensions, S = (uint32_t)num_subvectors, C = (uint32_t)num_centroids, subdim = d / S, sub_chunks = (subdim + 3) / 4,
                   subf = sub_chunks * 4;
    // the per-subvector centroid tables, as usearch_init lays them out from the same codebook ([C][dimensions])
    std::vector<float> centers((size_t)S * C * subf, 0.f);
    for(size_t sv = 0; sv < S; ++sv)
        for(size_t c = 0; c < C; ++c) std::memcpy(&centers[ (sv * C + c) * subf ], codebook + c * d + sv * subdim, (size_t)subdim * 4);
    const size_t       piece = std::min(n, kAddCompactStageRows);
    const PqEncodePlan plan = plan_pq_encode((int)metric, d, S, C, piece, true);
    const bool         fused = plan.why == kPqEncodeServed;
    float   *d_centers = nullptr, *d_stage = nullptr, *d_dist = nullptr, *d_sub = nullptr;
    uint8_t *d_codes = nullptr;
    uint32_t *d_near = nullptr;
    bool ok = hipMalloc((void **)&d_centers, centers.size() * 4) == hipSuccess && hipMalloc((void **)&d_stage, piece * (size_t)d * 4) == hipSuccess;
    if(fused) ok = ok && hipMalloc((void **)&d_codes, piece * (size_t)S) == hipSuccess && hipMalloc((void **)&d_dist, piece * (size_t)S * 4) == hipSuccess;
    else ok = ok && hipMalloc((void **)&d_sub, piece * (size_t)subf * 4) == hipSuccess && hipMalloc((void **)&d_near, piece * 8) == hipSuccess;
    ok = ok && hipMemcpy(d_centers, centers.data(), centers.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    std::vector<uint32_t> near;  // a pass's answers on the host: slots, then distances
    for(size_t at = 0; ok && at < n; at += piece) {
        const size_t m = std::min(piece, n - at);
        ok = hipMemcpy(d_stage, rows + at * d, m * (size_t)d * 4, hipMemcpyHostToDevice) == hipSuccess;
        ++rec.pieces;
        rec.rows += (uint32_t)m;
        if(fused) {
            const PqEncodeArgs a = { d_stage, d, (uint32_t)m, 0u, subdim, S, C, d_centers, d_codes, nullptr, 0u, out_distance ? d_dist : nullptr };
            ok = ok && launch_pq_encode((int)metric, a, nullptr) == hipSuccess;
            ++rec.fused;
            ok = ok && hipMemcpy(codes + at * S, d_codes, m * (size_t)S, hipMemcpyDeviceToHost) == hipSuccess;
            if(out_distance) ok = ok && hipMemcpy(out_distance + at * S, d_dist, m * (size_t)S * 4, hipMemcpyDeviceToHost) == hipSuccess;
            continue;
        }
        near.resize(m * 2);
        for(uint32_t sv = 0; ok && sv < S; ++sv) {
            ok = launch_pq_take(d_stage, d, 0, (uint32_t)m, sv, subdim, subf, d_sub, nullptr) == hipSuccess;
            ok = ok && exact_knn_device((int)metric, sub_chunks, (const uint4 *)(d_centers + (size_t)sv * C * subf), C, (const uint4 *)d_sub, m, 1, d_near,
                                        (float *)(d_near + m), nullptr);
            ok = ok && hipMemcpy(near.data(), d_near, m * 8, hipMemcpyDeviceToHost) == hipSuccess;
            ++rec.passes;
            for(size_t i = 0; ok && i < m; ++i) {
                codes[ (at + i) * S + sv ] = (uint8_t)near[ i ];
                if(out_distance) std::memcpy(&out_distance[ (at + i) * S + sv ], &near[ m + i ], 4);
            }
        }
    }
    for(void *p : { (void *)d_centers, (void *)d_stage, (void *)d_dist, (void *)d_sub, (void *)d_codes, (void *)d_near })
        if(p) (void)hipFree(p);
    if(!ok) {
        (void)hipGetLastError();
        FAIL(e, "lantern_gpu: HIP failure in pq_encode");
    }
}
LANTERN_ABI_CATCH_VOID(e)

}  // extern "C"
