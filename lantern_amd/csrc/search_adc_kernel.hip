// search_adc_kernel.hip -- k_search_adc: usearch_search_ef (scan.c:220-228) over a pq = true index that keeps only its CODE
// BYTES in HBM (usearch_storage.cpp:29-31: a node carries num_subvectors bytes; scan.c:75-81, build.c:497-500,
// product_quantization.c:207-240).  The walk is walk.hpp's; what changes is the evaluation of a row:
//
//   per query   the table lut[s][c] (s < num_subvectors, c < num_centroids) = the metric's partial sum between subvector s of
//               the query and centroid c of that subvector: l2sq: one fma chain of (q - c)^2 over the subvector's dimensions in
//               memory order; cos: the chain of q * c.  98 KB of LDS at 96 subvectors x 256 centroids (one workgroup per CU).
//   per row     num_subvectors table entries added up: lane l of the row's 8-lane group owns the 16 codes of chunk l and adds
//               their entries in code order; the lanes' sums meet in the 8-lane tree (device_common.hpp RowAcc<M_*_ADC>).
//               cos: 1 - sum / (|q| * |row|), |row| = the cached norm of the row's decoding, |q| in the f32 kernels' own order.
//
// A distance to a decoded vector, as the reference defines a PQ index's distances -- in ADC's summation order, which is ours
// to define (the fork's is not in the tree): the oracle restates exactly this (oracle/hnsw.c lo_set_pq_view), device and
// oracle agree bit for bit, and both agree with the decoded-row distances to 1e-5 relative.  PARITY UNPINNED BY THE REFERENCE.
// Memory: 10M x 768 at 96 subvectors = 0.96 GB of rows instead of 30.7 GB.
#include "adc_stage.hpp"
#include "search_kernel.hpp"

namespace lgpu {

// SPEC: the latency-bound walk of walk_spec.hpp in its lone-query shape (three role waves + eight row waves, one barrier per hop,
// neighbour lists fetched with the rows).  A table of 96 x 256 entries leaves room for ONE workgroup per CU, so every query of
// a batch walks alone on its CU whatever the batch size: the walk that is fastest alone is the one to run.
// (SPEC 2 = the lone-query shape.  A two-nodes-per-round form of the walk was measured here too -- 1.98 -> 1.65 M queries/s at
// 96 subvectors -- and is not instantiated.)
// EACH: the per-query-parameter form, as k_search's (search_kernel.hpp): the launch's queries come from FrameArgs::qlist, every
// query's k, expansion and skip from its row of SearchArgs::qparams, answer rows are k_stride wide.
// The frame around the walk -- pick, bind, answer rows, close -- is query_frame.hpp's; the staging is adc_stage.hpp's (the raw
// query row, the table, and |query| by the chain of the query's own width), shared with the filtered kernels over ADC rows.
template <int METRIC, int KPL, int SPEC = 0, bool EACH = false>
__global__ void __launch_bounds__(SPEC ? 704 : 512, SPEC ? 1 : 2) k_search_adc(SearchArgs)
{
    // (arguments are re-read from the kernarg segment where a query needs them -- query_frame.hpp: kept live across the
    // persistent loop they cost the hop loop ~120 scalar-register spill reloads)
    constexpr int G = 8;  // rows are at most 8 chunks (128 codes)
    const int     tid = threadIdx.x, T = blockDim.x;
    WalkLds       s;
    SpecLds       sc;
    uint32_t      lut_chunks;
    {
        const KernargBytes ka = kernarg_opaque();
        lut_chunks = LGPU_VIEW_ARG(ka, SearchArgs, chunks) * 16 * ADC_LUT_STRIDE / 4;
        unsigned char *end = carve_walk(lgpu_smem, s, lut_chunks + LGPU_SEARCH_ARG(ka, adc_qchunks), LGPU_SEARCH_ARG(ka, ef), LGPU_VIEW_ARG(ka, SearchArgs, M0),
                                        LGPU_FRAME_ARG(ka, SearchArgs, vis_slots));  // s.q = the table, then the raw query row
        if constexpr(SPEC != 0) carve_spec(end, sc, LGPU_VIEW_ARG(ka, SearchArgs, M0), LGPU_SEARCH_ARG(ka, spec_prefetch), LGPU_SEARCH_ARG(ka, spec_cache));
        else (void)end;
    }
    float *const       lut = (float *)s.q;
    const uint4 *const rawq4 = s.q + lut_chunks;
    for(uint32_t pos = blockIdx.x; pos < LGPU_FRAME_ARG(kernarg_opaque(), SearchArgs, nq);) {
        uint32_t    q = pos;
        QueryParams each{};
        if constexpr(EACH) {
            const KernargBytes ka = kernarg_opaque();
            q = frame_query<SearchArgs, true>(ka, pos);
            each = query_params(ka, q);
        }
        uint32_t D = 0, E = 0;
        int      cnt = 0;
        if(!EACH || each.k != 0) {  // (a query that wants no rows needs no table)
            const KernargBytes ka = kernarg_opaque();
            const uint32_t     S = LGPU_SEARCH_ARG(ka, adc_S), C = LGPU_SEARCH_ARG(ka, adc_C), subdim = LGPU_SEARCH_ARG(ka, adc_subdim),
                           qchunks = LGPU_SEARCH_ARG(ka, adc_qchunks), S16 = LGPU_VIEW_ARG(ka, SearchArgs, chunks) * 16;
            adc_stage<METRIC>(tid, T, s, lut, (uint4 *)rawq4, LGPU_FRAME_ARG(ka, SearchArgs, queries), q, LGPU_SEARCH_ARG(ka, adc_centers), S, C, subdim, qchunks, S16);
        }
        {
            const KernargBytes ka = kernarg_opaque();
            View               v;
            LGPU_LOAD_VIEW(v, ka, SearchArgs)
            uint32_t        bm_words;
            uint32_t *const bitmap = frame_bind<SearchArgs>(ka, s, bm_words);
            const int       ef = EACH ? (int)each.ef : (int)LGPU_SEARCH_ARG(ka, ef);
            if(v.n != 0 && (!EACH || each.k != 0)) {
                if constexpr(SPEC != 0) {
                    static_assert(SPEC == 0 || KPL > 0, "the latency-bound walk keeps its list in registers");
                    const uint32_t start = greedy_descent_spec<METRIC, G>(v, s, v.entry, v.max_level, 0, D);
                    cnt = search_level_spec<METRIC, G, (KPL > 0 ? KPL : 1), 1, 2, true, false>(v, s, sc, bitmap, bm_words, start, ef, D, E, nullptr);
                } else {
                    const uint32_t start = greedy_descent<METRIC, G>(v, s, v.entry, v.max_level, 0, D);
                    if constexpr(KPL > 0) cnt = search_level_reg<METRIC, G, KPL>(v, s, bitmap, bm_words, start, 0, ef, D, E);
                    else cnt = search_level<METRIC, G>(v, s, bitmap, bm_words, start, 0, ef, D, E);
                }
            }
        }
        const KernargBytes kb = kernarg_opaque();
        const uint32_t     k = EACH ? each.k : LGPU_SEARCH_ARG(kb, k), skip = EACH ? each.skip : LGPU_SEARCH_ARG(kb, skip);
        const uint32_t     kw = EACH ? LGPU_SEARCH_ARG(kb, k_stride) : k;  // the width of an answer row
        const int          got = frame_answer_rows<SearchArgs>(tid, T, kb, s, q, cnt, k, skip, kw);
        pos = frame_close<SearchArgs>(tid, kb, s, q, pos, got, D, E);
    }
}

// the record of an instantiation (lantern_gpu_last_search_cells): k_search_adc's own parameter list with its defaults; rows are walked by
// 8-lane groups, PROF and ROWS are no parameters of this kernel
template <int METRIC, int KPL, int SPEC = 0, bool EACH = false> static inline void note_search_adc(const SearchArgs &a)
{
    note_search_cell(2, METRIC, 8, 0, 0, KPL, SPEC, EACH, a);
}

size_t search_adc_lds_bytes(uint32_t code_chunks, uint32_t qchunks, uint32_t ef_cap, uint32_t M0, uint32_t vis_slots)
{
    return walk_lds_bytes(code_chunks * 16 * ADC_LUT_STRIDE / 4 + qchunks, ef_cap, M0, vis_slots);
}

hipError_t launch_search_adc(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream)
{
    if(a.view.chunks == 0 || a.view.chunks > 8 || a.adc_C == 0 || a.adc_C > (uint32_t)ADC_LUT_STRIDE) return hipErrorInvalidValue;
    const int kpl = a.lds_list ? 0 : a.ef <= 64 ? 1 : a.ef <= 128 ? 2 : 0;
    if(a.spec && (kpl == 0 || waves < 4 || waves > 11 || a.view.M0 > 64 || a.view.M0 < 2)) return hipErrorInvalidValue;
    const size_t lds = search_adc_lds_bytes(a.view.chunks, a.adc_qchunks, a.ef, a.view.M0, a.frame.vis_slots) + (a.spec ? spec_lds_bytes(a.view.M0, a.spec_prefetch, a.spec_cache) : 0);
#define LGPU_ADC2(...)                                                                             \
    {                                                                                              \
        note_search_adc<__VA_ARGS__>(a);                                                           \
        LGPU_LAUNCH_LDS((k_search_adc<__VA_ARGS__>), grid, 64 * waves, lds, stream, a)             \
    }
#define LGPU_ADC1(MM, KK, SS)                                    \
    {                                                            \
        if(a.qparams) LGPU_ADC2(MM, KK, SS, true)                \
        else LGPU_ADC2(MM, KK, SS, false)                        \
    }
#define LGPU_ADC(MM)                                  \
    {                                                 \
        if(a.spec) {                                  \
            if(kpl == 1) LGPU_ADC1(MM, 1, 2)          \
            else LGPU_ADC1(MM, 2, 2)                  \
        } else if(kpl == 1) LGPU_ADC1(MM, 1, 0)       \
        else if(kpl == 2) LGPU_ADC1(MM, 2, 0)         \
        else LGPU_ADC1(MM, 0, 0)                      \
    }
    if(metric == M_L2SQ_ADC) LGPU_ADC(M_L2SQ_ADC)
    else if(metric == M_COS_ADC) LGPU_ADC(M_COS_ADC)
    else return hipErrorInvalidValue;
#undef LGPU_ADC
#undef LGPU_ADC1
#undef LGPU_ADC2
    return hipGetLastError();
}

}  // namespace lgpu
