// filter.hpp -- filtered k-NN search: the allow-set over the slots of one index and the two kernels that honour it
// (search_filtered_kernel.hip: the filtered graph walk and the exact pass over the allowed rows; filter.hip: building a filter and
// the entry points).  Semantics: include/lantern_gpu.h "Filtered search" and DESIGN.md 4.9.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernels.hpp"

namespace lgpu {

struct Index;

constexpr uint64_t kFilterMagic = 0x4C414E5446494C54ull;  // "LANTFILT": the first word of every live filter handle

// An allow-set over the slots of ONE index at ONE size (the size after the flush every search performs).  Used on another index,
// or once the index has grown, it is refused -- never silently extended.
struct Filter
{
    uint64_t  magic = kFilterMagic;
    Index    *ix = nullptr;
    int       device = 0;
    size_t    n = 0;                // the index's size when the filter was built
    uint64_t  epoch = 0;            // ... and its Index::epoch: a compaction renumbers the slots (lantern_gpu_compact_deleted)
    size_t    words = 0;            // 32-bit words of the bitmap (whole multiples of 4)
    uint32_t *d_bits = nullptr;     // [words]: bit s of word s / 32 = slot s is allowed; bits >= n are zero
    uint32_t *d_slots = nullptr;    // [count]: the allowed slots, ascending (the exact path's work list)
    size_t    count = 0;            // popcount of the bitmap
};

// One query's filter in the per-query form of the two kernels (FilteredArgs::descs): what FilteredArgs::allow_* are to a whole launch.
struct FilterDesc
{
    const uint32_t *bits;        // the filter's bitmap (unused when `unfiltered`)
    const uint32_t *slots;       // [count] the allowed slots, ascending (the exact path's work list; the seeded walk's seeds)
    uint32_t        count;       // allowed slots; 0 without `unfiltered`: an empty filter, the empty answer
    uint32_t        unfiltered;  // != 0: every slot is allowed and there is no bitmap (a NULL entry of the caller's filter array)
};

// kernel arguments of both filtered kernels.  Fields are re-read from the kernarg segment at the points of a query that need them
// (query_frame.hpp "kernarg re-read").
struct FilteredArgs
{
    View            view;
    FrameArgs       frame;       // (kernels.hpp; bitmaps, bm_words, undo_cap and vis_slots: walk only)
    uint32_t        k, skip;
    uint32_t        exp;         // expansion = max(ef, k + skip): the capacity of `top` (walk) / k + skip (exact)
    uint32_t        cand_cap;    // C: the capacity of `next` (walk only; >= exp)
    const uint32_t *allow_bits;  // [words] the filter's bitmap
    const uint32_t *allow_slots; // [allow_count] the allowed slots, ascending (exact only)
    uint32_t        allow_count;
    uint32_t        rows_per_round;  // exact only: rows evaluated per round (2 per G-lane group)
    // the per-query form (descs != NULL; allow_* unused): `frame.nq` counts the entries of the selection list `frame.qlist`, every
    // output row is indexed by the query a position selects, and that query's filter is descs[query]
    const FilterDesc *descs;     // [queries of the call]
    // the seeded walk (per-query form only): > 0 = a query whose descriptor has count >= 1 starts from min(seeds, count) allowed rows
    // taken at even strides from the descriptor's slot list (search_filtered_kernel.hip "SEEDED"); 0 = off
    uint32_t          seeds;
    // the per-query-parameter form (with descs; k_search_filtered / k_search_exact_allowed <.., PARAMS = true>); NULL otherwise
    const uint4      *qparams;   // [queries of the call] {k, expansion (exact: k + skip), skip, C} by query; `k` above is then the width of an
                                 // answer row, `skip` unused, `exp` and `cand_cap` the launch's largest: the LDS carve
    // ADC over the code rows of a compact pq index (search_filtered_pq_kernel.hip, M_*_ADC; view.vec = the code rows, view.chunks = 16-byte
    // chunks per code row): SearchArgs' fields of the same names
    const float      *adc_centers;  // [S][C][sub_floats] per-subvector centroid tables, rows zero padded to whole chunks
    uint32_t          adc_S, adc_C, adc_subdim;
    uint32_t          adc_qchunks;  // 16-byte chunks of a (raw f32) query row
};

size_t     filtered_walk_lds_bytes(uint32_t chunks, uint32_t exp, uint32_t cand_cap, uint32_t M0, uint32_t vis_slots);
size_t     filtered_exact_lds_bytes(uint32_t chunks, uint32_t kk, uint32_t rows_per_round);
hipError_t launch_search_filtered(int metric, const FilteredArgs &a, int waves, int grid, hipStream_t stream);
hipError_t launch_search_exact_allowed(int metric, const FilteredArgs &a, int waves, int grid, hipStream_t stream);
// the same two kernels over a compact pq index (search_filtered_pq_kernel.hip): metric = M_*_PQD (view.chunks: of the DECODED row, the
// view's pq_* fields set) or M_*_ADC (view.chunks: of the code row, 1..8; adc_* set, adc_C <= 256).  The *_lds_bytes above take the
// chunks in front of the lists: the decoded row's, or filtered_adc_lds_chunks'.
hipError_t launch_search_filtered_pq(int metric, const FilteredArgs &a, int waves, int grid, hipStream_t stream);
hipError_t launch_search_exact_allowed_pq(int metric, const FilteredArgs &a, int waves, int grid, hipStream_t stream);
uint32_t   filtered_adc_lds_chunks(uint32_t code_chunks, uint32_t qchunks);  // the ADC table's chunks (code_chunks x 16 KiB) + the raw query row's

}  // namespace lgpu
