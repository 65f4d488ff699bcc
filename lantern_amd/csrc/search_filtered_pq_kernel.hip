// search_filtered_pq_kernel.hip -- the filtered k-NN search's two kernels (search_filtered_kernel.hpp) over a COMPACT pq index, which
// keeps only its code bytes in HBM (lantern_gpu_set_filter_compact; DESIGN.md 4.9 "Compact pq indexes"):
//
//  * M_*_PQD: rows decoded on the fly from the L2-resident centroid tables (device_common.hpp PqdRow), G by the DECODED row.  The
//    arithmetic, the carve and so every bit of every answer, D and E are the expanded index's.
//  * M_*_ADC: rows are code chunks (at most 8: G = 8) added up over the per-query table, which takes the first
//    code_chunks x 16 KiB of the LDS with the raw query row behind it; the lists and the visited set follow.  The distances are
//    k_search_adc's, bit for bit (one staging body: adc_stage.hpp; one row routine: RowAcc<M_*_ADC>), on the walk and the exact path.
//
// A unit of its own, so that search_filtered_kernel.hip compiles what it compiled before these instantiations existed.
// PARITY UNPINNED BY THE REFERENCE: the filter semantics are this repository's (search_filtered_kernel.hpp), and so is ADC's summation
// order (search_adc_kernel.hip); tests/filtered_walk_ref.py over the oracle's ADC distances (tests/filtered_adc_ref.py) restates both.
#include "search_filtered_kernel.hpp"

namespace lgpu {

uint32_t filtered_adc_lds_chunks(uint32_t code_chunks, uint32_t qchunks) { return adc_lds_chunks(code_chunks, qchunks); }

// as launch_search_adc's guard: a code row of 1..8 chunks, a table row of at most ADC_LUT_STRIDE centroids
static bool adc_args_ok(const FilteredArgs &a)
{
    return a.view.chunks >= 1 && a.view.chunks <= 8 && a.adc_C >= 1 && a.adc_C <= (uint32_t)ADC_LUT_STRIDE && a.adc_centers && a.adc_qchunks >= 1;
}

hipError_t launch_search_filtered_pq(int metric, const FilteredArgs &a, int waves, int grid, hipStream_t stream)
{
    if((a.seeds || a.qparams) && !a.descs) return hipErrorInvalidValue;
    if(mcode_is_adc(metric)) {
        if(!adc_args_ok(a)) return hipErrorInvalidValue;
        const size_t lds = filtered_walk_lds_bytes(adc_lds_chunks(a.view.chunks, a.adc_qchunks), a.exp, a.cand_cap, a.view.M0, a.frame.vis_slots);
        if(metric == M_L2SQ_ADC) LGPU_FILTERED_WALK_FORMS(M_L2SQ_ADC, 8)
        else if(metric == M_COS_ADC) LGPU_FILTERED_WALK_FORMS(M_COS_ADC, 8)
        else return hipErrorInvalidValue;
    } else {
        if(!a.view.pq_centers || !a.view.pq_inv) return hipErrorInvalidValue;
        const size_t lds = filtered_walk_lds_bytes(a.view.chunks, a.exp, a.cand_cap, a.view.M0, a.frame.vis_slots);
        PQD_G(metric, a.view.chunks, LGPU_FILTERED_WALK_FORMS);
    }
    return hipGetLastError();
}

hipError_t launch_search_exact_allowed_pq(int metric, const FilteredArgs &a, int waves, int grid, hipStream_t stream)
{
    if(a.qparams && !a.descs) return hipErrorInvalidValue;
    if(mcode_is_adc(metric)) {
        if(!adc_args_ok(a)) return hipErrorInvalidValue;
        const size_t lds = filtered_exact_lds_bytes(adc_lds_chunks(a.view.chunks, a.adc_qchunks), a.exp, a.rows_per_round);
        if(metric == M_L2SQ_ADC) LGPU_FILTERED_EXACT_FORMS(M_L2SQ_ADC, 8)
        else if(metric == M_COS_ADC) LGPU_FILTERED_EXACT_FORMS(M_COS_ADC, 8)
        else return hipErrorInvalidValue;
    } else {
        if(!a.view.pq_centers || !a.view.pq_inv) return hipErrorInvalidValue;
        const size_t lds = filtered_exact_lds_bytes(a.view.chunks, a.exp, a.rows_per_round);
        PQD_G(metric, a.view.chunks, LGPU_FILTERED_EXACT_FORMS);
    }
    return hipGetLastError();
}

}  // namespace lgpu
