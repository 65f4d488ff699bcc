// filtered_plan.cpp -- the plan of a filtered call (filtered_plan.hpp): the carves of the two launches, the path rule, the two steps
// every form of a call plans through, and the device-free entry points that show the plan (include/lantern_gpu.h
// lantern_gpu_plan_filtered_params / _compact).  Host arithmetic only.
#include "filtered_plan.hpp"

#include <algorithm>
#include <cstring>

#include "filter.hpp"

namespace lgpu {

// What lies in front of the lists in a launch's LDS, in chunks: the query row -- ADC: the table first (code_chunks x 16 KiB:
// RowAcc<M_*_ADC> reads it from the first LDS bytes), the raw query row behind it
static uint32_t plan_lds_chunks(const FilterPlanIn &p) { return p.adc_code_chunks ? filtered_adc_lds_chunks(p.adc_code_chunks, p.chunks) : p.chunks; }
static size_t   plan_table_bytes(const FilterPlanIn &p) { return (size_t)filtered_adc_lds_chunks(p.adc_code_chunks, 0) * 16; }
// lanes per row: a code row has at most 8 chunks
static int plan_lanes(const FilterPlanIn &p) { return p.adc_code_chunks ? 8 : group_lanes_for(p.chunks); }

static const char *kWalkOverBudget = "lantern_gpu: ef/k exceed the 160 KiB LDS budget of the filtered search kernel";
static const char *kExactOverBudget = "lantern_gpu: k + skip exceed the 160 KiB LDS budget of the exact filtered search kernel";
static const char *kJointOverBudget =
    "lantern_gpu: the queries fit the 160 KiB LDS budget of the filtered search kernel one by one, but the largest expansion and the largest "
    "candidate cap of the batch do not fit together: split the batch";

// whether the exact launch of this index is the screened kernel's (search_filtered_screen_kernel.hip), or the first reason it is not
FilterScreenWhy filter_screen_why(const FilterPlanIn &p, size_t kk)
{
    if(!p.screen_on) return kFilterScreenOff;
    if(p.mcode != M_L2SQ && p.mcode != M_COS) return kFilterScreenMetric;
    if(!screen_rows_for(p.chunks)) return kFilterScreenWidth;
    if(!p.screen_table) return kFilterScreenNoTable;
    if(p.pq_compact || p.adc_code_chunks) return kFilterScreenCompact;
    // (a list that fits today's carve and not this one keeps today's kernel: the switch refuses nothing)
    if(filtered_exact_screen_lds_bytes(p.chunks, (uint32_t)kk, 2 * kFilterScreenThreads / 64) > kFilteredLds) return kFilterScreenLds;
    return kFilterScreenTaken;
}
int filtered_screen_per_cu(size_t lds) { return (int)std::max<size_t>(1, std::min<size_t>(kFilterScreenPerCuMax, kFilteredLds / std::max<size_t>(lds, 1))); }
// the exact launch's carve for a list of kk keys: today's kernel's, or -- the one place where an exact launch becomes the screened one --
// the screened kernel's (512 threads, so twice the rows per f32 round; + the query's screen block and the survivor queue)
static void exact_carve(const FilterPlanIn &p, size_t kk, FilteredShape &s)
{
    s.exp = (uint32_t)kk;
    s.screened = filter_screen_why(p, kk) == kFilterScreenTaken;
    if(s.screened) {
        s.rows_per_round = (uint32_t)(2 * kFilterScreenThreads / 64);
        s.lds = filtered_exact_screen_lds_bytes(p.chunks, s.exp, s.rows_per_round);
        return;
    }
    s.rows_per_round = (uint32_t)(2 * 64 * kFilteredWaves / plan_lanes(p));
    s.lds = filtered_exact_lds_bytes(plan_lds_chunks(p), s.exp, s.rows_per_round);
}
// the walk launch's carve for `exp` keys of top and `cap` of next: the visited set takes what is left of the LDS target -- beside an
// ADC table, which alone may exceed that target, what is left of the workgroup's LDS (at most 2048 slots either way)
static void walk_carve(const FilterPlanIn &p, size_t exp, size_t cap, FilteredShape &s)
{
    s.exp = (uint32_t)exp;
    s.cand_cap = (uint32_t)cap;
    const uint32_t chunks = plan_lds_chunks(p);
    const size_t   target = p.adc_code_chunks ? kFilteredLds : kFilteredLdsTarget;
    uint32_t vis_slots = 2048;
    while(vis_slots && filtered_walk_lds_bytes(chunks, s.exp, s.cand_cap, p.M0, vis_slots) > target)
        vis_slots = vis_slots > 256 ? vis_slots - 256 : 0;
    if(vis_slots && vis_slots < 4 * p.M0) vis_slots = 0;
    s.vis_slots = vis_slots;
    s.lds = filtered_walk_lds_bytes(chunks, s.exp, s.cand_cap, p.M0, vis_slots);
}
// The part of a launch's shape that depends on (k + skip, expansion, index) only -- not on the filter.  NULL, or the refusal.
static const char *filtered_shape_of(const FilterPlanIn &p, bool exact, size_t kk, size_t exp, FilteredShape &s)
{
    if(exact) {
        exact_carve(p, kk, s);
        if(s.lds > kFilteredLds) return kExactOverBudget;
    } else {
        const size_t base = filtered_walk_lds_bytes(plan_lds_chunks(p), (uint32_t)exp, 0, p.M0, 0);
        if(base + exp * 16 > kFilteredLds) return kWalkOverBudget;
        size_t cap = p.cand_cap ? std::max(p.cand_cap, exp) : std::max<size_t>(4 * exp, 256);
        cap = std::min(cap, (kFilteredLds - base) / 16);
        if(p.cand_cap && cap < std::max(p.cand_cap, exp)) return "lantern_gpu: the candidate cap exceeds the 160 KiB LDS budget of the filtered search kernel";
        walk_carve(p, exp, cap, s);
    }
    return nullptr;
}

int filtered_per_cu(size_t lds) { return (int)std::max<size_t>(1, std::min<size_t>(4, kFilteredLds / std::max<size_t>(lds, 1))); }

// the path of a query under a filter of `count` rows: forced, or the rule of DESIGN.md 4.9 -- a walk under selectivity s evaluates
// about D / s rows, the exact pass `allowed`
bool count_takes_exact(const FilterPlanIn &p, size_t count, size_t ef_sel)
{
    if(p.path) return p.path == 2;
    return (double)count * (double)count <= p.exact_factor * (double)ef_sel * (double)p.n;
}

std::string plan_filtered_paths(const FilterPlanIn &p, const int64_t *counts, size_t nq, const lantern_gpu_query_params *params, FilteredAsk uniform,
                                bool lone_riders_launch, FilteredCallPlan &out)
{
    out = FilteredCallPlan{};
    out.lone_riders_launch = lone_riders_launch;
    out.path.assign(nq, 0);
    if(params) out.rows.assign(nq * 4, 0u);
    size_t max_exp = 0, max_cap = 0, max_kk = 0;
    // what a query -- a uniform call: a path -- asks of its launch, into the launch's maxima and the query's row.  NULL, or the refusal
    auto shape = [ & ](bool exact, const FilteredAsk &q, uint32_t *row) -> const char * {
        const size_t  ef_sel = q.ef ? q.ef : p.ef_default;
        const size_t  kk = std::min<size_t>(q.k + q.skip, (size_t)1 << 20), exp = std::min<size_t>(std::max(ef_sel, q.k + q.skip), (size_t)1 << 20);
        FilteredShape s;
        if(const char *why = filtered_shape_of(p, exact, kk, exp, s)) return why;
        if(row) row[ 1 ] = s.exp, row[ 3 ] = s.cand_cap;
        if(exact) max_kk = std::max<size_t>(max_kk, s.exp);
        else max_exp = std::max<size_t>(max_exp, s.exp), max_cap = std::max<size_t>(max_cap, s.cand_cap);
        return nullptr;
    };
    for(size_t i = 0; i < nq; ++i) {
        const FilteredAsk q = params ? FilteredAsk{ params[ i ].k, params[ i ].ef, params[ i ].skip } : uniform;
        uint32_t *const   row = params ? &out.rows[ 4 * i ] : nullptr;
        if(row) row[ 0 ] = (uint32_t)q.k, row[ 2 ] = (uint32_t)q.skip;
        out.n_k0 += q.k == 0;
        if(q.k == 0 || p.n == 0 || counts[ i ] == 0) { out.riders.push_back((uint32_t)i); continue; }
        const bool exact = counts[ i ] >= 0 && count_takes_exact(p, (size_t)counts[ i ], q.ef ? q.ef : p.ef_default);
        out.path[ i ] = exact ? 2 : 1;
        (exact ? out.exact : out.walk).push_back((uint32_t)i);
        out.counts.unfiltered += counts[ i ] < 0;  // (a NULL entry walks whatever the policy)
        if(!params) continue;
        if(const char *why = shape(exact, q, row)) return std::string(why) + " (params[" + std::to_string(i) + "])";
    }
    out.counts.walk = (uint32_t)out.walk.size(), out.counts.exact = (uint32_t)out.exact.size(), out.counts.empty = (uint32_t)out.riders.size();
    const bool exact_launch = !out.exact.empty() || (lone_riders_launch && out.walk.empty() && !out.riders.empty());
    if(!params) {
        if(!out.walk.empty())
            if(const char *why = shape(false, uniform, nullptr)) return why;
        if(exact_launch)
            if(const char *why = shape(true, uniform, nullptr)) return why;
    }
    // one carve per launch.  The exact list's is the carve of its largest k + skip, which fits because that query does; the walk's
    // joins the largest expansion with the largest C, which two different queries may have brought
    if(!out.walk.empty()) {
        if(filtered_walk_lds_bytes(plan_lds_chunks(p), (uint32_t)max_exp, (uint32_t)max_cap, p.M0, 0) > kFilteredLds) return kJointOverBudget;
        walk_carve(p, max_exp, max_cap, out.sw);
    }
    if(exact_launch) exact_carve(p, max_kk, out.se);
    return "";
}

void plan_filtered_close(const int64_t *counts, FilteredCallPlan &plan)
{
    if(!plan.rows.empty())  // (a uniform call's walk list is of one expansion)
        std::stable_sort(plan.walk.begin(), plan.walk.end(), [ & ](uint32_t x, uint32_t y) { return plan.rows[ 4 * x + 1 ] > plan.rows[ 4 * y + 1 ]; });
    std::stable_sort(plan.exact.begin(), plan.exact.end(), [ & ](uint32_t x, uint32_t y) { return counts[ x ] > counts[ y ]; });
    const bool             walk_only = plan.exact.empty() && !plan.walk.empty();
    std::vector<uint32_t> &host = walk_only ? plan.walk : plan.exact;
    if(!plan.walk.empty() || !plan.exact.empty() || plan.lone_riders_launch) host.insert(host.end(), plan.riders.begin(), plan.riders.end());
}

}  // namespace lgpu

using namespace lgpu;

// the plan without a device (include/lantern_gpu.h has the field order): `cols` words of a launch's row are written
static const char *plan_flat(const FilterPlanIn &p, const int64_t counts[], const lantern_gpu_query_params params[], size_t nq, uint32_t per_query[][ 4 ],
                             uint32_t *launch, int cols)
{
    static thread_local std::string msg;
    static const lantern_gpu_query_params none{};
    FilteredCallPlan plan;
    msg = plan_filtered_paths(p, counts, nq, params ? params : &none, FilteredAsk{}, false, plan);
    if(!msg.empty()) return msg.c_str();
    plan_filtered_close(counts, plan);
    for(size_t i = 0; i < nq; ++i) {
        per_query[ i ][ 0 ] = plan.path[ i ], per_query[ i ][ 1 ] = plan.rows[ 4 * i + 1 ], per_query[ i ][ 2 ] = plan.rows[ 4 * i + 3 ], per_query[ i ][ 3 ] = 0;
    }
    for(int l = 0; l < 2; ++l) {
        const std::vector<uint32_t> &list = l ? plan.exact : plan.walk;
        const FilteredShape         &s = l ? plan.se : plan.sw;
        for(size_t at = 0; at < list.size(); ++at) per_query[ list[ at ] ][ 3 ] = (uint32_t)at;
        const uint32_t row[ 7 ] = { (uint32_t)list.size(), s.exp, s.cand_cap, l ? s.rows_per_round : s.vis_slots, (uint32_t)s.lds,
                                    list.empty() ? 0u : (uint32_t)filtered_per_cu(s.lds), list.empty() ? 0u : (uint32_t)plan_table_bytes(p) };
        std::copy(row, row + cols, launch + l * cols);
    }
    return nullptr;
}
static FilterPlanIn plan_in_flat(const int64_t in[ 8 ])
{
    double factor;
    std::memcpy(&factor, &in[ 6 ], 8);
    return FilterPlanIn{ (uint32_t)in[ 0 ], (uint32_t)in[ 1 ], (size_t)in[ 2 ], (size_t)in[ 3 ], (int)in[ 4 ], (size_t)in[ 5 ], factor, (size_t)in[ 7 ] };
}

extern "C" {

const char *lantern_gpu_plan_filtered_params(const int64_t in[ 8 ], const int64_t counts[], const lantern_gpu_query_params params[], size_t nq,
                                             uint32_t per_query[][ 4 ], uint32_t launch[ 2 ][ 6 ])
try {
    if(!in || !launch || (nq && (!counts || !params || !per_query))) return "lantern_gpu: null array";
    return plan_flat(plan_in_flat(in), counts, params, nq, per_query, &launch[ 0 ][ 0 ], 6);
}
catch(...) {
    return "lantern_gpu: out of memory planning a filtered search";
}

const char *lantern_gpu_plan_filtered_screen(const int64_t in[ 6 ], uint32_t out[ 4 ])
{
    if(!in || !out) return "lantern_gpu: null array";
    if(in[ 2 ] < 1 || in[ 2 ] > 500) return "lantern_gpu: a stored row has 1 to 500 chunks";
    if(in[ 5 ] < 1 || in[ 5 ] > ((int64_t)1 << 20)) return "lantern_gpu: k + skip must be 1 to 2^20";
    FilterPlanIn p{};
    p.chunks = (uint32_t)in[ 2 ];
    p.screen_on = in[ 0 ] != 0, p.mcode = (int)in[ 1 ], p.screen_table = in[ 3 ] != 0, p.pq_compact = in[ 4 ] != 0;
    const FilterScreenWhy why = filter_screen_why(p, (size_t)in[ 5 ]);
    const bool            taken = why == kFilterScreenTaken;
    const size_t          lds = taken ? filtered_exact_screen_lds_bytes(p.chunks, (uint32_t)in[ 5 ], 2 * kFilterScreenThreads / 64) : 0;
    out[ 0 ] = taken, out[ 1 ] = (uint32_t)why, out[ 2 ] = (uint32_t)lds, out[ 3 ] = taken ? (uint32_t)filtered_screen_per_cu(lds) : 0u;
    return nullptr;
}

const char *lantern_gpu_plan_filtered_compact(const int64_t in[ 9 ], const int64_t counts[], const lantern_gpu_query_params params[], size_t nq,
                                              uint32_t per_query[][ 4 ], uint32_t launch[ 2 ][ 7 ])
try {
    if(!in || !launch || (nq && (!counts || !params || !per_query))) return "lantern_gpu: null array";
    if(in[ 8 ] < 0 || in[ 8 ] > 8) return "lantern_gpu: a code row has 1 to 8 chunks (0: rows decoded on the fly)";
    FilterPlanIn p = plan_in_flat(in);
    p.adc_code_chunks = (uint32_t)in[ 8 ];
    return plan_flat(p, counts, params, nq, per_query, &launch[ 0 ][ 0 ], 7);
}
catch(...) {
    return "lantern_gpu: out of memory planning a filtered search";
}

}  // extern "C"
