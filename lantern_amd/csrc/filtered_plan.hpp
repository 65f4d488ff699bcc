// filtered_plan.hpp -- the plan of a filtered call: every query's path, expansion and C, the two selection lists and the two launches'
// carves, as a pure function of the index's fields, the filters' counts and the call's (k, ef, skip) -- uniform or per query.  All
// three forms of a call (filtered_search.cpp) plan through it, and lantern_gpu_plan_filtered_params / _compact show it without a
// device (include/lantern_gpu.h; the rules: DESIGN.md 4.9).  No Index, no stream: filtered_plan.cpp makes no HIP runtime call.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lantern_gpu.h"

namespace lgpu {

constexpr size_t kFilteredLds = 160 * 1024;  // a workgroup's LDS
constexpr size_t kFilteredLdsTarget = 64 * 1024;  // what the visited set may grow the walk's LDS to (two workgroups per CU)
constexpr int    kFilteredWaves = 4;

// What the shape and the path of a filtered launch are computed from: the index's fields and its filter policy, nothing else -- so
// that the plan is a pure function of what the launch really reads.
struct FilterPlanIn
{
    uint32_t chunks, M0;
    size_t   n, ef_default;
    int      path;  // lantern_gpu_set_filter_policy
    size_t   cand_cap;
    double   exact_factor;
    size_t   seeds;  // lantern_gpu_set_filter_seeds (changes no shape: a round of seeds is at most M0 rows, a hop's)
    // a compact pq index served by ADC (search_filtered_pq_kernel.hip): 16-byte chunks of a code row, 1..8; `chunks` is then the raw query
    // row's.  0: rows of `chunks` chunks, stored -- or decoded on the fly, whose shape is the expanded index's
    uint32_t adc_code_chunks = 0;
    // the screened exact pass (lantern_gpu_set_filter_screen): the switch, and what decides whether an exact launch of this index can take
    // it -- the metric code, whether the int8 screen copy is there, whether the index is in its compact pq form
    bool screen_on = false;
    int  mcode = 0;
    bool screen_table = false, pq_compact = false;
};

// whether an exact launch screens (search_filtered_screen_kernel.hip), and if not why: the reasons in the order a call meets them
// (lantern_gpu_plan_filtered_screen's out[1])
enum FilterScreenWhy : int
{
    kFilterScreenTaken = 0,
    kFilterScreenOff,      // the switch is 0
    kFilterScreenMetric,   // not f32 rows under l2sq / cos
    kFilterScreenWidth,    // rows the screen is not built for (screen_rows_for: fewer than 128 chunks)
    kFilterScreenNoTable,  // the index holds no screen copy
    kFilterScreenCompact,  // a compact pq index: today's kernels over its code rows
    kFilterScreenLds       // k + skip keys fit today's carve but not the screened one
};
FilterScreenWhy filter_screen_why(const FilterPlanIn &p, size_t kk);  // kk: the launch's largest k + skip
// workgroups of the screened launch that a CU holds: by its LDS, and two by its registers (512 threads of at most 128 VGPRs)
constexpr size_t kFilterScreenPerCuMax = 2;
int              filtered_screen_per_cu(size_t lds);

// exp, cand_cap, vis_slots / rows_per_round and the LDS bytes of one launch
struct FilteredShape
{
    uint32_t exp = 0, cand_cap = 0, vis_slots = 0, rows_per_round = 0;
    size_t   lds = 0;
    bool     screened = false;  // the exact launch only: k_exact_allowed_screened, whose carve `lds` then is
};

// the queries of a call by what becomes of them (lantern_gpu_last_filtered_each [0..4)); `empty`: every rider
struct EachCounts { uint32_t walk, exact, unfiltered, empty; };

// a uniform call's parameters (the per-query form's are the caller's lantern_gpu_query_params rows)
struct FilteredAsk { size_t k, ef, skip; };

struct FilteredCallPlan
{
    std::vector<uint32_t> walk, exact;  // the selection lists; closed (plan_filtered_close): in launch order, the riders behind them
    std::vector<uint32_t> riders;       // the queries without a path -- an empty filter, k == 0, an empty index -- in call order
    std::vector<uint32_t> rows;         // per-query parameters only: [nq][4] {k, expansion (exact: k + skip), skip, C}
    std::vector<uint8_t>  path;         // [nq] 0 none, 1 walk, 2 exact
    EachCounts            counts{};     // by the path rule (a dense route that answers exact-path queries changes none of them)
    uint32_t              n_k0 = 0;     // queries with k == 0
    FilteredShape         sw, se;       // the launches' carves: the largest expansion with the largest C; the largest k + skip
    bool                  lone_riders_launch = false;  // as given to plan_filtered_paths
};

// Step 1, paths and carves: every query's path, expansion and C by the one set of rules, the lists as the path rule leaves them (call
// order), and each launch's carve.  "" or the refusal.  counts[i]: the allowed count of query i's filter, -1 for a NULL entry.
// params: a row per query -- its refusals name the query, " (params[i])" -- or NULL: every query asks for `uniform`, which is shaped
// once per path, the walk's first.  Both are clamped to 2^20 keys before anything is narrowed to 32 bits: far past the LDS budget, so
// refused.  lone_riders_launch: a call of nothing but riders is still one exact launch that carries them, which needs the exact
// carve (the per-query-filter form with uniform parameters; the other two forms answer such a call without a launch).
std::string plan_filtered_paths(const FilterPlanIn &p, const int64_t *counts, size_t nq, const lantern_gpu_query_params *params, FilteredAsk uniform,
                                bool lone_riders_launch, FilteredCallPlan &out);
// Step 2, closing the lists as they stand now (a dense route between the steps takes queries out of the exact list and appends the
// ones its certificate refused): the walk list by expansion descending, the exact list by allowed count descending, both stable -- the
// longest first, so that a launch's tail is a short one -- and the riders behind the exact list, or behind the walk list when that
// is the only one with a query in it.
void plan_filtered_close(const int64_t *counts, FilteredCallPlan &plan);

bool   count_takes_exact(const FilterPlanIn &p, size_t count, size_t ef_sel);  // the path rule
int    filtered_per_cu(size_t lds);  // workgroups of a filtered launch that a CU holds

}  // namespace lgpu
