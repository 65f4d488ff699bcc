// search_plan.cpp -- the unfiltered search launch: plan_search decides its shape (pure: lantern_gpu_plan_search shows it without a device),
// search_launch makes ONE launch of a plan, search_params_locked plans and launches a batch whose queries bring their own (k, ef, skip).
#include "index.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace lgpu {

SearchEnv search_env()
{
    SearchEnv e;
    if(const char *se = std::getenv("LANTERN_GPU_SPEC")) { e.spec_set = true; e.spec = std::atoi(se); }
    if(const char *se = std::getenv("LANTERN_GPU_ADC_SPEC")) { e.adc_spec_set = true; e.adc_spec = std::atoi(se) != 0; }
    if(const char *pa = std::getenv("LANTERN_GPU_PQ_ADC")) e.pq_adc = std::atoi(pa) != 0;
    if(const char *sw = std::getenv("LANTERN_GPU_SPEC_WAVES")) e.spec_waves = std::atoi(sw);
    // LANTERN_GPU_LDS_LIST=1: walks keep their candidate list in LDS even when it fits wave 0's registers (walk.hpp search_level vs
    // search_level_reg; identical results -- the switch exists for A/B timing and for the parity test that runs both)
    if(const char *ll = std::getenv("LANTERN_GPU_LDS_LIST")) e.lds_list = std::atoi(ll) != 0;
    if(const char *lp = std::getenv("LANTERN_GPU_SCREEN_LIST_PREFETCH")) e.screen_list_prefetch = std::atoi(lp) != 0;
    if(const char *sd = std::getenv("LANTERN_GPU_SCREEN_DESCENT")) e.screen_descent = std::atoi(sd) != 0;
    static const int  wide_env = std::getenv("LANTERN_GPU_WIDE_ROWS") ? std::atoi(std::getenv("LANTERN_GPU_WIDE_ROWS")) : -1;
    static const int  forced = std::getenv("LANTERN_GPU_WAVES_PER_CU") ? std::atoi(std::getenv("LANTERN_GPU_WAVES_PER_CU")) : 0;
    e.wide_rows = wide_env, e.waves_per_cu = forced;
    return e;
}

SearchPlanIn search_plan_in(const Index *ix, size_t nq, size_t k, size_t ef, size_t skip, int waves)
{
    SearchPlanIn in;
    in.chunks = ix->chunks; in.M = ix->M; in.M0 = ix->M0; in.ef_default = ix->ef;
    in.mcode = ix->mcode; in.n = ix->n; in.num_cus = ix->num_cus;
    in.pq_compact = ix->pq_compact; in.pqd_inv = ix->pqd_inv; in.pq_S16 = ix->pq_S16;
    in.search_vis_slots = ix->search_vis_slots; in.search_max_wg = ix->search_max_wg;
    in.phase_profile = ix->phase_profile; in.spec_profile = ix->spec_profile;
    in.screen = ix->d_screen && ix->d_screen_meta;
    in.nq = nq; in.k = k; in.ef = ef; in.skip = skip; in.waves = waves;
    in.env = search_env();
    return in;
}

SearchPlan plan_search(const SearchPlanIn &in)
{
    const SearchEnv &env = in.env;
    const size_t     nq = in.nq;
    int              waves = in.waves;
    SearchPlan       p;
    size_t expansion = in.ef ? in.ef : in.ef_default;
    if(expansion < in.k + in.skip) expansion = in.k + in.skip;  // usearch: expansion = max(expansion, wanted)
    if(in.each) expansion = in.max_expansion;                   // (the per-query form: the largest of the list's own)
    p.expansion = (uint32_t)expansion;
    p.lds_list = env.lds_list;
    // ---- a compact pq index whose subvectors are whole 16-byte chunks: the f32 walk below over rows DECODED ON THE FLY from the
    // L2-resident centroid tables (device_common.hpp PqdRow) -- the arithmetic, and so every bit of every answer, of the expanded
    // form of the same index.  (LANTERN_GPU_PQ_ADC=1, or subvectors of another width: the table walk of search_adc_kernel.hip.)
    const bool pqd = in.pq_compact && !env.pq_adc && in.pqd_inv != 0;
    if(in.pq_compact && !pqd) {
        // ---- a compact pq index: ADC over the code rows (search_adc_kernel.hip).  One 8-wave workgroup per query; the per-query
        // table takes num_subvectors16 x 256 floats of LDS (98 KB at 96 subvectors: one workgroup per CU, three at 32).
        const uint32_t code_chunks = in.pq_S16 / 16;
        uint32_t       vis_slots = 2048;
        if(in.search_vis_slots >= 0) vis_slots = (uint32_t)in.search_vis_slots / 4 * 4;
        while(vis_slots && search_adc_lds_bytes(code_chunks, in.chunks, (uint32_t)expansion, in.M0, vis_slots) > 150 * 1024) vis_slots = vis_slots > 256 ? vis_slots - 256 : 0;
        if(vis_slots && vis_slots < 4 * in.M0) vis_slots = 0;
        size_t lds = search_adc_lds_bytes(code_chunks, in.chunks, (uint32_t)expansion, in.M0, vis_slots);
        if(lds > 160 * 1024) { p.refusal = "lantern_gpu: ef/k exceed the 160 KiB LDS budget of the ADC search kernel"; return p; }
        int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, (160 * 1024) / lds));
        // A table that leaves room for one workgroup per CU anyway (96 subvectors x 256 centroids): every query walks alone on
        // its CU, so it runs the walk that is fastest alone -- walk_spec.hpp's lone-query shape, 3 role + 8 row waves
        // (LANTERN_GPU_ADC_SPEC=0|1 overrides; an explicit wave count selects the classic kernel as for the f32 walk).
        bool adc_spec = false;
        const uint32_t adc_prefetch = in.M0 % 4 == 0 && in.M0 <= 32 ? 1u : 0u, adc_cache = adc_prefetch ? 128u : 0u;  // (8-lane groups: four list words per lane)
        if(waves <= 0 && in.M0 >= 2 && in.M0 <= 64 && expansion <= 128 && !env.lds_list) {
            const size_t with_spec = lds + search_spec_lds_bytes(in.M0, adc_prefetch, adc_cache);
            adc_spec = with_spec <= 160 * 1024 && (env.adc_spec_set ? env.adc_spec : (per_cu == 1 || nq <= (size_t)in.num_cus * 2));  // (small batches: as the f32 walk)
            if(adc_spec) {
                lds = with_spec;
                per_cu = 1;
            }
        }
        // (rows of at most 8 chunks: a row wave holds eight 8-lane groups, so FOUR row waves cover a 32-entry list in one pass --
        // measured, LANTERN_GPU_SPEC_WAVES=7: 1.84 M queries/s against 1.96 M with eight: the shorter row waves matter more)
        int aw = adc_spec ? 11 : waves > 0 ? std::min(waves, 8) : 8;
        if(adc_spec && env.spec_waves >= 4 && env.spec_waves <= 11) aw = env.spec_waves;
        // (the grid is this path's own: LANTERN_GPU_WAVES_PER_CU does not reach it)
        size_t g = (size_t)in.num_cus * (size_t)per_cu;
        if(in.search_max_wg > 0) g = (size_t)in.search_max_wg;
        p.path = kSearchAdc, p.spec = adc_spec ? 2 : 0, p.took_spec = adc_spec;
        p.waves = aw, p.grid = (int)std::max<size_t>(1, std::min(g, nq));
        p.vis_slots = vis_slots, p.lds = lds;
        p.spec_prefetch = adc_spec ? adc_prefetch : 0, p.spec_cache = adc_spec ? adc_cache : 0;
        return p;
    }
    // Launch shape.  Batches that fill the chip: four waves per query, six workgroups per CU -- the walk is HBM-bound and its
    // serial phases hide behind other walks' row loads.  Batches that cannot (and the lone query): the latency-bound walk of
    // walk_spec.hpp -- one barrier per hop, speculative row loads, neighbour lists fetched with the rows:
    //   spec 2: at most one query per CU: three role waves + eight row waves per query (a whole list in one pass);
    //   spec 1: up to four four-wave workgroups per CU (on request: LANTERN_GPU_SPEC=1).
    // An explicit wave count (lantern_gpu_set_search_shape; tests, tuning) selects the classic kernel; LANTERN_GPU_SPEC=0|1|2
    // overrides the automatic choice.
    int spec = 0;
    if(waves <= 0) {
        // (the per-query form has no instrumented instantiation: a profiling mode sends it to the classic shape)
        const bool can = in.M0 >= 2 && in.M0 <= 64 && expansion <= 128 && !in.phase_profile && !env.lds_list && !(in.each && in.spec_profile);
        if(can) {
            // (measured, 1M x 768 cosine, one 1024-query batch: the four-wave latency-bound shape 796 k QPS, the classic kernel
            // 819 k -- with every walk of the batch resident the row loads saturate HBM for most of the launch and the speculative
            // rows cost bandwidth; so spec 1 is chosen only on request, spec 2 up to two queries per CU -- one workgroup per CU, the
            // second query after the first: two workgroups side by side measure the same, 631 vs 627 k at 512 queries)
            if(env.spec_set) spec = env.spec;
            else if(nq <= (size_t)in.num_cus * 2) spec = 2;  // (1M x 768 cosine: 384 queries 528 k vs 389 k, 512: 624 k vs 500 k, 768: 658 k vs 691 k)
            if(spec < 0 || spec > 4) spec = 0;
            if(in.each) spec = spec >= 2 ? 2 : 0;  // the per-query form exists for the 3 + 8 wave shape only: spec 1 falls back to the classic shape
            if(spec >= 3) spec = 2;  // (3 and 4 named walks since removed: they mean the default latency-bound walk)
        }
        // (measured, classic kernel, 1M x 768 cosine, 1024 queries: 4 waves 693 k QPS, 6 waves 525 k, 8 waves 594 k -- more waves
        // only make its serial phases costlier; so four waves per query whatever the batch size)
        waves = spec >= 2 ? 11 : spec == 1 ? 4 : waves < 0 ? -waves : 4;  // (a negative count: the caller's classic fallback)
        // tuning: LANTERN_GPU_SPEC_WAVES = waves per query of the latency-bound shapes (spec 1: 2..8; spec 2: 4..11)
        if(spec && env.spec_waves >= (spec >= 2 ? 4 : 2) && env.spec_waves <= (spec >= 2 ? 11 : 8)) waves = env.spec_waves;
    }
    // list prefetch of the latency-bound walk: every lane of a row's group fetches LW words of the row's own list
    const int      G_ = group_lanes_for(in.chunks), LW_ = G_ >= 32 ? 1 : G_ == 16 ? 2 : 4;
    const uint32_t spec_prefetch = spec && in.M0 % (uint32_t)LW_ == 0 && in.M0 <= (uint32_t)(G_ * LW_) ? 1u : 0u;
    const uint32_t spec_cache = !spec_prefetch ? 0u : spec >= 2 ? 128u : 64u;
    const size_t   spec_lds = spec ? search_spec_lds_bytes(in.M0, spec_prefetch, spec_cache) : 0;
    // LDS visited set: sized for ~3x the planner's estimate of visited nodes per query (hnsw.c:89-132 puts it at
    // about 2 M ef S with S ~ 3), capped so that SIX workgroups fit on a CU (more walks in flight beat a roomier
    // set: 1.106 -> 1.17 M QPS at 1M x 768) -- four for the four-wave latency-bound shape, one for the lone-query shape;
    // it spills to the bitmap beyond
    const size_t lds_budget = spec >= 2 ? 96 * 1024 : spec == 1 ? 39 * 1024 : 26 * 1024;
    // The launches that screen (search_kernel.hpp SCREEN: the classic shape of an index with an int8 screen, its list in registers,
    // never the instrumented walk) also hold the query's int8 planes (walk.hpp screen_stage_query): a block of their own behind the
    // visited set, paid for out of vis_slots -- 1.5 KB at 768-d, where 4 864 slots remain of 5 376 and three quarters of them still hold
    // a walk's ~2 150 visits.  Every other launch carves, and plans, what it did before.
    const bool   screened = in.screen && spec == 0 && !pqd && screen_rows_for(in.chunks) && (in.mcode == M_L2SQ || in.mcode == M_COS) &&
                          !(in.phase_profile && !in.each) && !env.lds_list && expansion <= 128;
    const size_t screen_lds = screened ? screen_query_lds_bytes(in.chunks) : 0;
    uint32_t vis_slots = 1024;
    while(vis_slots < 8192 && vis_slots / 4 * 3 < expansion * in.M0 * 2) vis_slots <<= 1;
    if(in.search_vis_slots >= 0) vis_slots = (uint32_t)in.search_vis_slots / 4 * 4;
    while(vis_slots && search_lds_bytes(in.chunks, (uint32_t)expansion, in.M0, vis_slots) + spec_lds + screen_lds > lds_budget)
        vis_slots = vis_slots > 256 ? vis_slots - 256 : 0;
    if(vis_slots && vis_slots < 4 * in.M0) vis_slots = 0;
    p.lds = search_lds_bytes(in.chunks, (uint32_t)expansion, in.M0, vis_slots) + spec_lds + screen_lds;
    p.screen_lds = (uint32_t)screen_lds;
    // the front's list one hop ahead (walk.hpp search_level_reg): in the launches that screen, where the list fetch is a quarter of a hop's
    // dependent round trips; lists of at most 64 entries (one per lane of the visit wave)
    p.list_prefetch = screened && LGPU_SCREEN_LIST_PREFETCH != 0 && in.M0 <= 64 &&
                      (env.screen_list_prefetch >= 0 ? env.screen_list_prefetch != 0 : LGPU_SCREEN_LIST_PREFETCH >= 2);
    // the descent's rows through the screen as well (walk.hpp greedy_descent): a choice of the launches that screen, no part of their shape
    p.screen_descent = screened && (env.screen_descent >= 0 ? env.screen_descent != 0 : LGPU_SCREEN_DESCENT >= 2);
    if(p.lds > 160 * 1024) { p.refusal = "lantern_gpu: ef/k exceed the 160 KiB LDS budget of the search kernel"; return p; }
    p.path = pqd ? kSearchPqd : spec == 0 ? kSearchClassic : spec == 1 ? kSearchSpec1 : kSearchSpec2;
    p.spec = spec, p.took_spec = spec != 0;
    p.waves = waves, p.grid = search_grid(in.num_cus, in.search_max_wg, env.waves_per_cu, nq, waves, spec >= 2 ? waves : spec == 1 ? 16 : 24);
    p.vis_slots = vis_slots, p.spec_prefetch = spec_prefetch, p.spec_cache = spec_cache;
    // small batch (at most four 4-wave workgroups per CU would be resident anyway): four rows in flight per group
    p.wide_rows = spec ? 0 : env.wide_rows >= 0 ? env.wide_rows : (nq * (size_t)waves <= (size_t)in.num_cus * 16 && nq >= 64);
    return p;
}

// ONE launch of plan `p` over nq queries: the launch slot (which orders the launch after inserts and holds the walk's visited bitmaps),
// the kernel arguments, the ticket, the launch through the path's launcher and its counts.  `each`: NULL, or the launch is one class of
// a per-query-parameter call: its table and query list go into the scratch of the launch's slot (one copy in front of the launch; a slot's
// earlier launch is over before its next one starts), or are read where the caller's device-mapped block has them.  false -> ix->err.
static bool search_launch(Index *ix, const SearchPlan &p, const uint4 *d_queries, size_t nq, size_t k, size_t skip, const SearchOut &out,
                          hipStream_t stream, uint32_t *done, uint32_t *done_flags, const EachLaunch *each)
{
    const bool adc = p.path == kSearchAdc, pqd = p.path == kSearchPqd;
    ix->last_search_grid = p.grid;
    const int slot = acquire_search_slot(ix, stream, (size_t)p.grid);
    if(slot < 0) return false;
    SearchArgs a{};
    a.view = ix->view();
    a.frame.queries = d_queries;
    a.frame.nq = (uint32_t)nq, a.k = (uint32_t)k, a.ef = p.expansion, a.skip = (uint32_t)skip;
    a.frame.labels = ix->d_labels;
    a.frame.out_labels = out.labels, a.frame.out_dists = out.dists, a.frame.out_slots = out.slots;
    a.frame.out_counts = out.counts, a.frame.out_D = out.D, a.frame.out_E = out.E;
    a.frame.bitmaps = ix->slot_bitmaps[ slot ], a.frame.bm_words = (uint32_t)ix->slot_words[ slot ], a.frame.undo_cap = vis_undo_cap();
    a.frame.vis_slots = p.vis_slots;
    a.frame.totals = ix->d_totals + kTotSearch;
    a.screen_totals = ix->d_screen ? ix->d_totals + kTotSearchScreen : nullptr;  // lantern_gpu_search_screen_stats
    a.frame.ticket = next_ticket(ix, nq, p.grid, stream);
    a.done = done, a.done_flags = done_flags;
    a.lds_list = p.lds_list, a.wide_rows = p.wide_rows;
    a.spec = p.spec, a.spec_prefetch = p.spec_prefetch, a.spec_cache = p.spec_cache;
    a.list_prefetch = p.list_prefetch, a.screen_descent = p.screen_descent;
    hipError_t e = hipSuccess;
    if(!p.screen_lds) a.view.screen = nullptr, a.view.screen_meta = nullptr, a.view.screen_chunks = 0;  // no planes' block: the launch does not screen
    if(adc || pqd) a.view.vec = (const uint4 *)ix->d_codes16;
    if(adc) {
        a.view.chunks = ix->pq_S16 / 16;
        a.adc_centers = ix->d_centers;
        a.adc_S = ix->pq_S, a.adc_C = ix->pq_C, a.adc_subdim = ix->pq_subdim, a.adc_qchunks = ix->chunks;
    } else {
        if(pqd) {
            a.view.pq_centers = (const uint4 *)ix->d_centers;
            a.view.pq_cps = ix->pq_subdim / 4;
            a.view.pq_C = ix->pq_C;
            a.view.pq_inv = ix->pqd_inv;
            a.view.pq_row_bytes = ix->pq_S16;
        }
        // (there is no instrumented instantiation of the decoding walk: a compact pq launch ignores phase_profile)
        const bool prof_walk = ix->phase_profile && !pqd && !each;  // (nor of the per-query form)
        a.phase_cycles = each ? nullptr : p.spec ? (ix->spec_profile ? ix->d_totals + kTotSpecProfile : nullptr) : prof_walk ? ix->d_totals + kTotPhaseProfile : nullptr;
        // the row bitmap only when unique-rows mode asked for it AND it covers every slot the walk can name (a reserve / add since
        // it was sized would otherwise let mark_touched write past it)
        a.touched = (!p.spec && prof_walk && ix->unique_rows_on && ix->d_touched && ix->touched_words * 32 >= ix->cap) ? ix->d_touched : nullptr;
        if(!p.spec && prof_walk && ix->trace_on && ix->d_trace && nq <= ix->trace_nq) {  // (lantern_gpu_search_row_trace: the launch's own counts start at zero)
            e = hipMemsetAsync(ix->d_trace_count, 0, nq * 4, stream);
            a.trace = ix->d_trace, a.trace_count = ix->d_trace_count, a.trace_cap = (uint32_t)ix->trace_cap;
        }
    }
    if(each) {
        const char *d_tbl = each->d_table;
        if(!d_tbl) {
            char *const d = (char *)scratch(ix, launch_table_scratch(slot), each->table_bytes);
            if(!d) return false;
            if(hipMemcpyAsync(d, each->h_table, each->table_bytes, hipMemcpyHostToDevice, stream) != hipSuccess)
                return set_err(ix, "lantern_gpu: HIP failure (per-query parameter table)"), false;
            d_tbl = d;
        }
        a.qparams = (const uint4 *)d_tbl;
        a.frame.qlist = (const uint32_t *)(d_tbl + each->list_at);
        a.k_stride = a.k;
    }
    if(e == hipSuccess) {
        if(adc) e = launch_search_adc(ix->metric + M_ADC, a, p.waves, p.grid, stream);
        else e = launch_search(pqd ? ix->metric + M_PQD : ix->mcode, a, p.waves, p.grid, stream);
    }
    if(e != hipSuccess) return set_err(ix, std::string("lantern_gpu: HIP error launching the search: ") + hipGetErrorString(e)), false;
    if(done) ix->slot_pending[ slot ] = false;  // the caller waits for the kernel itself: nothing to order later launches against
    else if(!release_search_slot(ix, slot, stream)) return false;
    ix->c_search_queries += nq;
    return true;
}

bool run_search_device(Index *ix, const uint4 *d_queries, size_t nq, size_t k, size_t ef, size_t skip, const SearchOut &out, hipStream_t stream, int waves, uint32_t *done, uint32_t *done_flags)
{
    if(nq == 0 || k == 0) return true;
    const SearchPlan p = plan_search(search_plan_in(ix, nq, k, ef, skip, waves));
    if(p.refusal) return set_err(ix, p.refusal), false;
    return search_launch(ix, p, d_queries, nq, k, skip, out, stream, done, done_flags, nullptr);
}

// ---- per-query k, ef and skip (lantern_gpu_search_batch_params*) --------------------------------------------------
std::string params_check(const lantern_gpu_query_params *params, size_t nq, size_t k_stride)
{
    if(nq && !params) return "lantern_gpu: null parameter array";
    for(size_t i = 0; i < nq; ++i) {
        const char *why = params[ i ].reserved != 0 ? "lantern_gpu: a query's reserved parameter word must be 0"
                          : params[ i ].k > k_stride ? "lantern_gpu: k_stride is smaller than a query's k"
                                                     : nullptr;
        if(why) return std::string(why) + " (params[" + std::to_string(i) + "])";
    }
    return "";
}

bool search_params_locked(Index *ix, const uint4 *d_queries, size_t nq, const lantern_gpu_query_params *params, size_t k_stride,
                          const SearchOut &out, hipStream_t stream, int waves, uint32_t *done_flags, char *h_block, const char *d_block)
{
    const std::string why = params_check(params, nq, k_stride);
    if(!why.empty()) return set_err(ix, why), false;
    if(nq == 0) return true;
    // the table {k, expansion, skip, 0} by batch position (plan_search's rule: expansion = max(ef or the index's, k + skip)), and
    // the three classes of the list placement (search_kernel.hip: one key per lane up to 64, two up to 128, the LDS list beyond)
    std::vector<char> pageable;
    if(!h_block) { pageable.resize(params_table_bytes(nq)); h_block = pageable.data(); d_block = nullptr; }
    uint32_t *const tbl = (uint32_t *)h_block;
    std::vector<uint32_t> cls[ 3 ];
    uint32_t              top[ 3 ] = { 0, 0, 0 };
    auto class_of = [](uint32_t exp) { return exp <= 64 ? 0 : exp <= 128 ? 1 : 2; };
    for(size_t i = 0; i < nq; ++i) {
        size_t exp = params[ i ].ef ? params[ i ].ef : ix->ef;
        exp = std::max(exp, (size_t)params[ i ].k + (size_t)params[ i ].skip);
        exp = std::min<size_t>(exp, (size_t)1 << 20);  // (far past the LDS budget already: refused below, and it fits the table's word)
        tbl[ 4 * i ] = params[ i ].k, tbl[ 4 * i + 1 ] = (uint32_t)exp, tbl[ 4 * i + 2 ] = params[ i ].skip, tbl[ 4 * i + 3 ] = 0;
        const int c = class_of((uint32_t)exp);
        cls[ c ].push_back((uint32_t)i);
        top[ c ] = std::max(top[ c ], (uint32_t)exp);
    }
    // refusals are for the whole call and come before anything is queued: every class's launch is planned first (a class's size
    // decides its shape, and so its LDS sum)
    SearchPlan plans[ 3 ];
    for(int c = 2; c >= 0; --c) {
        if(cls[ c ].empty()) continue;
        SearchPlanIn in = search_plan_in(ix, cls[ c ].size(), k_stride, 0, 0, waves);
        in.each = true, in.max_expansion = top[ c ];
        plans[ c ] = plan_search(in);
        if(!plans[ c ].refusal) continue;
        for(uint32_t i : cls[ c ]) {  // (batch order: the first position whose own expansion is refused)
            in.max_expansion = tbl[ 4 * i + 1 ];
            if(plan_search(in).refusal) return set_err(ix, std::string(plans[ c ].refusal) + " (params[" + std::to_string(i) + "])"), false;
        }
        return set_err(ix, plans[ c ].refusal), false;
    }
    // within a list: by expansion descending, stable -- the longest walks first, so that the launch's tail is a short one
    uint32_t *lists = tbl + 4 * nq;
    size_t    at = 0;
    uint32_t  launches = 0, any_spec = 0;
    EachLaunch each[ 3 ];
    for(int c = 0; c < 3; ++c) {
        std::stable_sort(cls[ c ].begin(), cls[ c ].end(), [&](uint32_t x, uint32_t y) { return tbl[ 4 * x + 1 ] > tbl[ 4 * y + 1 ]; });
        each[ c ] = EachLaunch{ h_block, nq * 20, d_block, (nq * 4 + at) * 4 };
        if(!cls[ c ].empty()) std::memcpy(lists + at, cls[ c ].data(), cls[ c ].size() * 4);
        at += cls[ c ].size();
    }
    for(int c = 0; c < 3; ++c) {
        if(cls[ c ].empty()) continue;
        if(!search_launch(ix, plans[ c ], d_queries, cls[ c ].size(), k_stride, 0, out, stream, nullptr, done_flags, &each[ c ])) return false;
        launches += 1;
        any_spec |= plans[ c ].took_spec ? 1u : 0u;
    }
    const uint32_t shape[ 6 ] = { launches, (uint32_t)cls[ 0 ].size(), (uint32_t)cls[ 1 ].size(), (uint32_t)cls[ 2 ].size(), std::max(top[ 0 ], std::max(top[ 1 ], top[ 2 ])), any_spec };
    std::copy(std::begin(shape), std::end(shape), ix->last_params);
    return true;
}

// ---- which instantiation a launch took (lantern_gpu_last_search_cells) -------------------------------------------------------------
// A ring of the calling thread's last four unfiltered search launches (a per-query-parameter call makes at most three) and their count
// since the ring was last read.
static const size_t             kCellRing = 4, kCellWords = 10;
static thread_local uint32_t    cell_ring[ kCellRing ][ kCellWords ];
static thread_local size_t      cell_count = 0;

void note_search_cell(int kernel, int metric, int G, int prof, int rows, int kpl, int spec, int each, const SearchArgs &a)
{
    const uint32_t row[ kCellWords ] = { (uint32_t)kernel, (uint32_t)metric, (uint32_t)G, (uint32_t)prof, (uint32_t)rows, (uint32_t)kpl, (uint32_t)spec,
                                         (uint32_t)each, a.view.screen ? 1u : 0u, a.frame.nq };
    std::copy(std::begin(row), std::end(row), cell_ring[ cell_count++ % kCellRing ]);
}

static size_t take_search_cells(uint32_t *cells, size_t cap)
{
    const size_t made = cell_count, kept = std::min(made, kCellRing);
    for(size_t i = 0; cells && i < std::min(kept, cap); ++i)  // oldest first
        std::copy(cell_ring[ (made - kept + i) % kCellRing ], cell_ring[ (made - kept + i) % kCellRing ] + kCellWords, cells + i * kCellWords);
    cell_count = 0;
    return made;
}

}  // namespace lgpu

extern "C" size_t lantern_gpu_last_search_cells(uint32_t *cells, size_t cap) { return lgpu::take_search_cells(cells, cap); }

// the plan without a device (include/lantern_gpu.h has the field order)
static const char *plan_search_flat(const int64_t *in, bool screen, uint32_t *out, uint32_t *screen_lds, int screen_list_prefetch = -1, uint32_t *list_prefetch = nullptr)
{
    if(!in || !out) return "lantern_gpu: null array";
    lgpu::SearchPlanIn s;
    s.screen = screen;
    s.chunks = (uint32_t)in[ 0 ]; s.M = (uint32_t)in[ 1 ]; s.M0 = (uint32_t)in[ 2 ]; s.mcode = (int)in[ 3 ]; s.n = (size_t)in[ 4 ];
    s.ef_default = (uint32_t)in[ 5 ]; s.num_cus = (int)in[ 6 ]; s.pq_compact = in[ 7 ] != 0; s.pqd_inv = (uint32_t)in[ 8 ]; s.pq_S16 = (uint32_t)in[ 9 ];
    s.search_vis_slots = (int)in[ 10 ]; s.search_max_wg = (int)in[ 11 ]; s.phase_profile = in[ 12 ] != 0; s.spec_profile = in[ 13 ] != 0;
    s.nq = (size_t)in[ 14 ]; s.k = (size_t)in[ 15 ]; s.ef = (size_t)in[ 16 ]; s.skip = (size_t)in[ 17 ]; s.waves = (int)in[ 18 ];
    s.each = in[ 19 ] != 0; s.max_expansion = (uint32_t)in[ 20 ];
    s.env.spec_set = in[ 21 ] != 0; s.env.spec = (int)in[ 22 ]; s.env.adc_spec_set = in[ 23 ] != 0; s.env.adc_spec = in[ 24 ] != 0;
    s.env.pq_adc = in[ 25 ] != 0; s.env.spec_waves = (int)in[ 26 ]; s.env.lds_list = in[ 27 ] != 0; s.env.wide_rows = (int)in[ 28 ];
    s.env.waves_per_cu = (int)in[ 30 ];  // (in[ 29 ]: reserved, ignored)
    s.env.screen_list_prefetch = screen_list_prefetch;
    const lgpu::SearchPlan p = lgpu::plan_search(s);
    const uint32_t flat[ 12 ] = { (uint32_t)p.path, (uint32_t)p.spec, p.expansion, (uint32_t)p.waves, (uint32_t)p.grid, p.vis_slots, (uint32_t)p.lds,
                                  p.spec_prefetch, p.spec_cache, (uint32_t)p.wide_rows, p.took_spec ? 1u : 0u, (uint32_t)p.lds_list };
    std::copy(std::begin(flat), std::end(flat), out);
    if(screen_lds) *screen_lds = p.screen_lds;
    if(list_prefetch) *list_prefetch = p.list_prefetch;
    return p.refusal;
}
extern "C" const char *lantern_gpu_plan_search(const int64_t in[ 31 ], uint32_t out[ 12 ]) { return plan_search_flat(in, false, out, nullptr); }
// ... of an index that has (in[31] != 0) or has not an int8 screen; out[12]: the bytes of the query's int8 planes in the launch's LDS
extern "C" const char *lantern_gpu_plan_search_screen(const int64_t in[ 32 ], uint32_t out[ 13 ])
{
    if(!in || !out) return "lantern_gpu: null array";
    return plan_search_flat(in, in[ 31 ] != 0, out, out + 12);
}
// ... with in[32] = LANTERN_GPU_SCREEN_LIST_PREFETCH (-1: unset, 0, 1); out[13]: the launch requests the front's neighbour list one hop ahead
// (only ever != 0 where out[12] != 0)
extern "C" const char *lantern_gpu_plan_search_screen_prefetch(const int64_t in[ 33 ], uint32_t out[ 14 ])
{
    if(!in || !out) return "lantern_gpu: null array";
    return plan_search_flat(in, in[ 31 ] != 0, out, out + 12, in[ 32 ] < 0 ? -1 : in[ 32 ] != 0, out + 13);
}
