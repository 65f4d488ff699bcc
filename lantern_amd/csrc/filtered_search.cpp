// filtered_search.cpp -- filtered k-NN search, everything that queues work: the three forms of a call -- one filter, a filter per
// query, a filter and (k, ef, skip) per query -- each as "plan (filtered_plan.hpp), optional dense route (filtered_dense.hip), close
// the lists, launch"; the cursor's search; the policy setters and getters; and the batched entry points (include/lantern_gpu.h
// "Filtered search"; semantics: DESIGN.md 4.9).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <iterator>
#include <mutex>
#include <string>
#include <vector>

#include "abi_guard.hpp"
#include "filtered_search.hpp"
#include "host_trip.hpp"

namespace lgpu {

static const char *kFilteredBatchFailed = "lantern_gpu: HIP failure during filtered batched search";
constexpr size_t   kFilterSeedsMax = 4096;  // lantern_gpu_set_filter_seeds refuses more

// a compact pq index's row routine, by plan_search's own condition (search_plan.cpp): decoded on the fly, else ADC
static bool compact_adc(const Index *ix) { return ix->pq_compact && (search_env().pq_adc || ix->pqd_inv == 0); }
static FilterPlanIn filter_plan_in(const Index *ix)
{
    FilterPlanIn p{ ix->chunks, ix->M0, ix->n, ix->ef, ix->filter_path, ix->filter_cand_cap, ix->filter_exact_factor, ix->filter_seeds };
    if(compact_adc(ix)) p.adc_code_chunks = ix->pq_S16 / 16;
    p.screen_on = ix->filter_screen, p.mcode = ix->mcode, p.screen_table = ix->d_screen && ix->d_screen_meta, p.pq_compact = ix->pq_compact;
    return p;
}

// (checked after the filters)  A compact pq index is served once lantern_gpu_set_filter_compact has said so.
static bool filtered_index_ok(Index *ix)
{
    const bool refused = ix->pq_compact && !ix->filter_compact;
    if(refused) set_err(ix, "lantern_gpu: filtered search does not run on a compact pq index: expand it first (lantern_gpu_pq_expand)");
    return !refused;
}

// the kernel arguments that depend neither on the filter nor on the path
static FilteredArgs filtered_args(const Index *ix, const uint4 *d_q, size_t k, size_t skip, const SearchOut &out)
{
    FilteredArgs a{};
    a.view = ix->view();
    a.frame.queries = d_q;
    a.k = (uint32_t)k;
    a.skip = (uint32_t)skip;
    a.frame.labels = ix->d_labels;
    a.frame.out_labels = out.labels, a.frame.out_dists = out.dists, a.frame.out_slots = out.slots;
    a.frame.out_counts = out.counts, a.frame.out_D = out.D, a.frame.out_E = out.E;
    a.frame.totals = ix->d_totals + kTotSearch;
    if(ix->pq_compact) {  // the code rows, with what their row routine reads (as search_plan.cpp search_launch fills SearchArgs)
        a.view.vec = (const uint4 *)ix->d_codes16;
        if(compact_adc(ix)) {
            a.view.chunks = ix->pq_S16 / 16;
            a.adc_centers = ix->d_centers;
            a.adc_S = ix->pq_S, a.adc_C = ix->pq_C, a.adc_subdim = ix->pq_subdim, a.adc_qchunks = ix->chunks;
        } else {
            a.view.pq_centers = (const uint4 *)ix->d_centers;
            a.view.pq_cps = ix->pq_subdim / 4;
            a.view.pq_C = ix->pq_C;
            a.view.pq_inv = ix->pqd_inv;
            a.view.pq_row_bytes = ix->pq_S16;
        }
    }
    return a;
}
// a launch's carve into its arguments
static void shape_into(const FilteredShape &s, FilteredArgs &a, size_t &lds)
{
    a.exp = s.exp, a.cand_cap = s.cand_cap, a.rows_per_round = s.rows_per_round, a.frame.vis_slots = s.vis_slots;
    lds = s.lds;
    // no screen block in the carve: the launch does not screen (filtered_launch reads the choice here, as search_plan.cpp's launches do)
    if(!s.screened) a.view.screen = nullptr, a.view.screen_meta = nullptr, a.view.screen_chunks = 0;
}

// the empty answer in every row of a call, kw wide, with no launch
static bool empty_answers(Index *ix, const SearchOut &out, size_t nq, size_t kw, hipStream_t stream)
{
    if(out.labels && kw && hipMemsetAsync(out.labels, 0, nq * kw * 8, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    if(out.dists && kw && hipMemsetD32Async((hipDeviceptr_t)out.dists, 0x7F800000, nq * kw, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    if(out.slots && kw && hipMemsetAsync(out.slots, 0xFF, nq * kw * 4, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    if(out.counts && hipMemsetAsync(out.counts, 0, nq * 4, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    if(out.D && hipMemsetAsync(out.D, 0, nq * 8, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    if(out.E && hipMemsetAsync(out.E, 0, nq * 8, stream) != hipSuccess) return set_err(ix, "lantern_gpu: HIP failure (memset)"), false;
    return true;
}

EachTables each_tables(const Index *ix, char *blk, size_t nq, const Filter *const *filters, const Filter *one, const std::vector<uint32_t> &walk,
                       const std::vector<uint32_t> &exact, const uint32_t *rows)
{
    const size_t off_par = rows ? ((size_t)walk.size() * 4 + 15) & ~(size_t)15 : ((size_t)walk.size() * 4 + 7) & ~(size_t)7;
    const size_t off_desc = off_par + (rows ? nq * 16 : 0), off_sel_e = off_desc + nq * sizeof(FilterDesc);
    const size_t tbl_bytes = off_sel_e + exact.size() * 4;
    if(!walk.empty()) std::memcpy(blk, walk.data(), walk.size() * 4);
    if(rows) std::memcpy(blk + off_par, rows, nq * 16);
    if(!exact.empty()) std::memcpy(blk + off_sel_e, exact.data(), exact.size() * 4);
    FilterDesc *const hd = (FilterDesc *)(blk + off_desc);
    for(size_t i = 0; i < nq; ++i) {
        const Filter *f = filters ? filters[ i ] : one;
        hd[ i ] = f ? FilterDesc{ f->d_bits, f->d_slots, (uint32_t)f->count, 0u } : FilterDesc{ nullptr, nullptr, 0u, ix->n ? 1u : 0u };
    }
    return EachTables{ EachTable{ blk, off_sel_e, off_desc, 0, rows ? off_par : kNoTable },
                       EachTable{ blk + off_par, tbl_bytes - off_par, off_desc - off_par, off_sel_e - off_par, rows ? 0 : kNoTable } };
}

int filtered_launch(Index *ix, bool exact, FilteredArgs &a, size_t lds, hipStream_t stream, const EachTable *tbl)
{
    const bool screened = exact && a.view.screen;  // (shape_into: the plan's choice)
    const int  waves = screened ? kFilterScreenThreads / 64 : kFilteredWaves;
    const int  per_cu = screened ? filtered_screen_per_cu(lds) : filtered_per_cu(lds);
    const int  grid = search_grid(ix, a.frame.nq, waves, waves * per_cu);
    const int slot = acquire_search_slot(ix, stream, (size_t)grid);
    if(slot < 0) return -1;
    if(tbl) {
        char *const d_tbl = (char *)scratch(ix, launch_table_scratch(slot), tbl->bytes);
        if(!d_tbl) return -1;
        if(hipMemcpyAsync(d_tbl, tbl->host, tbl->bytes, hipMemcpyHostToDevice, stream) != hipSuccess) {
            set_err(ix, "lantern_gpu: HIP failure (per-query filter table)");
            return -1;
        }
        a.descs = (const FilterDesc *)(d_tbl + tbl->descs_at);
        a.frame.qlist = (const uint32_t *)(d_tbl + tbl->select_at);
        if(tbl->params_at != kNoTable) a.qparams = (const uint4 *)(d_tbl + tbl->params_at);
    }
    a.frame.bitmaps = ix->slot_bitmaps[ slot ];
    a.frame.bm_words = (uint32_t)ix->slot_words[ slot ];
    a.frame.undo_cap = vis_undo_cap();
    a.frame.ticket = next_ticket(ix, a.frame.nq, grid, stream);
    hipError_t e;
    if(screened) {
        // lantern_gpu_last_filtered_screen: the call's first screened launch starts its counters from zero, on the launch's own stream
        if(ix->last_screen_launches == 0 && hipMemsetAsync(ix->d_totals + kTotFilterScreen, 0, 3 * sizeof(unsigned long long), stream) != hipSuccess) {
            set_err(ix, "lantern_gpu: HIP failure (memset)");
            return -1;
        }
        ix->last_screen_launches += 1;
        e = launch_exact_allowed_screened(ix->mcode, a, grid, stream);
    } else if(ix->pq_compact) {
        const int metric = ix->metric + (a.adc_centers ? M_ADC : M_PQD);
        e = exact ? launch_search_exact_allowed_pq(metric, a, kFilteredWaves, grid, stream) : launch_search_filtered_pq(metric, a, kFilteredWaves, grid, stream);
    } else {
        e = exact ? launch_search_exact_allowed(ix->mcode, a, kFilteredWaves, grid, stream) : launch_search_filtered(ix->mcode, a, kFilteredWaves, grid, stream);
    }
    if(e != hipSuccess) {
        set_err(ix, std::string("lantern_gpu: HIP error launching the filtered search: ") + hipGetErrorString(e));
        return -1;
    }
    if(!release_search_slot(ix, slot, stream)) return -1;
    (exact ? ix->c_filter_exact : ix->c_filter_walk) += 1;
    return grid;
}

// ---- one filter for the whole call ---------------------------------------------------------------------------------------------------
// The caller holds ix->mu and has flushed.  false -> ix->err.  Every query stands behind the one filter, so the call is planned as
// ONE of them: all are riders (the empty answer, no launch), or all take one path in a launch without a table -- unless the walk is
// seeded, which exists in the per-query form only: then every query's descriptor is this filter, the selection list the identity.
// batch_call: one of the two single-filter batch entry points, which alone may take the exact path's dense route
// (lantern_gpu_set_filter_dense); a cursor's search never does.
static bool filtered_search_locked(Index *ix, const Filter *f, const uint4 *d_q, size_t nq, size_t k, size_t ef, size_t skip, const SearchOut &out,
                                   hipStream_t stream, bool batch_call = false)
{
    const std::string why = filter_mismatch(ix, f);
    if(!why.empty()) return set_err(ix, why), false;
    if(!filtered_index_ok(ix)) return false;
    if(nq == 0 || k == 0) return true;
    std::fill(std::begin(ix->last_seeds), std::end(ix->last_seeds), 0u);
    ix->last_screen_launches = 0;
    const int64_t     count = (int64_t)f->count;
    FilteredCallPlan  plan;
    const std::string bad = plan_filtered_paths(filter_plan_in(ix), &count, 1, nullptr, FilteredAsk{ k, ef, skip }, false, plan);
    if(!bad.empty()) return set_err(ix, bad), false;
    if(plan.path[ 0 ] == 0) {  // nothing allowed: the empty answer, no launch
        std::fill(std::begin(ix->last_filtered), std::end(ix->last_filtered), 0u);
        return empty_answers(ix, out, nq, k, stream);
    }
    const bool   exact = plan.path[ 0 ] == 2;
    FilteredArgs a = filtered_args(ix, d_q, k, skip, out);
    a.frame.nq = (uint32_t)nq;
    a.allow_bits = f->d_bits;
    a.allow_slots = f->d_slots;
    a.allow_count = (uint32_t)f->count;
    size_t lds = 0;
    shape_into(exact ? plan.se : plan.sw, a, lds);
    if(batch_call && ix->filter_dense_min) {  // the exact path's second implementation: the same answers from the contraction
        const DenseEnv    env = dense_env();
        FilteredDensePlan dense;
        const char *const no = plan_filtered_dense(ix->mcode, ix->chunks, (int64_t)f->count, (int64_t)nq, (int64_t)k, (int64_t)skip,
                                                   (int64_t)ix->filter_dense_min, exact, ix->pq_compact, env.native, env.fused, dense);
        if(!no && dense.why == kDenseTaken) return filtered_dense_locked(ix, f, dense, env.native, d_q, nq, k, skip, out, a, lds, stream);
    }
    int grid;
    if(!exact && ix->filter_seeds) {
        std::vector<uint32_t> identity(nq);
        for(size_t i = 0; i < nq; ++i) identity[ i ] = (uint32_t)i;
        std::vector<char> tbl(each_table_bytes(nq));
        const EachTables  t = each_tables(ix, tbl.data(), nq, nullptr, f, identity, {}, nullptr);
        a.seeds = (uint32_t)ix->filter_seeds;
        grid = filtered_launch(ix, false, a, lds, stream, &t.walk);  // (pageable staging: the copy completes before this returns)
        ix->last_seeds[ 1 ] = (uint32_t)std::min(ix->filter_seeds, f->count);
        ix->last_seeds[ 2 ] = (uint32_t)nq;
    } else {
        grid = filtered_launch(ix, exact, a, lds, stream);
        if(!exact) ix->last_seeds[ 3 ] = (uint32_t)nq;
    }
    if(grid < 0) return false;
    const uint32_t shape[ 6 ] = { exact ? 2u : 1u, (uint32_t)grid, a.exp, a.cand_cap, a.frame.vis_slots, (uint32_t)lds };
    std::copy(std::begin(shape), std::end(shape), ix->last_filtered);
    ix->c_search_queries += nq;
    return true;
}

// ---- the per-query forms: filters[i] is query i's filter -----------------------------------------------------------------------------
// Every entry of filters[] is NULL or a live filter of this index at its present size; else ix->err names the first offender.
static bool each_filters_ok(Index *ix, const Filter *const *filters, size_t nq)
{
    for(size_t i = 0; i < nq; ++i) {
        const Filter *f = filters[ i ];
        if(!f) continue;
        const std::string why = f->magic != kFilterMagic ? std::string(kNotAFilter) : filter_mismatch(ix, f);
        if(why.empty()) continue;
        set_err(ix, why + " (filters[" + std::to_string(i) + "])");
        return false;
    }
    return filtered_index_ok(ix);
}
// the allowed count of every query's filter as the plan reads it: -1 for a NULL entry
static std::vector<int64_t> each_counts(const Filter *const *filters, size_t nq)
{
    std::vector<int64_t> counts(nq);
    for(size_t i = 0; i < nq; ++i) counts[ i ] = filters[ i ] ? (int64_t)filters[ i ]->count : -1;
    return counts;
}

// The launches of a per-query call whose plan is closed: each list that holds a query is ONE launch over it, and every answer lands
// in the caller's row of its query; what rides in a launch without a path gets the empty answer from a descriptor with count 0,
// without touching a row.  kw: the width of an answer row; skip: the uniform call's (a parameter row brings its own).
// `h_tbl`: a page-locked block of each_table_bytes(nq, parameter rows) that stays untouched until the stream work is done, or NULL
// (pageable staging: the copies then complete before this returns).  false -> ix->err.
static bool each_launches(Index *ix, const FilteredCallPlan &plan, const Filter *const *filters, const uint4 *d_q, size_t nq, size_t kw, size_t skip,
                          const SearchOut &out, hipStream_t stream, char *h_tbl)
{
    std::vector<const Filter *> distinct;
    for(size_t i = 0; i < nq; ++i)
        if(filters[ i ]) distinct.push_back(filters[ i ]);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());

    const uint32_t *const rows = plan.rows.empty() ? nullptr : plan.rows.data();
    std::vector<char>     pageable;
    if(!h_tbl) { pageable.resize(each_table_bytes(nq, rows != nullptr)); h_tbl = pageable.data(); }
    const EachTables t = each_tables(ix, h_tbl, nq, filters, nullptr, plan.walk, plan.exact, rows);

    uint32_t launches = 0;
    for(int pass = 0; pass < 2; ++pass) {
        const bool                   ex = pass == 1;
        const std::vector<uint32_t> &list = ex ? plan.exact : plan.walk;
        if(list.empty()) continue;
        FilteredArgs a = filtered_args(ix, d_q, kw, skip, out);
        a.frame.nq = (uint32_t)list.size();
        if(!ex) a.seeds = (uint32_t)ix->filter_seeds;  // (an unfiltered entry has no slot list: it runs the unseeded walk in the same launch)
        size_t lds = 0;
        shape_into(ex ? plan.se : plan.sw, a, lds);
        if(filtered_launch(ix, ex, a, lds, stream, ex ? &t.exact : &t.walk) < 0) return false;
        launches += 1;
    }
    const EachCounts &c = plan.counts;
    const uint32_t    shape[ 6 ] = { c.walk, c.exact, c.unfiltered, c.empty, (uint32_t)distinct.size(), launches };
    std::copy(std::begin(shape), std::end(shape), ix->last_each);
    const uint32_t n_seeded = ix->filter_seeds ? c.walk - c.unfiltered : 0u;
    ix->last_seeds[ 2 ] = n_seeded;
    ix->last_seeds[ 3 ] = c.walk - n_seeded;
    ix->c_search_queries += nq;
    return true;
}

// Per-query filters, uniform (k, ef, skip).  The caller holds ix->mu and has flushed.  A call of nothing but riders is still one exact
// launch that carries them.  false -> ix->err; nothing has been launched unless the failure is HIP's.
// dense_call: one of the two entry points that may send groups of exact-path queries sharing a filter handle through the dense route
// (lantern_gpu_set_filter_dense_each): those queries leave the exact list, the dense run answers them in front of the launches, and
// the ones its certificate refuses come back into the exact list -- the carves, and their refusals, are by the lists as the path rule
// left them: the dense route changes neither.  The lane form never does.  With a dense group the sentence above holds up to the
// dense run only: when a launch behind it is then refused for a reason that is not HIP's (a scratch block, a launch slot), the call
// fails with the certified dense queries' rows already written and their D already in the cumulative counter.
static bool filtered_each_locked(Index *ix, const Filter *const *filters, const uint4 *d_q, size_t nq, size_t k, size_t ef, size_t skip,
                                 const SearchOut &out, hipStream_t stream, char *h_tbl, bool dense_call = false)
{
    if(!each_filters_ok(ix, filters, nq)) return false;
    std::fill(std::begin(ix->last_each_dense), std::end(ix->last_each_dense), 0u);
    std::fill(std::begin(ix->last_each_dense_launches), std::end(ix->last_each_dense_launches), 0u);
    ix->last_screen_launches = 0;
    if(nq == 0 || k == 0) return true;
    const std::vector<int64_t> counts = each_counts(filters, nq);
    FilteredCallPlan           plan;
    const std::string          bad = plan_filtered_paths(filter_plan_in(ix), counts.data(), nq, nullptr, FilteredAsk{ k, ef, skip }, true, plan);
    if(!bad.empty()) return set_err(ix, bad), false;

    if(dense_call && ix->filter_dense_each_min && !plan.exact.empty()) {
        const DenseEnv       env = dense_env();
        std::vector<int64_t> ids(nq), allowed(nq);
        std::vector<uint8_t> is_exact(nq);
        for(size_t i = 0; i < nq; ++i) {
            ids[ i ] = filters[ i ] ? (int64_t)(uintptr_t)filters[ i ] : -1;  // (a handle's address is a user-space one: never negative)
            allowed[ i ] = std::max<int64_t>(counts[ i ], 0);
            is_exact[ i ] = plan.path[ i ] == 2;
        }
        EachDensePlan     dense;
        const char *const no = plan_filtered_each_dense(ix->mcode, ix->chunks, (int64_t)k, (int64_t)skip, (int64_t)ix->filter_dense_each_min, ix->pq_compact,
                                                        env.native, ids.data(), allowed.data(), is_exact.data(), nq, dense);
        if(!no && dense.why == kEachDenseTaken) {
            std::vector<uint32_t> refused;
            if(!filtered_each_dense_locked(ix, filters, dense, d_q, k, skip, out, stream, refused)) return false;
            std::vector<uint32_t> &exact = plan.exact;
            exact.erase(std::remove_if(exact.begin(), exact.end(), [ & ](uint32_t q) { return dense.group[ q ] != 0xFFFFFFFFu; }), exact.end());
            exact.insert(exact.end(), refused.begin(), refused.end());
        }
    }
    plan_filtered_close(counts.data(), plan);
    return each_launches(ix, plan, filters, d_q, nq, k, skip, out, stream, h_tbl);
}

// Per-query filters AND per-query (k, ef, skip), step 1: the filters checked, the call planned and -- no dense route stands between
// the steps of this form -- closed.  The caller holds ix->mu and has flushed.  false -> ix->err; nothing is queued.
static bool each_params_plan_locked(Index *ix, const Filter *const *filters, const lantern_gpu_query_params *params, size_t nq, FilteredCallPlan &plan)
{
    static const lantern_gpu_query_params none{};
    if(!each_filters_ok(ix, filters, nq)) return false;
    const std::vector<int64_t> counts = each_counts(filters, nq);
    const std::string          why = plan_filtered_paths(filter_plan_in(ix), counts.data(), nq, params ? params : &none, FilteredAsk{}, false, plan);
    if(!why.empty()) return set_err(ix, why), false;
    plan_filtered_close(counts.data(), plan);
    return true;
}

// ... step 2, under the same hold of the mutex: the launches.  A batch is planned whatever its width (k_stride == 0 is a batch of
// k_i == 0); a call of nothing but riders is answered without a launch.  `h_tbl` as each_launches', of each_table_bytes(nq, true).
static bool filtered_each_params_locked(Index *ix, const FilteredCallPlan &plan, const Filter *const *filters, const uint4 *d_q, size_t nq, size_t k_stride,
                                        const SearchOut &out, hipStream_t stream, char *h_tbl)
{
    std::fill(std::begin(ix->last_each_dense), std::end(ix->last_each_dense), 0u);
    std::fill(std::begin(ix->last_each_dense_launches), std::end(ix->last_each_dense_launches), 0u);  // (a per-query-filter call that makes no dense run)
    ix->last_screen_launches = 0;
    if(nq == 0) return true;
    const uint32_t shape[ 4 ] = { plan.sw.exp, plan.sw.cand_cap, plan.se.exp, plan.n_k0 };
    std::copy(std::begin(shape), std::end(shape), ix->last_each_params);
    if(plan.walk.empty() && plan.exact.empty()) {
        const uint32_t none[ 6 ] = { 0, 0, 0, plan.counts.empty, 0, 0 };
        std::copy(std::begin(none), std::end(none), ix->last_each);
        ix->last_seeds[ 2 ] = ix->last_seeds[ 3 ] = 0;
        return empty_answers(ix, out, nq, k_stride, stream);
    }
    return each_launches(ix, plan, filters, d_q, nq, k_stride, 0, out, stream, h_tbl);  // (k: the width of an answer row)
}

// one query through `cur` (streaming: never a row twice): the first k allowed rows not handed out before
static size_t cursor_search_filtered_locked(Index *ix, const Filter *f, Cursor *cur, const void *query, int kind, size_t k, size_t ef, bool streaming,
                                            uint64_t *labels, float *distances)
{
    if(!cursor_epoch_ok(ix, cur, streaming)) return 0;
    if(ix->n == 0 || k == 0) return 0;
    const size_t want = std::max<size_t>(1, std::min(cur->seen.size() + k, std::max<size_t>(f->count, 1)));
    const size_t row = (size_t)ix->chunks * 16;
    std::vector<uint32_t> padded((size_t)ix->chunks * 4);
    pad_row(ix, query, kind, padded.data());
    char *dq = (char *)scratch(ix, kScratchCallIn, row);
    char *dout = (char *)scratch(ix, kScratchCallOut, want * 16 + 16);
    if(!dq || !dout) return 0;
    bool ok = hipMemcpyAsync(dq, padded.data(), row, hipMemcpyHostToDevice, ix->stream) == hipSuccess;
    const SearchOut out{ (uint64_t *)dout, (float *)(dout + want * 8), (uint32_t *)(dout + want * 12), (uint32_t *)(dout + want * 16), nullptr, nullptr };
    ok = ok && filtered_search_locked(ix, f, (const uint4 *)dq, 1, want, ef, 0, out, ix->stream);
    std::vector<char> h(want * 16 + 4);
    ok = ok && hipMemcpyAsync(h.data(), dout, want * 16 + 4, hipMemcpyDeviceToHost, ix->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(ix->stream) == hipSuccess;
    if(!ok) {
        if(ix->err.empty()) set_err(ix, "lantern_gpu: HIP failure during filtered search");
        return 0;
    }
    uint32_t got;
    std::memcpy(&got, h.data() + want * 16, 4);
    return take_unseen(cur, (const uint64_t *)h.data(), (const float *)(h.data() + want * 8), (const uint32_t *)(h.data() + want * 12), got, k, labels, distances);
}

}  // namespace lgpu

// =====================================================================================================
// C ABI
// =====================================================================================================
using namespace lgpu;

// the tail of a policy setter or getter, behind its own argument checks: the handle, then `f(ix)` under the index's mutex
template <class F> static void with_locked(usearch_index_t h, usearch_error_t *e, F f)
{
    Index *ix = H(h, e);
    if(!ix) return;
    std::lock_guard<std::mutex> g(ix->mu);
    f(ix);
}
// a record array of the index copied out under the mutex: the lantern_gpu_last_* and *_stats getters
template <class T, size_t N> static void record_out(usearch_index_t h, T (Index::*record)[ N ], T *out, usearch_error_t *e)
{
    Index *ix = H(h, e);
    if(!ix) return;
    if(!out) { FAIL(e, "lantern_gpu: null output array"); return; }
    std::lock_guard<std::mutex> g(ix->mu);
    std::copy(std::begin(ix->*record), std::end(ix->*record), out);
}

// The handles of a per-query call: the filter array, then the index.  Whether every entry belongs to the index can only be told with the
// index in hand (each_filters_ok, which names the first offender of any kind); without one, an entry that is no filter at all is
// still worth naming.
static Index *FHS(usearch_index_t h, const lantern_gpu_filter_t *const *filters, size_t nq, usearch_error_t *e)
{
    static thread_local std::string msg;
    if(nq && !filters) { FAIL(e, "lantern_gpu: null filter array"); return nullptr; }
    Index *ix = H(h, e);
    if(ix) return ix;
    for(size_t i = 0; i < nq; ++i) {
        if(!filters[ i ] || ((const Filter *)filters[ i ])->magic == kFilterMagic) continue;
        msg = std::string(kNotAFilter) + " (filters[" + std::to_string(i) + "])";
        FAIL(e, msg.c_str());
        break;
    }
    return nullptr;
}
// The refusals every entry point of a per-query family makes before its trip, in their order: the handles (FHS); the parameter array
// if the family has one (k_stride: its rows' width); the scalar kind of host queries (kind < 0: the device form, whose rows are the
// index's own).  What a form says about its own buffers follows in the form.
static Index *each_head(usearch_index_t h, const lantern_gpu_filter_t *const *filters, size_t nq, const lantern_gpu_query_params *params, size_t k_stride,
                        bool with_params, int kind, usearch_error_t *e)
{
    static thread_local std::string msg;
    Index *ix = FHS(h, filters, nq, e);
    if(!ix) return nullptr;
    if(with_params) {
        msg = params_check(params, nq, k_stride);
        if(!msg.empty()) { FAIL(e, msg.c_str()); return nullptr; }
    }
    if(kind >= 0 && !kind_accepted(ix, kind)) { FAIL(e, kKindMismatch); return nullptr; }
    return ix;
}

extern "C" {

void lantern_gpu_set_filter_policy(usearch_index_t h, int path, size_t cand_cap, double exact_factor, usearch_error_t *e)
try {
    CLEAR(e);
    if(path < 0 || path > 2) { FAIL(e, "lantern_gpu: filter path must be 0 (auto), 1 (walk) or 2 (exact)"); return; }
    if(!(exact_factor >= 0) || std::isinf(exact_factor)) { FAIL(e, "lantern_gpu: exact_factor must be a finite number >= 0"); return; }
    with_locked(h, e, [ & ](Index *ix) {
        ix->filter_path = path;
        ix->filter_cand_cap = cand_cap;
        ix->filter_exact_factor = exact_factor;
    });
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_set_filter_seeds(usearch_index_t h, size_t seeds, usearch_error_t *e)
try {
    CLEAR(e);
    if(seeds > kFilterSeedsMax) { FAIL(e, "lantern_gpu: filter seeds must be at most 4096 (0 = off)"); return; }
    with_locked(h, e, [ & ](Index *ix) { ix->filter_seeds = seeds; });
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_set_filter_compact(usearch_index_t h, int on, usearch_error_t *e)
try {
    CLEAR(e);
    if(on != 0 && on != 1) { FAIL(e, "lantern_gpu: filter_compact must be 0 (compact pq indexes refused) or 1 (served)"); return; }
    with_locked(h, e, [ & ](Index *ix) { ix->filter_compact = on != 0; });
}
LANTERN_ABI_CATCH_VOID(e)

int lantern_gpu_filter_compact(usearch_index_t h, usearch_error_t *e)
try {
    CLEAR(e);
    int served = 0;
    with_locked(h, e, [ & ](Index *ix) { served = !ix->filter_compact ? 0 : !ix->pq_compact ? 1 : compact_adc(ix) ? 3 : 2; });
    return served;
}
LANTERN_ABI_CATCH(e)

void lantern_gpu_set_filter_screen(usearch_index_t h, int on, usearch_error_t *e)
try {
    CLEAR(e);
    if(on != 0 && on != 1) { FAIL(e, "lantern_gpu: filter_screen must be 0 (today's exact pass) or 1 (screened where the index qualifies)"); return; }
    with_locked(h, e, [ & ](Index *ix) { ix->filter_screen = on != 0; });
}
LANTERN_ABI_CATCH_VOID(e)

int lantern_gpu_filter_screen(usearch_index_t h, usearch_error_t *e)
try {
    CLEAR(e);
    int on = 0;
    with_locked(h, e, [ & ](Index *ix) { on = ix->filter_screen ? 1 : 0; });
    return on;
}
LANTERN_ABI_CATCH(e)

void lantern_gpu_last_filtered_screen(usearch_index_t h, uint64_t out[ 4 ], usearch_error_t *e)
try {
    CLEAR(e);
    if(!out) { FAIL(e, "lantern_gpu: null output array"); return; }
    out[ 0 ] = out[ 1 ] = out[ 2 ] = out[ 3 ] = 0;
    with_locked(h, e, [ & ](Index *ix) {
        if(ix->last_screen_launches == 0) return;  // (the unscreened launch writes nothing: the counters are an earlier call's)
        unsigned long long t[ 3 ] = {};
        if(hipDeviceSynchronize() != hipSuccess || hipMemcpy(t, ix->d_totals + kTotFilterScreen, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess) {
            FAIL(e, "lantern_gpu: HIP failure reading the screen counters");
            return;
        }
        out[ 0 ] = ix->last_screen_launches, out[ 1 ] = t[ 0 ], out[ 2 ] = t[ 1 ], out[ 3 ] = t[ 2 ];
    });
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_set_filter_dense(usearch_index_t h, size_t min_queries, usearch_error_t *e)
try {
    CLEAR(e);
    with_locked(h, e, [ & ](Index *ix) { ix->filter_dense_min = min_queries; });
}
LANTERN_ABI_CATCH_VOID(e)

size_t lantern_gpu_filter_dense(usearch_index_t h, usearch_error_t *e)
try {
    CLEAR(e);
    size_t min_queries = 0;
    with_locked(h, e, [ & ](Index *ix) { min_queries = ix->filter_dense_min; });
    return min_queries;
}
LANTERN_ABI_CATCH(e)

void lantern_gpu_filter_dense_stats(usearch_index_t h, uint64_t out[ 4 ], usearch_error_t *e)
try {
    CLEAR(e);
    record_out(h, &Index::c_filter_dense, out, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_set_filter_dense_each(usearch_index_t h, size_t min_group, usearch_error_t *e)
try {
    CLEAR(e);
    with_locked(h, e, [ & ](Index *ix) { ix->filter_dense_each_min = min_group; });
}
LANTERN_ABI_CATCH_VOID(e)

size_t lantern_gpu_filter_dense_each(usearch_index_t h, usearch_error_t *e)
try {
    CLEAR(e);
    size_t min_group = 0;
    with_locked(h, e, [ & ](Index *ix) { min_group = ix->filter_dense_each_min; });
    return min_group;
}
LANTERN_ABI_CATCH(e)

void lantern_gpu_last_filtered_each_dense(usearch_index_t h, uint32_t out[ 6 ], usearch_error_t *e)
try {
    CLEAR(e);
    record_out(h, &Index::last_each_dense, out, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_set_filter_dense_each_batched(usearch_index_t h, int on, usearch_error_t *e)
try {
    CLEAR(e);
    if(on != 0 && on != 1) { FAIL(e, "lantern_gpu: filter_dense_each_batched must be 0 (one launch per step) or 1 (one per batch)"); return; }
    with_locked(h, e, [ & ](Index *ix) { ix->filter_dense_each_batched = on != 0; });
}
LANTERN_ABI_CATCH_VOID(e)

int lantern_gpu_filter_dense_each_batched(usearch_index_t h, usearch_error_t *e)
try {
    CLEAR(e);
    int on = 0;
    with_locked(h, e, [ & ](Index *ix) { on = ix->filter_dense_each_batched ? 1 : 0; });
    return on;
}
LANTERN_ABI_CATCH(e)

void lantern_gpu_last_filtered_each_dense_launches(usearch_index_t h, uint32_t out[ 4 ], usearch_error_t *e)
try {
    CLEAR(e);
    record_out(h, &Index::last_each_dense_launches, out, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_last_filtered_seeds(usearch_index_t h, uint32_t out[ 4 ], usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return;
    if(!out) { FAIL(e, "lantern_gpu: null output array"); return; }
    std::lock_guard<std::mutex> g(ix->mu);
    out[ 0 ] = (uint32_t)ix->filter_seeds;  // (the setting, not a record: last_seeds[0] is unused)
    std::copy(ix->last_seeds + 1, ix->last_seeds + 4, out + 1);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_filter_stats(usearch_index_t h, uint64_t *walk_launches, uint64_t *exact_launches, usearch_error_t *e)
try {
    CLEAR(e);
    with_locked(h, e, [ & ](Index *ix) {
        if(walk_launches) *walk_launches = ix->c_filter_walk;
        if(exact_launches) *exact_launches = ix->c_filter_exact;
    });
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_last_filtered_launch(usearch_index_t h, uint32_t out[ 6 ], usearch_error_t *e)
try {
    CLEAR(e);
    record_out(h, &Index::last_filtered, out, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_last_filtered_each(usearch_index_t h, uint32_t out[ 6 ], usearch_error_t *e)
try {
    CLEAR(e);
    record_out(h, &Index::last_each, out, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_last_filtered_each_params(usearch_index_t h, uint32_t out[ 4 ], usearch_error_t *e)
try {
    CLEAR(e);
    record_out(h, &Index::last_each_params, out, e);
}
LANTERN_ABI_CATCH_VOID(e)

// ---- one filter ----------------------------------------------------------------------------------------------------------------------
void lantern_gpu_search_batch_filtered_device(usearch_index_t h, const lantern_gpu_filter_t *filter, const void *d_queries, size_t query_stride_bytes,
                                              size_t nq, size_t k, size_t ef, size_t skip, uint64_t *d_labels, float *d_distances, uint32_t *d_slots,
                                              uint32_t *d_counts, uint64_t *d_D, uint64_t *d_E, void *stream, usearch_error_t *e)
try {
    CLEAR(e);
    const Filter *f = FF(filter, e);
    if(!f) return;
    Index *ix = H(h, e);
    if(!ix) return;
    const SearchOut out{ d_labels, d_distances, d_slots, d_counts, d_D, d_E };
    device_trip(ix, stride_is(query_stride_bytes),
                [ & ] { return filtered_search_locked(ix, f, (const uint4 *)d_queries, nq, k, ef, skip, out, (hipStream_t)stream, true); }, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_search_batch_filtered(usearch_index_t h, const lantern_gpu_filter_t *filter, const void *queries, size_t nq, usearch_scalar_kind_t kind,
                                       size_t k, size_t ef, usearch_label_t *labels, float *distances, uint32_t *counts, usearch_error_t *e)
try {
    CLEAR(e);
    const Filter *f = FF(filter, e);
    if(!f) return;
    Index *ix = H(h, e);
    if(!ix) return;
    if(!kind_accepted(ix, (int)kind)) { FAIL(e, kKindMismatch); return; }
    if(nq == 0 || k == 0) return;
    if(!queries || !labels || !distances) { FAIL(e, "lantern_gpu: null query or result pointer"); return; }
    host_trip_sync(ix, nq, k, 0, queries, (int)kind, kFilteredBatchFailed, nullptr,
                   [ = ](const HostBatch &b) { return filtered_search_locked(ix, f, (const uint4 *)b.d_q, nq, k, ef, 0, b.out(b.d_out), b.stream, true); }, labels,
                   distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

size_t lantern_gpu_cursor_search_filtered(lantern_gpu_cursor_t *c, const lantern_gpu_filter_t *filter, const void *query, usearch_scalar_kind_t kind,
                                          size_t k, size_t ef, bool streaming, usearch_label_t *labels, float *distances, usearch_error_t *e)
try {
    CLEAR(e);
    if(!c) { FAIL(e, "lantern_gpu: null cursor"); return 0; }
    const Filter *f = FF(filter, e);
    if(!f) return 0;
    Index *ix = H(c->ix, e);
    if(!ix) return 0;
    if(!kind_accepted(ix, (int)kind)) { FAIL(e, "lantern_gpu: scalar kind of the query does not match the index"); return 0; }
    if(k == 0) return 0;
    if(!query || !labels || !distances) { FAIL(e, "lantern_gpu: null query or result pointer"); return 0; }
    std::lock_guard<std::mutex> g(ix->mu);
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return 0; }
    ix->err.clear();
    const size_t out = cursor_search_filtered_locked(ix, f, &c->cur, query, (int)kind, k, ef, streaming, labels, distances);
    if(!ix->err.empty()) FAIL(e, ix->err.c_str());
    return out;
}
LANTERN_ABI_CATCH(e)

// ---- a filter per query, uniform (k, ef, skip) -----------------------------------------------------------------------------------------
// the filter check and the launch of the host forms, of either host trip (the tables go into the staging block's extra area)
static auto each_validate(const lantern_gpu_filter_t *const *filters, size_t nq)
{
    return [ = ](Index *ix) { return each_filters_ok(ix, (const Filter *const *)filters, nq); };
}
static auto each_launch(Index *ix, const lantern_gpu_filter_t *const *filters, size_t nq, size_t k, size_t ef, bool dense_call)
{
    return [ = ](const HostBatch &b) {
        return filtered_each_locked(ix, (const Filter *const *)filters, (const uint4 *)b.d_q, nq, k, ef, 0, b.out(b.d_out), b.stream, b.h_extra(), dense_call);
    };
}

void lantern_gpu_search_batch_filtered_each_device(usearch_index_t h, const lantern_gpu_filter_t *const *filters, const void *d_queries,
                                                   size_t query_stride_bytes, size_t nq, size_t k, size_t ef, size_t skip, uint64_t *d_labels,
                                                   float *d_distances, uint32_t *d_slots, uint32_t *d_counts, uint64_t *d_D, uint64_t *d_E,
                                                   void *stream, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = each_head(h, filters, nq, nullptr, 0, false, -1, e);
    if(!ix) return;
    const SearchOut out{ d_labels, d_distances, d_slots, d_counts, d_D, d_E };
    device_trip(ix, stride_is(query_stride_bytes), [ & ] {
        return filtered_each_locked(ix, (const Filter *const *)filters, (const uint4 *)d_queries, nq, k, ef, skip, out, (hipStream_t)stream, nullptr, true);
    }, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_search_batch_filtered_each(usearch_index_t h, const lantern_gpu_filter_t *const *filters, const void *queries, size_t nq,
                                            usearch_scalar_kind_t kind, size_t k, size_t ef, usearch_label_t *labels, float *distances,
                                            uint32_t *counts, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = each_head(h, filters, nq, nullptr, 0, false, (int)kind, e);
    if(!ix) return;
    if(nq && k && (!queries || !labels || !distances)) { FAIL(e, "lantern_gpu: null query or result pointer"); return; }
    host_trip_sync(ix, nq, k, each_table_bytes(nq), queries, (int)kind, kFilteredBatchFailed, each_validate(filters, nq),
                   each_launch(ix, filters, nq, k, ef, true), labels, distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

// lantern_gpu_search_batch_lane with a filter per query: the lane trip, the selection lists and descriptor table in the block's extra area
void lantern_gpu_search_batch_filtered_each_lane(usearch_index_t h, int lane, const lantern_gpu_filter_t *const *filters, const void *queries,
                                                 size_t nq, usearch_scalar_kind_t kind, size_t k, size_t ef, usearch_label_t *labels,
                                                 float *distances, uint32_t *counts, usearch_error_t *e)
try {
    CLEAR(e);
    if(!lane_ok(lane, e)) return;
    Index *ix = each_head(h, filters, nq, nullptr, 0, false, (int)kind, e);
    if(!ix) return;
    if(nq && k && (!queries || !labels || !distances)) { FAIL(e, "lantern_gpu: null buffer"); return; }
    host_trip_lane(ix, lane, nq, k, each_table_bytes(nq), queries, (int)kind, kFilteredBatchFailed, each_validate(filters, nq),
                   each_launch(ix, filters, nq, k, ef, false), labels, distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

// ---- a filter and (k, ef, skip) per query (include/lantern_gpu.h has the contract and the order of the refusals) -----------------------
// refusals 3 to 6 of the host forms, of either host trip: the filters, then the plan, which the launch of the same trip reads
struct EachParamsValidate
{
    static constexpr bool              zero_width_rows = true;  // (host_trip.hpp: k_stride == 0 is a batch of k_i == 0, whose counts are written)
    const lantern_gpu_filter_t *const *filters;
    const lantern_gpu_query_params    *params;
    size_t                             nq;
    FilteredCallPlan                  *plan;
    bool operator()(Index *ix) const { return each_params_plan_locked(ix, (const Filter *const *)filters, params, nq, *plan); }
};
static auto each_params_launch(Index *ix, const FilteredCallPlan *plan, const lantern_gpu_filter_t *const *filters, size_t nq, size_t k_stride)
{
    return [ = ](const HostBatch &b) {
        return filtered_each_params_locked(ix, *plan, (const Filter *const *)filters, (const uint4 *)b.d_q, nq, k_stride, b.out(b.d_out), b.stream, b.h_extra());
    };
}

void lantern_gpu_search_batch_filtered_each_params_device(usearch_index_t h, const lantern_gpu_filter_t *const *filters, const void *d_queries,
                                                          size_t query_stride_bytes, size_t nq, const lantern_gpu_query_params *params,
                                                          size_t k_stride, uint64_t *d_labels, float *d_distances, uint32_t *d_slots,
                                                          uint32_t *d_counts, uint64_t *d_D, uint64_t *d_E, void *stream, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = each_head(h, filters, nq, params, k_stride, true, -1, e);
    if(!ix) return;
    const SearchOut out{ d_labels, d_distances, d_slots, d_counts, d_D, d_E };
    device_trip(ix, stride_is(query_stride_bytes), [ & ] {
        FilteredCallPlan plan;
        return each_params_plan_locked(ix, (const Filter *const *)filters, params, nq, plan) &&
               filtered_each_params_locked(ix, plan, (const Filter *const *)filters, (const uint4 *)d_queries, nq, k_stride, out, (hipStream_t)stream, nullptr);
    }, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_search_batch_filtered_each_params(usearch_index_t h, const lantern_gpu_filter_t *const *filters, const void *queries, size_t nq,
                                                   usearch_scalar_kind_t kind, const lantern_gpu_query_params *params, size_t k_stride,
                                                   usearch_label_t *labels, float *distances, uint32_t *counts, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = each_head(h, filters, nq, params, k_stride, true, (int)kind, e);
    if(!ix) return;
    if(nq && (!queries || (k_stride && (!labels || !distances)))) { FAIL(e, "lantern_gpu: null query or result pointer"); return; }
    FilteredCallPlan plan;
    host_trip_sync(ix, nq, k_stride, each_table_bytes(nq, true), queries, (int)kind, kFilteredBatchFailed, EachParamsValidate{ filters, params, nq, &plan },
                   each_params_launch(ix, &plan, filters, nq, k_stride), labels, distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_search_batch_filtered_each_params_lane(usearch_index_t h, int lane, const lantern_gpu_filter_t *const *filters, const void *queries,
                                                        size_t nq, usearch_scalar_kind_t kind, const lantern_gpu_query_params *params, size_t k_stride,
                                                        usearch_label_t *labels, float *distances, uint32_t *counts, usearch_error_t *e)
try {
    CLEAR(e);
    if(!lane_ok(lane, e)) return;
    Index *ix = each_head(h, filters, nq, params, k_stride, true, (int)kind, e);
    if(!ix) return;
    if(nq && (!queries || (k_stride && (!labels || !distances)))) { FAIL(e, "lantern_gpu: null buffer"); return; }
    FilteredCallPlan plan;
    host_trip_lane(ix, lane, nq, k_stride, each_table_bytes(nq, true), queries, (int)kind, kFilteredBatchFailed,
                   EachParamsValidate{ filters, params, nq, &plan }, each_params_launch(ix, &plan, filters, nq, k_stride), labels, distances, counts, e);
}
LANTERN_ABI_CATCH_VOID(e)

}  // extern "C"
