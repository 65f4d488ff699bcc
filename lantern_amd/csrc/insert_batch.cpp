// insert_batch.cpp -- one insertion batch: plan_insert decides the shape of its k_insert launch (pure: lantern_gpu_plan_insert shows it
// without a device), run_batch queues the batch -- walk, selection, grouping, reverse links, and in a sharded build the exchanges
// between them -- with the build-profile marks around its phases.  The insertion counterpart of search_plan.cpp; what decides WHICH
// rows form a batch, stages them and drives the sharded builds stays in index.cpp.
#include "index.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "comm.hpp"

namespace lgpu {

// The environment switches of a batch, as values.  LANTERN_GPU_INSERT_SPEC (=0: no lone-insertion walk) and LANTERN_GPU_GROUP_ALL
// are read ONCE PER PROCESS, at the first batch: a test that wants another value starts a process of its own
// (tests/visited_undo_probe.py).  LANTERN_GPU_INSERT_VIS_SLOTS (the LDS visited set's size, for tuning), LANTERN_GPU_REPRUNE_STATE
// and LANTERN_GPU_DEBUG_GROUPS are read ON EVERY BATCH: in-process tests set them between calls (tests/test_gpu_visited_regimes.py).
InsertEnv insert_env()
{
    static const bool spec = !(std::getenv("LANTERN_GPU_INSERT_SPEC") && std::atoi(std::getenv("LANTERN_GPU_INSERT_SPEC")) == 0);
    static const bool group_all = std::getenv("LANTERN_GPU_GROUP_ALL") && std::atoi(std::getenv("LANTERN_GPU_GROUP_ALL")) != 0;
    InsertEnv e;
    e.spec = spec, e.group_all = group_all;
    if(const char *vs = std::getenv("LANTERN_GPU_INSERT_VIS_SLOTS")) e.vis_slots = std::max(0, std::atoi(vs));
    if(const char *rs = std::getenv("LANTERN_GPU_REPRUNE_STATE")) e.reprune_state = std::atoi(rs) != 0;
    e.debug_groups = std::getenv("LANTERN_GPU_DEBUG_GROUPS") != nullptr;
    return e;
}

// ---- build profile: HIP events around the phases of every batch, resolved lazily (never a wait on fresh work) -----
static const int kProfMarks = 6;  // start | walk | connect | exchange 1 + grouping | reverse links | exchange 2
static hipEvent_t prof_event(Index *ix)
{
    if(!ix->prof_free.empty()) {
        hipEvent_t e = ix->prof_free.back();
        ix->prof_free.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if(hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}
static void prof_mark(Index *ix, int which)
{
    if(!ix->profiling) return;
    if(which == 0) ix->prof_pending.emplace_back();
    hipEvent_t e = prof_event(ix);
    ix->prof_pending.back().ev[ which ] = e;
    if(e) (void)hipEventRecord(e, ix->stream);
}
void prof_resolve(Index *ix, size_t keep)
{
    while(ix->prof_pending.size() > keep) {
        Index::ProfBatch &pb = ix->prof_pending.front();
        bool ok = true;
        for(int i = 0; i < kProfMarks; ++i) ok = ok && pb.ev[ i ] != nullptr;
        if(ok && hipEventSynchronize(pb.ev[ kProfMarks - 1 ]) == hipSuccess) {
            float ms[ kProfMarks - 1 ] = {};
            for(int i = 0; i + 1 < kProfMarks; ++i) (void)hipEventElapsedTime(&ms[ i ], pb.ev[ i ], pb.ev[ i + 1 ]);
            ix->prof.walk_ms += ms[ 0 ];
            ix->prof.connect_ms += ms[ 1 ];
            ix->prof.group_ms += ms[ 2 ];
            ix->prof.revlink_ms += ms[ 3 ];
            ix->prof.exchange_ms += ms[ 4 ];
            ix->prof.batches += 1;
        }
        for(int i = 0; i < kProfMarks; ++i)
            if(pb.ev[ i ]) ix->prof_free.push_back(pb.ev[ i ]);
        ix->prof_pending.pop_front();
    }
}

// The initial mode of Index::insert_screen where LANTERN_GPU_INSERT_SCREEN does not say.  On: the same-box A/B of DESIGN.md 4.4
// (profiles/insert_screen_build_ab.json) -- Gaussian 1M x 768 builds at 894 k vectors/s against 580 k, clustered at the same speed.
const bool kInsertScreenByDefault = true;

// The shape of a batch's k_insert launch (run_batch below; lantern_gpu_plan_insert shows it without a device).
// Lone walk: a handful of insertions -- ldb_aminsert's one row, the first batches of a build -- walk alone on their CUs: level 0 by the
// lone-query walk (insert_spec_kernel.hip), up to two insertions per CU one after the other.
// Screened: level 0 tests its candidates on the int8 row copy first (insert_kernel.hip k_insert<.., SCREEN = true>) iff the index's mode
// is on, it has the table, the rows are f32 l2sq / cosine of >= 128 chunks, the list lives in registers (efc <= 128, no LDS list), the
// walk is split over two or more waves, has a level 0 and is not the lone walk.  The query's int8 planes then come out of vis_slots.
InsertPlan plan_insert(const InsertPlanIn &in)
{
    InsertPlan p;
    p.lone = in.lone_ok && in.rows <= (size_t)in.num_cus * 2 && insert_spec_supported(in.mcode, in.efc, in.M0) && !in.lds_list;
    p.screened = in.mode == 1 && in.screen_table && (in.mcode == M_L2SQ || in.mcode == M_COS) && screen_rows_for(in.chunks) && in.efc <= 128 &&
                 !in.lds_list && !p.lone && !in.only_upper && in.waves >= 2;
    p.screen_lds = p.screened ? screen_query_lds_bytes(in.chunks) : 0;
    // LDS visited set for the ef_construction-wide walk (spills to the bitmap when 3/4 full); env override for tuning
    // the largest table that still lets FIVE workgroups share a CU (160 KB / 5, minus the walk's lists): 6400 slots at
    // 768-d / efc 128, enough for the ~3700 nodes such a walk visits at the 3/4 load limit
    uint32_t ivis = 8192;
    if(in.vis_slots_env >= 0) ivis = (uint32_t)in.vis_slots_env / 4 * 4;
    const int G_ = group_lanes_for(in.chunks), LW_ = G_ >= 32 ? 1 : G_ == 16 ? 2 : 4;  // list words a lane of a row's group fetches
    p.spec_prefetch = p.lone && in.M0 % (uint32_t)LW_ == 0 && in.M0 <= (uint32_t)(G_ * LW_) ? 1u : 0u;
    p.spec_cache = p.spec_prefetch ? 128u : 0u;
    auto ins_lds = [&](uint32_t vis) {
        return (p.lone ? insert_spec_lds_bytes(in.chunks, in.efc, in.M0, vis, p.spec_prefetch, p.spec_cache) : insert_lds_bytes(in.chunks, in.efc, in.M0, vis)) + p.screen_lds;
    };
    while(ivis && ins_lds(ivis) > (p.lone ? 96u : 31u) * 1024) ivis = ivis > 256 ? ivis - 256 : 0;  // (one workgroup per CU in the lone-walk shape)
    if(ivis && ivis < 4 * in.M0) ivis = 0;
    p.vis_slots = ivis;
    p.lds = ins_lds(ivis);
    if(p.lds > 160 * 1024) p.refusal = "lantern_gpu: ef_construction/dimensions exceed the 160 KiB LDS budget";
    return p;
}

// Row-sharded build (index.cpp add_row_sharded_locked, step 2): a batch's level-0 candidates from the shards' graphs
static bool row_shard_candidates(Index *ix, const RowShard &rs, size_t first, size_t b, const uint32_t *d_link_off, uint64_t *d_tops, uint32_t *d_top_count)
{
    Index       *loc = rs.loc;
    Comm        *comm = rs.comm;
    const int    W = comm->world, R = comm->rank;
    const size_t K = rs.K, part = b * K, row = (size_t)ix->chunks * 16;
    char *d_all = (char *)scratch(ix, kScratchShardParts, (size_t)W * part * 12 + 64);  // [W][b][K] labels | [W][b][K] distances
    if(!d_all) return false;
    uint64_t *g_lab = (uint64_t *)d_all;
    float    *g_dist = (float *)(d_all + (size_t)W * part * 8);
    bool ok = true;
    if(loc->n == 0) {
        std::vector<float> inf(part, __builtin_inff());
        ok = hipMemsetAsync(g_lab + (size_t)R * part, 0, part * 8, ix->stream) == hipSuccess &&
             hipMemcpyAsync(g_dist + (size_t)R * part, inf.data(), part * 4, hipMemcpyHostToDevice, ix->stream) == hipSuccess &&
             hipStreamSynchronize(ix->stream) == hipSuccess;  // `inf` is a local
    } else {
        std::lock_guard<std::mutex> gl(loc->mu);
        ok = run_search_device(loc, (const uint4 *)((const char *)ix->d_vec + first * row), b, K, rs.ef, 0,
                               SearchOut{ g_lab + (size_t)R * part, g_dist + (size_t)R * part, nullptr, nullptr, nullptr, nullptr }, ix->stream, loc->search_waves);
        if(!ok) set_err(ix, "lantern_gpu: row-sharded build, candidate search: " + loc->err);
    }
    if(ok && W > 1) {
        std::vector<size_t> off((size_t)W), cnt((size_t)W);
        for(int r = 0; r < W; ++r) { off[ (size_t)r ] = (size_t)r * part * 8; cnt[ (size_t)r ] = part * 8; }
        ok = comm->allgatherv_device(g_lab, off.data(), cnt.data(), ix->stream);
        for(int r = 0; r < W; ++r) { off[ (size_t)r ] = (size_t)r * part * 4; cnt[ (size_t)r ] = part * 4; }
        ok = ok && comm->allgatherv_device(g_dist, off.data(), cnt.data(), ix->stream);
        if(!ok) set_err(ix, "lantern_gpu: row-sharded build, exchange of the candidate lists: " + comm->err);
    }
    ok = ok && launch_merge_candidates(g_lab, g_dist, (uint32_t)W, (uint32_t)b, (uint32_t)K, (uint32_t)first, d_link_off, ix->M, ix->efc, d_tops, d_top_count,
                                       ix->stream) == hipSuccess;
    if(!ok && ix->err.empty()) set_err(ix, "lantern_gpu: HIP failure during the row-sharded build");
    return ok;
}

// Work-sharded build (comm != nullptr): the batch is the same as on one GPU, but every rank
// walks and connects only its share [b_lo, b_hi) of the new nodes, the ranks all-gather the resulting top-M
// neighbour lists (= the reverse-link requests: 16 bytes per pick), each rank applies the reverse links of the
// nodes it owns (close % world), and the re-written adjacency rows are all-gathered.  Every step is
// deterministic and independent of who executes it, so all replicas end up bit-identical to the graph one GPU
// builds with the same batch plan.  Batches with fewer than kShardMinPerRank vectors per rank (the ramp at the
// start of a build) are executed redundantly by every rank: no exchange, same result.
static const size_t kShardMinPerRank = 8;

bool run_batch(Index *ix, size_t b, const int *lv, Comm *comm, const RowShard *rs)
{
    const size_t first = ix->n;
    const int    W = comm ? comm->world : 1, R = comm ? comm->rank : 0;
    const bool   split = W > 1 && b >= (size_t)W * kShardMinPerRank;
    const size_t b_lo = split ? b * (size_t)R / (size_t)W : 0, b_hi = split ? b * ((size_t)R + 1) / (size_t)W : b;
    std::vector<uint32_t> &link_off = ix->h_link_off;  // host copy: sizes the exchanges and the launches (never uploaded)
    link_off.resize(b);
    size_t total_links = 0;
    for(size_t i = 0; i < b; ++i) {
        link_off[ i ] = (uint32_t)total_links;
        total_links += (size_t)ix->M * (size_t)(lv[ i ] + 1);
    }
    // one "item" per (new node, level): the walk result the selection kernel works on
    const size_t items = total_links / ix->M;
    uint32_t *d_link_off = (uint32_t *)scratch(ix, kScratchLinkOff, b * 4 + items * 4 + items * 4);
    LinkReq  *d_links = (LinkReq *)scratch(ix, kScratchLinks, total_links * sizeof(LinkReq));
    uint64_t *d_tops = (uint64_t *)scratch(ix, kScratchTops, items * (size_t)ix->efc * 8);
    LinkReq  *d_reqs = (LinkReq *)scratch(ix, kScratchReqs, total_links * sizeof(LinkReq));
    // groups | ngroups | owner counts
    char     *d_grp = (char *)scratch(ix, kScratchGroups, total_links * sizeof(uint2) + 16 + (size_t)W * 4);
    void     *d_work = scratch(ix, kScratchWork, total_links * 8 + 16);
    const size_t temp_bytes = group_temp_bytes(total_links);
    char     *d_sort = (char *)scratch(ix, kScratchSort, total_links * 24 + temp_bytes + 64);
    if(!d_link_off || !d_links || !d_tops || !d_reqs || !d_grp || !d_work || !d_sort) return false;
    uint32_t *d_item_node = d_link_off + b, *d_top_count = d_item_node + items;
    uint2    *d_groups = (uint2 *)d_grp;
    uint32_t *d_ngroups = (uint32_t *)(d_grp + total_links * sizeof(uint2));
    uint32_t *d_owner = d_ngroups + 4;
    GroupScratch gs;
    gs.keys_a = (uint64_t *)d_sort;
    gs.keys_b = gs.keys_a + total_links;
    gs.idx_a = (uint32_t *)(gs.keys_b + total_links);
    gs.idx_b = gs.idx_a + total_links;
    gs.temp = (void *)(((uintptr_t)(gs.idx_b + total_links) + 63) & ~(uintptr_t)63);
    gs.temp_bytes = temp_bytes;

    prof_mark(ix, 0);
    HIPCHK(ix, launch_batch_layout(ix->d_levels + first, (uint32_t)b, ix->M, d_link_off, d_item_node, ix->stream));

    // the launch's shape: plan_insert (above).  The batch's switches as values (insert_env, above: which is read when)
    const InsertEnv env = insert_env();
    InsertPlanIn pin;
    pin.mcode = ix->mcode, pin.num_cus = ix->num_cus, pin.waves = ix->insert_waves;
    pin.chunks = ix->chunks, pin.M0 = ix->M0, pin.efc = ix->efc;
    pin.rows = b_hi - b_lo;
    pin.screen_table = ix->d_screen && ix->d_screen_meta;
    pin.mode = ix->insert_screen;
    pin.lds_list = search_env().lds_list;
    pin.only_upper = rs != nullptr;
    pin.lone_ok = env.spec && !comm && !rs;
    pin.vis_slots_env = env.vis_slots;
    const InsertPlan ip = plan_insert(pin);
    if(ip.refusal) { set_err(ix, ip.refusal); return false; }
    const bool ins_spec = ip.lone;
    const int  ins_waves = ins_spec ? 11 : ix->insert_waves;
    const int  grid = ins_spec ? (int)std::max<size_t>(1, std::min<size_t>(b_hi - b_lo, (size_t)ix->num_cus)) : search_grid(ix, b_hi - b_lo, ix->insert_waves, 20);
    if(!ensure_bitmaps(ix, (size_t)grid)) return false;
    if(!order_launch(ix, ix->stream)) return false;  // a search may still be running on a caller's stream
    auto link_at = [&](size_t i) { return i < b ? (size_t)link_off[ i ] : total_links; };

    InsertArgs ia;
    ia.view = ix->view();  // size/entry/max_level as they were BEFORE the batch
    if(!ip.screened) ia.view.screen = nullptr, ia.view.screen_meta = nullptr, ia.view.screen_chunks = 0;  // no planes' block: the launch does not screen
    ia.first_slot = (uint32_t)first;
    ia.b_begin = (uint32_t)b_lo;
    ia.count = (uint32_t)b_hi;
    ia.efc = ix->efc;
    ia.link_off = d_link_off;
    ia.tops = d_tops;
    ia.top_count = d_top_count;
    ia.bitmaps = ix->d_bitmaps;
    ia.bm_words = (uint32_t)ix->bm_words;
    ia.undo_cap = vis_undo_cap();
    ia.lds_list = pin.lds_list;
    ia.only_upper = rs ? 1u : 0u;
    ia.spec_prefetch = ip.spec_prefetch;
    ia.spec_cache = ip.spec_cache;
    ia.vis_slots = ip.vis_slots;
    ia.totals = ix->d_totals + kTotInsert;  // (a screened launch: and [kInsertScreenTotals..+1] from there)
    ia.ticket = next_ticket(ix, b_hi - b_lo, grid, ix->stream);
    if(ins_spec) HIPCHK(ix, launch_insert_spec(ix->mcode, ia, ins_waves, grid, ix->stream));
    else {
        HIPCHK(ix, launch_insert(ix->mcode, ia, ix->insert_waves, grid, ix->stream));
        (ip.screened ? ix->insert_launches_screened : ix->insert_launches_plain) += 1;
    }
    if(rs && !row_shard_candidates(ix, *rs, first, b, d_link_off, d_tops, d_top_count)) return false;  // level 0: from the shards' graphs
    prof_mark(ix, 1);

    ConnectArgs ca;
    ca.view = ia.view;
    ca.first_slot = (uint32_t)first;
    ca.item_begin = (uint32_t)(link_at(b_lo) / ix->M);
    ca.items = (uint32_t)((link_at(b_hi) - link_at(b_lo)) / ix->M);
    ca.efc = ix->efc;
    ca.link_off = d_link_off;
    ca.item_node = d_item_node;
    ca.tops = d_tops;
    ca.top_count = d_top_count;
    ca.links = d_links;
    ca.totals = ix->d_totals + kTotConnect;
    HIPCHK(ix, launch_connect(ix->mcode, ca, ix->stream));
    prof_mark(ix, 2);

    if(split) {
        // exchange 1: the ranks' top-M neighbour lists (one LinkReq per pick).  Afterwards every rank holds all
        // requests of the batch; the own lists of the nodes a peer connected are rebuilt from them.
        std::vector<size_t> off((size_t)W), cnt((size_t)W);
        for(int r = 0; r < W; ++r) {
            const size_t lo = b * (size_t)r / (size_t)W, hi = b * ((size_t)r + 1) / (size_t)W;
            off[ (size_t)r ] = link_at(lo) * sizeof(LinkReq);
            cnt[ (size_t)r ] = (link_at(hi) - link_at(lo)) * sizeof(LinkReq);
        }
        if(!comm->allgatherv_device(d_links, off.data(), cnt.data(), ix->stream)) { set_err(ix, comm->err); return false; }
        HIPCHK(ix, launch_apply_own_links(ia.view, (uint32_t)first, d_link_off, d_links, (uint32_t)total_links, ix->stream));
    }

    // reverse links: group by (close, level); within a group apply in new-slot order -- on the device (grouping.hip).
    // In a sharded batch a rank keeps only the groups of the nodes it owns (close % world) and counts the others'
    // (the sizes of the second exchange's segments must be known to every rank's HOST: the one value read back).
    // (the pass also zeroes the reverse-link kernels' work counter, d_work[0]: one node less on the stream)
    std::vector<uint32_t> owner_reqs((size_t)W, 0);
    // A sharded batch sorts and gathers only the requests THIS rank owns (1 / W of them: DESIGN.md 6): their keys are appended while
    // the owners are counted, the counts come back in the batch's one host wait, and the sort runs on owner_reqs[R] keys.
    // (LANTERN_GPU_GROUP_ALL=1: the replicated pass over every request, kept for A/B runs; positions need 24 bits.)
    const bool owned_only = split && !env.group_all && total_links < (1u << 24);
    if(owned_only) HIPCHK(ix, launch_group_keys_owned(d_links, (uint32_t)total_links, gs, d_ngroups, W, R, d_owner, ix->stream, (uint32_t *)d_work));
    else HIPCHK(ix, launch_group_requests(d_links, (uint32_t)total_links, gs, d_reqs, d_groups, d_ngroups, split ? W : 1, R, d_owner, ix->stream, (uint32_t *)d_work));
    if(split) {
        HIPCHK(ix, hipMemcpyAsync(owner_reqs.data(), d_owner, (size_t)W * 4, hipMemcpyDeviceToHost, ix->stream));
        if(!sync_stream(ix, comm)) return false;
        if(owned_only) HIPCHK(ix, launch_group_sort_owned(d_links, owner_reqs[ (size_t)R ], gs, d_reqs, d_groups, d_ngroups, ix->stream));
    }
    prof_mark(ix, 3);
    if(env.debug_groups) {  // debugging aid: the size distribution of this batch's groups
        HIPCHK(ix, hipStreamSynchronize(ix->stream));
        uint32_t ng = 0;
        HIPCHK(ix, hipMemcpy(&ng, d_ngroups, 4, hipMemcpyDeviceToHost));
        std::vector<uint2> hg(ng);
        if(ng) HIPCHK(ix, hipMemcpy(hg.data(), d_groups, (size_t)ng * 8, hipMemcpyDeviceToHost));
        uint32_t mx = 0, over[ 5 ] = {};
        uint64_t sum = 0;
        for(const uint2 &g2 : hg) {
            const uint32_t sz = g2.y - g2.x;
            mx = std::max(mx, sz);
            sum += sz;
            over[ 0 ] += sz > 8;
            over[ 1 ] += sz > 32;
            over[ 2 ] += sz > 128;
            over[ 3 ] += sz > 512;
            over[ 4 ] += sz > 2048;
        }
        std::fprintf(stderr, "batch first=%zu b=%zu groups=%u reqs=%llu max=%u >8:%u >32:%u >128:%u >512:%u >2048:%u\n", first, b, ng,
                     (unsigned long long)sum, mx, over[ 0 ], over[ 1 ], over[ 2 ], over[ 3 ], over[ 4 ]);
    }
    RevlinkArgs ra;
    ra.view = ix->view();
    ra.ngroups = d_ngroups;
    ra.groups = d_groups;
    ra.max_groups = split ? owner_reqs[ (size_t)R ] : (uint32_t)total_links;
    ra.reqs = d_reqs;
    ra.totals = ix->d_totals + kTotRevlink;
    // the persistent re-prune state is kept by one-GPU builds (a work-sharded build overwrites other ranks' rows wholesale);
    // whatever changes lists without maintaining it (a sharded batch, an imported graph, the switch below) marks it stale
    const bool use_state = !split && env.reprune_state;  // LANTERN_GPU_REPRUNE_STATE=0: every full list takes the all-pairs path (A/B, tests)
    if(!use_state) {
        ix->radius_stale = true;
    } else if(ix->radius_stale) {
        if(ix->d_radius0) HIPCHK(ix, hipMemsetAsync(ix->d_radius0, 0xFF, ix->cap * 4, ix->stream));
        if(ix->d_radius_upper) HIPCHK(ix, hipMemsetAsync(ix->d_radius_upper, 0xFF, ix->upper_cap * 4, ix->stream));
        ix->radius_stale = false;
    }
    ra.radius0 = use_state ? ix->d_radius0 : nullptr;
    ra.radius_upper = use_state ? ix->d_radius_upper : nullptr;
    HIPCHK(ix, launch_revlink(ix->mcode, ra, (char *)d_work + 16, (uint32_t *)d_work, ix->num_cus, ix->stream, true));
    prof_mark(ix, 4);
    if(split) {
        // exchange 2: the adjacency rows the ranks re-wrote, one record [close, level, list[0..M0)] per group.
        // A rank's segment is sized by the number of requests it owned (>= its number of groups; every rank can
        // compute it from the request array) and padded with EMPTY records.
        const size_t rec_bytes = ((size_t)ix->M0 + 2) * 4;
        std::vector<size_t> off((size_t)W), cnt((size_t)W);
        size_t total_recs = 0;
        for(int r = 0; r < W; ++r) {
            off[ (size_t)r ] = total_recs * rec_bytes;
            cnt[ (size_t)r ] = owner_reqs[ (size_t)r ] * rec_bytes;
            total_recs += owner_reqs[ (size_t)r ];
        }
        if(total_recs) {
            char *d_rec = (char *)scratch(ix, kScratchCallIn, total_recs * rec_bytes);
            if(!d_rec) return false;
            if(cnt[ (size_t)R ]) HIPCHK(ix, hipMemsetAsync(d_rec + off[ (size_t)R ], 0xFF, cnt[ (size_t)R ], ix->stream));
            HIPCHK(ix, launch_pack_lists(ra, (uint32_t *)(d_rec + off[ (size_t)R ]), ix->stream));
            if(!comm->allgatherv_device(d_rec, off.data(), cnt.data(), ix->stream)) { set_err(ix, comm->err); return false; }
            HIPCHK(ix, launch_apply_lists(ra.view, (const uint32_t *)d_rec, (uint32_t)total_recs, ix->stream));
        }
        // the host transport's staging buffers are reused by the next batch: it waits here.  RCCL works in place in HBM on the
        // index stream: the next batch queues behind this one, and the one wait per batch that is left (the owner counts that
        // size exchange 2, above) is where a stuck collective meets its deadline
        if(!comm->rccl && !sync_stream(ix, comm)) return false;
    }
    prof_mark(ix, 5);
    // behind the LAST kernel that rewrites lists: a search on another stream that waits for `insert_done` sees the whole batch
    if(!record_launch(ix, ix->stream)) return false;
    if(ix->profiling) prof_resolve(ix, 192);  // only batches the device finished long ago are waited for
    ix->n = first + b;
    if(b == 1 && lv[ 0 ] > ix->max_level) {  // "Updating the entry point if needed"
        ix->entry = (uint32_t)first;
        ix->max_level = lv[ 0 ];
    }
    ix->c_add_vectors += b;
    ix->c_add_batches += 1;
    return true;
}

}  // namespace lgpu
