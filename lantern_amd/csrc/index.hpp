// index.hpp -- the device-resident HNSW index behind the usearch-shaped C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <functional>
#include <vector>

#include "../../include/lantern_gpu.h"
#include "kernels.hpp"

namespace lgpu {

// what one scan has been handed so far (device slots): a continuation searches for |seen| + k results and returns the
// first k that were not returned before, so a scan never sees a row twice even though a wider search may rank the
// earlier rows differently
struct Cursor
{
    std::unordered_set<uint32_t> seen;
    uint64_t                     epoch = 0;  // Index::epoch when `seen` was started: slots of another epoch name other rows (cursor_epoch_ok)
};

constexpr int kIndexLanes = 8;  // Index::kLanes, Index::kSearchSlots

// ---- the device scratch buffers (Index::d_scratch) by name ---------------------------------------------------------------------
enum ScratchSlot : int
{
    // an insert batch (flush_locked)
    kScratchLinkOff,
    kScratchLinks,
    kScratchReqs,
    kScratchGroups,
    kScratchWork,
    kScratchTops,
    kScratchSort,
    kScratchShardParts,  // the sharded build's gathered candidate lists
    // The input and the output of ONE CALL on the index stream (the host forms of every batched, cursor, exact and partitioned search,
    // the distance gather, the sharded insert's list records).  Shared safely: every user queues its work under ix->mu and on the
    // index stream, which runs one call's work after the other's.
    kScratchCallIn,
    kScratchCallOut,
    // the filtered exact path's dense route: the re-ranked (slot, distance) rows and the certificate's flags of one call, which has
    // waited for its stream when it returns (under ix->mu): nothing queued reads the block when the next call takes it.  A
    // per-query-filter call's dense groups keep their concatenated slot list, tables and gathered queries here too: everything that
    // reads them is queued in front of that call's one wait
    kScratchDenseAnswers,
    kScratchLanes,                                     // 2 per lane: queries, answers (lantern_gpu_search_batch_lane*)
    kScratchTables = kScratchLanes + 2 * kIndexLanes,  // 1 per launch slot: a per-query filtered launch's selection list + descriptors
    kScratchCount = kScratchTables + kIndexLanes
};
inline int lane_query_scratch(int lane) { return kScratchLanes + 2 * lane; }
inline int lane_answer_scratch(int lane) { return kScratchLanes + 2 * lane + 1; }
inline int launch_table_scratch(int launch_slot) { return kScratchTables + launch_slot; }

constexpr uint64_t kIndexMagic = 0x4C414E5445524E31ull;  // "LANTERN1": the first word of every live index handle

struct Index
{
    uint64_t magic = kIndexMagic;  // checked by every entry point (abi_guard.hpp H()): a stale, freed or foreign pointer handed over as a
                                   // usearch_index_t is refused with an error string instead of being dereferenced as an index
    // ---- configuration (usearch_init_options_t as Lantern fills it) -------------------------------
    usearch_init_options_t opts{};
    int      metric = 0;         // usearch_metric_kind_t
    int      mcode = 0;          // kernel metric code: metric, +100 for f16 storage (device_common.hpp)
    int      scalar = 0;         // STORAGE kind: usearch_scalar_f32_k, _f16_k (quant_bits=16) or _b1_k
    uint32_t words = 0;          // 4-byte words per vector as the caller supplies it
    uint32_t chunks = 0;         // 16-byte chunks per stored row (zero padded)
    uint32_t natural_chunks = 0; // the vector's own length in 16-byte chunks; < chunks where rows are stored at a widened stride (bit rows of 65 .. 127 bytes)
    uint32_t M = 16, M0 = 32, efc = 128, ef = 64;
    uint64_t seed = 42;
    size_t   add_batch_max = 8192, add_min_ratio = 16;
    int      search_waves = 0 /* automatic */, search_max_wg = 0, insert_waves = 4;
    int      search_vis_slots = -1;  // -1 = automatic size of the LDS visited set, 0 = HBM bitmap only

    // ---- quantised views of f32 input ----------------------------------------------------------------------------
    // quant_bits = 1 on real[] (options.c:154-155, test/sql/hnsw_sq.sql "binary > 0 quantization"): an l2sq index whose
    // rows are one bit per dimension, bit = (x > 0); sum (a - b)^2 over {0, 1} values IS the Hamming distance, so the
    // Hamming kernels run it exactly.  Callers still hand f32 arrays to usearch_add / usearch_search_ef.
    bool     b1_from_f32 = false;
    // pq = true (build.c:497-500, scan.c:75-81): the vector block holds every row's DECODING (concatenated centroids),
    // d_codes its num_subvectors code bytes (what the file / the pages carry: usearch_storage.cpp:29-31)
    bool     pq = false;
    uint32_t pq_S = 0, pq_C = 0, pq_subdim = 0;
    std::vector<float> h_codebook;       // [pq_C][dimensions]: row c = centroid c of every subvector, concatenated (pqtable.c:194-240)
    float   *d_codebook = nullptr;
    float   *d_centers = nullptr;        // [pq_S][pq_C][sub_floats]: the per-subvector centroid tables, rows zero padded to chunks
    uint8_t *d_codes = nullptr;          // [cap][pq_S]
    // COMPACT form of a pq index (lantern_gpu_pq_compact): the decodings are gone from HBM (d_vec == NULL) and searches run
    // ADC over the code rows (search_adc_kernel.hip); whatever needs rows again -- an insert, the exact search -- decodes
    // them back first (pq_expand_locked)
    bool     pq_compact = false;
    uint8_t *d_codes16 = nullptr;        // [n][pq_S16]: the code rows zero padded to whole 16-byte chunks
    uint32_t pq_S16 = 0;
    uint32_t pqd_inv = 0;                // compact form: the checked multiply-shift inverse of chunks-per-subvector (0: decode-on-the-fly not possible -> the ADC table walk)

    // ---- graph state ------------------------------------------------------------------------------
    size_t   n = 0, cap = 0;
    uint32_t entry = EMPTY;
    int      max_level = -1;
    size_t   upper_blocks = 0, upper_cap = 0;
    // bumped by every lantern_gpu_compact_deleted that moved a row: slots mean other rows afterwards, so whatever remembers slots -- a
    // Filter, a Cursor's `seen` -- records the epoch it was made in and is refused in another
    uint64_t epoch = 0;

    // ---- HBM ---------------------------------------------------------------------------------------
    uint4    *d_vec = nullptr;
    float    *d_norm2 = nullptr;  // ||row||^2 per stored row, cosine metrics only (device_common.hpp "cached row norms")
    // the int8 SCREEN copy of every row (f32 l2sq or cosine rows of >= 128 chunks; walk.hpp hop_distances_screened): derived data, filled
    // wherever rows enter d_vec (rows_stored), never serialised.  screen = false (LANTERN_GPU_SCREEN=0, or another kind): not allocated
    bool      screen = false;
    uint4    *d_screen = nullptr;       // [cap][screen_chunks_for(chunks)]
    float2   *d_screen_meta = nullptr;  // [cap] (s, r); a cosine index: (s / norm, rho)
    uint64_t *d_labels = nullptr;
    uint8_t  *d_levels = nullptr;
    uint32_t *d_nbr0 = nullptr;
    uint32_t *d_upper_off = nullptr;
    uint32_t *d_upper_nbr = nullptr;
    float    *d_radius0 = nullptr, *d_radius_upper = nullptr;  // re-prune state per list (kernels.hpp RevlinkArgs::radius0)
    bool      radius_stale = false;  // lists changed without the state being maintained: reset it before the next use
    uint32_t *d_bitmaps = nullptr;
    size_t    bitmap_slots = 0, bm_words = 0;
    uint32_t *d_tickets = nullptr;  // ring of work tickets, one per launch in flight (kernels.hpp SearchArgs::ticket)
    uint32_t  ticket_next = 0;
    bool      use_tickets = true;   // LANTERN_GPU_TICKETS=0: static striding (tuning / debugging)
    unsigned long long *d_totals = nullptr;  // [kTotalsWords] cumulative device counters: the slots are TotalsSlot (kernels.hpp)
    // the int8 screen in the insertion walk (plan_insert below, insert_batch.cpp; lantern_gpu_set_insert_screen): 0 off, 1 on where the launch qualifies
    int      insert_screen = 0;
    uint64_t insert_launches_screened = 0, insert_launches_plain = 0;  // k_insert launches since init (lantern_gpu_insert_screen_stats)

    // scratch (grown on demand): device buffers named by ScratchSlot (below the struct)
    static const int kLanes = kIndexLanes;   // lantern_gpu_search_batch_lane: batches one caller each may keep in flight side by side
    static const int kSearchSlots = kLanes;  // search launches in flight side by side ("launch slots", below)
    void  *d_scratch[ kScratchCount ] = {};
    size_t scratch_bytes[ kScratchCount ] = {};
    hipStream_t lane_stream[ kLanes ] = {};  // created on first use
    char       *lane_host[ kLanes + 1 ] = {};  // page-locked staging of queries and answers: the lanes (one caller each), [kLanes] lantern_gpu_search_batch (under mu)
    size_t      lane_host_bytes[ kLanes + 1 ] = {};

    // ---- host mirrors ------------------------------------------------------------------------------
    std::vector<uint64_t> labels;
    std::vector<uint8_t>  levels;
    std::vector<uint32_t> upper_off;

    // ---- buffered inserts --------------------------------------------------------------------------
    std::mutex            mu;  // add_raw is called from N threads on one index (server.rs:333-356)
    std::vector<uint64_t> pend_labels;
    std::vector<uint32_t> pend_rows;    // chunks*4 words per pending vector, zero padded
    std::vector<int>      pend_levels;  // -1 = draw with level_for()

    // host copy of a batch's layout (sizes the launches and the exchanges; the device derives its own from the levels)
    std::vector<uint32_t> h_link_off;

    // ---- build profile (lantern_gpu_set_profiling): HIP events around the phases of every batch
    struct ProfBatch { hipEvent_t ev[ 6 ] = {}; };
    bool                    profiling = false;
    bool                    phase_profile = false;  // diagnostics: instrumented walk kernel (lantern_gpu_search_phase_profile)
    bool                    spec_profile = false;   // diagnostics: the instrumented latency-bound walk (lantern_gpu_spec_profile)
    uint32_t               *d_touched = nullptr;    // diagnostics: one bit per row evaluated by the instrumented searches (lantern_gpu_search_unique_rows)
    size_t                  touched_words = 0;
    bool                    unique_rows_on = false; // the bitmap is handed to a launch only in this mode, and only while it covers `cap`
    uint32_t               *d_trace = nullptr, *d_trace_count = nullptr;  // diagnostics: [trace_nq][trace_cap] + [trace_nq] (lantern_gpu_search_row_trace)
    size_t                  trace_nq = 0, trace_cap = 0;
    bool                    trace_on = false;
    float                   last_gather_ms = 0.f;   // kernel time of the last lantern_gpu_distance_gather launch (HIP events on the index stream)
    float                   last_compact_ms[ 2 ] = {};  // the last compaction that moved rows: all its kernels; k_compact_rows over the vector block alone (lantern_gpu_last_compact_ms)
    int                     last_search_grid = 0;   // workgroups of the last unfiltered search launch, whatever its path (lantern_gpu_last_search_grid)
    std::deque<ProfBatch>   prof_pending;
    std::vector<hipEvent_t> prof_free;
    lantern_gpu_build_profile prof{};

    // ---- streaming continuation of usearch_search_ef (scan.c:273-281) ----------------------------
    // In the reference every scan owns its own usearch handle (scan.c:99), so "what this scan has been handed so far"
    // is per handle there.  Here ONE resident index serves many scans, so that state is a Cursor owned by the scan
    // (lantern_scan, a scan-service connection, lantern_gpu_cursor_*); usearch_search_ef itself -- one handle, one
    // scan, as in the reference -- uses the index's default cursor.
    Cursor default_cursor;

    // ---- page slots of a mirrored index (usearch_view_mem_lazy): device id -> the node's 48-bit slot in the PostgreSQL
    // pages (an ItemPointer, external_index.c:380-409), and back.  usearch_add_external writes the lists it changes
    // through retriever_mut in that form.
    bool                                   page_mode = false;  // attached through usearch_view_mem_lazy
    // the header's node count at attach time and the mirror's: they differ by the nodes no walk can reach (a re-prune
    // may drop a node's last in-link; such nodes stay in the pages and in the header's count)
    size_t                                 page_declared = 0, page_attach_n = 0;
    std::vector<uint64_t>                  page_slots;
    std::unordered_map<uint64_t, uint32_t> page_ids;
    // A mirror kept by the cache (mirror_cache.cpp) outlives the RetrieverCtx it was built with and is shared by holders that
    // each bring their own (scan.c:34,132, insert.c:130,247): its callbacks are looked up PER HOLDER -- a holder is a host
    // thread (a PostgreSQL backend is one; a threaded service runs one holder per thread) -- instead of in `opts`.
    struct HolderBinding { usearch_node_retriever_t retriever = nullptr, retriever_mut = nullptr; void *ctx = nullptr; };
    bool                                               holder_bound = false;  // true: `holders` decides, `opts.retriever*` are unused
    std::unordered_map<std::thread::id, HolderBinding> holders;
    // the calling thread's callbacks (ix->mu held)
    HolderBinding current_holder() const
    {
        if(!holder_bound) return HolderBinding{ opts.retriever, opts.retriever_mut, opts.retriever_ctx };
        auto it = holders.find(std::this_thread::get_id());
        return it == holders.end() ? HolderBinding{} : it->second;
    }

    // ---- single-query path (usearch_search_ef): one pinned, device-mapped block [query row | labels | distances |
    // slots | count] -- the kernel reads the query from it and writes the answer into it, so a lone query costs one
    // launch and one stream synchronisation, no copy commands
    char  *h_single = nullptr, *h_single_dev = nullptr;  // host / device address of the block
    size_t h_single_bytes = 0;
    // page-locked staging of a SMALL insertion (ldb_aminsert's one row): rows | labels | upper offsets | levels are read
    // from here by ONE kernel over the bus (k_stage_small): no copies, no wait before the batch's kernels
    char  *h_stage = nullptr, *h_stage_dev = nullptr;  // host / device address of the block
    size_t h_stage_bytes = 0;

    // ---- launches that share per-index scratch are ordered across streams.  The walk kernels use per-workgroup visited
    // bitmaps indexed by blockIdx only, so two launches may overlap only if they use different bitmap slabs.  SEARCH launches
    // have two slabs ("launch slots"): two batches on two streams run side by side (the second fills the machine while the
    // first one's longest walks drain); a third waits for the slot it reuses.  INSERT batches mutate the graph: they wait for
    // every search in flight, and searches on other streams wait for them.
    // one slab of visited bitmaps per search launch in flight (allocated on first use)
    uint32_t   *slot_bitmaps[ kSearchSlots ] = {};  // [0] aliases d_bitmaps (the slab inserts use too)
    size_t      slot_rows[ kSearchSlots ] = {}, slot_words[ kSearchSlots ] = {};
    hipEvent_t  slot_done[ kSearchSlots ] = {};
    hipStream_t slot_stream[ kSearchSlots ] = {};
    bool        slot_pending[ kSearchSlots ] = {};
    unsigned    slot_next = 0;
    hipEvent_t  insert_done = nullptr;
    bool        insert_pending = false;

    // ---- counters ----------------------------------------------------------------------------------
    uint64_t c_search_queries = 0, c_add_vectors = 0, c_add_batches = 0;

    // ---- filtered search (filter.hip): the path policy (lantern_gpu_set_filter_policy) and which path each launch took
    int      filter_path = 0;           // 0 auto, 1 walk, 2 exact
    size_t   filter_cand_cap = 0;       // 0: max(4 expansion, 256), capped by LDS
    double   filter_exact_factor = 5.6;  // auto: exact iff allowed^2 <= factor * ef * n; the measured crossover
    uint64_t c_filter_walk = 0, c_filter_exact = 0;
    size_t   filter_dense_min = 0;      // lantern_gpu_set_filter_dense: 0 off; m > 0: single-filter exact-path calls of nq >= m queries take the dense route
    uint64_t c_filter_dense[ 4 ] = {};  // lantern_gpu_filter_dense_stats: dense calls, their queries, certified, recomputed
    size_t   filter_dense_each_min = 0;  // lantern_gpu_set_filter_dense_each: 0 off; m > 0: in a per-query-filter call, m exact-path queries behind one filter handle take the dense route
    uint32_t last_each_dense[ 6 ] = {};  // lantern_gpu_last_filtered_each_dense: dense groups, their queries, certified, recomputed, rows gathered, contraction steps
    bool     filter_compact = false;    // lantern_gpu_set_filter_compact: filtered searches serve this index in its compact pq form too (default: refused)
    size_t   filter_seeds = 0;          // lantern_gpu_set_filter_seeds: 0 off; > 0: the walk path starts from that many allowed rows
    uint32_t last_seeds[ 4 ] = {};      // lantern_gpu_last_filtered_seeds: [1] S' of the last single-filter walk launch, [2] [3] the last call's seeded / unseeded walk queries ([0] is filter_seeds)
    uint32_t last_each[ 6 ] = {};  // the last per-query filtered call: queries on the walk path, on the exact path, unfiltered, empty; distinct filters; launches
    uint32_t last_each_params[ 4 ] = {};  // the last per-query filtered call with per-query parameters: largest walk expansion, largest C, largest k + skip on the exact path, queries with k == 0 (lantern_gpu_last_filtered_each_params)
    uint32_t last_params[ 6 ] = {};  // the last per-query-parameter call: launches, queries per list-placement class (3), largest expansion, any spec shape (lantern_gpu_last_params_launch)
    uint32_t last_filtered[ 6 ] = {};  // path (3: the dense route, [2] = k + skip, the rest 0), grid, expansion, cand_cap, vis_slots, LDS bytes of the last filtered launch (lantern_gpu_last_filtered_launch)

    hipStream_t stream = nullptr;
    int         device = 0;
    int         num_cus = 256;
    std::string err;

    View view() const;
};

// the six answer arrays of a search, device addresses; every one may be NULL
struct SearchOut { uint64_t *labels; float *dists; uint32_t *slots, *counts; uint64_t *D, *E; };

// ---- one batched search's trip through the host ---------------------------------------------------------------------------------
// The block `padded queries | labels | distances | counts [| extra]` as it lies in a page-locked staging block (every region at a
// multiple of 64 bytes; the answers lie the same way in their device buffer), and the stream and buffers the trip uses.  `which`
// names them all: a lane (its own stream, staging block and device buffers: one caller at a time), or kLanes -- the index stream,
// the index's own staging block and the per-call scratch, all three under ix->mu.  One copy up, one down, at the link's rate.
// The pieces below are put together in three places only (host_trip.hpp: the locking rule of each is stated there, once), and every
// lantern_gpu_search_batch* entry point is its refusals, its handles and one call with its launch as a callable:
//   host_trip_sync   the index's own block and stream, everything under ix->mu, ended by batch_finish_locked
//   host_trip_lane   staged without ix->mu; device buffers, upload, launch and download queued under it; the wait and the unpacking
//                    outside it; the error text in the calling thread's own string
//   device_trip      the caller's device memory and stream: lock, stride rule, flush, launch
// (lane_notify, index.cpp, keeps a body of its own: device-mapped block, no download, polling.)
struct HostBatch
{
    size_t      nq = 0, k = 0, q_bytes = 0, out_at = 0, out_bytes = 0, extra_at = 0, extra_bytes = 0;
    int         which = Index::kLanes;
    char       *hs = nullptr;                     // the staging block (batch_stage)
    hipStream_t stream = nullptr;                 // (batch_device)
    char       *d_q = nullptr, *d_out = nullptr;  // device: the queries, the answers (batch_device)

    size_t    bytes() const { return extra_at + extra_bytes + 64; }
    char     *h_out() const { return hs + out_at; }
    char     *h_extra() const { return hs + extra_at; }
    // the three answer arrays of a block that starts at `block` (host or device)
    SearchOut out(char *block) const { return { (uint64_t *)block, (float *)(block + nq * k * 8), nullptr, (uint32_t *)(block + nq * k * 12), nullptr, nullptr }; }
};
constexpr const char *kNoStage = "lantern_gpu: cannot allocate the page-locked staging block";  // batch_stage failed: the index's block, a lane's
constexpr const char *kNoLaneStage = "lantern_gpu: cannot allocate the lane's page-locked staging block";
HostBatch batch_layout(const Index *ix, int which, size_t nq, size_t k, size_t extra_bytes = 0);
bool      batch_stage(Index *ix, HostBatch &b, const void *queries, int kind);  // the staging block, the queries padded into it; false: no block (ix->err untouched: lanes stage without ix->mu)
bool      batch_device(Index *ix, HostBatch &b, bool buffers = true);  // under ix->mu: the stream (a lane's is created on first use), the two device buffers; false -> ix->err
bool      batch_upload(const HostBatch &b);    // queue staging -> d_q
bool      batch_download(const HostBatch &b);  // queue d_out -> staging
void      batch_unpack(const HostBatch &b, size_t first, size_t count, uint64_t *labels, float *distances, uint32_t *counts /* or NULL */);  // staged rows -> the caller's arrays
// under ix->mu throughout: the answers down, the wait, the caller's arrays; false -> ix->err (`what` if nothing more specific is there)
bool      batch_finish_locked(Index *ix, const HostBatch &b, bool ok, const char *what, uint64_t *labels, float *distances, uint32_t *counts);
// Before a search on behalf of `cur` (ix->mu held): a non-streaming call starts the scan over; an empty `seen` set adopts the index's
// epoch; slots remembered in an earlier epoch are refused (false -> ix->err: "the index was compacted: rescan")
bool      cursor_epoch_ok(Index *ix, Cursor *cur, bool streaming);
// the first k of `got` results whose slot `cur` has not handed out before, recorded in cur->seen as they are taken; returns how many
size_t    take_unseen(Cursor *cur, const uint64_t *labels, const float *dists, const uint32_t *slots, uint32_t got, size_t k, uint64_t *out_labels,
                      float *out_dists);

// implemented in index.cpp
const char *set_err(Index *ix, const std::string &msg);
// `expr` failed: ix->err names it, the enclosing function returns false
#define HIPCHK(ix, expr)                                                                  \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if(e_ != hipSuccess) {                                                            \
            set_err(ix, std::string("lantern_gpu: HIP error in " #expr ": ") + hipGetErrorString(e_)); \
            return false;                                                                 \
        }                                                                                 \
    } while(0)
bool        flush_locked(Index *ix);            // false -> ix->err set
bool        ensure_bitmaps(Index *ix, size_t slots);
bool        pq_encode_rows(Index *ix, size_t first, size_t count);  // raw f32 rows [first, first+count) in d_vec -> codes + decodings
bool        pq_decode_rows(Index *ix, size_t first, size_t count);  // d_codes -> d_vec
bool        pq_compact_locked(Index *ix);  // drop the decodings, keep the codes (searches: ADC)
bool        pq_expand_locked(Index *ix);   // decode them back (no-op unless compact)
bool        rows_stored(Index *ix, size_t first, size_t count);  // after rows [first, first + count) are in d_vec: their norms, their screen
void       *scratch(Index *ix, int which, size_t bytes);
bool        pad_row(const Index *ix, const void *vec, int kind_in, uint32_t *dst);
size_t      input_bytes(const Index *ix, int kind_in);
bool        kind_accepted(const Index *ix, int kind_in);
void        pad_rows(const Index *ix, const void *rows, int kind, size_t count, uint32_t *padded);
uint32_t   *next_ticket(Index *ix, size_t work, int grid, hipStream_t stream);  // a zeroed work ticket of a persistent launch, or NULL
uint32_t    vis_undo_cap();
int         search_grid(const Index *ix, size_t nq, int waves, int waves_per_cu);
int         search_grid(int num_cus, int max_wg, int forced_waves_per_cu, size_t nq, int waves, int waves_per_cu);  // the same, pure
// ---- the unfiltered search launch: a pure plan (plan_search), then one launch of it (search_plan.cpp) ---------------------------------
// the environment switches of the launch shape, as values (search_env reads them: LANTERN_GPU_SPEC, _ADC_SPEC, _PQ_ADC, _SPEC_WAVES and
// _LDS_LIST on every call -- in-process tests set them between calls --, _WIDE_ROWS and _WAVES_PER_CU once per process)
struct SearchEnv
{
    bool spec_set = false, adc_spec_set = false;                          // LANTERN_GPU_SPEC / _ADC_SPEC are present
    int  spec = 0, spec_waves = 0, wide_rows = -1, waves_per_cu = 0;      // their values; 0, -1, 0: absent
    bool adc_spec = false, pq_adc = false, lds_list = false;  // != 0
    int  screen_list_prefetch = -1;                                       // LANTERN_GPU_SCREEN_LIST_PREFETCH (read on every call): 0 / 1, -1: absent
    int  screen_descent = -1;                                             // LANTERN_GPU_SCREEN_DESCENT (read on every call): 0 / 1, -1: absent
};
SearchEnv search_env();
// what the shape rules read: the index's fields by their Index names, the call, the environment.  `each`: the launch is ONE CLASS of a
// per-query-parameter call (search_params_locked): nq = the queries of its list, k = the answer rows' width, ef and skip unused -- every
// query's own come from the table, the launch is shaped by max_expansion, the largest expansion of the list.
struct SearchPlanIn
{
    uint32_t  chunks = 0, M = 0, M0 = 0, ef_default = 0, pqd_inv = 0, pq_S16 = 0;                            // the index
    int       mcode = 0, num_cus = 0, search_vis_slots = -1, search_max_wg = 0;
    bool      pq_compact = false, phase_profile = false, spec_profile = false;
    bool      screen = false;  // the index has an int8 screen (d_screen)
    size_t    n = 0, nq = 0, k = 0, ef = 0, skip = 0;                                                         // (n: the index's rows) the call
    int       waves = 0;  // > 0: explicit (the classic kernel); < 0: automatic, the classic fallback takes -waves
    bool      each = false;
    uint32_t  max_expansion = 0;
    SearchEnv env;
};
// path: the rows and the launcher -- ADC over the code rows of a compact pq index (spec 0 or 2), the f32 walk over rows decoded on the fly
// (any spec), or the plain walk by its shape: classic (spec 0), spec 1, spec 2
enum SearchPath : uint32_t { kSearchAdc, kSearchPqd, kSearchClassic, kSearchSpec1, kSearchSpec2 };
struct SearchPlan
{
    SearchPath  path = kSearchClassic;
    int         spec = 0, waves = 0, grid = 0, wide_rows = 0, lds_list = 0;  // spec, wide_rows, lds_list: SearchArgs'
    uint32_t    expansion = 0, vis_slots = 0, spec_prefetch = 0, spec_cache = 0;
    size_t      lds = 0;             // dynamic LDS of a workgroup
    uint32_t    screen_lds = 0;      // ... of which the query's int8 planes (screen_query_lds_bytes): != 0 iff the launch screens
    uint32_t    list_prefetch = 0;   // SearchArgs::list_prefetch: only ever set in a launch that screens
    uint32_t    screen_descent = 0;  // SearchArgs::screen_descent: likewise (not among lantern_gpu_plan_search's outputs: the launch's shape does not depend on it)
    bool        took_spec = false;   // a latency-bound shape
    const char *refusal = nullptr;   // NULL: accepted; else the error text, and only `expansion` above is meaningful
};
SearchPlan   plan_search(const SearchPlanIn &in);  // pure: no HIP runtime call, no Index, no getenv, no allocation
SearchPlanIn search_plan_in(const Index *ix, size_t nq, size_t k, size_t ef, size_t skip, int waves);  // the index's fields, the call, search_env()
// ---- the k_insert launch of a batch (insert_batch.cpp run_batch): a pure plan, shown without a device by lantern_gpu_plan_insert -----------
struct InsertPlanIn
{
    int      mcode = 0, num_cus = 0, waves = 0;
    uint32_t chunks = 0, M0 = 0, efc = 0;
    size_t   rows = 0;             // the batch members this launch walks
    bool     screen_table = false; // the index has an int8 screen (d_screen)
    int      mode = 0;             // Index::insert_screen
    bool     lds_list = false;     // LANTERN_GPU_LDS_LIST
    bool     only_upper = false;   // the row-sharded build: no level-0 walk
    bool     lone_ok = false;      // a handful of rows may take the lone-insertion walk (one index, LANTERN_GPU_INSERT_SPEC != 0)
    int      vis_slots_env = -1;   // LANTERN_GPU_INSERT_VIS_SLOTS, or -1
};
struct InsertPlan
{
    bool        screened = false;  // k_insert<.., SCREEN = true>: the planes' block is part of lds and came out of vis_slots
    bool        lone = false;      // the lone-insertion walk (insert_spec_kernel.hip), never screened
    uint32_t    vis_slots = 0, screen_lds = 0, spec_prefetch = 0, spec_cache = 0;
    size_t      lds = 0;           // dynamic LDS of a workgroup
    const char *refusal = nullptr;
};
InsertPlan plan_insert(const InsertPlanIn &in);  // pure: no HIP runtime call, no Index, no getenv, no allocation
extern const bool kInsertScreenByDefault;  // the initial mode of Index::insert_screen where LANTERN_GPU_INSERT_SCREEN does not say
// the environment switches of a batch, as values (insert_env, insert_batch.cpp, says which is read once per process and which on every batch)
struct InsertEnv
{
    bool spec = true;            // LANTERN_GPU_INSERT_SPEC != 0: a handful of rows may take the lone-insertion walk
    bool group_all = false;      // LANTERN_GPU_GROUP_ALL != 0
    int  vis_slots = -1;         // LANTERN_GPU_INSERT_VIS_SLOTS (>= 0), or -1: absent
    bool reprune_state = true;   // LANTERN_GPU_REPRUNE_STATE != 0
    bool debug_groups = false;   // LANTERN_GPU_DEBUG_GROUPS is present
};
InsertEnv insert_env();
// (the exact k-NN's two switches, LANTERN_GPU_DENSE_NATIVE and _DENSE_FUSED, as values: DenseEnv / dense_env, dense.hpp)
struct Comm;
// Row-sharded build (index.cpp add_row_sharded_locked): where a batch's level-0 candidates come from
struct RowShard
{
    Index *loc;   // this rank's graph over ITS rows (labels = global slot + 1)
    Comm  *comm;
    size_t K;     // candidates a shard answers with per row
    size_t ef;    // ... found with this expansion (>= K)
};
// one batch of b new nodes at slots [ix->n, ix->n + b) with levels lv, rows and metadata already in HBM (insert_batch.cpp); false -> ix->err
bool run_batch(Index *ix, size_t b, const int *lv, Comm *comm, const RowShard *rs = nullptr);
bool sync_stream(Index *ix, Comm *comm);  // wait for the index stream (a sharded build: with the collective's deadline); false -> ix->err
// the table of a per-query-parameter launch (search_params_locked)
struct EachLaunch
{
    const char *h_table = nullptr;   // host: the call's table {k, expansion, skip, 0} by batch position, then the classes' query lists
    size_t      table_bytes = 0;     // ... copied into the scratch of the launch's slot; or
    const char *d_table = nullptr;   // ... the same block as the device names it (page-locked, device-mapped): read in place, no copy
    size_t      list_at = 0;         // byte offset of this launch's list in the block
};
// plan + refuse (ix->err, nothing acquired) + launch.
// `done`: NULL, or a device-visible counter the kernel bumps per finished query; the caller then WAITS ON IT (not on the
// stream) and no completion event is queued behind the launch
bool        run_search_device(Index *ix, const uint4 *d_queries, size_t nq, size_t k, size_t ef, size_t skip, const SearchOut &out,
                              hipStream_t stream, int waves, uint32_t *done = nullptr, uint32_t *done_flags = nullptr);
// A batch whose queries bring their own (k, ef, skip) (lantern_gpu_search_batch_params*; the caller holds ix->mu and has flushed): the
// planning of the whole call -- parameter checks, expansions, the split into at most three launches, the table.  Answer rows are
// k_stride wide.  `h_block`: NULL, or a page-locked block of params_table_bytes(nq) that stays untouched until the stream work is done;
// `d_block`: the same block's device address if the kernels are to read it in place.  false -> ix->err, nothing launched or written
// unless the failure is HIP's.
std::string params_check(const lantern_gpu_query_params *params, size_t nq, size_t k_stride);  // the checks that need no index: "" or the message
inline size_t params_table_bytes(size_t nq) { return nq * 20 + 16; }
bool        search_params_locked(Index *ix, const uint4 *d_queries, size_t nq, const lantern_gpu_query_params *params, size_t k_stride,
                                 const SearchOut &out, hipStream_t stream, int waves, uint32_t *done_flags, char *h_block, const char *d_block);

// one usearch_search_ef on behalf of `cur` (the caller holds ix->mu); returns the number of results
size_t      search_one_locked(Index *ix, Cursor *cur, const void *query, int kind, size_t k, size_t ef, bool streaming,
                              uint64_t *labels, float *distances);
// usearch_size of the index: for a mirror, the header's count plus what was inserted since
void        index_memory_bytes(const Index *ix, size_t &row_bytes, size_t &other_bytes);  // lantern_gpu_memory_usage's two numbers (ix->mu held)
inline size_t logical_size(const Index *ix) { return ix->page_mode ? ix->page_declared + (ix->n - ix->page_attach_n) : ix->n; }
void        prof_resolve(Index *ix, size_t keep);          // fold finished batches' event times into ix->prof
bool        order_launch(Index *ix, hipStream_t stream);   // before an insert batch (exclusive use of the index)
bool        record_launch(Index *ix, hipStream_t stream);  // behind it
bool        order_after_inserts(Index *ix, hipStream_t stream);  // work queued on `stream` from here on runs behind the pending insert batches
int         acquire_search_slot(Index *ix, hipStream_t stream, size_t grid);  // before a search launch: its bitmap slab (< 0: error)
bool        release_search_slot(Index *ix, int slot, hipStream_t stream);     // behind it
bool        import_graph_locked(Index *ix, size_t size, const void *vectors, const uint64_t *labels, const uint8_t *levels,
                                const uint32_t *nbr0, const uint32_t *upper_off, const uint32_t *upper_nbr, uint32_t entry_slot,
                                int32_t max_level, bool vectors_are_codes = false);  // pq: `vectors` = num_subvectors code bytes per row

// usearch-format serialisation (usearch_file.cpp)
size_t serialized_length(Index *ix);
bool   serialize(Index *ix, char *buf, size_t len);
using SpanSink = std::function<bool(const lantern_gpu_span *, size_t)>;
bool   serialize_stream(Index *ix, const SpanSink &sink);  // the same bytes as a sequence of spans (rows staged in chunks)
bool   deserialize(Index *ix, const char *buf, size_t len);

}  // namespace lgpu

// one scan's share of the streaming contract (lantern_gpu_cursor_*: index.cpp, filter.hip)
struct lantern_gpu_cursor
{
    lgpu::Index *ix;
    lgpu::Cursor cur;
};
