// kernels.hpp -- host-callable launchers of the gfx950 kernels (definitions in kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "device_common.hpp"
#include <atomic>

namespace lgpu {

// What a persistent search workgroup does AROUND one query reads these fields (query_frame.hpp: pick, stage, bind, answer rows,
// close).  SearchArgs and FilteredArgs (filter.hpp) each embed one as `frame`, so that the frame is written once.
struct FrameArgs
{
    const uint4    *queries;   // [nq][chunks], zero padded
    uint32_t        nq;
    const uint64_t *labels;    // [n]
    uint64_t       *out_labels;  // [nq][k] or NULL
    float          *out_dists;   // [nq][k] or NULL
    uint32_t       *out_slots;   // [nq][k] or NULL
    uint32_t       *out_counts;  // [nq] or NULL
    uint64_t       *out_D;       // [nq] or NULL
    uint64_t       *out_E;       // [nq] or NULL
    uint32_t       *bitmaps;     // [grid][bm_words + kVisUndoWords]: a workgroup's visited bitmap (all-zero between walks) + its undo log
    uint32_t        bm_words;    // multiple of 4
    uint32_t        undo_cap;    // entries of the undo log a walk may use (<= kVisUndoWords; LANTERN_GPU_VIS_UNDO for tests of the overflow path)
    uint32_t        vis_slots;   // LDS visited-set slots (a multiple of 4; 0 = HBM bitmap only)
    unsigned long long *totals;  // [2] cumulative D, E (atomicAdd) or NULL
    uint32_t       *ticket;      // zeroed before the launch: queries beyond the first gridDim.x are handed out dynamically
                                 // (NULL = static striding); results do not depend on who runs a query
    // the launches that serve a LIST of queries (k_search<.., EACH = true>; the per-query form of the filtered kernels); NULL otherwise
    const uint32_t *qlist;       // [nq] ticket position -> query of the caller's batch; answers land in the row of that query
};

struct SearchArgs
{
    View            view;
    FrameArgs       frame;
    uint32_t        k, ef, skip;
    int             lds_list;    // keep the candidate list in LDS even when it fits wave 0's registers (LANTERN_GPU_LDS_LIST=1: the
                                 // round-1 walk, kept for A/B parity runs and for ef > 128)
    int             wide_rows;   // small batch: the four-rows-in-flight instantiation (k_search<.., ROWS = 4>)
    int             spec;        // latency-bound launches (walk_spec.hpp): 1 = four-wave shape, 2 = dedicated role waves (3 + 8 waves);
                                 // 0 = off
    uint32_t        spec_prefetch;  // fetch every evaluated row's own level-0 list with the row (M0 % 4 == 0, M0 / 4 <= lanes per row)
    uint32_t        spec_cache;     // entries of the LDS list cache (power of two; 0 = none)
    // ADC over PQ codes (search_adc_kernel.hip; view.vec = the code rows, view.chunks = 16-byte chunks per code row)
    const float    *adc_centers;    // [S][C][sub_floats] per-subvector centroid tables, rows zero padded to whole chunks
    uint32_t        adc_S, adc_C, adc_subdim;
    uint32_t        adc_qchunks;    // 16-byte chunks of a (raw f32) query row
    unsigned long long *phase_cycles;  // diagnostics (lantern_gpu_search_phase_profile): [8] shader-clock cycles summed over the
    uint32_t       *done;        // NULL, or a counter in host-visible memory: +1 (system scope) per finished query, after its answers
    uint32_t       *done_flags;  // NULL, or [nq] words in host-visible memory: query q's word = 1 (system scope, release) once its answers
                                 // are written -- a host that keeps the answers in device-mapped memory hands each one on as ITS walk ends
                                 // instead of when the launch's longest walk does (lantern_gpu_search_batch_lane_notify)
    uint32_t       *touched;     // diagnostics (lantern_gpu_search_unique_rows; the instrumented instantiations only): [ceil(n / 32)] one
                                 // bit per row, set when any query of the launch evaluates the row; NULL = off
    uint32_t       *trace;       // diagnostics (lantern_gpu_search_row_trace; the instrumented instantiations only): [nq][trace_cap] the
    uint32_t       *trace_count; // memory objects every query asks for, in order (walk.hpp trace_append), and [nq] how many; NULL = off
    uint32_t        trace_cap;
    unsigned long long *screen_totals;  // [2] cumulative row evaluations and how many of them read the f32 row (the int8 screen:
                                        // lantern_gpu_search_screen_stats) of the launches whose view has a screen, or NULL
    // the per-query-parameter form (k_search<.., EACH = true>, lantern_gpu_search_batch_params*; with frame.qlist); NULL / 0 otherwise
    const uint4    *qparams;     // [caller's batch] {k, expansion, skip, 0} by position; `k`, `skip` above are unused, `ef` is the list's largest expansion
    uint32_t        k_stride;    // width of an answer row
    uint32_t        list_prefetch;  // the launches that screen: request the front's neighbour list one hop ahead (walk.hpp search_level_reg; LGPU_SCREEN_LIST_PREFETCH)
    uint32_t        screen_descent; // the launches that screen: the descent's upper-level rows go through the screen too (walk.hpp greedy_descent; LGPU_SCREEN_DESCENT)
};                             // launch's queries by phase: pop | list + visited | distances | merge | descent | whole query

// one reverse-link request produced by the insert pass: add `new_slot` to `close`'s list at `level`
struct LinkReq
{
    uint32_t close;  // EMPTY = unused entry
    uint32_t level;
    uint32_t new_slot;
    float    d;  // metric(new_slot, close)
};

struct InsertArgs
{
    View            view;       // n = size BEFORE the batch; entry/max_level frozen
    uint32_t        first_slot; // the batch occupies slots [first_slot, first_slot + count)
    uint32_t        b_begin;    // this launch walks the batch members [b_begin, count) -- a rank of a work-sharded
    uint32_t        count;      // build (shard.cpp) walks only its own sub-range; 0 / batch size otherwise
    uint32_t        efc;
    const uint32_t *link_off;   // [batch] first LinkReq of each new node (M*(level+1) entries each); /M = first item
    uint64_t       *tops;       // [items][efc] walk results, ascending (distance, slot) keys
    uint32_t       *top_count;  // [items]
    uint32_t       *bitmaps;     // as SearchArgs
    uint32_t        bm_words;
    uint32_t        undo_cap;
    uint32_t        vis_slots;   // LDS visited-set slots (0 = HBM bitmap only)
    unsigned long long *totals;  // [2] cumulative D, E (and, screened launches, [kInsertScreenTotals..+1] below)
    uint32_t       *ticket;      // as SearchArgs::ticket, over the batch members
    int             lds_list;    // as SearchArgs::lds_list
    uint32_t        spec_prefetch, spec_cache;  // the latency-bound form (insert_spec_kernel.hip): as SearchArgs'
    uint32_t        only_upper = 0;  // k_insert only: 1 = walk levels >= 1 only (the row-sharded build takes a node's level-0 candidates from the shards)
};
// The slots of Index::d_totals, the block of cumulative device counters (atomicAdd; one allocation, zeroed at init).  A kernel gets a
// pointer AT its range: SearchArgs / FilteredArgs frame.totals -> kTotSearch, InsertArgs::totals -> kTotInsert, ConnectArgs::totals
// -> kTotConnect, RevlinkArgs::totals -> kTotRevlink, SearchArgs::phase_cycles -> one of the profiles, ::screen_totals -> kTotSearchScreen.
enum TotalsSlot : int
{
    kTotSearch = 0,         // [2] the searches' D, E
    kTotInsert = 2,         // [2] the insert walk's D, E
    kTotConnect = 4,        // [1] k_connect's pair evaluations
    kTotRevlink = 5,        // [2] the reverse links' pair evaluations, re-prunes
    kTotPhaseProfile = 8,   // [kTotPhaseProfileWords] lantern_gpu_search_phase_profile
    kTotSpecProfile = 16,   // [kTotSpecProfileWords] lantern_gpu_spec_profile
    kTotSearchScreen = 48,  // [2] the searches' screen: row evaluations, of which read the f32 row
    kTotInsertScreen = 50,  // [2] k_insert's screen: rows tested, rows rejected
    kTotUnlink = 52,        // [2] lantern_gpu_unlink_deleted's reverse links: pair evaluations, re-prunes (unlink.hip; not a build counter)
    kTotalsWords = 64       // the block's size
};
constexpr int kTotPhaseProfileWords = 8, kTotSpecProfileWords = 32;
static_assert(kTotSearch + 2 <= kTotInsert && kTotInsert + 2 <= kTotConnect && kTotConnect + 1 <= kTotRevlink && kTotRevlink + 2 <= kTotPhaseProfile &&
                  kTotPhaseProfile + kTotPhaseProfileWords <= kTotSpecProfile && kTotSpecProfile + kTotSpecProfileWords <= kTotSearchScreen &&
                  kTotSearchScreen + 2 <= kTotInsertScreen && kTotInsertScreen + 2 <= kTotUnlink && kTotUnlink + 2 <= kTotalsWords,
              "the ranges of Index::d_totals are disjoint and inside the block");
// k_insert's screened launches (view.screen set) add the rows they put to the int8 screen test, and the rows it rejected, to
// kTotInsertScreen, reached from InsertArgs::totals: totals[kInsertScreenTotals], [+ 1] (lantern_gpu_insert_screen_stats).
// An offset rather than a field: the argument block of the unscreened kernels stays as it was.
constexpr int kInsertScreenTotals = kTotInsertScreen - kTotInsert;

// neighbour selection of the new nodes: one item per (new node, level)
struct ConnectArgs
{
    View            view;
    uint32_t        first_slot;
    uint32_t        item_begin;  // first item of this launch (a rank's sub-range of a work-sharded build; 0 otherwise)
    uint32_t        items;       // items of this launch
    uint32_t        efc;
    const uint32_t *link_off;    // [count]
    const uint32_t *item_node;   // [items] index of the new node within the batch
    const uint64_t *tops;
    const uint32_t *top_count;
    LinkReq        *links;       // [sum M*(level+1)]
    unsigned long long *totals;  // [1] cumulative pair evaluations
};

struct RevlinkArgs
{
    View            view;
    const uint32_t *ngroups;      // device: number of (close, level) groups of this batch (written by the grouping pass)
    const uint2    *groups;       // device: [*ngroups] {begin, end} into reqs; any order (groups are independent of one another)
    uint32_t        max_groups;   // host-side upper bound on *ngroups (sizes grids and the worklist)
    const LinkReq  *reqs;         // sorted by (close, level), stable: within a group in new-slot order
    unsigned long long *totals;   // [2] cumulative pair evaluations, re-prunes
    // Persistent re-prune state (k_revlink_pairs), or NULL: radius[node] / radius_upper[upper block] = d(node, LAST list entry)
    // when that list is FULL, greedy-consistent and stored in ascending (distance, tie) order -- i.e. it is exactly what a
    // re-prune left -- and NaN otherwise.  A request whose own distance sorts behind the radius is cut without reading a row;
    // any other request to such a list starts the chain form (<= cap distances) instead of the all-pairs table.
    float          *radius0, *radius_upper;
};

// The grouping pass (grouping.hip): the reverse-link requests of a batch, as k_connect left them (new-slot-major, EMPTY
// entries in between), become `sorted` -- stable radix sort by (close, level) -- and the list of groups.  Everything stays
// on the device and on `stream`: the batches of a build queue up without a host round trip.
// world > 1 (work-sharded build): only the requests whose `close` this rank owns (close % world == rank) are kept;
// owner_counts[world] (device, zeroed here) receives the number of requests per owner.
struct GroupScratch
{
    uint64_t *keys_a, *keys_b;   // [n]
    uint32_t *idx_a, *idx_b;     // [n]
    void     *temp;              // rocPRIM temporary storage
    size_t    temp_bytes;
};
size_t     group_temp_bytes(size_t n);
hipError_t launch_group_requests(const LinkReq *links, uint32_t n, const GroupScratch &gs, LinkReq *sorted, uint2 *groups, uint32_t *ngroups,
                                 int world, int rank, uint32_t *owner_counts, hipStream_t stream, uint32_t *zero_me = nullptr);
hipError_t launch_group_keys_owned(const LinkReq *links, uint32_t n, const GroupScratch &gs, uint32_t *ngroups, int world, int rank, uint32_t *owner_counts,
                                   hipStream_t stream, uint32_t *zero_me = nullptr);
hipError_t launch_group_sort_owned(const LinkReq *links, uint32_t m, const GroupScratch &gs, LinkReq *sorted, uint2 *groups, uint32_t *ngroups,
                                   hipStream_t stream);
// (zero_me: a device word the pass sets to 0 on the way -- the reverse-link kernels' work counter; launch_revlink is then told so)
// link_off[i] = M * sum_{j<i} (level_j + 1), item_node[item] = i for the (level_i + 1) items of node i -- the layout of
// one batch, from the levels already in HBM (no per-batch host upload)
hipError_t launch_batch_layout(const uint8_t *levels, uint32_t b, uint32_t M, uint32_t *link_off, uint32_t *item_node, hipStream_t stream);
// a few new rows and their metadata from a device-mapped host block to their places (one kernel instead of four copies)
hipError_t launch_stage_small(const void *rows, const uint64_t *labels, const uint32_t *upper_off, const uint8_t *levels, uint32_t count, uint32_t chunks,
                              void *d_rows, uint64_t *d_labels, uint32_t *d_upper_off, uint8_t *d_levels, hipStream_t stream);

// ---- compaction (compact.hip; lantern_gpu_compact_deleted) -------------------------------------------------------
// The renumbering of n old slots, all in device memory.  Every array but src_of holds n + 1 words: word n of `map` is the number of live
// slots, word n of `uoff` the upper blocks they own.
struct CompactMap
{
    uint32_t *flags;   // [n + 1] scan input: 1 for a live slot (label != 0), 0 for a tombstone and at n
    uint32_t *lv;      // [n + 1] scan input: a live slot's level, 0 for a tombstone and at n
    uint32_t *map;     // [n + 1] old slot -> new slot (the live slots below it), EMPTY for a tombstone
    uint32_t *uoff;    // [n + 1] old slot -> the first upper block of its new slot (the levels of the live slots below it)
    uint32_t *src_of;  // [live]  new slot -> old slot
    void     *temp;    // rocPRIM temporary storage
    size_t    temp_bytes;
};
size_t     compact_temp_bytes(size_t n);
hipError_t launch_compact_map(const uint64_t *labels, const uint8_t *levels, size_t n, const CompactMap &m, hipStream_t stream);
// dst row j = src row src_of[j] for j < live, rows of row_bytes each (16-byte units where row_bytes is a multiple of 16, bytes otherwise)
hipError_t launch_compact_rows(const void *src, void *dst, const uint32_t *src_of, size_t live, size_t row_bytes, int num_cus, hipStream_t stream);
// level 0 (old_levels == NULL): list j of W entries = list src_of[j] through the map.  Upper levels: the level[src_of[j]] blocks of W
// entries at old_uoff[src_of[j]] -> the blocks at m.uoff[src_of[j]].  *dangling += the entries that are neither EMPTY nor mapped.
hipError_t launch_compact_lists(const uint32_t *old_nbr, uint32_t *new_nbr, const CompactMap &m, uint32_t n_old, size_t live, uint32_t W,
                                const uint8_t *old_levels, const uint32_t *old_uoff, unsigned long long *dangling, int num_cus, hipStream_t stream);
struct CompactMeta
{
    const uint64_t *labels;  uint64_t *new_labels;
    const uint8_t  *levels;  uint8_t  *new_levels;
    const float    *norm2;   float    *new_norm2;        // or NULL
    const float2   *screen_meta; float2 *new_screen_meta; // or NULL
    uint32_t       *new_upper_off;
};
hipError_t launch_compact_meta(const CompactMeta &a, const CompactMap &m, size_t live, hipStream_t stream);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel instantiation, device, size reached) instead of on every launch:
// a driver call of microseconds that a lone query or a one-row insertion would repeat every time.  `cache` is a static of the
// launcher's expansion for ONE instantiation: zero-initialised, [device ordinal] = the largest size set so far.
struct LdsAttrCache { std::atomic<size_t> set[ 64 ]; };
inline void ensure_dynamic_lds(const void *fn, size_t lds, LdsAttrCache &cache)
{
    int dev = 0;
    if(hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        return;
    }
    if(cache.set[ dev ].load(std::memory_order_acquire) >= lds && lds > 0) return;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    size_t seen = cache.set[ dev ].load(std::memory_order_relaxed);
    while(seen < lds && !cache.set[ dev ].compare_exchange_weak(seen, lds, std::memory_order_release)) {}
}

// One instantiation KERNEL (in parentheses: its template arguments hold commas): its LdsAttrCache, the opt-in to `lds_` bytes of dynamic
// LDS, the launch with the arguments that follow.  A block, so that `if(..) LGPU_LAUNCH_LDS(..) else ..` reads as written.
#define LGPU_LAUNCH_LDS(KERNEL, grid_, block_, lds_, stream_, ...)                                  \
    {                                                                                               \
        static LdsAttrCache attr_;                                                                  \
        ensure_dynamic_lds((const void *)KERNEL, lds_, attr_);                                      \
        hipLaunchKernelGGL(KERNEL, dim3(grid_), dim3(block_), lds_, stream_, __VA_ARGS__);          \
    }

// Diagnostics (lantern_gpu_last_search_cells; search_plan.cpp): the launch macros of k_search (1) and k_search_adc (2) note the template
// arguments of the instantiation they launch in a thread-local ring, with whether the launch screens and its query count.  Host only:
// a few thread-local stores per launch.
void note_search_cell(int kernel, int metric, int G, int prof, int rows, int kpl, int spec, int each, const SearchArgs &a);

// All launchers return hipSuccess or the launch error.  `metric` is a usearch_metric_kind_t value.
hipError_t launch_search(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream);
hipError_t launch_search_spec(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream);  // a.spec != 0 (search_spec_kernel.hip)
// a.qparams != NULL: the per-query-parameter instantiations (search_each_kernel.hip: the classic shapes; search_each_spec_kernel.hip: a.spec == 2)
hipError_t launch_search_each(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream);
hipError_t launch_search_each_spec(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream);
size_t     search_spec_lds_bytes(uint32_t M0, uint32_t prefetch, uint32_t cache_entries);
hipError_t launch_search_adc(int metric, const SearchArgs &a, int waves, int grid, hipStream_t stream);  // metric = M_L2SQ_ADC / M_COS_ADC
size_t     search_adc_lds_bytes(uint32_t code_chunks, uint32_t qchunks, uint32_t ef_cap, uint32_t M0, uint32_t vis_slots);
hipError_t launch_insert(int metric, const InsertArgs &a, int waves, int grid, hipStream_t stream);
// a handful of insertions (ldb_aminsert, the first batches of a build): level 0 by the lone-query walk (f32 l2sq / cos, efc <= 128)
bool       insert_spec_supported(int metric, uint32_t efc, uint32_t M0);
size_t     insert_spec_lds_bytes(uint32_t chunks, uint32_t efc, uint32_t M0, uint32_t vis_slots, uint32_t prefetch, uint32_t cache_entries);
hipError_t launch_insert_spec(int metric, const InsertArgs &a, int waves, int grid, hipStream_t stream);
hipError_t launch_connect(int metric, const ConnectArgs &a, hipStream_t stream);
// work: scratch of max_groups x 8 bytes; work_count: one u32 (both device memory)
hipError_t launch_revlink(int metric, const RevlinkArgs &a, void *work, uint32_t *work_count, int num_cus, hipStream_t stream,
                          bool work_count_is_zero = false);
// ---- work-sharded build (shard.cpp): the exchange steps either side of the RCCL all-gathers -------------
// Every rank holds the complete request array after the first all-gather; the own lists of the nodes another
// rank connected are rebuilt from their requests: list(new_slot, level)[i] = links[link_off[b] + level*M + i].close
hipError_t launch_apply_own_links(const View &v, uint32_t first_slot, const uint32_t *link_off, const LinkReq *links,
                                  uint32_t total_links, hipStream_t stream);
// One record per reverse-link group a rank owned: [close, level, list[0..M0)] (rec_words = M0 + 2 u32 words).
// pack: records[g] for g in [0, ngroups); apply: every record with close != EMPTY is written into the local replica.
hipError_t launch_pack_lists(const RevlinkArgs &a, uint32_t *records, hipStream_t stream);
hipError_t launch_apply_lists(const View &v, const uint32_t *records, uint32_t nrecords, hipStream_t stream);

// ---- product quantisation (grouping.hip): a PQ index holds every row's DECODING in the vector block (all distances are
// distances to / between decoded vectors) and the codes -- what the file and the pages carry -- beside it
hipError_t launch_pq_take(const float *rows, uint32_t row_floats, uint32_t first, uint32_t count, uint32_t s, uint32_t subdim, uint32_t sub_floats,
                          float *sub, hipStream_t stream);
hipError_t launch_pq_put(float *rows, uint32_t row_floats, uint32_t first, uint32_t count, uint32_t s, uint32_t subdim, uint32_t S, const uint32_t *nearest,
                         const float *codebook, uint32_t dims, uint8_t *codes, hipStream_t stream);
hipError_t launch_pq_decode(float *rows, uint32_t row_floats, uint32_t first, uint32_t count, uint32_t subdim, uint32_t S, const float *codebook, uint32_t dims,
                            const uint8_t *codes, hipStream_t stream);

// f32 rows -> the stored rows of an f16 / i8 / b1 index, on the device (the rules of pad_row, element for element)
hipError_t launch_merge_parts(const uint64_t *labels, const float *dists, uint32_t world, uint32_t nq, uint32_t k, uint64_t *out_labels,
                              float *out_dists, uint32_t *out_counts, hipStream_t stream);
// row-sharded build: the shards' candidate lists, merged, as the selection kernel's level-0 input
hipError_t launch_merge_candidates(const uint64_t *labels, const float *dists, uint32_t world, uint32_t nq, uint32_t k, uint32_t first_slot,
                                   const uint32_t *link_off, uint32_t M, uint32_t stride, uint64_t *tops, uint32_t *top_count, hipStream_t stream);
hipError_t launch_store_quantised(const float *src, uint32_t dims, uint32_t count, int kind, uint32_t *rows, uint32_t row_words, hipStream_t stream);

// ||row||^2 of rows [first, first + count) into norm2 (cosine metrics only; no-op otherwise)
hipError_t launch_fill_norms(int metric, const View &v, uint32_t first, uint32_t count, float *norm2, hipStream_t stream);
// the int8 screen rows and (s, r) of the f32 rows [first, first + count) (walk.hpp hop_distances_screened); norm2 != NULL (a cosine
// index: the rows' cached rooted norms, filled before this on the same stream): (s / norm, rho) instead
hipError_t launch_fill_screen(const View &v, uint32_t first, uint32_t count, uint4 *screen, float2 *meta, const float *norm2, hipStream_t stream);
// diagnostics (screen_probe_kernel.hip): out[i] = 1 where hop_distances_screened rejects slots[i] (n <= 64) for `query` at `radius`,
// run by one workgroup of `threads` (256 or 512); the view must have a screen
hipError_t launch_screen_probe(int metric, const View &v, const uint4 *query, const uint32_t *slots, uint32_t n, float radius, int threads,
                               uint8_t *out, hipStream_t stream);
// out[i] = metric(query, row(slots[i]))
hipError_t launch_gather(int metric, const View &v, const uint4 *query, const uint32_t *slots, uint32_t n, float *out,
                         hipStream_t stream);
// out[i*nb + j] = metric(a[i], b[j]) in the graph walk's exact reduction order
hipError_t launch_pairs(int metric, const uint4 *a, uint32_t na, const uint4 *b, uint32_t nb, uint32_t chunks, float *out,
                        hipStream_t stream);

// dense contraction + exact k-NN building blocks (bruteforce.hip)
hipError_t launch_dequant_f16(const uint4 *src, size_t nchunks, uint4 *dst, hipStream_t stream);
hipError_t launch_dequant_i8(const uint4 *src, size_t nchunks, uint4 *dst, hipStream_t stream);
// The dense contraction out[i * ldo + j] ~ metric(Q[i], B[j]) on rows of `chunks` uint4.  kind is the plan's operand kind
// (lantern_gpu_plan_exact_knn): 0 -- f32 rows on the fp32 MFMA (k_dense_f32), or bit rows under the popcount metrics (k_dense_ham, which
// reads no norms); 1 / 2 -- rows STORED as f16 / i8, on the MFMAs of that operand type (k_dense_native, dense_native.hip).  metric is
// the base metric.  qn / bn: one 32-bit word per row, as launch_norms wrote them for the same kind and metric: f32 and f16 rows -- the
// f32 |x|^2; i8 -- the exact int32 sum of squares (l2sq) or the bits of its IEEE root (cos).  The i8 outputs are the pair kernel's
// distances bit for bit.  Refused with hipErrorInvalidValue: another kind, a metric the kind has no kernel for, a Hamming row over
// 16384 words.
struct DenseOperands
{
    int          kind, metric;
    const uint4 *Q;
    uint32_t     nq;
    const uint4 *B;
    uint32_t     nb, chunks;
    const void  *qn, *bn;
};
struct DenseTopk;  // dense_tile.hpp
// topk == NULL: the matrix goes to out (leading dimension ldo).  Otherwise out and ldo are unused: the tile epilogue appends what can
// still enter a query's running top-kk to the candidate lists of *topk (l2sq / cos only)
hipError_t launch_contraction(const DenseOperands &o, float *out, uint32_t ldo, const DenseTopk *topk, hipStream_t stream);
hipError_t launch_norms(int kind, int metric, const uint4 *rows, uint32_t n, uint32_t chunks, void *out, hipStream_t stream);
hipError_t launch_select_candidates(uint32_t nq, uint64_t *best, uint32_t kk, const uint64_t *cand, uint32_t *cnt, uint32_t cap, uint32_t *overflow,
                                    hipStream_t stream);
hipError_t launch_select(const float *dist, uint32_t ldo, uint32_t nq, uint32_t ncols, uint32_t c_base, uint64_t *best, uint32_t kk,
                         hipStream_t stream);
// list: NULL, or the ascending slot list the keys' low words are positions in (k_rerank)
hipError_t launch_rerank(int metric, const uint4 *Q, uint32_t nq, const uint4 *B, uint32_t chunks, const uint64_t *best, uint32_t kk,
                         uint32_t k, uint32_t *out_slots, float *out_dists, const uint32_t *list, hipStream_t stream);
// rows list[0..n) of src into the contiguous dst with their norm words, as launch_norms(kind, metric, dst, ...) would write them,
// in one pass (k_gather_rows_norms).  kind 3: no norms (bit rows, rows dequantised before the contraction), norms may be NULL
hipError_t launch_gather_rows_norms(int kind, int metric, const uint4 *src, uint32_t chunks, const uint32_t *list, uint32_t n, uint4 *dst, void *norms,
                                    hipStream_t stream);
// the exact k-NN's certificate (flag[q] = 1: certified; flag[nq] != 0: a cosine row norm out of the bound's range) and the
// exact-order fallback's row gather / result scatter (bruteforce.hip)
hipError_t launch_certify(int metric, const uint64_t *best, uint32_t kk, const float *dists, uint32_t k, const float *qn, uint32_t nq, const float *bn,
                          uint32_t nb, uint32_t dims, uint32_t *flag, hipStream_t stream);
hipError_t launch_gather_rows(const uint4 *src, uint32_t chunks, const uint32_t *idx, uint32_t n, uint4 *dst, hipStream_t stream);
hipError_t launch_emit_topk(const uint64_t *best, uint32_t k, const uint32_t *idx, uint32_t n, uint32_t *out_slots, float *out_dists, hipStream_t stream);

size_t search_lds_bytes(uint32_t chunks, uint32_t ef_cap, uint32_t M0, uint32_t vis_slots);
size_t insert_lds_bytes(uint32_t chunks, uint32_t efc, uint32_t M0, uint32_t vis_slots);

}  // namespace lgpu
