// dense.hpp -- the dense path's host side (dense.cpp): the exact k-NN as a pure plan and one run of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace lgpu {

// the environment switches of the exact k-NN, as values (dense_env reads both on every call -- in-process tests set them between calls)
struct DenseEnv
{
    int native = -1;  // LANTERN_GPU_DENSE_NATIVE: 0 -- f16 / i8 rows are contracted on an f32 copy, else as they are stored; -1: absent (kDenseNativeDefault)
    int fused = -1;   // LANTERN_GPU_DENSE_FUSED: 0 -- always the unfused path (A/B, tests); -1: absent
};
DenseEnv dense_env();

// one contraction launch of an exact k-NN: queries [q0, q0 + nqt) against base rows [col0, col0 + cols).  fused == 0: the matrix goes
// to dd and launch_select folds it into the queries' best lists; 1: the fused epilogue, then launch_select_candidates
struct KnnStep
{
    uint32_t q0, nqt, col0, cols, fused;
};
// Everything an exact k-NN call decides before it touches the device; lantern_gpu_plan_exact_knn shows it without one.
struct ExactKnnPlan
{
    // the call's own numbers
    int      mcode = 0;
    uint32_t chunks = 0, k = 0;
    size_t   nb = 0, nq = 0;
    // the operands (lantern_gpu_plan_dense projects these)
    int      kind = 0;            // DenseOperands::kind: 0 f32 (or bit) rows, 1 / 2 f16 / i8 rows as stored, kDensePq (4) the code rows of a compact pq index (mcode M_*_PQD)
    int      copy = 0;            // the rows are dequantised to f32 for the contraction: 0 no, 1 from f16, 2 from i8
    uint32_t fchunks = 0;         // 16-byte chunks of a row as the contraction reads it
    bool     bits = false;        // a popcount metric: no MFMA contraction, no norms, never fused
    bool     exact_keys = false;  // the pre-selection ranks on the exact-order distance itself: nothing to certify
    uint32_t dims = 0;            // the dims the certificate is told (0 iff exact_keys)
    uint32_t k_steps = 0;         // K steps (128 bytes of a row each) per output tile
    size_t   fb_bytes = 0;        // the f32 copy of one chunk of base rows (0: no copy)
    size_t   gb_bytes = 0;        // a run over a slot list: one gathered chunk of base rows as stored (plan_filtered_dense; 0 otherwise)
    // the launches and their buffers
    uint32_t kk = 0;                                     // survivors per query, k + 16: re-ranked in exact order, then cut to k
    uint32_t chunk_rows = 0, qtile = 0, seed_cols = 0;    // base rows and queries per launch; the columns that give every query a radius
    uint32_t cand_cap = 0;                                // fused: candidate keys per query
    bool     fused = false;                               // asked for, not a popcount metric, and more than seed_cols rows
    uint32_t ldd = 0;                                     // leading dimension of dd
    size_t   aux_bytes = 0, dd_bytes = 0, cand_bytes = 0, fq_bytes = 0;  // the pooled blocks (cand: 0 unless fused); the queries' f32 copy
    size_t   qn_off = 0, bn_off = 0, best_off = 0, flag_off = 0;         // inside aux: norms, the best lists (8-byte aligned), the certificate's flags
    size_t   cnt_off = 0, over_off = 0;                                  // inside cand, behind the lists: their counters, the overflow word
    // the ordered contraction steps: chunk-major, query-tile-minor, plain before fused; computed by index, so a plan allocates nothing
    size_t  n_steps = 0;
    KnnStep step(size_t i) const;
};
// pure: no HIP runtime call, no getenv.  native / fused: DenseEnv's.  NULL, or why the call is refused (static text)
const char *plan_exact_knn(int64_t mcode, int64_t chunks, int64_t nb, int64_t nq, int64_t k, int native, int fused, ExactKnnPlan &p);

// The filtered exact path's dense route (DESIGN.md 4.9 "Dense exact path"): whether a single-filter call takes it, and the exact k-NN
// it then runs over the filter's `allowed` rows with k := k + skip.  lantern_gpu_plan_filtered_dense shows it without a device.
enum FilteredDenseWhy : uint32_t
{
    kDenseTaken = 0,
    kDenseOff,        // min_queries == 0
    kDenseFewQueries, // nq < min_queries
    kDenseWalkPath,   // the query's path is the walk
    kDenseWide,       // k + skip > 240
    kDenseCompact,    // a compact pq index
    kDenseEmpty       // nothing allowed, or nothing asked for: no launch at all
};
struct FilteredDensePlan
{
    FilteredDenseWhy why = kDenseOff;
    ExactKnnPlan     knn;              // taken: plan_exact_knn(mcode, chunks, nb = allowed, nq, k + skip), and knn.gb_bytes
    uint32_t         gather_rows = 0;  // rows per gathered chunk
    size_t           norm_bytes = 0;   // the gathered rows' norm words (0: bit rows)
};
// pure, as plan_exact_knn.  NULL, or why the input is refused; a call that is not taken is not refused (why != kDenseTaken)
const char *plan_filtered_dense(int64_t mcode, int64_t chunks, int64_t allowed, int64_t nq, int64_t k, int64_t skip, int64_t min_queries, bool exact,
                                bool compact, int native, int fused, FilteredDensePlan &p);
// One run of a taken plan: rows d_base[d_list[0..allowed)] (d_list ascending).  Result (device): slots[nq][k + skip] ascending by
// (exact-order distance, slot), dists alike, flags[nq] = 1 where the certificate holds; the queries it refuses are listed in
// `refused` and their rows of the result are not the answer: the caller recomputes them.  Waits for `st`.
bool filtered_dense_device(const FilteredDensePlan &p, int native, const uint4 *d_base, const uint32_t *d_list, const uint4 *d_q, uint32_t *d_slots,
                           float *d_dists, uint32_t *d_flags, hipStream_t st, std::vector<uint32_t> &refused);

// The dense route of a PER-QUERY-FILTER call (DESIGN.md 4.9 "Dense exact path, per-query filters"): the exact-path queries that share
// a filter handle form a group; the groups of at least min_group queries are answered by ONE segmented run of the exact k-NN -- group
// g's queries against group g's rows only.  lantern_gpu_plan_filtered_each_dense shows the plan without a device.
enum EachDenseWhy : uint32_t
{
    kEachDenseTaken = 0,
    kEachDenseOff,       // min_group == 0
    kEachDenseWide,      // k + skip > 240
    kEachDenseCompact,   // a compact pq index
    kEachDenseTooMany,   // the dense groups' rows, concatenated, do not fit 32 bits
    kEachDenseNoGroup    // no filter handle stands behind min_group exact-path queries (or nothing asked for)
};
struct EachDensePlan
{
    EachDenseWhy          why = kEachDenseOff;
    std::vector<uint32_t> group;  // [nq] the dense group of a query, 0xFFFFFFFF: none (it runs as without the setting)
    std::vector<uint32_t> order;  // the dense queries as the run holds them: groups by the first query that names them, a group's queries in call order
    std::vector<uint32_t> qoff;   // [groups + 1] group g's queries are order[qoff[g], qoff[g + 1])
    std::vector<uint32_t> seg;    // [groups + 1] group g's rows are positions [seg[g], seg[g + 1]) of the concatenated slot list L
    // plan_exact_knn(mcode, chunks, nb = seg.back(), nq = order.size(), k + skip), unfused, with gb_bytes: the run's buffers.  Its own
    // n_steps / step() are the unsegmented run's and are not used: the run executes `steps`
    ExactKnnPlan          knn;
    uint32_t              gather_rows = 0;  // rows per gathered chunk of L
    // a tile (<= qtile) of one group's queries against that group's positions inside one chunk of L: chunk-major, then by group, then
    // by tile; q0 in `order` coordinates, col0 in L coordinates
    std::vector<KnnStep>  steps;
    size_t groups() const { return qoff.empty() ? 0 : qoff.size() - 1; }
};
// pure, as plan_exact_knn.  Per query i: ids[i] -- -1 for a NULL entry, else equal for equal handles; counts[i] -- its filter's allowed
// rows; exact[i] -- its path is exact.  NULL, or why the input is refused; a call without a dense group is not refused.
const char *plan_filtered_each_dense(int64_t mcode, int64_t chunks, int64_t k, int64_t skip, int64_t min_group, bool compact, int native, const int64_t *ids,
                                     const int64_t *counts, const uint8_t *exact, size_t nq, EachDensePlan &p);
// The batched form of that run (DESIGN.md 4.9 "Dense exact path, per-query filters: batched"): a BATCH is a run of consecutive steps
// of one gathered chunk whose blocks, packed one behind the other, fit the run's dd block; one k_dense_seg launch contracts every
// tile of a batch and one k_select_seg launch folds its blocks into the best lists (dense_seg.hip).  Step s's block is row-major, one
// row per query of the step, leading dimension = the step's columns.  lantern_gpu_plan_filtered_each_dense_batches shows the plan.
enum EachBatchWhy : uint32_t
{
    kEachBatchTaken = 0,
    kEachBatchNoRun,     // the call makes no dense run (EachDensePlan::why says why)
    kEachBatchOperands,  // not f32 rows under l2sq / cos contracted as stored: f16 / i8 rows (native or dequantised), popcount metrics
    kEachBatchWideRow    // rows of more than 65 536 chunks: a tile's byte offsets would leave 31 bits
};
struct EachDenseBatch
{
    uint32_t step0, n_steps, floats;  // steps [step0, step0 + n_steps) of EachDensePlan::steps; the floats of their packed blocks
    uint32_t tile0, tiles, skinny;    // its entries of the call's tile table; how many of them are skinny tiles
    uint32_t query0, queries;         // its entries of the call's selection table: one per (step, query)
};
struct EachDenseBatches
{
    EachBatchWhy                why = kEachBatchNoRun;
    uint64_t                    capacity = 0;        // floats a batch may pack
    std::vector<EachDenseBatch> batches;             // in plan order; none crosses a chunk
    std::vector<uint32_t>       off, skinny, big;    // per step: its block's offset inside its batch's packed matrix, its tiles in each shape
    size_t tiles() const { return batches.empty() ? 0 : batches.back().tile0 + batches.back().tiles; }
    size_t queries() const { return batches.empty() ? 0 : batches.back().query0 + batches.back().queries; }
};
// pure, as plan_filtered_each_dense.  dd_floats: the capacity, 0: the plan's own dd block (every step fits that one alone).  NULL, or
// why the input is refused (a capacity that a step alone exceeds); a run that is not batched is not refused (why != kEachBatchTaken)
const char *plan_each_dense_batches(const EachDensePlan &p, uint64_t dd_floats, EachDenseBatches &b);
// the two device tables of a taken batch plan, for the whole call: tiles [tiles()] (entries of a step adjacent, column tile major) and
// selection entries [queries()]
struct SegTile;
struct SegQuery;
void each_dense_seg_tables(const EachDensePlan &p, const EachDenseBatches &b, SegTile *tiles, SegQuery *queries);
// what a run is given beside its plan, and what it reports: batches NULL (or not taken) -- the per-step run; else the batched one, from
// the two tables on the device.  launches: lantern_gpu_last_filtered_each_dense_launches' four words
struct EachDenseRun
{
    const EachDenseBatches *batches = nullptr;
    const SegTile          *d_tiles = nullptr;
    const SegQuery         *d_queries = nullptr;
    uint32_t                launches[ 4 ] = {};
};

// One run of a taken plan.  d_list: L; d_q: the dense queries' rows, gathered in the plan's order.  Result (device), per dense query:
// slots[k + skip] ascending by (exact-order distance, slot), dists alike.  `answers`, queued behind the certificate and in front of
// the run's ONE wait for `st`, is given the device flags -- [q] 1: certified, [nq] != 0: a cosine row norm of ANY segment is outside the
// certificate's range, which refuses every query of the run -- or NULL: every query is certified (exact keys).  `refused`: the
// dense queries (positions in the plan's order) whose rows of the result are not the answer; the caller recomputes them.
using EachDenseAnswers = std::function<bool(const uint32_t *d_flags)>;
bool filtered_each_dense_device(const EachDensePlan &p, const uint4 *d_base, const uint32_t *d_list, const uint4 *d_q, uint32_t *d_slots, float *d_dists,
                                hipStream_t st, const EachDenseAnswers &answers, std::vector<uint32_t> &refused, EachDenseRun *run = nullptr);

// Exact k-NN of nq device-resident query rows over nb device-resident base rows (both `chunks` uint4 per row).
// Result (device): slots[nq][k] ascending by (exact-order distance, slot), dists[nq][k].
// pq (mcode M_L2SQ_PQD / M_COS_PQD): d_base is the CODE rows of a compact pq index, pq->row_bytes each, and `chunks` those of a decoded
// row; nothing of nb x chunks x 16 bytes is allocated (lantern_gpu_set_exact_compact).
// adc (pq only; NULL or a taken plan_exact_adc): every contraction step pre-selects by table lookups (k_scan_adc) instead of k_dense_pq.
struct DensePqRows;
struct ExactAdcPlan;
bool exact_knn_device(int mcode, uint32_t chunks, const uint4 *d_base, size_t nb, const uint4 *d_q, size_t nq, size_t k, uint32_t *d_slots,
                      float *d_dists, hipStream_t st, const DensePqRows *pq = nullptr, const ExactAdcPlan *adc = nullptr);

// lantern_gpu_exact_search on a compact pq index (DESIGN.md 4.5 "Compact pq indexes"): does the call run on the code rows, and if not
// why.  lantern_gpu_plan_exact_compact shows it without a device; the entry point and lantern_gpu_exact_compact decide through it.
enum ExactCompactWhy : uint32_t
{
    kExactCompactTaken = 0,
    kExactCompactOff,        // lantern_gpu_set_exact_compact is 0
    kExactCompactExpanded,   // the index is not compact: stored rows, as ever
    kExactCompactNoDecode,   // subvectors that are not whole 16-byte chunks (pqd_inv == 0): the call expands the index
    kExactCompactMetric      // not l2sq / cos over f32 rows
};
struct ExactCompactPlan
{
    ExactCompactWhy why = kExactCompactOff;
    int             mcode = 0;           // taken: the decoding metric code the run is planned with
    ExactKnnPlan    knn;                 // taken: the run
    size_t          run_bytes = 0;       // taken: every device byte the certified run allocates (aux + dd + cand)
    size_t          fallback_bytes = 0;  // taken: one decoded chunk of base rows, allocated only if the certificate refuses a query
    size_t          expand_bytes = 0;    // not taken on a compact index: the f32 row block the call decodes into (nb rows)
};
const char *plan_exact_compact(int64_t mcode, int64_t chunks, int64_t nb, int64_t nq, int64_t k, bool on, bool compact, uint32_t pqd_inv, uint32_t pq_S16,
                               int fused, ExactCompactPlan &p);

// The same call's pre-selection by table lookups (DESIGN.md 4.5 "Compact pq indexes: ADC pre-selection"; lantern_gpu_set_exact_adc):
// does a call that runs on the code rows scan them against per-query tables (k_scan_adc, dense_adc.hip) instead of contracting them
// (k_dense_pq), and if not why.  lantern_gpu_plan_exact_adc shows it without a device; the entry point decides through it.
enum ExactAdcWhy : uint32_t
{
    kExactAdcTaken = 0,
    kExactAdcOff,          // lantern_gpu_set_exact_adc is 0
    kExactAdcNotCompact,   // plan_exact_compact does not take the call: there are no code rows to scan
    kExactAdcManyQueries,  // nq above the switch's value
    kExactAdcShape,        // more than 128 subvectors or 256 centroids, or subvectors that do not fill the row
    kExactAdcBudget        // the queries' tables exceed kAdcTablesMax
};
constexpr size_t kAdcTablesMax = (size_t)256 << 20;  // 2730 queries at 96 subvectors; pooled, so it stays with the process
struct ExactAdcPlan
{
    ExactAdcWhy why = kExactAdcOff;
    uint32_t    S16 = 0;          // taken (as all below): rows of a query's table -- the subvectors rounded up to 16
    uint32_t    T = 0;            // queries of a scanning workgroup: the largest of 4, 2, 1 whose tables fit kAdcScanLdsMax
    uint32_t    block = 0;        // its threads
    size_t      lds_bytes = 0;    // its dynamic LDS: the T tables
    size_t      table_bytes = 0;  // the call's table block: [nq][S16][ADC_LUT_STRIDE] f32
};
// the arguments of plan_exact_compact, then the switch's value, the index's subvectors and centroids
const char *plan_exact_adc(int64_t mcode, int64_t chunks, int64_t nb, int64_t nq, int64_t k, bool on, bool compact, uint32_t pqd_inv, uint32_t pq_S16, int fused,
                           int64_t max_queries, int64_t S, int64_t C, ExactAdcPlan &p);

}  // namespace lgpu
