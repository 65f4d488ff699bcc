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
    int      kind = 0;            // DenseOperands::kind: 0 f32 (or bit) rows, 1 / 2 f16 / i8 rows as stored
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
// One run of a taken plan.  d_list: L; d_q: the dense queries' rows, gathered in the plan's order.  Result (device), per dense query:
// slots[k + skip] ascending by (exact-order distance, slot), dists alike.  `answers`, queued behind the certificate and in front of
// the run's ONE wait for `st`, is given the device flags -- [q] 1: certified, [nq] != 0: a cosine row norm of ANY segment is outside the
// certificate's range, which refuses every query of the run -- or NULL: every query is certified (exact keys).  `refused`: the
// dense queries (positions in the plan's order) whose rows of the result are not the answer; the caller recomputes them.
using EachDenseAnswers = std::function<bool(const uint32_t *d_flags)>;
bool filtered_each_dense_device(const EachDensePlan &p, const uint4 *d_base, const uint32_t *d_list, const uint4 *d_q, uint32_t *d_slots, float *d_dists,
                                hipStream_t st, const EachDenseAnswers &answers, std::vector<uint32_t> &refused);

// Exact k-NN of nq device-resident query rows over nb device-resident base rows (both `chunks` uint4 per row).
// Result (device): slots[nq][k] ascending by (exact-order distance, slot), dists[nq][k].
bool exact_knn_device(int mcode, uint32_t chunks, const uint4 *d_base, size_t nb, const uint4 *d_q, size_t nq, size_t k, uint32_t *d_slots,
                      float *d_dists, hipStream_t st);

}  // namespace lgpu
