// filtered_search.hpp -- what the host units of filtered search share: the handle checks (filter.hip), one launch of either kernel with
// its per-query table (filtered_search.cpp), and the two dense routes (filtered_dense.hip).  The plan is filtered_plan.hpp's.
#pragma once
#include <string>
#include <vector>

#include "dense.hpp"
#include "filter.hpp"
#include "filtered_plan.hpp"
#include "index.hpp"

namespace lgpu {

// ---- handles (filter.hip) ------------------------------------------------------------------------------------------------------------
extern const char *const kNotAFilter;
// (lantern_gpu_filter_t stays an incomplete type: a handle is a Filter, recognised by its magic word)  NULL -> *e
Filter *FF(const lantern_gpu_filter_t *f, usearch_error_t *e);
// Why `f` cannot serve a search of `ix` as it stands now; empty: it can.
std::string filter_mismatch(const Index *ix, const Filter *f);

// ---- one launch (filtered_search.cpp) ------------------------------------------------------------------------------------------------
// the per-query form's table of one launch: host bytes that go into the scratch of the launch's slot, and where in them the launch's
// descriptors and selection list lie
constexpr size_t kNoTable = ~(size_t)0;
struct EachTable
{
    const char *host;
    size_t      bytes, descs_at, select_at;
    size_t      params_at = kNoTable;  // the per-query-parameter form: where the launch's rows {k, expansion, skip, C} lie
};
struct EachTables { EachTable walk, exact; };
// bytes of the host block each_tables lays a call's tables out in (`params`: with the per-query-parameter form's rows)
inline size_t each_table_bytes(size_t nq, bool params = false) { return nq * (sizeof(FilterDesc) + 4) + 16 + (params ? nq * 16 + 16 : 0); }
// The tables of a call of nq queries into `blk` (each_table_bytes(nq, rows) bytes, page-locked or pageable): walk selection list |
// parameter rows (by query; `rows` NULL: none) | descriptor table (by query) | exact selection list -- each launch copies its list and
// the tables in one piece.  Query i's descriptor is filters[i]'s (a NULL entry: unfiltered) or, filters NULL, `one`'s for every query.
EachTables each_tables(const Index *ix, char *blk, size_t nq, const Filter *const *filters, const Filter *one, const std::vector<uint32_t> &walk,
                       const std::vector<uint32_t> &exact, const uint32_t *rows);
// ONE launch of either kernel over a.frame.nq queries, `a` shaped by the plan: the grid, the launch slot (which orders the launch
// after inserts and holds the walk's visited bitmaps), the per-query table if there is one, the ticket, the launch and its count.
// Returns the grid; < 0 -> ix->err.
int filtered_launch(Index *ix, bool exact, FilteredArgs &a, size_t lds, hipStream_t stream, const EachTable *tbl = nullptr);

// ---- the dense routes (filtered_dense.hip; DESIGN.md 4.9 "Dense exact path") -----------------------------------------------------------
// One single-filter call on the dense route, planned by `plan` (taken).  `a`, `lds`: the exact launch's arguments and carve, which the
// recomputed queries run with.  Waits for the stream (the certificate's flags cross to the host).
bool filtered_dense_locked(Index *ix, const Filter *f, const FilteredDensePlan &plan, int native, const uint4 *d_q, size_t nq, size_t k, size_t skip,
                           const SearchOut &out, FilteredArgs &a, size_t lds, hipStream_t stream);
// The dense groups of one per-query-filter call, planned by `plan` (taken): L, the tables and the gathered queries into the dense
// scratch block, the segmented run with the answer kernel queued in front of its wait.  refused: the call's queries (original
// indices) the certificate refused, which the call's exact launch answers.  Waits for the stream, once.
bool filtered_each_dense_locked(Index *ix, const Filter *const *filters, const EachDensePlan &plan, const uint4 *d_q, size_t k, size_t skip,
                                const SearchOut &out, hipStream_t stream, std::vector<uint32_t> &refused);

}  // namespace lgpu
