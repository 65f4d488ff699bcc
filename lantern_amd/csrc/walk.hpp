// walk.hpp -- the HNSW graph walk as one workgroup's cooperative device functions.
//
// Follows usearch's search_for_one_ / search_to_find_in_base_ / search_to_insert_ / refine_ as
// Lantern reaches them through usearch_search_ef (lantern_hnsw/src/hnsw/scan.c:220-228) and
// usearch_add (lantern_hnsw/src/hnsw/build.c:128), re-shaped for a 64-lane machine:
//
//  * usearch keeps two structures per search: `next` (a heap of candidates) and `top` (the ef best
//    so far).  Under the total order (distance, slot) an element evicted from `top` can never be
//    expanded later, so a single sorted list with an "expanded" bit per entry is equivalent:
//    "pop the best candidate" = "first unexpanded entry"; the walk ends when there is none.
//  * all unvisited neighbours of the popped node are evaluated at once (one G-lane group per row,
//    several rows in flight per wave), then merged into the list.  The result equals inserting them one by
//    one: the list ends up holding the ef smallest of (old list U new), whatever the order of insertion.
//    Two forms of the list: in one wave's REGISTERS (search_level_reg: ef <= 128, the usual case; a hop's
//    bookkeeping split over two waves) and in LDS with a parallel rank-merge (search_level: any ef).
//  * the visited set is an open-addressing hash set in LDS (four-slot buckets) that spills to a bitmap in HBM
//    owned by the workgroup when three quarters full (visit_test_and_set / hop_is_new below).
//
// All functions must be called by every thread of the workgroup (they contain barriers).
#pragma once
#include <type_traits>

#include "device_common.hpp"

namespace lgpu {

// scalar slots in LDS
enum { S_POS = 0, S_NNEW, S_CNT, S_ANY, S_BAD, S_CUR, S_CURD, S_CHANGED, S_VISCNT, S_SPILL, S_QN2, S_NNEW0, S_NNEW1, S_ANY0, S_ANY1,
       S_FRONT = 16, S_WORST = 20,  // two u64 each (by hop parity): search_level_reg's hand-off from the list wave to the visit wave
       S_MASK = 24,                 // two u64 (by hop parity): walk_spec.hpp's "which neighbours of the hop were new"
       S_SCALARS = 28,
       // the int8 screen of search_level_reg and of the screened greedy_descent, in slots that walk leaves alone: the screened hop's survivor count, the walk's rejected rows,
       // and (set by k_search before the walk) two u64: View::screen and View::screen_meta -- in LDS rather than in scalar registers,
       // which the hop loop has none of to spare
       S_NSURV = S_ANY0, S_NREJ = S_ANY1, S_SCREEN = S_MASK,
       S_NTEST = 15 };  // TALLY (k_insert's screened walks): the rows the walk put to the screen test
// S_QN2: ||query||^2 as float bits (cosine metrics; set by the kernel before a walk: device_common.hpp "cached row norms")

struct WalkLds
{
    uint4    *q;        // the query row (chunks uint4)
    uint64_t *keys;     // current list   (ef_cap)
    uint64_t *keys2;    // merge target   (ef_cap)
    uint64_t *newkeys;  // keys of this hop's new neighbours (cap_max)
    uint64_t *sorted;   // the same, sorted                  (cap_max); search_level_reg, greedy_descent: the screened hop's / step's survivors (u32)
    uint32_t *newids;   // unvisited neighbour slots         (cap_max)
    int      *scal;     // S_* scalars
    uint32_t *vis;      // visited hash set (vis_slots entries, any multiple of 4; 0 = the HBM bitmap only)
    uint32_t  vis_slots;
    uint32_t *touched;  // diagnostic instantiations only (PROF): one bit per row of the index, set when ANY query of the launch
                        // evaluates the row (lantern_gpu_search_unique_rows); never read, and never set, elsewhere
    // diagnostic instantiations only (PROF; lantern_gpu_search_row_trace): THIS query's memory-object trace, in the order the walk
    // asks for them -- a row evaluation is the row's slot, an adjacency list read is the node's slot | TRACE_LIST0 (level 0) or
    // | TRACE_LISTU (an upper level).  trace_count is bumped atomically (the lanes of a hop append side by side); entries beyond
    // trace_cap are counted, not stored.  The input of the cache model behind bench.py's frac_dram_model.
    uint32_t *trace, *trace_count;
    uint32_t  trace_cap;
    // the UNDO LOG of the workgroup's HBM visited bitmap (VisUndo below): undo_cap entries behind the bitmap's words
    uint32_t *undo;
    uint32_t  undo_cap;
};
constexpr uint32_t TRACE_LIST0 = 0x80000000u, TRACE_LISTU = 0xC0000000u;

// a workgroup's slab of a launch's `bitmaps`: its visited bitmap (bm_words words) with its undo log (kVisUndoWords) behind it
__device__ __forceinline__ uint32_t *vis_slab(uint32_t *bitmaps, uint32_t bm_words) { return bitmaps + (size_t)blockIdx.x * (bm_words + kVisUndoWords); }

template <bool PROF> __device__ __forceinline__ void trace_append(const WalkLds &s, uint32_t entry)
{
    if constexpr(PROF) {
        if(s.trace) {
            const uint32_t p = atomicAdd(s.trace_count, 1u);
            if(p < s.trace_cap) s.trace[ p ] = entry;
        }
    } else {
        (void)s;
        (void)entry;
    }
}

// PROF: record that row `id` was evaluated by this launch (the union over the launch's queries = the rows the launch needs at
// least once from HBM: the cold-miss lower bound of its DRAM traffic)
template <bool PROF> __device__ __forceinline__ void mark_touched(const WalkLds &s, uint32_t id)
{
    if constexpr(PROF) {
        if(s.touched) atomicOr(&s.touched[ id >> 5 ], 1u << (id & 31));
        trace_append<PROF>(s, id);
    } else {
        (void)s;
        (void)id;
    }
}

// the first operand of a (query, row) evaluation: the query row in LDS -- or, for ADC over PQ codes, just the chunk index (the
// table sits at the start of LDS: device_common.hpp AdcQuery)
template <int METRIC> __device__ __forceinline__ auto walk_query(const WalkLds &s)
{
    if constexpr(METRIC >= M_ADC && METRIC < M_PQD) return AdcQuery{};
    else return (const uint4 *)s.q;
}

// Carve the workgroup's dynamic LDS.  Every offset stays 16-byte aligned.
__device__ __forceinline__ unsigned char *carve_walk(unsigned char *p, WalkLds &s, uint32_t chunks, uint32_t ef_cap, uint32_t cap_max,
                                                     uint32_t vis_slots = 0)
{
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    s.q = (uint4 *)p;            p += (size_t)chunks * 16;
    s.keys = (uint64_t *)p;      p += up16((size_t)ef_cap * 8);
    s.keys2 = (uint64_t *)p;     p += up16((size_t)ef_cap * 8);
    s.newkeys = (uint64_t *)p;   p += up16((size_t)cap_max * 8);
    s.sorted = (uint64_t *)p;    p += up16((size_t)cap_max * 8);
    s.newids = (uint32_t *)p;    p += up16((size_t)cap_max * 4);
    s.scal = (int *)p;           p += S_SCALARS * 4;
    s.vis = (uint32_t *)p;       p += (size_t)vis_slots * 4;
    s.vis_slots = vis_slots;
    return p;
}
__host__ inline size_t walk_lds_bytes(uint32_t chunks, uint32_t ef_cap, uint32_t cap_max, uint32_t vis_slots = 0)
{
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    return (size_t)chunks * 16 + 2 * up16((size_t)ef_cap * 8) + 2 * up16((size_t)cap_max * 8) + up16((size_t)cap_max * 4) + S_SCALARS * 4 +
           (size_t)vis_slots * 4;
}

// ---- visited set ------------------------------------------------------------------------------------------
// usearch keeps a growing hash set of visited slots per search.  Here: an open-addressing hash set in LDS
// (no HBM round trip per hop, nothing to clear in HBM per query) that SPILLS to the workgroup's HBM bitmap once it
// is three quarters full: from then on new slots are recorded in the bitmap (all-zero whenever a walk starts: VisUndo below) and a
// lookup consults both.  With vis_slots == 0 only the bitmap is used.
// multiply-shift onto [0, slots): any table size, so the set can be sized to the LDS a given occupancy leaves
__device__ __forceinline__ uint32_t vis_hash(uint32_t x, uint32_t buckets) { return __umulhi(x * 0x9E3779B1u, buckets); }

// The LDS visited set: open addressing over BUCKETS of four slots (one ds_read_b128 looks at a whole bucket).  A slot id lives
// in the first bucket, counting from its home, that had a free slot when it arrived; buckets never lose entries, so a lookup
// ends at the first bucket that holds the id or still has a free slot.  Insert-only, exact; used by the lanes of wave 0.
struct VisProbe
{
    bool found;  // the id is in the bucket
    int  e;      // a free slot of the bucket (-1: none), searched from slot `rot` on so that lanes spread over the free slots
};
__device__ __forceinline__ VisProbe vis_look(const WalkLds &s, uint32_t bucket, uint32_t x, int rot)
{
    asm volatile("" ::: "memory");  // the bucket is re-read after every CAS
    const uint4    w = ((const uint4 *)s.vis)[ bucket ];
    const uint32_t v[ 4 ] = { w.x, w.y, w.z, w.w };
    VisProbe       r;
    r.found = w.x == x || w.y == x || w.z == x || w.w == x;
    r.e = -1;
#pragma unroll
    for(int i = 3; i >= 0; --i) {
        const int j = (rot + i) & 3;
        if(v[ j ] == EMPTY) r.e = j;
    }
    return r;
}

// ---- the HBM bitmap is kept ALL-ZERO between walks, by undoing instead of clearing [r6] ------------------------------------
// Until round 5 a walk whose LDS set filled up CLEARED its workgroup's whole bitmap before the first bit went in: cap / 8 bytes of
// writes per spilling walk -- 1.25 MB at 10M rows, where at ef = 128 most walks spill: 7.8 GB of writes per 8192-query launch, 7 % of
// the launch's fabric traffic (profiles/r06_bench_line_10Mx768_ef128.json), and 10 % of a 10M-row build's.  Now the bitmap is zero when
// a walk starts (zeroed when it is allocated; every walk leaves it as it found it): the ids a walk records in it are also appended
// to an undo log behind the bitmap, and when the walk ends the visit wave zeroes the words the log names (a word's other bits are
// the same walk's).  A walk that overflows the log clears the whole bitmap at its end, as a spilling walk used to at its spill.
struct VisUndo
{
    uint32_t cnt = 0;      // entries in the log (wave-uniform in the visit wave)
    bool     over = false; // more ids were recorded than the log holds: clear everything at the end
};
// after a filter pass that recorded ids in the BITMAP: `mine` = this lane recorded `id`; newmask = __ballot(mine).  Visit wave only.
__device__ __forceinline__ void undo_record(const WalkLds &s, VisUndo &u, bool mine, uint32_t id, unsigned long long newmask, int lane)
{
    const uint32_t n = (uint32_t)__popcll(newmask);
    if(n == 0 || u.over) return;
    if(u.cnt + n <= s.undo_cap) {
        if(mine) __hip_atomic_store(&s.undo[ u.cnt + (uint32_t)__popcll(newmask & ((1ull << lane) - 1ull)) ], id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        u.cnt += n;
    } else {
        u.over = true;
    }
}
// at the end of a walk, by the visit wave: the bitmap goes back to all-zero.  FRESH_ZERO (the screened search walks, which have no VGPR
// to spare): the zeros of the rare whole-bitmap clear are made where they are stored -- left to itself the compiler keeps a zero uint4
// live through the whole kernel for this one loop and spills it around every row block.
template <bool FRESH_ZERO = false>
__device__ __forceinline__ void undo_apply(const WalkLds &s, uint32_t *bitmap, uint32_t bm_words, const VisUndo &u, int lane)
{
    if(u.over) {
        uint4 *b4 = (uint4 *)bitmap;
        uint32_t z = 0;
        if constexpr(FRESH_ZERO) asm volatile("" : "+v"(z));
        for(uint32_t i = (uint32_t)lane; i < bm_words / 4; i += 64) b4[ i ] = make_uint4(z, z, z, z);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // the clears reach L2 before the next walk's atomics on these words
    } else if(u.cnt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the log's own stores have left
        for(uint32_t i = (uint32_t)lane; i < u.cnt; i += 64) {
            const uint32_t id = __hip_atomic_load(&s.undo[ i ], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)atomicAnd(&bitmap[ id >> 5 ], 0u);  // (an atomic, like the atomicOr's that set the bits: same path to L2, in order)
        }
    }
}

// true if `x` was already visited; otherwise records it.  Called by the lanes of wave 0 only.
__device__ __forceinline__ bool visit_test_and_set(WalkLds &s, uint32_t *bitmap, uint32_t x, bool spilled)
{
    if(s.vis_slots) {
        const uint32_t nb4 = s.vis_slots >> 2;
        uint32_t       b = vis_hash(x, nb4);
        for(;;) {
            const VisProbe p = vis_look(s, b, x, (int)(threadIdx.x & 3));
            if(p.found) return true;
            if(p.e < 0) {  // a full bucket: the id may live further on
                b = b + 1 == nb4 ? 0u : b + 1;
                continue;
            }
            if(spilled) break;  // not in the LDS set (read-only once spilled): the bitmap decides
            const uint32_t cur = atomicCAS(&s.vis[ 4 * b + (uint32_t)p.e ], EMPTY, x);
            if(cur == EMPTY) return false;  // recorded; the caller counts the slots it added (one ballot per pass)
            if(cur == x) return true;
            // another lane took that slot in the meantime: look at the bucket again
        }
    }
    const uint32_t bit = 1u << (x & 31);
    return (atomicOr(&bitmap[ x >> 5 ], bit) & bit) != 0;
}

// One lane's share of a hop's visited filter: is neighbour `nb` (EMPTY = no neighbour) new?  The common case is straight-line
// code for the whole wave -- one bucket read, one CAS -- and only lanes that met a full bucket or lost a slot to another lane
// take the probing loop (its divergent control flow costs more scalar instructions than the LDS accesses themselves).
__device__ __forceinline__ bool hop_is_new(WalkLds &s, uint32_t *bitmap, uint32_t nb, bool spilled)
{
    bool isnew = false;
    if(s.vis_slots && !spilled) {
        const bool     valid = nb != EMPTY;
        const uint32_t b = vis_hash(valid ? nb : 0u, s.vis_slots >> 2);
        const VisProbe p = vis_look(s, b, nb, (int)(threadIdx.x & 3));
        const bool     attempt = valid && !p.found && p.e >= 0;
        uint32_t       cur = nb;
        if(attempt) cur = atomicCAS(&s.vis[ 4 * b + (uint32_t)(p.e & 3) ], EMPTY, nb);
        isnew = attempt && cur == EMPTY;
        const bool unsettled = valid && !p.found && !isnew && !(attempt && cur == nb);
        if(__ballot(unsettled) != 0ull) {
            if(unsettled) isnew = !visit_test_and_set(s, bitmap, nb, false);
        }
    } else if(nb != EMPTY) {
        isnew = !visit_test_and_set(s, bitmap, nb, spilled);
    }
    return isnew;
}

__device__ __forceinline__ int lower_bound_keys(const uint64_t *a, int n, uint64_t k)
{
    int lo = 0, hi = n;
    while(lo < hi) {
        int mid = (lo + hi) >> 1;
        if(a[ mid ] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- merge helpers: four adjacent lanes (a quad) share the LDS reads of one key's position --------------------------
// sum over the quad (every lane of the quad gets it): two DPP adds
template <int L> __device__ __forceinline__ int quad_sum(int x)  // L = 2 or 4 cooperating lanes
{
    uint32_t v = (uint32_t)x;
    v = v + dpp_take<0xB1, 0xF>(v);
    if(L == 4) v = v + dpp_take<0x4E, 0xF>(v);
    return (int)v;
}
// #{j < n : a[j] < k} with the reads split over the quad (sub = lane & 3): 16-byte reads of two keys, all of a lane's reads
// independent of one another (one LDS round trip per eight keys of the lane's share)
template <int L> __device__ __forceinline__ int quad_count_below(const uint64_t *a, int n, uint64_t k, int sub)
{
    const uint4 *a4 = (const uint4 *)a;  // a is 16-byte aligned (carve_walk)
    const int    pairs = n >> 1;
    int          c = 0;
    for(int p = sub; p < pairs; p += L) {
        const uint4    w = a4[ p ];
        const uint64_t k0 = ((uint64_t)w.y << 32) | w.x, k1 = ((uint64_t)w.w << 32) | w.z;
        c += (k0 < k) + (k1 < k);
    }
    if((n & 1) && sub == 0) c += a[ n - 1 ] < k;
    return quad_sum<L>(c);
}
// lower_bound over the sorted a[0..n) as two rounds of independent reads instead of log2(n) dependent ones: first the last
// key of every block of eight (how many whole blocks lie below k), then the eight keys of the block k falls into
template <int L> __device__ __forceinline__ int quad_lower_bound(const uint64_t *a, int n, uint64_t k, int sub)
{
    const int nb = (n + 7) >> 3;
    int       c = 0;
    for(int b = sub; b < nb; b += L) {
        const int last = 8 * b + 7 < n ? 8 * b + 7 : n - 1;
        c += a[ last ] < k;
    }
    const int blk = quad_sum<L>(c);
    if(blk >= nb) return n;
    const int lo = 8 * blk, len = n - lo < 8 ? n - lo : 8;
    int       d = 0;
    for(int j = sub; j < len; j += L) d += a[ lo + j ] < k;
    return lo + quad_sum<L>(d);
}

// ---- search_for_one_: greedy descent over levels (begin, end] ---------------------------------------
// Returns the closest slot (same value in every thread).  D counts distance evaluations.
//
// SCREEN (k_search's screened instantiations: search_kernel.hpp), in a launch that carved the planes' block (s.scal[S_SCREEN] set) and
// asks for it (screen_descent = SearchArgs::screen_descent): a step's listed rows go through the int8 screen of the level-0 hops
// (hop_distances_screened below, as it stands) at radius = the best distance when the step starts, and only the rows it cannot reject are
// read in f32 -- all of a step's survivors requested before the first is consumed (hop_distances: two rows per group), by the chain
// of group_dist_n, same bits.  A rejected row's f32 distance is strictly above that radius; the scan takes a row only if it is strictly
// below the running best, which is never above the radius: the rejected row could not have been taken, and nothing else changes.  D
// counts every listed row; the rejected ones go to s.scal[S_NREJ] with the hops' (lantern_gpu_search_screen_stats).
// LDS, screened step: the distances are the 64-bit keys of the hop (s.newkeys[i] = make_key(d, id); ~0 for a rejected row, whose
// key_dist is a NaN: below nothing) instead of floats in the same words; the survivors' positions are in s.sorted; S_NSURV / S_NREJ
// (= S_ANY0 / S_ANY1, which only the LDS-list walk uses) and S_SCREEN (= S_MASK, walk_spec.hpp's) share no word with S_NNEW, S_CUR,
// S_CURD, S_CHANGED.
template <int METRIC, int G> __device__ __forceinline__ void descent_distances_screened(const View &v, WalkLds &s, int nn, float qn2);  // (behind hop_distances_screened)
template <int METRIC, int G, bool PROF = false, bool SCREEN = false>
__device__ uint32_t greedy_descent(const View &v, WalkLds &s, uint32_t start, int begin_level, int end_level, uint32_t &D, uint32_t screen_descent = 0)
{
    static_assert(!SCREEN || ((METRIC == M_L2SQ || METRIC == M_COS) && !PROF), "the screen serves the f32 l2sq and cosine walks");
    const int tid = threadIdx.x, T = blockDim.x, g = tid / G, gl = tid % G, NG = T / G;
    float *newd = (float *)s.newkeys;  // reuse: one f32 per neighbour
    const float qn2 = __int_as_float(s.scal[ S_QN2 ]);
    const bool  screen_on = SCREEN && screen_descent != 0 && ((const uint64_t *)&s.scal[ S_SCREEN ])[ 0 ] != 0;
    if(g == 0) {
        float d = group_dist_n<METRIC, G>(walk_query<METRIC>(s), row_of_m<METRIC>(v, start), (int)v.chunks, gl, qn2, row_norm<METRIC>(v, start));
        if(gl == G - 1) { s.scal[ S_CUR ] = (int)start; s.scal[ S_CURD ] = __float_as_int(d); mark_touched<PROF>(s, start); }
    }
    D += 1;
    __syncthreads();
    for(int level = begin_level; level > end_level; --level) {
        for(;;) {
            uint32_t        cur = (uint32_t)s.scal[ S_CUR ];
            uint32_t        cap;
            const uint32_t *list = neighbors_of(v, cur, level, cap);
            // gather the (EMPTY-terminated, hole-free) list: wave 0, one ballot per 64 slots (an LDS atomicMax here is
            // serialised by the compiler into a scalar loop over the lanes)
            if(tid < 64) {
                if(tid == 0) trace_append<PROF>(s, cur | (level > 0 ? TRACE_LISTU : TRACE_LIST0));
                int count = 0;
                for(uint32_t off = 0; off < cap; off += 64) {
                    const uint32_t i = off + (uint32_t)(tid & 63);
                    const uint32_t nb = i < cap ? list[ i ] : EMPTY;
                    if(i < cap) s.newids[ i ] = nb;
                    count += (int)__popcll(__ballot(nb != EMPTY));
                }
                if(tid == 0) {
                    s.scal[ S_NNEW ] = count;
                    if constexpr(SCREEN) s.scal[ S_NSURV ] = 0;  // (the previous step's survivor count was read two barriers ago)
                }
            }
            __syncthreads();
            const int nn = s.scal[ S_NNEW ];
            if(screen_on) {
                if constexpr(SCREEN) descent_distances_screened<METRIC, G>(v, s, nn, qn2);
            } else
            for(int i = g; i < nn; i += NG) {
                const uint32_t id = s.newids[ i ];
                float d = group_dist_n<METRIC, G>(walk_query<METRIC>(s), row_of_m<METRIC>(v, id), (int)v.chunks, gl, qn2, row_norm<METRIC>(v, id));
                if(gl == G - 1) { newd[ i ] = d; mark_touched<PROF>(s, id); }
            }
            D += (uint32_t)nn;
            __syncthreads();
            if(tid == 0) {
                // the sequential scan of search_for_one_: first strictly-closer wins, in list order
                float    best = __int_as_float(s.scal[ S_CURD ]);
                uint32_t bslot = cur;
                int      changed = 0;
                for(int i = 0; i < nn; ++i) {
                    const float d = screen_on ? key_dist(s.newkeys[ i ]) : newd[ i ];
                    if(d < best) { best = d; bslot = s.newids[ i ]; changed = 1; }
                }
                s.scal[ S_CUR ] = (int)bslot;
                s.scal[ S_CURD ] = __float_as_int(best);
                s.scal[ S_CHANGED ] = changed;
            }
            __syncthreads();
            if(!s.scal[ S_CHANGED ]) break;
        }
    }
    uint32_t r = (uint32_t)s.scal[ S_CUR ];
    __syncthreads();
    return r;
}

// ---- search_to_find_in_base_ / search_to_insert_ -----------------------------------------------------
// On return s.keys[0..cnt) holds the result ascending by (distance, slot); returns cnt.
//
// One hop = three phases, three barriers:
//   (1) wave 0 alone, no barrier inside: pop (first unexpanded entry: one ballot per 64 entries), the popped node's
//       neighbour list (ONE 128-byte request), the visited test-and-set (LDS hash set, spilling to the HBM bitmap), the
//       ballot compaction of the new ids into LDS.  The other waves wait at the barrier.
//   (2) all waves: one G-lane group per row, two rows in flight per group -> keys.
//   (3) all waves: rank-merge into the ef-bounded list -- a thread per key, every position computed from the UNSORTED new
//       keys (old key i goes to i + #{new < it}, new key t to #{new < it} + lower_bound(old, it)), so there is no
//       intermediate sort and no barrier inside the phase.
// Round 1 took six barriers per hop, found the pop position with an LDS atomicMin (which the compiler serialises into a
// scalar loop over the active lanes: ~1.4 us per hop on its own) and sorted the new keys before merging; measured with
// the instrumented kernel (scripts/profile_hop_phases.py) the three serial phases cost 3 000 - 4 000 cycles EACH, more
// than the row evaluation of a 128-d hop.  The scalars wave 0 publishes are double-buffered by hop parity, so a wave that
// is slow to read them is never overtaken by the next hop's values.
// PROF (diagnostic instantiations only): thread 0 accumulates shader-clock cycles per phase into prof[0..6): [4] pop, [5] the
// neighbour list's arrival, [0] visited filter + compaction (together: wave 0's section) | [1] wait at the first barrier |
// [2] distances | [3] merge.
// One hop's distance phase: keys of the nnew unvisited neighbours in s.newids -> s.newkeys.  One G-lane group per row, ROWS rows in
// flight per group.  ANY: also raise *any_slot when a key beats `worst` (the LDS-list walk skips its merge otherwise).  SEL: evaluate
// only the nnew entries sel[0..nnew) name (positions in s.newids / s.newkeys: the survivors of the int8 screen), all when sel is NULL.
template <int METRIC, int G, int ROWS, bool ANY, bool SEL = false>
__device__ __forceinline__ void hop_distances(const View &v, WalkLds &s, int nnew, float qn2, uint64_t worst, int *any_slot,
                                              const uint32_t *sel = nullptr)
{
    const int tid = threadIdx.x, T = blockDim.x, g = tid / G, gl = tid % G, NG = T / G;
    auto at = [&](int j) { if constexpr(SEL) return sel ? (int)sel[ j ] : j; else return j; };
    // SEL: the positions are read again for the stores rather than kept live across the row loads (the walk has no VGPR to spare)
    auto reread = [&]() { if constexpr(SEL) asm volatile("" ::: "memory"); };
    if constexpr(ROWS > 2) {
        for(int i = g; i < nnew; i += ROWS * NG) {
            decltype(row_of_m<METRIC>(v, 0u)) rows[ ROWS ];
            uint32_t     ids[ ROWS ];
            float        n2[ ROWS ], d[ ROWS ];
#pragma unroll
            for(int r = 0; r < ROWS; ++r) {
                const int j = i + r * NG;
                ids[ r ] = s.newids[ at(j < nnew ? j : i) ];
                rows[ r ] = row_of_m<METRIC>(v, ids[ r ]);
                n2[ r ] = row_norm<METRIC>(v, ids[ r ]);
            }
            group_distR_n<METRIC, G, ROWS>(walk_query<METRIC>(s), rows, (int)v.chunks, gl, qn2, n2, d);
            if(gl == G - 1) {
                bool any = false;
                reread();
#pragma unroll
                for(int r = 0; r < ROWS; ++r) {
                    const int j = i + r * NG;
                    if(j < nnew) {
                        const uint64_t k = make_key(d[ r ], ids[ r ]);
                        s.newkeys[ at(j) ] = k;
                        any |= k < worst;
                    }
                }
                if(ANY && any) *any_slot = 1;
            }
        }
    } else
    for(int i = g; i < nnew; i += 2 * NG) {
        const int      j = i + NG;
        const uint32_t id0 = s.newids[ at(i) ];
        const uint32_t id1 = j < nnew ? s.newids[ at(j) ] : id0;
        float          d0, d1;
        group_dist2_n<METRIC, G>(walk_query<METRIC>(s), row_of_m<METRIC>(v, id0), row_of_m<METRIC>(v, id1), (int)v.chunks, gl, qn2, row_norm<METRIC>(v, id0),
                                 row_norm<METRIC>(v, id1), d0, d1);
        if(gl == G - 1) {
            reread();
            uint64_t k0 = make_key(d0, id0);
            s.newkeys[ at(i) ] = k0;
            bool any = k0 < worst;
            if(j < nnew) {
                uint64_t k1 = make_key(d1, id1);
                s.newkeys[ at(j) ] = k1;
                any |= k1 < worst;
            }
            if(ANY && any) *any_slot = 1;
        }
    }
}

// ---- the int8 screen -------------------------------------------------------------------------------------
// The distance phase of a hop of an f32 l2sq or cosine walk whose list is full (radius = the key `worst`): most new rows land
// outside the radius and are read only to be thrown away.  So first every new row's distance is BOUNDED from below on its int8
// screen copy y' = s * c (a quarter of the bytes; View::screen), and only the rows the bound cannot reject pay for the f32 row.
// The bound is formed in INTEGERS against a 16-bit copy of the query: u = 2^-24, e = max(2^-12, (2 chunks + 64) u).
//
// The query's copy (screen_stage_query, once per query, wave 0; tests/test_screen_bound_int.py restates every step):
//   sx = max |x_i| / 32639,  q_i = fl(x_i / sx),  X_i = rint(q_i) in [-32639, 32639] (|q_i| <= 32639 (1 + 2 u): nothing to clip),
//   X = 256 h + l with h = (X + 128) >> 8 in [-127, 127], l = X - 256 h in [-128, 127]: both int8 (32639 = 127 * 256 + 127); x' = sx X (exact reals).
//   delta >= ||x - x'||:  |x_i / sx - X_i| <= |q_i - X_i| + |q_i| u < rho_i + 2^-9 with rho_i = |q_i - X_i| exact in f32 (the fraction of
//   an f32 below 2^16), so delta = fl(sx sqrt(S)) (1 + 2^-10), S = sum (rho_i + 2^-9)^2 in f32 (positive terms: within 64 u of the exact
//   sum; a quotient flushed below the normal range moves rho_i by 2^-150, inside the slack 2^-9 - 32640 u).  Scale-free: no term
//   underflows whatever sx is.  sum X^2 = 65536 sum h^2 + 512 sum h l + sum l^2 reaches 2^41 at d = 2000: the three sums are int32
//   (<= 2000 * 128^2 < 2^25), combined in double, exact.  ||x'||^2 = sx^2 sum X^2 =: P.
//   A query with a non-finite value, max |x| = 0 or a scale outside the range (l2sq: screen_l2_scale_ok(sx); cosine: sx normal) publishes
//   zero planes and delta = +inf: it rejects nothing, as a cosine query whose norm is outside screen_cos_norm_ok.
// The row's sums (eight lanes per row): Ih = <h, c>, Il = <l, c> and, l2sq, C2 = <c, c> by v_dot4_i32_i8, three per screen word.  A lane
//   sees at most 256 values (d = 2000): each of its sums is <= 256 * 128 * 127 < 2^22; an eight-lane sum is <= 2000 * 128 * 127 < 2^25: int32
//   holds them and no order of summation matters.  I = 256 Ih + Il = <X, c> reaches 2000 * 32639 * 127 = 8.3e9 and does NOT fit int32:
//   it is formed in double (exact) and rounded to f32 once, fI = I (1 + u).
// l2sq (r >= ||y - y~||, k_fill_screen: in double, rounded up, against the F32 products y~_i = fl(s c_i); +inf for rows with non-finite
//   values or a zero / subnormal scale):  ||x - y|| >= ||x' - y~|| - delta - r  (triangle inequality, twice), and with y' = s c exact,
//   Q = ||y'||^2 = s^2 C2, A = ||x' - y'||:   A^2 = P - 2 sx s I + Q   exactly.
//   eta.  ||y~ - y'|| <= u ||y'||, so ||x' - y~||^2 >= A^2 - 2 A u ||y'|| >= A^2 - u (2 P + 3 Q)  (2 a b <= a^2 + b^2, A^2 <= 2 (P + Q)).
//   The f32 value d' = fl(fl(P~ - R~) + Q~): P~ = fl(fl(sx sx) fl(sum X^2)) errs by 3 u P, R~ = fl(fl(2 fl(sx s)) fI) by 3 u |R| <= 3 u
//   (P + Q) (|R| = 2 sx s |I| <= 2 sqrt(P Q)), Q~ = fl(fl(s s) fl(C2)) by 3 u Q, the two additions by u (2 P + Q) and 2 u (P + Q) --
//   to first order, all scales inside screen_l2_scale_ok, so nothing under- or overflows: |d' - A^2| <= (10 P + 9 Q) 1.01 u.  Together
//   ||x' - y~||^2 >= d' - 13.2 u (P + Q) >= d' - eta,  eta = 16 u fl(P~ + Q~).  (The expansion cancels where x ~ y: there d' - eta < 0
//   and the row is kept.)  For a row near or beyond the radius d' is of the order of P + Q: eta takes about 1e-6 of it, no rejections.
//   LB = max(0, sqrt(max(0, d' - eta)) (1 - e) - r - delta)^2 <= ||x - y||^2: the subtraction, the root, the product and the two
//   subtractions round by 5 u, far inside (1 - e); and the device's f32 distance d of the row is within (1 - e) of its exact value, e
//   being far above the rounding of its sum.  A row is rejected iff LB (1 - e) > dist(worst) -- strictly, and a NaN anywhere fails the
//   test -- so a rejected row's d is strictly above the radius: its exact key could not have entered the list, and since the
//   radius only shrinks it never can.  Its key becomes ~0 (above every radius: the visit wave's choice and the list wave's merge
//   skip it, as they would skip the exact key).  Survivors get the exact evaluation of hop_distances, same chain, same tree, same
//   bits (the caller runs it over the survivors, s.sorted[0..ns), ns returned).
// cosine (the device's distance is d = fl(1 - fl(ab / fl(ra rb))): ab the 64-lane chain of <x, y>, ra = qn2 and rb = norm2[slot] the
// rooted norms; X = ||x||, Y = ||y||, u = 2^-24, m = ceil(chunks / 64) 4 + 6 the length of a 64-lane chain and tree):
//   <x, y> = <x', y~> + <x', y - y~> + <x - x', y> <= <x', y~> + (X + delta) ||y - y~|| + delta Y  (Cauchy-Schwarz), so
//   sigma = <x, y> / (X Y) <= <x', y~> / (X Y) + rho (1 + dq) + dq,   rho >= ||y - y~|| / Y,  dq >= delta / X
//   (rho: k_fill_screen<true>, both norms in double, rounded up; +inf for rows with non-finite values, a zero / subnormal scale, or rb
//   outside screen_cos_norm_ok -- the zero rows among them; dq = fl(delta / ra) (1 + 2^-10), ra = X (1 + a) below).  Where ra and rb are
//   inside screen_cos_norm_ok:
//   (a) the device's similarity.  ab = <x, y> + alpha X Y with |alpha| <= m u (every partial sum of products is at most X Y in
//       magnitude); ra = X (1 + a), rb = Y (1 + b) with |a|, |b| <= (m / 2 + 1) u + 2^-20 (the chain of squares has positive terms;
//       the last term is what squares flushed below the normal range can take); fl(ra rb) and the divide round once each.  With
//       |sigma| <= 1:  |fl(ab / fl(ra rb)) - sigma| <= (2 m + 4) u + 2^-19 =: e1, and the final subtraction is monotone and rounds
//       by at most 2 u:  d >= 1 - sigma - e1 - 2 u.
//   (b) the screen's similarity.  <x', y'> = sx s I exactly, and <x', y~ - y'> <= (X + delta) u ||y'|| with ||y'|| <= 2 Y: 3 u on the
//       similarity scale.  sim8 = fl(fl(fl(fI sx) t) / ra) with the folded constant t = fl(s / rb) = (s / Y)(1 + tau), |tau| <= |b| + u:
//       four roundings and |a|, |tau| relative to a value of magnitude at most 2 (1 + dq) (no step leaves the normal range: sx |I| >=
//       2^-126 unless I = 0):  |sim8 - sx s I / (X Y)| <= 9 u + 2.1 (|a| + |b| + u) =: e2.
//   (c) the test's own f32 steps (1 + dq, rho times that, (sim8 + it) + dq, + e, 1 - that, - e: values of magnitude <= 4 wherever a row
//       can be rejected) round by at most 24 u together.
//   At 128 <= chunks <= 500 (m <= 38): e1 + 2 u + 3 u + e2 + 24 u < 600 u < 8192 u = 2^-11 = 2 e, so with u_ = sim8 + rho (1 + dq) + dq
//   + e:  1 - u_ - e <= 1 - sigma - e1 - 2 u <= d.  The (2 chunks + 64) 2^-24 arm of e keeps the inequality for longer rows (both e1 and
//   e2 grow by less than chunks u each).  A row is rejected iff 1 - u_ - e > dist(worst), strictly; a NaN anywhere fails the test, and
//   so do rho = +inf and dq = +inf.  Nothing in (a) - (c) depends on the scale of x or of y inside the range.

// The block of the query's planes: behind the visited set, in the launches that carve it (device_common.hpp screen_query_lds_bytes)
__device__ __forceinline__ uint32_t *screen_query_block(const WalkLds &s) { return s.vis + s.vis_slots; }

// Stage the 16-bit copy of the query in s.q (frame_stage has run) into the workgroup's planes block: wave 0, then a barrier.
// Scalars: [0] sx, [1] delta (cosine: dq), [2] ||x'||^2 (l2sq).  qn2: the query's rooted norm (cosine).
template <int METRIC> __device__ __forceinline__ void screen_stage_query(const int tid, const WalkLds &s, uint32_t chunks, float qn2)
{
    uint32_t *const blk = screen_query_block(s);
    if(__builtin_amdgcn_readfirstlane(tid) < 64) {
        const uint32_t lane = (uint32_t)tid, sch = screen_chunks_for(chunks);
        uint32_t       mb = 0;  // max |x_i| as bits: a NaN or an infinity is above every finite value
        for(uint32_t i = lane; i < chunks; i += 64) {
            const uint4 x = s.q[ i ];
            mb = max(max(mb, x.x & 0x7FFFFFFFu), max(max(x.y & 0x7FFFFFFFu, x.z & 0x7FFFFFFFu), x.w & 0x7FFFFFFFu));
        }
        for(int off = 32; off > 0; off >>= 1) mb = max(mb, (uint32_t)__shfl_xor((int)mb, off));
        const float sx = __uint_as_float(mb) / 32639.f;
        const bool  ok = mb < 0x7F800000u && mb != 0u && (METRIC == M_COS ? (sx >= 0x1p-126f && sx <= 0x1p100f) : screen_l2_scale_ok(sx));
        float    S = 0.f;
        uint32_t hh = 0, hl = 0, ll = 0;
        for(uint32_t i = lane; i < 4 * sch; i += 64) {  // query chunk i: word i % 4 of both planes of screen chunk i / 4 (beyond the row: zeros)
            const uint4 x = i < chunks ? s.q[ i ] : make_uint4(0u, 0u, 0u, 0u);
            const float xs[ 4 ] = { __uint_as_float(x.x), __uint_as_float(x.y), __uint_as_float(x.z), __uint_as_float(x.w) };
            uint32_t    hw = 0, lw = 0;
#pragma unroll
            for(int b = 0; b < 4; ++b) {
                const float q = ok ? xs[ b ] / sx : 0.f;
                const float Xf = fminf(fmaxf(__builtin_rintf(q), -32639.f), 32639.f);
                const float rho = __builtin_fabsf(q - Xf) + 0x1p-9f;
                S = __builtin_fmaf(rho, rho, S);
                const int X = (int)Xf, h = (X + 128) >> 8, l = X - 256 * h;
                hw |= ((uint32_t)h & 0xFFu) << (8 * b);
                lw |= ((uint32_t)l & 0xFFu) << (8 * b);
            }
            hh = (uint32_t)dot4_i8(hw, hw, (int)hh);
            hl = (uint32_t)dot4_i8(hw, lw, (int)hl);
            ll = (uint32_t)dot4_i8(lw, lw, (int)ll);
            blk[ 4 + 8 * (i / 4) + i % 4 ] = hw;
            blk[ 8 + 8 * (i / 4) + i % 4 ] = lw;
        }
        S = group_sum<64>(S);
        hh = group_sum<64>(hh), hl = group_sum<64>(hl), ll = group_sum<64>(ll);
        if(lane == 63) {
            float delta = __builtin_inff(), nx2 = 0.f;
            if(ok) {
                delta = (sx * __builtin_sqrtf(S)) * (1.f + 0x1p-10f);
                if constexpr(METRIC == M_COS) delta = (delta / qn2) * (1.f + 0x1p-10f);  // dq (qn2 outside the range: the test is not made)
                nx2 = (sx * sx) * (float)(65536.0 * (double)(int)hh + 512.0 * (double)(int)hl + (double)(int)ll);
            }
            blk[ 0 ] = __float_as_uint(ok ? sx : 0.f);
            blk[ 1 ] = __float_as_uint(delta);
            blk[ 2 ] = __float_as_uint(nx2);
            blk[ 3 ] = 0u;
        }
    }
    __syncthreads();
}

#ifndef LGPU_SCREEN_NB  // uint4 of a screen row a lane requests before it consumes the first: 3 = half a 768-d row, 6 = the whole row (the insertion walks: always 3)
#define LGPU_SCREEN_NB 3
#endif
template <int METRIC, int G, int ROWS, bool TALLY = false>
__device__ __forceinline__ int hop_distances_screened(const View &v, WalkLds &s, int nnew, uint64_t worst, float qn2)
{
    static_assert(METRIC == M_L2SQ || METRIC == M_COS, "the screen serves the f32 l2sq and cosine walks");
    // Eight lanes per screen row, each lane's chunks requested in blocks of NB before the first of a block is consumed: a 768-d row
    // is 48 chunks = six uint4 per lane = two blocks (NB = 3), and a workgroup of 256 lanes takes a hop of up to 32 new rows in one round
    // of groups -- two memory round trips per hop (16-lane groups with two chunks in flight, then a third, over two rounds took four).
    // Rows of up to 125 chunks (d = 2000) take ceil(sch / (8 NB)) blocks, the last one partial; a chunk beyond the row is neither
    // requested nor consumed.  Only exec-mask arithmetic stands between the loads of a block in the instruction stream, and (s, r) is
    // requested ahead of them, in the same block.  The sums are integers: the order of consumption is free.  NB = 6, the whole 768-d row
    // in ONE block, builds with no more spills than NB = 3 did before and was measured: not faster (DESIGN.md 4.3,
    // profiles/screen_block6_ab.jsonl), so NB stays 3.  The insertion walks (TALLY) take 3 whatever the switch says.
    // A screen chunk meets 32 B of the query's planes, 16 B of h then 16 B of l: the eight lanes of a ds_read_b128 service group read
    // addresses 32 B apart (eight bank sets: no conflict), the groups of a wave read the same addresses (broadcast).
    constexpr int GS = 8, NB = TALLY ? 3 : LGPU_SCREEN_NB;
    static_assert(G % GS == 0, "a screen group lies within one wave");
    const int       tid = threadIdx.x, T = blockDim.x, gs = tid / GS, NGS = T / GS;
    int             gsl = tid % GS;
    // (the search walks: the lane's offset into a row is formed HERE.  Left to itself the compiler forms it once per kernel, spills it,
    // and reloads it in front of the row block -- and the wait for a scratch reload is a wait for every load in flight, the list
    // fetched ahead among them)
    if constexpr(!TALLY) asm volatile("" : "+v"(gsl));
    uint32_t *const surv = (uint32_t *)s.sorted;
    // (the two tables are read through global-memory pointers: a pointer fetched from LDS is generic to the compiler, and flat loads
    // count against the LDS reads' counter as well, so every wait for a query chunk would wait for the row block too)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef float    f32x2 __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(1))) u32x4 *ScreenRow;
    typedef const __attribute__((address_space(1))) f32x2 *ScreenMeta;
    auto uniform = [](uint64_t x) {  // a value every lane holds, moved to scalar registers (the hop loop has no VGPR to spare)
        return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x) |
               (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32;
    };
    const ScreenRow  screen = (ScreenRow)uniform(((const uint64_t *)&s.scal[ S_SCREEN ])[ 0 ]);
    const ScreenMeta screen_meta = (ScreenMeta)uniform(((const uint64_t *)&s.scal[ S_SCREEN ])[ 1 ]);
    const uint32_t   chunks = v.chunks, sch = screen_chunks_for(chunks);
    const uint32_t *const blk = screen_query_block(s);
    const uint4 *const    planes = (const uint4 *)(blk + 4);  // [sch][2]: h, l
    for(int j = gs; j < nnew; j += NGS) {
        const uint32_t id = s.newids[ j ];
        const ScreenRow row = screen + (size_t)id * sch;
        const f32x2     meta = screen_meta[ id ];
        int            ih = 0, il = 0, c2 = 0;
        for(uint32_t base = (uint32_t)gsl; base < sch; base += NB * GS) {
            u32x4 y[ NB ];
#pragma unroll
            for(int c = 0; c < NB; ++c)
                if(base + c * GS < sch) y[ c ] = row[ base + c * GS ];
#pragma unroll
            for(int c = 0; c < NB; ++c)
                if(base + c * GS < sch) {
                    const uint4    hq = planes[ 2 * (base + c * GS) ], lq = planes[ 2 * (base + c * GS) + 1 ];
                    const uint32_t w[ 4 ] = { y[ c ].x, y[ c ].y, y[ c ].z, y[ c ].w };
                    const uint32_t hs[ 4 ] = { hq.x, hq.y, hq.z, hq.w }, ls[ 4 ] = { lq.x, lq.y, lq.z, lq.w };
#pragma unroll
                    for(int k = 0; k < 4; ++k) {  // (words beyond the row are zero in the screen row and in the planes)
                        ih = dot4_i8(hs[ k ], w[ k ], ih);
                        il = dot4_i8(ls[ k ], w[ k ], il);
                        if constexpr(METRIC == M_L2SQ) c2 = dot4_i8(w[ k ], w[ k ], c2);
                    }
                }
        }
        ih = (int)group_sum<GS>((uint32_t)ih);
        il = (int)group_sum<GS>((uint32_t)il);
        if constexpr(METRIC == M_L2SQ) c2 = (int)group_sum<GS>((uint32_t)c2);
        if(gsl == GS - 1) {
            bool        reject = false;
            const float sx = __uint_as_float(blk[ 0 ]), delta = __uint_as_float(blk[ 1 ]);
            const float fI = (float)(256.0 * (double)ih + (double)il);  // <X, c>: beyond int32 at d = 2000; exact in double, one rounding
            const float rd = key_dist(worst), e = fmaxf(0x1p-12f, (float)(2 * chunks + 64) * 0x1p-24f);
            if constexpr(METRIC == M_COS) {
                // meta = (s / rb, rho); qn2 = ra; delta = dq.  The steps of (b) and (c), in this order (tests/test_screen_bound_int.py
                // restates them); a query whose norm is 0 or outside the range rejects nothing, a row's range is in rho.
                if(screen_cos_norm_ok(qn2)) {
                    const float sim8 = ((fI * sx) * meta.x) / qn2;
                    const float ub = ((sim8 + meta.y * (1.f + delta)) + delta) + e;
                    reject = (1.f - ub) - e > rd;
                }
            } else {
                // meta = (s, r).  d' and eta as derived above, in this order
                const float ome = 1.f - e;
                if(screen_l2_scale_ok(meta.x)) {
                    const float nx2 = __uint_as_float(blk[ 2 ]);
                    const float R = (2.f * (sx * meta.x)) * fI, Q = (meta.x * meta.x) * (float)c2;
                    const float m = ((nx2 - R) + Q) - 0x1p-20f * (nx2 + Q);
                    if(__builtin_isfinite(m)) {
                        const float a = (__builtin_sqrtf(fmaxf(m, 0.f)) * ome - meta.y) - delta;
                        const float lb = a > 0.f ? a * a : 0.f;
                        reject = lb > 0x1p-100f && lb * ome > rd;  // (lb > 2^-100: as in the float form; nothing here underflows)
                    }
                }
            }
            if(reject) s.newkeys[ j ] = ~0ull;
            else surv[ atomicAdd(&s.scal[ S_NSURV ], 1) ] = (uint32_t)j;
        }
    }
    __syncthreads();
    const int ns = s.scal[ S_NSURV ];
    if(tid == 0) {
        s.scal[ S_NREJ ] += nnew - ns;
        if constexpr(TALLY) s.scal[ S_NTEST ] += nnew;
    }
    return ns;
}

// A screened step of greedy_descent: the keys of the nn listed rows in s.newids -> s.newkeys, ~0 for the rows the screen rejects at
// radius = the best distance so far (S_CURD; the slot bits of the radius are not read), the exact key for every other row -- the
// survivors' rows all requested before the first is consumed.  S_NSURV is zero on entry.
template <int METRIC, int G> __device__ __forceinline__ void descent_distances_screened(const View &v, WalkLds &s, int nn, float qn2)
{
    const uint64_t radius = make_key(__int_as_float(s.scal[ S_CURD ]), 0u);
    const int      ns = hop_distances_screened<METRIC, G, 2>(v, s, nn, radius, qn2);
    hop_distances<METRIC, G, 2, false, true>(v, s, ns, qn2, ~0ull, nullptr, (const uint32_t *)s.sorted);
}

template <int METRIC, int G, bool PROF = false, int ROWS = 2>
__device__ int search_level(const View &v, WalkLds &s, uint32_t *bitmap, uint32_t bm_words, uint32_t start, int level, int ef,
                            uint32_t &D, uint32_t &E, unsigned long long *prof = nullptr)
{
    const int tid = threadIdx.x, T = blockDim.x, g = tid / G, gl = tid % G;
    const int lane = tid & 63;
    // "this is wave 0" as a value the compiler KNOWS is wave-uniform: the serial section below then runs under uniform control
    // flow (no exec save/restore around it, its counters and loop state in scalar registers)
    const bool wave0 = __builtin_amdgcn_readfirstlane(tid) < 64;
    unsigned long long tl = 0;
    if constexpr(PROF) tl = (unsigned long long)clock64();
#define LGPU_MARK(i)                                                  \
    if constexpr(PROF) {                                              \
        if(tid == 0) {                                                \
            const unsigned long long t_ = (unsigned long long)clock64(); \
            prof[ i ] += t_ - tl;                                     \
            tl = t_;                                                  \
        }                                                             \
    }
    // visits.clear(): the LDS set; the HBM bitmap is all-zero between walks (VisUndo)
    for(uint32_t i = tid; i < s.vis_slots; i += T) s.vis[ i ] = EMPTY;
    const float qn2 = __int_as_float(s.scal[ S_QN2 ]);
    if(g == 0) {
        float d = group_dist_n<METRIC, G>(walk_query<METRIC>(s), row_of_m<METRIC>(v, start), (int)v.chunks, gl, qn2, row_norm<METRIC>(v, start));
        if(gl == G - 1) { s.keys[ 0 ] = make_key(d, start); mark_touched<PROF>(s, start); }
    }
    D += 1;
    __syncthreads();
    // wave 0's private walk state: how many slots the LDS set holds, whether it has spilled to the bitmap, the bitmap's undo log
    uint32_t viscnt = 0;
    bool     spilled = false;
    VisUndo  undo;
    if(tid == 0) {
        (void)visit_test_and_set(s, bitmap, start, false);
        viscnt = s.vis_slots ? 1u : 0u;
    }
    viscnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)viscnt);  // uniform in wave 0 (tid 0 is its first lane); unused elsewhere
    if(wave0 && !s.vis_slots) undo_record(s, undo, lane == 0, start, 1ull, lane);  // bitmap-only mode: the start node's bit
    int      cnt = 1;
    for(int hop = 0;; ++hop) {
        int *const nnew_slot = &s.scal[ (hop & 1) ? S_NNEW1 : S_NNEW0 ];
        int *const any_slot = &s.scal[ (hop & 1) ? S_ANY1 : S_ANY0 ];
        // ---- (1) wave 0: pop + neighbour list + visited filter
        if(wave0) {
            int      pos = -1;
            uint32_t node = EMPTY;
            bool     mine = false;  // this lane holds the popped key
            uint64_t popped = 0;
            for(int base = 0; base < cnt; base += 64) {  // first unexpanded entry = pop of usearch's `next` heap
                const int                i = base + lane;
                const uint64_t           key = i < cnt ? s.keys[ i ] : 1ull;
                const unsigned long long m = __ballot(!key_expanded(key));
                if(m) {
                    const int first = (int)__builtin_ctzll(m);
                    pos = base + first;
                    const uint32_t lo = (uint32_t)key;  // slot : flag, the low word of the key
                    node = (uint32_t)__builtin_amdgcn_readlane((int)lo, first) >> 1;
                    mine = lane == first;
                    popped = key;
                    break;
                }
            }
            if(pos < 0) {
                if(lane == 0) *nnew_slot = -1;  // the walk is over
            } else {
                E += 1;
                LGPU_MARK(4)
                // the LDS set must keep room for one full neighbour list; otherwise spill to the HBM bitmap (the set holds
                // 3/4 * vis_slots slots, a search visits D of them).  The bitmap is all-zero (VisUndo): nothing to clear.
                if(s.vis_slots && !spilled && viscnt + v.M0 > s.vis_slots / 4 * 3) spilled = true;
                uint32_t        cap;
                const uint32_t *list = neighbors_of(v, node, level, cap);
                if(lane == 0) trace_append<PROF>(s, node | (level > 0 ? TRACE_LISTU : TRACE_LIST0));
                int nb_new = 0;
                for(uint32_t off = 0; off < cap; off += 64) {
                    const uint32_t i = off + (uint32_t)lane;
                    const uint32_t nb = i < cap ? list[ i ] : EMPTY;
                    if constexpr(PROF) {  // make the list's arrival visible to the phase clock
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        LGPU_MARK(5)
                    }
                    const bool isnew = hop_is_new(s, bitmap, nb, spilled);
                    const unsigned long long m = __ballot(isnew);
                    if(isnew) {
                        s.newids[ nb_new + __popcll(m & ((1ull << lane) - 1ull)) ] = nb;
                        mark_touched<PROF>(s, nb);
                    }
                    if(spilled || !s.vis_slots) undo_record(s, undo, isnew, nb, m, lane);  // these ids went into the HBM bitmap
                    nb_new += __popcll(m);
                }
                if(s.vis_slots && !spilled) viscnt += (uint32_t)nb_new;
                if(lane == 0) { *nnew_slot = nb_new; *any_slot = 0; }
                if(mine) s.keys[ pos ] = popped | 1ull;  // mark it expanded: the lane that read the key writes it back (no LDS read-modify-write)
            }
        }
        LGPU_MARK(0)
        __syncthreads();
        const int nnew = *nnew_slot;
        LGPU_MARK(1)
        if(nnew < 0) break;
        if(nnew == 0) continue;
        // ---- (2) distances: one G-lane group per row, two rows in flight per group (ROWS = 4: the small-batch shape)
        const uint64_t worst = cnt == ef ? s.keys[ cnt - 1 ] : ~0ull;
        hop_distances<METRIC, G, ROWS, true>(v, s, nnew, qn2, worst, any_slot);
        D += (uint32_t)nnew;
        __syncthreads();
        LGPU_MARK(2)
        if(!*any_slot) continue;  // nothing beats the current radius: list unchanged
        // ---- (3) merge: every key's position in the merged list straight from the unsorted new keys.  Two or four
        // adjacent lanes per key (four when the workgroup has the threads for one pass over ef + 2M keys): they split the
        // LDS reads -- all independent: no binary-search chain -- and sum with DPP adds.
        {
            const int total = cnt + nnew;
            auto merge_pass = [&](auto lanes) {
                constexpr int L = decltype(lanes)::value;
                const int     sub = tid & (L - 1);
                for(int t = tid / L; t < ((total + 63) & ~63); t += T / L) {
                    const bool     live = t < total, is_new = t >= cnt;
                    const uint64_t k = !live ? 0ull : is_new ? s.newkeys[ t - cnt ] : s.keys[ t ];
                    const int      below = quad_count_below<L>(s.newkeys, nnew, k, sub);  // new keys smaller than k (keys are distinct)
                    int            p = t + below;
                    if(is_new) p = below + quad_lower_bound<L>(s.keys, cnt, k, sub);
                    if(live && sub == 0 && p < ef) s.keys2[ p ] = k;
                }
            };
            if(T >= 4 * total) merge_pass(std::integral_constant<int, 4>{});
            else merge_pass(std::integral_constant<int, 2>{});
        }
        cnt = cnt + nnew < ef ? cnt + nnew : ef;
        uint64_t *tmp = s.keys; s.keys = s.keys2; s.keys2 = tmp;
        __syncthreads();
        LGPU_MARK(3)
    }
#undef LGPU_MARK
    if(wave0) undo_apply(s, bitmap, bm_words, undo, lane);  // the workgroup's HBM bitmap goes back to all-zero
    return cnt;
}

// ---------------------------------------------------------------------------------------------------
// The same walk with the candidate list in WAVE 0's REGISTERS (ef <= 64 * KPL): lane l of register r holds the (64 r + l)-th
// smallest key, ~0 past the end.  A hop's serial bookkeeping -- merge the previous hop's keys, pop, neighbour list, visited
// filter -- is then one barrier-free section of wave 0:
//   * pop     = one ballot over the expanded flags + one readlane,
//   * merge   = for every new key that beats the radius (few, once the list has settled): its rank is one ballot + popcount,
//               the insertion one wave-wide DPP shift (wave_shr:1) -- no LDS traffic, no second pass over the list,
// and a hop costs two barriers (after the section, after the distances) instead of three.  Inserting the keys one at a time into
// an ef-bounded sorted list leaves the ef smallest of (list U new keys), flags intact: the same list the merge of search_level
// produces, so results are identical (tests/test_gpu_parity.py runs both).
__device__ __forceinline__ uint64_t wave_shr1(uint64_t x)  // lane l <- lane l-1 (lane 0 keeps its own value)
{
    const int lo = __builtin_amdgcn_update_dpp((int)(uint32_t)x, (int)(uint32_t)x, 0x138, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(uint32_t)(x >> 32), (int)(uint32_t)(x >> 32), 0x138, 0xF, 0xF, false);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t readlane64(uint64_t x, int l)  // l uniform
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

#define LGPU_MARK(i)                                                  \
    if constexpr(PROF) {                                              \
        if(tid == 0) {                                                \
            const unsigned long long t_ = (unsigned long long)clock64(); \
            prof[ i ] += t_ - tl;                                     \
            tl = t_;                                                  \
        }                                                             \
    }
// SCREEN (k_search over f32 l2sq or cosine rows of >= 128 chunks, never the instrumented walk): level 0 of a split walk whose screen pointer
// (s.scal[S_SCREEN]) is set runs the hops whose list is full through hop_distances_screened, counting the rows it rejected in
// s.scal[S_NREJ] -- and, TALLY, the rows it tested in s.scal[S_NTEST] (k_insert: insert_kernel.hip).
template <int METRIC, int G, int KPL, bool PROF = false, int ROWS = 2, bool SCREEN = false, bool TALLY = false>
__device__ int search_level_reg(const View &v, WalkLds &s, uint32_t *bitmap, uint32_t bm_words, uint32_t start, int level, int ef,
                                uint32_t &D, uint32_t &E, unsigned long long *prof = nullptr, uint32_t screen_list_prefetch = 0)
{
    static_assert(!SCREEN || ((METRIC == M_L2SQ || METRIC == M_COS) && !PROF), "the screen serves the f32 l2sq and cosine walks");

    const int tid = threadIdx.x, T = blockDim.x, g = tid / G, gl = tid % G;
    const int lane = tid & 63;
    // Wave roles, as values the compiler KNOWS are wave-uniform (the serial sections then run under uniform control flow: no
    // exec save/restore, counters and loop state in scalar registers).  With two or more waves the hop's bookkeeping is SPLIT:
    //   visit wave (wave 0): which node to expand -> its neighbour list -> visited filter -> compaction of the new ids;
    //   list wave  (wave 1): merge of the previous hop's keys into the register list, pop + "expanded" mark, and the two
    //                        values the visit wave's NEXT decision needs: the list's first unexpanded key (`front`) and its
    //                        radius (`worst`), published in LDS slots double-buffered by hop parity.
    // The visit wave does not wait for the merge: the node to expand is min(front, smallest new key inside the radius) -- the
    // first unexpanded entry of the merged list (a key the merge truncates away is never that minimum) -- which it finds with a
    // few ballots over the unsorted new keys.  Merge and list fetch + visited filter, the two long serial chains of a hop, run
    // side by side.  A one-wave workgroup does the list role, then the visit role.
    const int  wv = __builtin_amdgcn_readfirstlane(tid) >> 6;
    const bool split = T >= 128;
    const bool visit_wave = wv == 0, list_wave = split ? wv == 1 : wv == 0;  // (which second wave makes no difference: measured)
    const bool screen_on = SCREEN && split && level == 0 && ((const uint64_t *)&s.scal[ S_SCREEN ])[ 0 ] != 0;  // (the radius is published in the split form only)
    // [r6] Speculative fetch of the FRONT's neighbour list.  The node a hop expands is min(front, best new key of the previous hop); the
    // front is published before the previous hop's distances are even requested, and it IS the next node in 88 % of the hops on
    // clustered data (49 % on i.i.d. Gaussian: scripts/experiments/front_hit_rate.py).  So the visit wave requests the front's list
    // (one 128-byte line at M = 16) right before the distance phase and finds it in a register one hop later; a wrong guess costs the
    // line.  Level 0 only (an upper list's address needs a load of its own), lists of at most 64 entries, never in the instrumented
    // walk (its trace is the logical access sequence).  LGPU_LIST_PREFETCH: 0 off, 1 rows of fewer than 128 chunks (G < 64), 2 all.
    // On 3 KiB rows the fetch bought nothing while a hop was five long row round trips; a SCREENED hop is three or four short ones (list,
    // screen block(s), survivors' rows), the list a third or a quarter of the chain: there the launch says whether to fetch ahead
    // (screen_list_prefetch = SearchArgs::list_prefetch; LGPU_SCREEN_LIST_PREFETCH != 0 compiles it in; never the insertion walks, TALLY).
    constexpr bool PF = !PROF && (LGPU_LIST_PREFETCH >= 2 || (LGPU_LIST_PREFETCH == 1 && G < 64));
    constexpr bool PFS = !PF && SCREEN && !TALLY && LGPU_SCREEN_LIST_PREFETCH != 0;
    const bool     pf_on = (PF || (PFS && screen_on && screen_list_prefetch != 0)) && split && level == 0 && v.M0 <= 64;
    uint32_t       pf_node = EMPTY, pf_nb = EMPTY;
    unsigned long long tl = 0;
    if constexpr(PROF) tl = (unsigned long long)clock64();
    for(uint32_t i = tid; i < s.vis_slots; i += T) s.vis[ i ] = EMPTY;  // (the HBM bitmap is all-zero between walks: VisUndo)
    const float qn2 = __int_as_float(s.scal[ S_QN2 ]);
    if(g == 0) {
        float d = group_dist_n<METRIC, G>(walk_query<METRIC>(s), row_of_m<METRIC>(v, start), (int)v.chunks, gl, qn2, row_norm<METRIC>(v, start));
        if(gl == G - 1) { s.newkeys[ 0 ] = make_key(d, start); mark_touched<PROF>(s, start); }
    }
    D += 1;
    __syncthreads();
    uint64_t *const front_pub = (uint64_t *)&s.scal[ S_FRONT ];  // [2] by hop parity
    uint64_t *const worst_pub = (uint64_t *)&s.scal[ S_WORST ];  // [2]
    // visit wave's private state: how many slots the LDS set holds, whether it has spilled to the bitmap, the bitmap's undo log
    uint32_t viscnt = 0;
    bool     spilled = false;
    VisUndo  undo;
    if(tid == 0) {
        (void)visit_test_and_set(s, bitmap, start, false);
        viscnt = s.vis_slots ? 1u : 0u;
    }
    viscnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)viscnt);
    if(visit_wave && !s.vis_slots) undo_record(s, undo, lane == 0, start, 1ull, lane);  // bitmap-only mode: the start node's bit
    // list wave's private state
    uint64_t           K[ KPL ];     // the list; lanes past position ef - 1 hold leftovers of the shifts and are masked out by
    unsigned long long live[ KPL ];  // `live`: the lanes of register r whose position 64 r + lane is below ef
#pragma unroll
    for(int r = 0; r < KPL; ++r) {
        K[ r ] = ~0ull;
        const int m = ef - 64 * r;
        live[ r ] = m >= 64 ? ~0ull : m <= 0 ? 0ull : (1ull << m) - 1ull;
    }
    int cnt = 1, pend = 0;
    if(list_wave) {
        const uint64_t k0 = s.newkeys[ 0 ];
        if(lane == 0) {
            K[ 0 ] = k0;
            front_pub[ 0 ] = k0;
            worst_pub[ 0 ] = ef == 1 ? k0 : ~0ull;
        }
    }
    if(split) __syncthreads();
    for(int hop = 0;; ++hop) {
        const int  par = hop & 1;
        int *const nnew_slot = &s.scal[ par ? S_NNEW1 : S_NNEW0 ];
        uint32_t   node = EMPTY;  // one-wave form: the list role hands the popped node to the visit role
        unsigned long long tw = 0;
        if constexpr(PROF) tw = (unsigned long long)clock64();
        if(list_wave) {
            // ---- merge the previous hop's keys: one at a time into the sorted registers (rank = one ballot, insertion = one
            // wave-wide DPP shift); only keys inside the radius, ~4 of a hop's ~30 once the list has settled
            for(int base = 0; base < pend; base += 64) {
                const uint64_t N = base + lane < pend ? s.newkeys[ base + lane ] : ~0ull;
                uint64_t       worst = ~0ull;
                if(cnt == ef) {
                    const int wl = (ef - 1) & 63;
#pragma unroll
                    for(int r = 0; r < KPL; ++r)
                        if(r == (ef - 1) >> 6) worst = readlane64(K[ r ], wl);
                }
                unsigned long long todo = __ballot(N < worst);
                while(todo) {
                    const int t = (int)__builtin_ctzll(todo);
                    todo &= todo - 1ull;
                    const uint64_t k = readlane64(N, t);
                    int            p = 0;
#pragma unroll
                    for(int r = 0; r < KPL; ++r) p += (int)__popcll(__ballot(K[ r ] < k) & live[ r ]);
                    if(p >= ef) continue;  // the radius moved in since `todo` was taken
                    const int r0 = p >> 6, l0 = p & 63;
#pragma unroll
                    for(int r = KPL - 1; r >= 0; --r) {
                        if(r < r0) continue;  // uniform
                        const uint64_t sh = wave_shr1(K[ r ]);
                        if(r > r0) {
                            const uint64_t carry = readlane64(K[ r - 1 > 0 ? r - 1 : 0 ], 63);
                            K[ r ] = lane == 0 ? carry : sh;
                        } else {
                            if(lane > l0) K[ r ] = sh;
                            if(lane == l0) K[ r ] = k;
                        }
                    }
                    cnt = cnt < ef ? cnt + 1 : ef;
                }
            }
            // ---- pop: the first unexpanded key (~0 carries the flag); mark it; publish the next hop's front and radius
            int first = -1, fr = 0;
#pragma unroll
            for(int r = 0; r < KPL; ++r) {
                const unsigned long long m = __ballot(!key_expanded(K[ r ])) & live[ r ];
                if(first < 0 && m) {
                    first = (int)__builtin_ctzll(m);
                    fr = r;
                    node = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)K[ r ], first) >> 1;
                }
            }
            if(first >= 0) {
#pragma unroll
                for(int r = 0; r < KPL; ++r)
                    if(r == fr && lane == first) K[ r ] |= 1ull;  // expanded
                if(split) {
                    uint64_t nf = ~0ull, nw = ~0ull;
                    bool     have = false;
#pragma unroll
                    for(int r = 0; r < KPL; ++r) {
                        const unsigned long long m = __ballot(!key_expanded(K[ r ])) & live[ r ];
                        if(!have && m) {
                            nf = readlane64(K[ r ], (int)__builtin_ctzll(m));
                            have = true;
                        }
                        if(cnt == ef && r == (ef - 1) >> 6) nw = readlane64(K[ r ], (ef - 1) & 63);
                    }
                    if(lane == 0) {
                        front_pub[ par ^ 1 ] = nf;
                        worst_pub[ par ^ 1 ] = nw;
                    }
                }
            }
            LGPU_MARK(3)
            if constexpr(PROF) {  // split form: the list wave's own clock (slot 4, which the visit wave leaves alone then)
                if(split && lane == 0) prof[ 4 ] += (unsigned long long)clock64() - tw;
            }
        }
        if(visit_wave) {
            if(split) {
                // ---- which node the list wave is popping right now: min(front, smallest new key inside the radius)
                const uint64_t f = front_pub[ par ], w = worst_pub[ par ];
                uint64_t       t = f != ~0ull ? f : w;
                bool           got = f != ~0ull;
                for(int base = 0; base < pend; base += 64) {
                    const uint64_t     N = base + lane < pend ? s.newkeys[ base + lane ] : ~0ull;
                    unsigned long long m = __ballot(N < t);
                    while(m) {  // each round at least halves the expected number of smaller keys
                        t = readlane64(N, (int)__builtin_ctzll(m));
                        got = true;
                        m = __ballot(N < t);
                    }
                }
                node = got ? (uint32_t)t >> 1 : EMPTY;
                LGPU_MARK(3)
            }
            if(node == EMPTY) {
                if(lane == 0) *nnew_slot = -1;  // the walk is over
            } else {
                E += 1;
                if(!split) LGPU_MARK(4)
                // the LDS set must keep room for one full neighbour list; otherwise spill to the HBM bitmap (the set holds
                // 3/4 * vis_slots slots, a search visits D of them).  The bitmap is all-zero (VisUndo): nothing to clear.
                if(s.vis_slots && !spilled && viscnt + v.M0 > s.vis_slots / 4 * 3) spilled = true;
                uint32_t        cap;
                const uint32_t *list = neighbors_of(v, node, level, cap);
                if(lane == 0) trace_append<PROF>(s, node | (level > 0 ? TRACE_LISTU : TRACE_LIST0));
                const bool have_list = pf_on && node == pf_node;  // (uniform) the speculative fetch of the previous hop was this node's list
                int nb_new = 0;
                for(uint32_t off = 0; off < cap; off += 64) {
                    const uint32_t i = off + (uint32_t)lane;
                    uint32_t       nb;
                    if(have_list) nb = pf_nb;  // (cap <= 64: one pass)
                    else nb = i < cap ? list[ i ] : EMPTY;
                    if constexpr(PROF) {  // make the list's arrival visible to the phase clock
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        LGPU_MARK(5)
                    }
                    const bool isnew = hop_is_new(s, bitmap, nb, spilled);
                    const unsigned long long m = __ballot(isnew);
                    if(isnew) {
                        s.newids[ nb_new + __popcll(m & ((1ull << lane) - 1ull)) ] = nb;
                        mark_touched<PROF>(s, nb);
                    }
                    if(spilled || !s.vis_slots) undo_record(s, undo, isnew, nb, m, lane);  // these ids went into the HBM bitmap
                    nb_new += __popcll(m);
                }
                if(s.vis_slots && !spilled) viscnt += (uint32_t)nb_new;
                if(lane == 0) {
                    *nnew_slot = nb_new;
                    if(SCREEN) s.scal[ S_NSURV ] = 0;  // (the previous hop's survivors were read before the barrier behind its distances)
                }
            }
        }
        LGPU_MARK(0)
        __syncthreads();
        const int nnew = *nnew_slot;
        LGPU_MARK(1)
        if(nnew < 0) break;
        pend = nnew;
        if(pf_on && visit_wave) {  // the next hop's front (the list wave published it before the barrier): request its list now
            const uint64_t nf = front_pub[ par ^ 1 ];
            pf_node = nf != ~0ull ? (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)nf >> 1)) : EMPTY;
            if(pf_node != EMPTY) pf_nb = (uint32_t)lane < v.M0 ? v.nbr0[ (size_t)pf_node * v.M0 + (uint32_t)lane ] : EMPTY;
        }
        if(nnew == 0) continue;
        // the radius the list wave published before the barrier (~0: the list is not full, nothing can be rejected)
        if constexpr(SCREEN) {  // one copy of the exact phase: over the screen's survivors, or over all rows
            const uint64_t radius = screen_on ? worst_pub[ par ^ 1 ] : ~0ull;
            int            ne = nnew;
            if(radius != ~0ull) ne = hop_distances_screened<METRIC, G, ROWS, TALLY>(v, s, nnew, radius, qn2);
            hop_distances<METRIC, G, ROWS, false, true>(v, s, ne, qn2, ~0ull, nullptr, radius != ~0ull ? (const uint32_t *)s.sorted : nullptr);
        } else {
            hop_distances<METRIC, G, ROWS, false>(v, s, nnew, qn2, ~0ull, nullptr);
        }
        D += (uint32_t)nnew;
        __syncthreads();
        LGPU_MARK(2)
    }
    if(visit_wave) undo_apply<SCREEN && !TALLY>(s, bitmap, bm_words, undo, lane);  // the workgroup's HBM bitmap goes back to all-zero
    // the result goes where the callers read it: s.keys, ascending
    if(list_wave) {
#pragma unroll
        for(int r = 0; r < KPL; ++r)
            if(r * 64 + lane < cnt) s.keys[ r * 64 + lane ] = K[ r ];
        if(lane == 0) s.scal[ S_CNT ] = cnt;
    }
    __syncthreads();
    return s.scal[ S_CNT ];
}
#undef LGPU_MARK

// ---- refine_: the neighbour-selection heuristic --------------------------------------------------------
struct RefineLds
{
    float    *cd;   // candidates in: distance to the centre
    uint32_t *cid;  //                slot
    float    *sd;   // sorted / selected out
    uint32_t *sid;
};
__device__ __forceinline__ unsigned char *carve_refine(unsigned char *p, RefineLds &r, uint32_t n_max)
{
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    r.cd = (float *)p;      p += up16((size_t)n_max * 4);
    r.cid = (uint32_t *)p;  p += up16((size_t)n_max * 4);
    r.sd = (float *)p;      p += up16((size_t)n_max * 4);
    r.sid = (uint32_t *)p;  p += up16((size_t)n_max * 4);
    return p;
}
__host__ inline size_t refine_lds_bytes(uint32_t n_max)
{
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    return 4 * up16((size_t)n_max * 4);
}

// in: r.cd/r.cid[0..n) in any order.  Sorts by (distance, tie_mix(slot, centre)) into r.sd/r.sid,
// then keeps an entry iff no already-kept entry is strictly closer to it than the centre is.
// Returns the number kept (<= needed), left in r.sd/r.sid[0..keep).  `scal` = WalkLds-style scalars.
template <int METRIC, int G>
__device__ int refine(const View &v, RefineLds &r, int *scal, int n, int needed, uint32_t centre, uint32_t &Dr)
{
    const int tid = threadIdx.x, T = blockDim.x, g = tid / G, gl = tid % G, NG = T / G;
    for(int t = tid; t < n; t += T) {
        const float    d = r.cd[ t ];
        const uint32_t id = r.cid[ t ];
        const uint64_t k = ((uint64_t)f2ord(d) << 32) | tie_mix(id, centre);
        int            rank = 0;
        for(int j = 0; j < n; ++j) {
            const uint64_t kj = ((uint64_t)f2ord(r.cd[ j ]) << 32) | tie_mix(r.cid[ j ], centre);
            rank += kj < k;
        }
        r.sd[ rank ] = d;
        r.sid[ rank ] = id;
    }
    if(tid == 0) scal[ S_BAD ] = 0;
    __syncthreads();
    if(n < needed) return n;
    int submitted = 1, consumed = 1;
    while(submitted < needed && consumed < n) {
        const uint32_t cid = r.sid[ consumed ];
        const float    cdist = r.sd[ consumed ];
        const float    cn2 = row_norm<METRIC>(v, cid);
        for(int i = g; i < submitted; i += NG) {
            const uint32_t kid = r.sid[ i ];
            float inter = group_dist_n<METRIC, G>(row_of_m<METRIC>(v, cid), row_of_m<METRIC>(v, kid), (int)v.chunks, gl, cn2, row_norm<METRIC>(v, kid));
            if(gl == G - 1 && inter < cdist) scal[ S_BAD ] = 1;
        }
        Dr += (uint32_t)submitted;
        __syncthreads();
        const bool good = scal[ S_BAD ] == 0;
        __syncthreads();
        if(tid == 0) {
            scal[ S_BAD ] = 0;
            if(good) { r.sid[ submitted ] = cid; r.sd[ submitted ] = cdist; }
        }
        if(good) submitted++;
        consumed++;
        __syncthreads();
    }
    return submitted;
}

}  // namespace lgpu
