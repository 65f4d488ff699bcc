// search_filtered_kernel.hpp -- the two kernel templates of the filtered k-NN search over an allow-set of slots (filter.hpp), instantiated
// by search_filtered_kernel.hip (rows stored in HBM) and search_filtered_pq_kernel.hip (compact pq indexes).  One workgroup per query,
// persistent over the batch (work handed out by ticket); the frame around a query's walk is query_frame.hpp's (kernel arguments
// re-read from the kernarg segment, the query picked, staged, answered and closed there):
//
//  * k_search_filtered: the base-layer walk with TWO lists in LDS, both ordered by the walk's total order (distance, slot):
//      top  -- at most `exp` keys, ALLOWED slots only (the answer is top[skip, skip + k));
//      next -- the candidates still to be expanded, at most C keys, popped at a head index.
//    Upper levels: greedy_descent exactly as k_search (the filter does not apply there).  Base layer: evaluate the start node, push
//    it to next (and to top if allowed).  While next is not empty: c = min(next); stop if |top| == exp and worst(top) < c; else pop
//    c (E += 1), evaluate every unvisited neighbour (D += 1 each, visited set of walk.hpp), and for each key x with |top| < exp or
//    x < worst(top): push x to next (a full next keeps its C smallest: x replaces the worst entry when smaller, else is dropped; a
//    dropped node stays visited), and insert x into top if its slot is allowed.
//    A hop evaluates its neighbours together and admits them against worst(top) AT THE START of the hop, where the definition
//    admits them one at a time against a radius that may shrink within the hop.  The extra keys this admits are >= the final
//    radius: they never enter top (it keeps its exp smallest allowed keys either way), and in next they can neither be popped
//    (next's minimum is >= worst(top) once only they remain: the walk stops) nor push out an entry that could be (an entry evicted
//    by one of them is larger still).  So the hop's batch gives the keys, D and E of the one-at-a-time definition.
//    The same holds for a ROUND of the seeded stage below (at most M0 seeds, or the start node alone): its rows are admitted
//    against worst(top) at the start of the round, and what that admits beyond the one-at-a-time radius is >= the final radius.
//    SEEDED (an index's lantern_gpu_set_filter_seeds > 0; per-query form only, a single filter goes through a descriptor table):
//    for a query whose filter has count >= 1 allowed rows, S' = min(seeds, count), the start node is NOT evaluated first.  Instead
//      seeding:      rounds of at most M0 slots x = allow_slots[(j * count) / S'], j = 0 .. S'-1 in order, through the hop's visited
//                    filter, distance phase and rank-merges (no pop: E is not touched; D += 1 per seed);
//      allowed-only: the hop loop, a disallowed neighbour presented to the visited filter as EMPTY (not marked, counted or
//                    evaluated), to the loop's own stop;
//      hand-over:    next := the keys of top (what the stage left in next lies beyond the radius and could never be popped), then
//                    the start node as a one-slot round through the same visited test (evaluated and counted only if unvisited);
//      today's loop, unchanged, to its stop.
//    The phase is wave-uniform and every thread derives it from what the whole workgroup reads (the round counter, the stop mark
//    in the hop's scalar slot); it, S' and the descriptor are per query and read anew for every ticket.  A NULL (unfiltered) entry
//    has no slot list: S' = 0, today's walk.
//    ALL-ALLOWED PROPERTY: with every slot allowed and C >= exp the walk returns exactly the ids, distance bits, D and E of the
//    unfiltered k_search.  Every entry of next that is smaller than worst(top) is in top (both lists received it, top drops only
//    entries larger than its worst); so an entry evicted from a full next has at least exp smaller entries in top and would never
//    have been popped, and the pops are those of the single-list walk ("first unexpanded entry of the ef list": walk.hpp).
//  * k_search_exact_allowed: every allowed slot (the filter's ascending slot list) evaluated with the walk's row-distance routine --
//    the same bits as the walk gives the row -- and a rank-merge into an LDS list of k + skip keys.  D = allowed count, E = 0.
//
// The allow bit of a slot travels in the LOW bit of its key (the "expanded" flag of the unfiltered walk, unused here): a slot is
// either allowed or not, so two keys of one slot carry the same bit and the order (distance, slot) is untouched.
//
// PARITY UNPINNED BY THE REFERENCE: the reference's usearch fork is not in the tree; these semantics are a definition of this
// repository (tests/filtered_walk_ref.py restates them on the CPU).
//
// COMPACT PQ INDEXES (lantern_gpu_set_filter_compact; instantiated in search_filtered_pq_kernel.hip): M_*_PQD rows are decoded on the fly
// (row_of_m returns a PqdRow: the expanded index's arithmetic, carve and answers, bit for bit); M_*_ADC rows are code chunks summed
// over the per-query table of search_adc_kernel.hip, which lies in the FIRST bytes of the LDS (RowAcc<M_*_ADC> reads it there) with
// the raw f32 query row behind it: the carve's "query row" is table + raw row, the lists and the visited set follow as ever.  The
// table, |q| and the raw row are staged anew for every ticket (adc_stage.hpp), and only for a query that evaluates a row.
#pragma once
#include "adc_stage.hpp"
#include "filter.hpp"
#include "search_kernel.hpp"

namespace lgpu {

template <int METRIC> constexpr bool kAdcRows = METRIC >= M_ADC && METRIC < M_PQD;
// chunks in front of the lists in the carve: the stored row's -- or, ADC, the table's and the raw query row's
__host__ __device__ inline uint32_t adc_lds_chunks(uint32_t code_chunks, uint32_t qchunks) { return code_chunks * 16 * ADC_LUT_STRIDE / 4 + qchunks; }

__device__ __forceinline__ uint64_t allow_bit(const uint32_t *bits, uint32_t slot) { return (uint64_t)((bits[ slot >> 5 ] >> (slot & 31)) & 1u); }
// the per-query form: a NULL bitmap is the descriptor's "unfiltered" mark (every slot allowed)
template <bool EACH> __device__ __forceinline__ uint64_t allow_bit_of(const uint32_t *bits, uint32_t slot)
{
    if constexpr(EACH) return bits ? allow_bit(bits, slot) : 1ull;
    else return allow_bit(bits, slot);
}

// #{j < n : a[j] < k}, every key of a[] taken
__device__ __forceinline__ int count_below(const uint64_t *a, int n, uint64_t k)
{
    int c = 0;
    for(int j = 0; j < n; ++j) c += a[ j ] < k;
    return c;
}
// #{j < n : a[j] < k and a[j]'s allow bit is set}
__device__ __forceinline__ int count_below_allowed(const uint64_t *a, int n, uint64_t k)
{
    int c = 0;
    for(int j = 0; j < n; ++j) c += (a[ j ] < k) & (int)(a[ j ] & 1u);
    return c;
}

// the carve of the walk's LDS: walk.hpp's (q, top, top merge target, new keys, new ids, scalars, visited set) + next and its merge target
__device__ __forceinline__ void carve_filtered(unsigned char *p, WalkLds &s, uint64_t *&nx, uint64_t *&nx2, uint32_t chunks, uint32_t exp,
                                               uint32_t cand_cap, uint32_t M0, uint32_t vis_slots)
{
    unsigned char *end = carve_walk(p, s, chunks, exp, M0, vis_slots);
    end = (unsigned char *)(((size_t)end + 15) & ~(size_t)15);
    nx = (uint64_t *)end;
    nx2 = nx + cand_cap;
}

// scalar slots of the filtered walk beyond walk.hpp's (the register-list walk's hand-off slots, unused here): new keys of the hop
// admitted to next / allowed among them, double-buffered by hop parity like the new-id count (a wave that leaves a hop early without
// a barrier must not see the next hop's reset)
enum { S_ADMIT0 = S_FRONT, S_ADMIT1, S_ALLOWED0, S_ALLOWED1 };

// the phases of a seeded walk (wave-uniform); a walk that is not seeded is in PH_FINAL from its first hop
enum { PH_FINAL = 0, PH_SEED, PH_ALLOWED, PH_START };

// The base layer of the filtered walk.  On return s.keys[0..cnt) holds top, ascending; returns cnt.
// SEEDED: seed_slots[0, seed_count) is the filter's ascending slot list and S = S' (0: this query is not seeded).
template <int METRIC, int G, bool EACH, bool SEEDED = false>
__device__ int search_level_filtered(const View &v, WalkLds &s, uint64_t *nx, uint64_t *nx2, const uint32_t *allow, uint32_t *bitmap,
                                     uint32_t bm_words, uint32_t start, int exp, int C, uint32_t &D, uint32_t &E,
                                     const uint32_t *seed_slots = nullptr, uint32_t seed_count = 0, uint32_t S = 0)
{
    const int  tid = threadIdx.x, T = blockDim.x, g = tid / G, gl = tid % G, NG = T / G;
    const int  lane = tid & 63;
    const bool wave0 = __builtin_amdgcn_readfirstlane(tid) < 64;
    for(uint32_t i = tid; i < s.vis_slots; i += T) s.vis[ i ] = EMPTY;
    const float qn2 = __int_as_float(s.scal[ S_QN2 ]);
    int      phase = PH_FINAL;
    uint32_t seed_base = 0;  // the first seed of the next round
    if constexpr(SEEDED) phase = S ? PH_SEED : PH_FINAL;
    int      tcnt = 0;            // |top|
    int      head = 0, ncnt = 0;  // next = nx[head, ncnt)
    uint32_t viscnt = 0;
    bool     spilled = false;
    VisUndo  undo;
    if(!SEEDED || phase == PH_FINAL) {
        if(g == 0) {
            float d = group_dist_n<METRIC, G>(walk_query<METRIC>(s), row_of_m<METRIC>(v, start), (int)v.chunks, gl, qn2, row_norm<METRIC>(v, start));
            if(gl == G - 1) {
                const uint64_t key = make_key(d, start) | allow_bit_of<EACH>(allow, start);
                nx[ 0 ] = key;
                s.keys[ 0 ] = key;
                s.scal[ S_CNT ] = (int)(key & 1u);
            }
        }
        D += 1;
        __syncthreads();
        tcnt = s.scal[ S_CNT ];
        ncnt = 1;
        if(tid == 0) {
            (void)visit_test_and_set(s, bitmap, start, false);
            viscnt = s.vis_slots ? 1u : 0u;
        }
        viscnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)viscnt);
        if(wave0 && !s.vis_slots) undo_record(s, undo, lane == 0, start, 1ull, lane);
    }
    __syncthreads();  // (S_CNT is read by every wave before wave 0 may reuse the scalars; a seeded walk: the visited set is EMPTY)
    for(int hop = 0;; ++hop) {
        int *const nnew_slot = &s.scal[ (hop & 1) ? S_NNEW1 : S_NNEW0 ];
        int *const admit_slot = &s.scal[ (hop & 1) ? S_ADMIT1 : S_ADMIT0 ];
        int *const allowed_slot = &s.scal[ (hop & 1) ? S_ALLOWED1 : S_ALLOWED0 ];
        // ---- (1) wave 0: stop test, pop, neighbour list, visited filter
        if(wave0) {
            const bool hopping = !SEEDED || phase == PH_FINAL || phase == PH_ALLOWED;  // a round of seeds, or the start node, pops nothing
            bool       stop = hopping && head >= ncnt;
            uint64_t   c = 0;
            if(hopping && !stop) {
                c = nx[ head ];
                stop = tcnt == exp && s.keys[ exp - 1 ] < c;
            }
            if(stop) {
                if(lane == 0) *nnew_slot = -1;
            } else {
                if(hopping) E += 1;
                const uint32_t node = key_slot(c);
                if(s.vis_slots && !spilled && viscnt + v.M0 > s.vis_slots / 4 * 3) spilled = true;
                uint32_t        cap;
                const uint32_t *list;
                if constexpr(SEEDED) {
                    if(phase == PH_SEED) { list = seed_slots; cap = S - seed_base < v.M0 ? S - seed_base : v.M0; }
                    else if(phase == PH_START) { list = seed_slots; cap = 1; }
                    else list = neighbors_of(v, node, 0, cap);
                } else {
                    list = neighbors_of(v, node, 0, cap);
                }
                int nb_new = 0;
                for(uint32_t off = 0; off < cap; off += 64) {
                    const uint32_t i = off + (uint32_t)lane;
                    uint32_t       nb = EMPTY;
                    if constexpr(SEEDED) {
                        if(i < cap) {
                            if(phase == PH_SEED) nb = list[ (uint32_t)(((uint64_t)(seed_base + i) * seed_count) / S) ];
                            else if(phase == PH_START) nb = start;
                            else {
                                nb = list[ i ];
                                if(phase == PH_ALLOWED && nb != EMPTY && !allow_bit_of<EACH>(allow, nb)) nb = EMPTY;
                            }
                        }
                    } else {
                        nb = i < cap ? list[ i ] : EMPTY;
                    }
                    const bool               isnew = hop_is_new(s, bitmap, nb, spilled);
                    const unsigned long long m = __ballot(isnew);
                    if(isnew) s.newids[ nb_new + __popcll(m & ((1ull << lane) - 1ull)) ] = nb;
                    if(spilled || !s.vis_slots) undo_record(s, undo, isnew, nb, m, lane);
                    nb_new += __popcll(m);
                }
                if(s.vis_slots && !spilled) viscnt += (uint32_t)nb_new;
                if(lane == 0) { *nnew_slot = nb_new; *admit_slot = 0; *allowed_slot = 0; }
            }
        }
        __syncthreads();
        const int nnew = *nnew_slot;
        if constexpr(SEEDED) {
            if(nnew < 0) {
                if(phase != PH_ALLOWED) break;
                // hand-over: next := the keys of top; then the start node, as a round of one slot
                for(int t = tid; t < tcnt; t += T) nx[ t ] = s.keys[ t ];
                head = 0;
                ncnt = tcnt;
                phase = PH_START;
                __syncthreads();
                continue;
            }
            if(phase == PH_SEED) {
                seed_base += v.M0;
                if(seed_base >= S) phase = PH_ALLOWED;
            } else if(phase == PH_START) {
                phase = PH_FINAL;
            } else {
                head += 1;  // the pop
            }
        } else {
            if(nnew < 0) break;
            head += 1;  // the pop
        }
        if(nnew == 0) continue;
        // ---- (2) distances: one G-lane group per row, two rows in flight per group (walk.hpp hop_distances), the allow bit in the key
        const uint64_t worst = tcnt == exp ? s.keys[ exp - 1 ] : ~0ull;
        for(int i = g; i < nnew; i += 2 * NG) {
            const int      j = i + NG;
            const uint32_t id0 = s.newids[ i ];
            const uint32_t id1 = j < nnew ? s.newids[ j ] : id0;
            const uint64_t a0 = allow_bit_of<EACH>(allow, id0), a1 = allow_bit_of<EACH>(allow, id1);
            float          d0, d1;
            group_dist2_n<METRIC, G>(walk_query<METRIC>(s), row_of_m<METRIC>(v, id0), row_of_m<METRIC>(v, id1), (int)v.chunks, gl, qn2,
                                     row_norm<METRIC>(v, id0), row_norm<METRIC>(v, id1), d0, d1);
            if(gl == G - 1) {
                const uint64_t k0 = make_key(d0, id0) | a0;
                s.newkeys[ i ] = k0;
                int adm = k0 < worst, alw = (k0 < worst) & (int)a0;
                if(j < nnew) {
                    const uint64_t k1 = make_key(d1, id1) | a1;
                    s.newkeys[ j ] = k1;
                    adm += k1 < worst;
                    alw += (k1 < worst) & (int)a1;
                }
                if(adm) atomicAdd(admit_slot, adm);
                if(alw) atomicAdd(allowed_slot, alw);
            }
        }
        D += (uint32_t)nnew;
        __syncthreads();
        const int n_admit = *admit_slot, n_allowed = *allowed_slot;
        if(n_admit == 0) continue;  // nothing enters either list
        // ---- (3) rank-merges: top U allowed admitted keys -> keys2 (exp), next U admitted keys -> nx2 (C); the new keys unsorted
        {
            const int total = tcnt + nnew;
            for(int t = tid; t < total; t += T) {
                if(t < tcnt) {
                    const uint64_t k = s.keys[ t ];
                    const int      p = t + count_below_allowed(s.newkeys, nnew, k < worst ? k : worst);
                    if(p < exp) s.keys2[ p ] = k;
                } else {
                    const uint64_t k = s.newkeys[ t - tcnt ];
                    if(!(k & 1u) || !(k < worst)) continue;
                    const int p = count_below_allowed(s.newkeys, nnew, k) + lower_bound_keys(s.keys, tcnt, k);
                    if(p < exp) s.keys2[ p ] = k;
                }
            }
            const uint64_t *nb = nx + head;
            const int       m = ncnt - head, ntotal = m + nnew;
            for(int t = tid; t < ntotal; t += T) {
                if(t < m) {
                    const uint64_t k = nb[ t ];
                    const int      p = t + count_below(s.newkeys, nnew, k < worst ? k : worst);
                    if(p < C) nx2[ p ] = k;
                } else {
                    const uint64_t k = s.newkeys[ t - m ];
                    if(!(k < worst)) continue;
                    const int p = count_below(s.newkeys, nnew, k) + lower_bound_keys(nb, m, k);
                    if(p < C) nx2[ p ] = k;
                }
            }
            tcnt = tcnt + n_allowed < exp ? tcnt + n_allowed : exp;
            ncnt = m + n_admit < C ? m + n_admit : C;
            head = 0;
            uint64_t *tmp = s.keys; s.keys = s.keys2; s.keys2 = tmp;
            tmp = nx; nx = nx2; nx2 = tmp;
        }
        __syncthreads();
    }
    if(wave0) undo_apply(s, bitmap, bm_words, undo, lane);
    return tcnt;
}

#define LGPU_FARG(base, field) LGPU_KARG(base, decltype(FilteredArgs::field), offsetof(FilteredArgs, field))

// a query's row {k, expansion (exact: k + skip), skip, C} of FilteredArgs::qparams (wave-uniform: q came through the scalar cache, and
// so does the row -- as query_params of search_kernel.hpp)
struct FilteredQueryParams { uint32_t k, exp, skip, cand_cap; };
__device__ __forceinline__ FilteredQueryParams filtered_query_params(KernargBytes ka, uint32_t q)
{
    const ConstWords row = (ConstWords)(uintptr_t)LGPU_FARG(ka, qparams) + (size_t)q * 4;
    return FilteredQueryParams{ row[ 0 ], row[ 1 ], row[ 2 ], row[ 3 ] };
}

// ADC rows: query q's raw row, table and |q| into the first LDS bytes, by k_search_adc's own staging (adc_stage.hpp) from
// FilteredArgs::adc_*.  Every thread of the workgroup calls it (it ends in a barrier).
template <int METRIC>
__device__ __forceinline__ void filtered_adc_stage(const int tid, const int T, KernargBytes ka, WalkLds &s, uint32_t q, uint32_t code_chunks)
{
    adc_stage<METRIC>(tid, T, s, (float *)s.q, s.q + adc_lds_chunks(code_chunks, 0), LGPU_FRAME_ARG(ka, FilteredArgs, queries), q, LGPU_FARG(ka, adc_centers),
                      LGPU_FARG(ka, adc_S), LGPU_FARG(ka, adc_C), LGPU_FARG(ka, adc_subdim), LGPU_FARG(ka, adc_qchunks), code_chunks * 16);
}

// EACH: the per-query form.  The launch serves the queries of its selection list (FrameArgs::qlist), and the filter of a query is
// its descriptor (FilteredArgs::descs[q]), read from memory anew for every query at the point that needs it: a workgroup serves many
// queries and carries nothing of one query's filter into the next.  A descriptor with count 0 (and no unfiltered mark) is an empty
// filter: no walk, the empty answer.
// SEEDED (with EACH only): the seeded walk of the header, S' = min(FilteredArgs::seeds, the descriptor's count), 0 for an unfiltered entry.
// PARAMS (with EACH only): the per-query-parameter form.  A query brings its own k, expansion, skip and C in its row of
// FilteredArgs::qparams, read anew for every ticket at the point that needs it, as the descriptor is: nothing of one query's
// parameters is carried into the next.  The LDS carve stays the launch's (FilteredArgs::exp and cand_cap: the largest of its list), the
// walk runs with the query's own expansion and C, the answer rows are FilteredArgs::k wide.  k = 0: no walk, the empty answer.
template <int METRIC, int G, bool EACH, bool SEEDED = false, bool PARAMS = false>
__global__ void __launch_bounds__(512) k_search_filtered(FilteredArgs)
{
    static_assert(EACH || !SEEDED, "the seeded walk is instantiated in the per-query form only");
    static_assert(EACH || !PARAMS, "the per-query-parameter form is instantiated in the per-query form only");
    const int tid = threadIdx.x, T = blockDim.x;
    WalkLds   s;
    uint64_t *nx, *nx2;
    {
        const KernargBytes ka = kernarg_opaque();
        uint32_t           chunks = LGPU_VIEW_ARG(ka, FilteredArgs, chunks);
        if constexpr(kAdcRows<METRIC>) chunks = adc_lds_chunks(chunks, LGPU_FARG(ka, adc_qchunks));  // s.q = the table, then the raw query row
        carve_filtered(lgpu_smem, s, nx, nx2, chunks, LGPU_FARG(ka, exp), LGPU_FARG(ka, cand_cap), LGPU_VIEW_ARG(ka, FilteredArgs, M0),
                       LGPU_FRAME_ARG(ka, FilteredArgs, vis_slots));
    }
    for(uint32_t pos = blockIdx.x; pos < LGPU_FRAME_ARG(kernarg_opaque(), FilteredArgs, nq);) {
        const uint32_t q = frame_query<FilteredArgs, EACH>(kernarg_opaque(), pos);
        uint32_t       D = 0, E = 0;
        int            cnt = 0;
        {
            const KernargBytes ka = kernarg_opaque();
            View               v;
            LGPU_LOAD_VIEW(v, ka, FilteredArgs)
            if constexpr(METRIC >= M_PQD) LGPU_LOAD_VIEW_PQD(v, ka, FilteredArgs)
            uint32_t        bm_words;
            uint32_t *const bitmap = frame_bind<FilteredArgs>(ka, s, bm_words);
            if constexpr(!kAdcRows<METRIC>) frame_stage<METRIC, G>(tid, T, s, LGPU_FRAME_ARG(ka, FilteredArgs, queries), q, v.chunks);
            const uint32_t *allow;
            bool            any = true;
            const uint32_t *seed_slots = nullptr;
            uint32_t        seed_count = 0, S = 0;
            if constexpr(EACH) {
                const FilterDesc *const d = LGPU_FARG(ka, descs) + q;
                const uint32_t          unfiltered = d->unfiltered;
                allow = unfiltered ? nullptr : d->bits;
                any = unfiltered || d->count != 0;
                if constexpr(SEEDED) {
                    if(!unfiltered) {
                        const uint32_t seeds = LGPU_FARG(ka, seeds);
                        seed_slots = d->slots;
                        seed_count = d->count;
                        S = seeds < seed_count ? seeds : seed_count;
                    }
                    S = (uint32_t)__builtin_amdgcn_readfirstlane((int)S);
                }
            } else {
                allow = LGPU_FARG(ka, allow_bits);
            }
            if constexpr(PARAMS) any = any && filtered_query_params(ka, q).k != 0;
            if(v.n != 0 && any) {
                if constexpr(kAdcRows<METRIC>) filtered_adc_stage<METRIC>(tid, T, ka, s, q, v.chunks);  // (a query that walks: workgroup-uniform)
                const uint32_t start = greedy_descent<METRIC, G>(v, s, v.entry, v.max_level, 0, D);
                if constexpr(PARAMS) {
                    const FilteredQueryParams p = filtered_query_params(ka, q);
                    cnt = search_level_filtered<METRIC, G, EACH, SEEDED>(v, s, nx, nx2, allow, bitmap, bm_words, start, (int)p.exp, (int)p.cand_cap, D, E,
                                                                         seed_slots, seed_count, S);
                } else {
                    cnt = search_level_filtered<METRIC, G, EACH, SEEDED>(v, s, nx, nx2, allow, bitmap, bm_words, start, (int)LGPU_FARG(ka, exp),
                                                                         (int)LGPU_FARG(ka, cand_cap), D, E, seed_slots, seed_count, S);
                }
            }
        }
        const KernargBytes kb = kernarg_opaque();
        int                got;
        if constexpr(PARAMS) {  // (FilteredArgs::k: the width of an answer row)
            const FilteredQueryParams p = filtered_query_params(kb, q);
            got = frame_answer_rows<FilteredArgs>(tid, T, kb, s, q, cnt, p.k, p.skip, LGPU_FARG(kb, k));
        } else {
            const uint32_t k = LGPU_FARG(kb, k);
            got = frame_answer_rows<FilteredArgs>(tid, T, kb, s, q, cnt, k, LGPU_FARG(kb, skip), k);
        }
        pos = frame_close<FilteredArgs>(tid, kb, s, q, pos, got, D, E);
    }
}

// The exact path: rows_per_round allowed rows per round (two per G-lane group, group_dist2_n as the walk's hops), merged into an
// LDS list of k + skip keys when any of them beats its worst.
// PARAMS (with EACH only): as k_search_filtered's -- the list is carved for the launch's largest k + skip, a query keeps its own.
template <int METRIC, int G, bool EACH, bool PARAMS = false>
__global__ void __launch_bounds__(512) k_search_exact_allowed(FilteredArgs)
{
    static_assert(EACH || !PARAMS, "the per-query-parameter form is instantiated in the per-query form only");
    const int tid = threadIdx.x, T = blockDim.x, g = tid / G, gl = tid % G, NG = T / G;
    WalkLds   s;
    {
        const KernargBytes ka = kernarg_opaque();
        uint32_t           chunks = LGPU_VIEW_ARG(ka, FilteredArgs, chunks);
        if constexpr(kAdcRows<METRIC>) chunks = adc_lds_chunks(chunks, LGPU_FARG(ka, adc_qchunks));  // s.q = the table, then the raw query row
        carve_walk(lgpu_smem, s, chunks, LGPU_FARG(ka, exp), LGPU_FARG(ka, rows_per_round), 0);
    }
    for(uint32_t pos = blockIdx.x; pos < LGPU_FRAME_ARG(kernarg_opaque(), FilteredArgs, nq);) {
        const uint32_t q = frame_query<FilteredArgs, EACH>(kernarg_opaque(), pos);
        int            cnt = 0;
        uint32_t       D = 0;
        {
            const KernargBytes ka = kernarg_opaque();
            View               v;
            LGPU_LOAD_VIEW(v, ka, FilteredArgs)
            if constexpr(METRIC >= M_PQD) LGPU_LOAD_VIEW_PQD(v, ka, FilteredArgs)
            float           qn2 = 0.f;
            if constexpr(!kAdcRows<METRIC>) {
                frame_stage<METRIC, G>(tid, T, s, LGPU_FRAME_ARG(ka, FilteredArgs, queries), q, v.chunks);
                qn2 = __int_as_float(s.scal[ S_QN2 ]);
            }
            const uint32_t *slots;
            int             count;
            if constexpr(EACH) {
                const FilterDesc *const d = LGPU_FARG(ka, descs) + q;
                slots = d->slots;
                count = (int)d->count;
            } else {
                slots = LGPU_FARG(ka, allow_slots);
                count = (int)LGPU_FARG(ka, allow_count);
            }
            int kk = 0;
            if constexpr(PARAMS) {
                const FilteredQueryParams p = filtered_query_params(ka, q);
                kk = (int)p.exp;
                if(p.k == 0) count = 0;  // no pass: D = 0
            }
            if constexpr(!PARAMS) kk = (int)LGPU_FARG(ka, exp);
            if constexpr(kAdcRows<METRIC>) {
                if(count > 0) filtered_adc_stage<METRIC>(tid, T, ka, s, q, v.chunks);  // (a query that evaluates a row: workgroup-uniform)
                qn2 = __int_as_float(s.scal[ S_QN2 ]);
            }
            const int R = 2 * NG;
            for(int base = 0, round = 0; base < count; base += R, ++round) {
                const int      nr = count - base < R ? count - base : R;
                const uint64_t worst = cnt == kk ? s.keys[ kk - 1 ] : ~0ull;
                int *const     any_slot = &s.scal[ (round & 1) ? S_ANY1 : S_ANY0 ];  // (by parity: a wave still reading the last round's)
                if(tid == 0) *any_slot = 0;
                __syncthreads();
                if(g < nr) {
                    const int      i = g, j = g + NG;
                    const uint32_t id0 = slots[ base + i ];
                    const uint32_t id1 = j < nr ? slots[ base + j ] : id0;
                    float          d0, d1;
                    group_dist2_n<METRIC, G>(walk_query<METRIC>(s), row_of_m<METRIC>(v, id0), row_of_m<METRIC>(v, id1), (int)v.chunks, gl, qn2,
                                             row_norm<METRIC>(v, id0), row_norm<METRIC>(v, id1), d0, d1);
                    if(gl == G - 1) {
                        const uint64_t k0 = make_key(d0, id0);
                        s.newkeys[ i ] = k0;
                        bool any = k0 < worst;
                        if(j < nr) {
                            const uint64_t k1 = make_key(d1, id1);
                            s.newkeys[ j ] = k1;
                            any |= k1 < worst;
                        }
                        if(any) *any_slot = 1;
                    }
                }
                __syncthreads();
                if(!*any_slot) continue;
                const int total = cnt + nr;
                for(int t = tid; t < total; t += T) {
                    const bool     is_new = t >= cnt;
                    const uint64_t k = is_new ? s.newkeys[ t - cnt ] : s.keys[ t ];
                    const int      below = count_below(s.newkeys, nr, k);
                    const int      p = is_new ? below + lower_bound_keys(s.keys, cnt, k) : t + below;
                    if(p < kk) s.keys2[ p ] = k;
                }
                cnt = total < kk ? total : kk;
                uint64_t *tmp = s.keys; s.keys = s.keys2; s.keys2 = tmp;
                __syncthreads();
            }
            D = (uint32_t)count;
        }
        const KernargBytes kb = kernarg_opaque();
        int                got;
        if constexpr(PARAMS) {  // (FilteredArgs::k: the width of an answer row)
            const FilteredQueryParams p = filtered_query_params(kb, q);
            got = frame_answer_rows<FilteredArgs>(tid, T, kb, s, q, cnt, p.k, p.skip, LGPU_FARG(kb, k));
        } else {
            const uint32_t k = LGPU_FARG(kb, k);
            got = frame_answer_rows<FilteredArgs>(tid, T, kb, s, q, cnt, k, LGPU_FARG(kb, skip), k);
        }
        pos = frame_close<FilteredArgs>(tid, kb, s, q, pos, got, D, 0);
    }
}

// one instantiation KERNEL<MM, GG, ...>: opt it in to its dynamic LDS size, then launch
#define LGPU_LAUNCH_FILTERED(KERNEL, LDS_, MM, GG, ...) LGPU_LAUNCH_LDS((KERNEL<MM, GG, __VA_ARGS__>), grid, 64 * waves, LDS_, stream, a)

// the forms of the two kernels by what a launch's arguments carry (`a`, `lds`, `grid`, `waves`, `stream` in scope): per-query parameters,
// seeds, a descriptor table, or a single filter
#define LGPU_FILTERED_WALK_FORMS(MM, GG)                                               \
    {                                                                                  \
        if(a.qparams && a.seeds) LGPU_LAUNCH_FILTERED(k_search_filtered, lds, MM, GG, true, true, true) \
        else if(a.qparams) LGPU_LAUNCH_FILTERED(k_search_filtered, lds, MM, GG, true, false, true) \
        else if(a.seeds) LGPU_LAUNCH_FILTERED(k_search_filtered, lds, MM, GG, true, true) \
        else if(a.descs) LGPU_LAUNCH_FILTERED(k_search_filtered, lds, MM, GG, true)    \
        else LGPU_LAUNCH_FILTERED(k_search_filtered, lds, MM, GG, false)               \
    }
#define LGPU_FILTERED_EXACT_FORMS(MM, GG)                                              \
    {                                                                                  \
        if(a.qparams) LGPU_LAUNCH_FILTERED(k_search_exact_allowed, lds, MM, GG, true, true) \
        else if(a.descs) LGPU_LAUNCH_FILTERED(k_search_exact_allowed, lds, MM, GG, true)    \
        else LGPU_LAUNCH_FILTERED(k_search_exact_allowed, lds, MM, GG, false)          \
    }

}  // namespace lgpu
