// search_filtered_screen_kernel.hip -- the SCREENED form of the filtered exact pass (search_filtered_kernel.hpp k_search_exact_allowed) for
// f32 l2sq / cosine rows of an index that holds the int8 screen copy of its rows (screen_rows_for: 128 to 500 chunks, so
// G = 64 lanes per f32 row).  Opt-in (lantern_gpu_set_filter_screen); filtered_plan.cpp decides, launch by launch.
//
// One workgroup of 512 threads per query, persistent by ticket, the frame query_frame.hpp's as the exact pass uses it.  A query's pass:
//   filling   -- until the list holds kk = k + skip keys there is no radius: rounds of R = 2 T / G = 16 allowed rows through the exact
//                pass's f32 round (group_dist2_n, two rows per 64-lane group) and its rank-merge, as today.
//   screening -- a screen round takes T / 8 = 64 consecutive entries of the slot list, eight lanes per screen row: a lane's uint4 of the
//                row are requested in blocks of NB, with the row's (s, r), before the first of a block is consumed, and summed by
//                integer dot4 against the query's (h, l) planes in LDS -- the load and LDS access shape of walk.hpp
//                hop_distances_screened, for its reasons.  The slot ids of the NEXT round are requested before this round's rows are
//                consumed.  Each group's last lane forms the walks' bound (same margin, same cases in which the test is
//                not made, same strictness) against the radius AS IT STOOD WHEN THE ROUND BEGAN and keeps the slot unless the bound puts
//                the row strictly outside it.  Kept slots go to a survivor queue in LDS: a ballot per wave, one LDS word per wave per
//                round (its count; every wave adds up the words of the waves in front of it), so the queue's order is the slot list's.
//   reading   -- no f32 row is read until the queue holds a full f32 round or the slot list ends.  Then one f32 round evaluates R queued
//                rows exactly as today (same routine, same summation order, same make_key), the rank-merge runs and the radius is
//                re-read.  With 1 - 3 % of the rows kept the f32 lanes would otherwise idle through every round.
// Queuing across rounds is sound because the radius only shrinks: a row kept against an older radius is at worst read needlessly; a
// rejected row's exact-order key is above the radius of its round, hence above the final one, hence in no answer.  So slots, distance
// bits, D (= allowed) and E (= 0) are k_search_exact_allowed's, bit for bit.
//
// LDS: the exact pass's carve (walk.hpp carve_walk with cap_max = R and no visited set), then the query's screen block (walk.hpp
// screen_stage_query builds it, once per ticket, behind frame_stage -- for a query whose slot list outlasts the filling), then the
// survivor queue: a ring of kQueueSlots slot ids (at most R - 1 left over + 64 of a round).  filtered_exact_screen_lds_bytes below is the
// carve's size for the launcher and for the plan.
// Diagnostics: rows bounded, rejected and read in f32 are tallied in LDS by thread 0 and added once per query to
// frame.totals[kFilterScreenTotals ..] (kernels.hpp; lantern_gpu_last_filtered_screen).
#include "search_filtered_kernel.hpp"

namespace lgpu {

namespace {

constexpr int      G = 64, GS = 8, NB = 3;  // lanes per f32 row, lanes per screen row, uint4 a lane requests before it consumes the first
constexpr int      R = 2 * kFilterScreenThreads / G;  // rows of an f32 round
constexpr uint32_t kQueueSlots = 128;
static_assert(kQueueSlots >= R - 1 + kFilterScreenRound && (kQueueSlots & (kQueueSlots - 1)) == 0, "the ring holds what an f32 round left and a screen round");

// scalar slots beyond the exact pass's (S_POS, S_QN2, S_ANY0, S_ANY1): a screen round's kept rows per wave, double-buffered by round
// parity (a wave still adding up the last round's), and the query's tallies
enum { X_WCNT0 = S_NNEW, X_WCNT1 = S_FRONT, X_BOUND = S_MASK, X_REJ, X_F32 };
constexpr int kWaves = kFilterScreenThreads / 64;
static_assert(X_WCNT0 + kWaves <= S_QN2 && X_WCNT1 + kWaves <= X_BOUND && X_F32 < S_SCALARS, "the slots are free in the exact pass and disjoint");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float    f32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) u32x4 *ScreenRow;
typedef const __attribute__((address_space(1))) f32x2 *ScreenMeta;

// The walks' bound on one screen row (walk.hpp "the int8 screen": the derivation, and hop_distances_screened: the steps, restated here in
// their order), by the eight lanes of a screen group.  True on the group's LAST lane iff the row's exact distance is strictly above
// key_dist(worst); false wherever the test is not made: a stored row whose meta says not ok, a cosine query norm outside the range, a
// NaN anywhere.
template <int METRIC>
__device__ __forceinline__ bool screen_rejects(ScreenRow screen, ScreenMeta screen_meta, uint32_t id, uint32_t chunks, uint32_t sch, const uint32_t *blk,
                                               int gsl, uint64_t worst, float qn2)
{
    const uint4 *const planes = (const uint4 *)(blk + 4);  // [sch][2]: h, l
    const ScreenRow    row = screen + (size_t)id * sch;
    const f32x2        meta = screen_meta[ id ];
    int                ih = 0, il = 0, c2 = 0;
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
    if(gsl != GS - 1) return false;
    bool        reject = false;
    const float sx = __uint_as_float(blk[ 0 ]), delta = __uint_as_float(blk[ 1 ]);
    const float fI = (float)(256.0 * (double)ih + (double)il);  // <X, c>: beyond int32 at d = 2000; exact in double, one rounding
    const float rd = key_dist(worst), e = fmaxf(0x1p-12f, (float)(2 * chunks + 64) * 0x1p-24f);
    if constexpr(METRIC == M_COS) {  // meta = (s / rb, rho); qn2 = ra; delta = dq
        if(screen_cos_norm_ok(qn2)) {
            const float sim8 = ((fI * sx) * meta.x) / qn2;
            const float ub = ((sim8 + meta.y * (1.f + delta)) + delta) + e;
            reject = (1.f - ub) - e > rd;
        }
    } else {  // meta = (s, r)
        const float ome = 1.f - e;
        if(screen_l2_scale_ok(meta.x)) {
            const float nx2 = __uint_as_float(blk[ 2 ]);
            const float Rt = (2.f * (sx * meta.x)) * fI, Q = (meta.x * meta.x) * (float)c2;
            const float m = ((nx2 - Rt) + Q) - 0x1p-20f * (nx2 + Q);
            if(__builtin_isfinite(m)) {
                const float a = (__builtin_sqrtf(fmaxf(m, 0.f)) * ome - meta.y) - delta;
                const float lb = a > 0.f ? a * a : 0.f;
                reject = lb > 0x1p-100f && lb * ome > rd;
            }
        }
    }
    return reject;
}

}  // namespace

// EACH, PARAMS: the forms of k_search_exact_allowed (search_filtered_kernel.hpp)
template <int METRIC, bool EACH, bool PARAMS>
__global__ void __launch_bounds__(kFilterScreenThreads) k_exact_allowed_screened(FilteredArgs)
{
    static_assert(METRIC == M_L2SQ || METRIC == M_COS, "the screen serves f32 l2sq and cosine rows");
    static_assert(EACH || !PARAMS, "the per-query-parameter form is instantiated in the per-query form only");
    const int tid = threadIdx.x, T = blockDim.x, g = tid / G, gl = tid % G, NG = T / G;
    const int gs = tid / GS, gsl = tid % GS, lane = tid & 63, wave = tid >> 6;
    WalkLds   s;
    uint32_t *queue;
    {
        const KernargBytes   ka = kernarg_opaque();
        const uint32_t       chunks = LGPU_VIEW_ARG(ka, FilteredArgs, chunks);
        unsigned char *const end = carve_walk(lgpu_smem, s, chunks, LGPU_FARG(ka, exp), R, 0);  // (s.vis: the screen block, as screen_query_block finds it)
        queue = (uint32_t *)(end + screen_query_lds_bytes(chunks));
    }
    for(uint32_t pos = blockIdx.x; pos < LGPU_FRAME_ARG(kernarg_opaque(), FilteredArgs, nq);) {
        const uint32_t q = frame_query<FilteredArgs, EACH>(kernarg_opaque(), pos);
        int            cnt = 0;
        uint32_t       D = 0;
        {
            const KernargBytes ka = kernarg_opaque();
            View               v;
            LGPU_LOAD_VIEW(v, ka, FilteredArgs)
            if(tid == 0) s.scal[ X_BOUND ] = 0, s.scal[ X_REJ ] = 0, s.scal[ X_F32 ] = 0;
            frame_stage<METRIC, G>(tid, T, s, LGPU_FRAME_ARG(ka, FilteredArgs, queries), q, v.chunks);
            const float     qn2 = __int_as_float(s.scal[ S_QN2 ]);
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
            // the rows of the filling rounds: whole rounds until the list is full
            const int fill = count < (kk + R - 1) / R * R ? count : (kk + R - 1) / R * R;
            if(fill < count) screen_stage_query<METRIC>(tid, s, v.chunks, qn2);  // (workgroup-uniform; ends in a barrier)

            // One f32 round of the exact pass over the nr <= R rows id_at(0 .. nr): keys, then the rank-merge where any of them beats the
            // list's worst.  Every thread calls it.
            int  f32_rounds = 0;
            auto f32_round = [ & ](auto id_at, const int nr) {
                const uint64_t worst = cnt == kk ? s.keys[ kk - 1 ] : ~0ull;
                int *const     any_slot = &s.scal[ (f32_rounds & 1) ? S_ANY1 : S_ANY0 ];  // (by parity: a wave still reading the last round's)
                f32_rounds += 1;
                if(tid == 0) { *any_slot = 0; s.scal[ X_F32 ] += nr; }
                __syncthreads();
                if(g < nr) {
                    const int      i = g, j = g + NG;
                    const uint32_t id0 = id_at(i);
                    const uint32_t id1 = j < nr ? id_at(j) : id0;
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
                if(!*any_slot) return;
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
            };

            // ---- filling
            for(int base = 0; base < fill; base += R) f32_round([ & ](int i) { return slots[ base + i ]; }, fill - base < R ? fill - base : R);

            // ---- screening and reading
            const ScreenRow       screen = (ScreenRow)(uint64_t)LGPU_VIEW_ARG(ka, FilteredArgs, screen);
            const ScreenMeta      screen_meta = (ScreenMeta)(uint64_t)LGPU_VIEW_ARG(ka, FilteredArgs, screen_meta);
            const uint32_t        sch = screen_chunks_for(v.chunks);
            const uint32_t *const blk = screen_query_block(s);
            int                   at = fill, head = 0, qcnt = 0;  // the next entry of the slot list; the queue is queue[head, head + qcnt) of the ring
            uint32_t              id_next = at + gs < count ? slots[ at + gs ] : EMPTY;
            for(int round = 0; at < count || qcnt > 0;) {
                if(qcnt >= R || at >= count) {
                    const int nr = qcnt < R ? qcnt : R;
                    f32_round([ & ](int i) { return queue[ (uint32_t)(head + i) & (kQueueSlots - 1) ]; }, nr);
                    head += nr;
                    qcnt -= nr;
                    continue;
                }
                const int      nrow = count - at < (int)kFilterScreenRound ? count - at : (int)kFilterScreenRound;
                const uint64_t worst = s.keys[ kk - 1 ];  // the radius as the round begins (the list is full: the filling is over)
                const uint32_t id = id_next;
                at += (int)kFilterScreenRound;
                id_next = at + gs < count ? slots[ at + gs ] : EMPTY;  // (the next round's ids: requested before this round's rows are consumed)
                bool keep = false;
                if(gs < nrow) {  // (all eight lanes of the group: the sums are theirs together)
                    const bool rejected = screen_rejects<METRIC>(screen, screen_meta, id, v.chunks, sch, blk, gsl, worst, qn2);
                    keep = gsl == GS - 1 && !rejected;
                }
                const unsigned long long m = __ballot(keep);
                int *const               wcnt = &s.scal[ (round & 1) ? X_WCNT1 : X_WCNT0 ];
                round += 1;
                if(lane == 0) wcnt[ wave ] = __popcll(m);
                __syncthreads();
                int before = 0, kept = 0;
                for(int w = 0; w < kWaves; ++w) {
                    const int c = wcnt[ w ];
                    kept += c;
                    before += w < wave ? c : 0;
                }
                if(keep) queue[ (uint32_t)(head + qcnt + before + __popcll(m & ((1ull << lane) - 1ull))) & (kQueueSlots - 1) ] = id;
                if(tid == 0) { s.scal[ X_BOUND ] += nrow; s.scal[ X_REJ ] += nrow - kept; }
                qcnt += kept;  // (the f32 round that reads the queue begins with a barrier)
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
        if(tid == 0) {
            unsigned long long *const totals = LGPU_FRAME_ARG(kb, FilteredArgs, totals);
            if(totals && s.scal[ X_F32 ]) {
                atomicAdd(&totals[ kFilterScreenTotals + 0 ], (unsigned long long)(uint32_t)s.scal[ X_BOUND ]);
                atomicAdd(&totals[ kFilterScreenTotals + 1 ], (unsigned long long)(uint32_t)s.scal[ X_REJ ]);
                atomicAdd(&totals[ kFilterScreenTotals + 2 ], (unsigned long long)(uint32_t)s.scal[ X_F32 ]);
            }
        }
        pos = frame_close<FilteredArgs>(tid, kb, s, q, pos, got, D, 0);
    }
}

uint32_t filtered_screen_queue_slots(uint32_t rows_per_round)
{
    uint32_t n = 1;
    while(n < rows_per_round - 1 + kFilterScreenRound) n *= 2;
    return n;
}
size_t filtered_exact_screen_lds_bytes(uint32_t chunks, uint32_t kk, uint32_t rows_per_round)
{
    return filtered_exact_lds_bytes(chunks, kk, rows_per_round) + screen_query_lds_bytes(chunks) + (size_t)filtered_screen_queue_slots(rows_per_round) * 4;
}

// the three forms by what the launch's arguments carry, as LGPU_FILTERED_EXACT_FORMS
#define LGPU_SCREENED_EXACT_FORMS(MM)                                                                                                   \
    {                                                                                                                                   \
        if(a.qparams) LGPU_LAUNCH_LDS((k_exact_allowed_screened<MM, true, true>), grid, kFilterScreenThreads, lds, stream, a)           \
        else if(a.descs) LGPU_LAUNCH_LDS((k_exact_allowed_screened<MM, true, false>), grid, kFilterScreenThreads, lds, stream, a)       \
        else LGPU_LAUNCH_LDS((k_exact_allowed_screened<MM, false, false>), grid, kFilterScreenThreads, lds, stream, a)                  \
    }

hipError_t launch_exact_allowed_screened(int metric, const FilteredArgs &a, int grid, hipStream_t stream)
{
    if(!a.view.screen || !a.view.screen_meta || !screen_rows_for(a.view.chunks) || a.rows_per_round != (uint32_t)R ||
       filtered_screen_queue_slots(a.rows_per_round) != kQueueSlots || (a.qparams && !a.descs))
        return hipErrorInvalidValue;
    const size_t lds = filtered_exact_screen_lds_bytes(a.view.chunks, a.exp, a.rows_per_round);
    if(metric == M_L2SQ) LGPU_SCREENED_EXACT_FORMS(M_L2SQ)
    else if(metric == M_COS) LGPU_SCREENED_EXACT_FORMS(M_COS)
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace lgpu
