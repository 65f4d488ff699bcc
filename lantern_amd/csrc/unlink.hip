// unlink.hip -- deleting rows of a resident index (include/lantern_gpu.h "Deleting rows").
//
//   lantern_gpu_remove_labels   ldb_ambulkdelete for the resident copy: the slots whose label is in a list get label 0
//                               (INVALID_ELEMENT_LABEL, hnsw.h:40).  The list is sorted on the device (rocPRIM, as filter.hip),
//                               k_remove_labels binary-searches it once per slot.  Only labels change.
//   lantern_gpu_unlink_deleted  takes the tombstones (label 0) out of the graph: every live list that holds one is stripped of
//                               them and offered the tombstones' own live neighbours as reverse-link requests, which the build's
//                               grouping pass and k_revlink_* apply unchanged.
//       k_unlink_flag      one thread per live node: the (node, level) lists that hold a tombstone -> the work list
//       k_unlink_count     one workgroup per work item: keep / offers in LDS, the number of offers (sizes the request array)
//       k_unlink_requests  the same, then metric(offer, p) by the walk's row routine (one request per offer, in offer order) and
//                          the stripped list written in place
//       k_unlink_clear     every tombstone's own lists emptied
//
// Why the stripped list goes straight into the adjacency: a work item (p, l) reads p's list at l and the lists of the TOMBSTONES
// in it.  p is live, so no other work item reads p's list; the tombstones' lists are written by k_unlink_clear only, behind every
// request and reverse-link kernel.  All reads are therefore of the graph as the call found it, whatever order the items run in,
// and the requests may be produced and applied in several rounds (a bounded request array).
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "abi_guard.hpp"
#include "dispatch.hpp"
#include "index.hpp"

namespace lgpu {

// ---- removal ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_remove_labels(uint64_t *slot_labels, size_t n, const uint64_t *sorted, size_t m, unsigned long long *removed)
{
    const size_t slot = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool         hit = false;
    if(slot < n) {
        const uint64_t l = slot_labels[ slot ];
        if(l != 0) {  // a slot that is 0 already does not count, and 0 in the list names nobody
            size_t lo = 0, hi = m;
            while(lo < hi) {
                const size_t mid = (lo + hi) >> 1;
                if(sorted[ mid ] < l) lo = mid + 1; else hi = mid;
            }
            hit = lo < m && sorted[ lo ] == l;
            if(hit) slot_labels[ slot ] = 0;
        }
    }
    const unsigned long long mask = __ballot(hit);
    if(mask && (int)(threadIdx.x & 63) == __builtin_ctzll(mask)) atomicAdd(removed, (unsigned long long)__popcll(mask));
}

// ---- unlink: the work list -------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_tombstone(const View &v, const uint64_t *labels, uint32_t slot) { return slot < v.n && labels[ slot ] == 0; }

__global__ void __launch_bounds__(256) k_unlink_flag(View v, const uint64_t *labels, uint2 *items, uint32_t *nitems)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if(p >= v.n || labels[ p ] == 0) return;
    const int top = (int)v.levels[ p ];
    for(int level = 0; level <= top; ++level) {
        uint32_t        cap;
        const uint32_t *list = neighbors_of(v, p, level, cap);
        bool            any = false;
        for(uint32_t i = 0; i < cap && !any; ++i) {
            const uint32_t e = list[ i ];
            if(e == EMPTY) break;
            any = is_tombstone(v, labels, e);
        }
        if(any) items[ atomicAdd(nitems, 1u) ] = make_uint2(p, (uint32_t)level);
    }
}

// ---- unlink: keep and offers of one (p, level), in LDS ---------------------------------------------------------------------------
__host__ __device__ inline uint32_t unlink_cut(uint32_t cap) { return 8 * cap > 256 ? 8 * cap : 256; }
__host__ __device__ inline uint32_t unlink_up4(uint32_t x) { return (x + 3) & ~3u; }
// keep[M0] | tomb[M0] | offers[cut(M0)] | round[256] | wave sums[4]
__host__ __device__ inline size_t unlink_lds_bytes(uint32_t M0) { return ((size_t)2 * unlink_up4(M0) + unlink_cut(M0) + 256 + 4) * 4; }
struct UnlinkLds
{
    uint32_t *keep, *tomb, *offers, *round, *wsum;
};
__device__ __forceinline__ UnlinkLds unlink_carve(uint32_t M0)
{
    UnlinkLds s;
    s.keep = (uint32_t *)lgpu_smem;
    s.tomb = s.keep + unlink_up4(M0);
    s.offers = s.tomb + unlink_up4(M0);
    s.round = s.offers + unlink_cut(M0);
    s.wsum = s.round + 256;
    return s;
}
// Position of this thread's element among the flagged elements of the workgroup (256 threads) in thread order, and how many there
// are.  Every thread calls it.
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t *wsum, uint32_t &total)
{
    const unsigned long long m = __ballot(flag);
    const int                lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    const uint32_t           below = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();  // the previous call's sums have been read
    if(lane == 0) wsum[ w ] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t base = 0;
    total = 0;
    for(int i = 0; i < 4; ++i) {
        if(i < w) base += wsum[ i ];
        total += wsum[ i ];
    }
    return base + below;
}
// keep = the live entries of p's list in stored order; offers = walking the list in stored order, the live entries of every
// tombstoned entry's own list at this level in stored order, without p, what is in keep and what was offered before, cut at
// cut(level).  The candidates are taken 256 at a time in that order; a round drops the ones an earlier thread of the round holds
// (equal slots are equally admissible, so the first of them decides for all) and appends the rest by their rank.
__device__ __forceinline__ void unlink_collect(const View &v, const uint64_t *labels, uint32_t p, int level, const UnlinkLds &s, uint32_t &cap,
                                               uint32_t &nkeep, uint32_t &noff)
{
    const uint32_t  tid = threadIdx.x;
    const uint32_t *list = neighbors_of(v, p, level, cap);
    uint32_t        nk = 0, nt = 0, tot;
    for(uint32_t base = 0; base < cap; base += 256) {
        const uint32_t i = base + tid;
        const uint32_t e = i < cap ? list[ i ] : EMPTY;
        const bool     valid = e != EMPTY && e < v.n;
        const bool     dead = valid && labels[ e ] == 0;
        uint32_t       r = block_rank(valid && !dead, s.wsum, tot);
        if(valid && !dead) s.keep[ nk + r ] = e;
        nk += tot;
        r = block_rank(dead, s.wsum, tot);
        if(dead) s.tomb[ nt + r ] = e;
        nt += tot;
    }
    __syncthreads();
    const uint32_t cut = unlink_cut(cap), stream = nt * cap;
    uint32_t       no = 0;
    for(uint32_t base = 0; base < stream && no < cut; base += 256) {
        const uint32_t j = base + tid;
        uint32_t       c = EMPTY;
        if(j < stream) {
            const uint32_t t = s.tomb[ j / cap ];
            if((int)v.levels[ t ] >= level) {
                uint32_t tc;
                c = neighbors_of(v, t, level, tc)[ j % cap ];
            }
        }
        bool ok = c != EMPTY && c < v.n && c != p && labels[ c ] != 0;
        for(uint32_t i = 0; ok && i < nk; ++i) ok = s.keep[ i ] != c;
        for(uint32_t i = 0; ok && i < no; ++i) ok = s.offers[ i ] != c;
        s.round[ tid ] = ok ? c : EMPTY;
        __syncthreads();
        for(uint32_t i = 0; ok && i < tid; ++i) ok = s.round[ i ] != c;
        const uint32_t r = block_rank(ok, s.wsum, tot);
        if(ok && no + r < cut) s.offers[ no + r ] = c;
        no = no + tot < cut ? no + tot : cut;
        __syncthreads();  // the offers are visible, round[] is free
    }
    nkeep = nk;
    noff = no;
}

__global__ void __launch_bounds__(256) k_unlink_count(View v, const uint64_t *labels, const uint2 *items, uint32_t nitems, uint32_t *counts)
{
    const UnlinkLds s = unlink_carve(v.M0);
    for(uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {
        uint32_t cap, nkeep, noff;
        unlink_collect(v, labels, items[ it ].x, (int)items[ it ].y, s, cap, nkeep, noff);
        if(threadIdx.x == 0) counts[ it ] = noff;
        __syncthreads();
    }
}

// The hot kernel: items [first, first + count) of the work list.  The requests of item `it` lie at reqs[off[it] - off[first] ..), in
// offer order -- the stable sort of the grouping pass keeps that order inside the (p, level) group.  d = metric(offer, p) by the
// walk's row routine at the walk's group width, two offers against p's row at a time (group_dist2_n: both rows' loads of a block
// in flight together), so a request's d has usearch_distance's bits.
template <int METRIC, int G>
__global__ void __launch_bounds__(256) k_unlink_requests(View v, const uint64_t *labels, const uint2 *items, const uint64_t *off, uint32_t first,
                                                         uint32_t count, LinkReq *reqs)
{
    const UnlinkLds s = unlink_carve(v.M0);
    const int       tid = (int)threadIdx.x, g = tid / G, gl = tid % G;
    constexpr int   NG = 256 / G;
    for(uint32_t it = first + blockIdx.x; it < first + count; it += gridDim.x) {
        const uint32_t p = items[ it ].x;
        const int      level = (int)items[ it ].y;
        uint32_t       cap, nkeep, noff;
        unlink_collect(v, labels, p, level, s, cap, nkeep, noff);
        uint32_t *list = neighbors_of(v, p, level, cap);
        for(uint32_t i = (uint32_t)tid; i < cap; i += 256) list[ i ] = i < nkeep ? s.keep[ i ] : EMPTY;  // compacted, no holes
        LinkReq    *out = reqs + (size_t)(off[ it ] - off[ first ]);
        const float pn = row_norm<METRIC>(v, p);
        for(uint32_t o = 2 * (uint32_t)g; o < noff; o += 2 * NG) {
            const uint32_t c0 = s.offers[ o ], c1 = o + 1 < noff ? s.offers[ o + 1 ] : c0;
            float          d0, d1;
            group_dist2_n<METRIC, G>(row_of(v, p), row_of(v, c0), row_of(v, c1), (int)v.chunks, gl, pn, row_norm<METRIC>(v, c0), row_norm<METRIC>(v, c1), d0, d1);
            if(gl == G - 1) {
                LinkReq r;
                r.close = p, r.level = (uint32_t)level, r.new_slot = c0, r.d = d0;
                out[ o ] = r;
                if(o + 1 < noff) {
                    r.new_slot = c1, r.d = d1;
                    out[ o + 1 ] = r;
                }
            }
        }
        __syncthreads();  // the next item reuses the LDS
    }
}

__global__ void __launch_bounds__(256) k_unlink_clear(View v, const uint64_t *labels, uint32_t *cleared)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= v.n || labels[ t ] != 0) return;
    bool      any = false;
    const int top = (int)v.levels[ t ];
    for(int level = 0; level <= top; ++level) {
        uint32_t  cap;
        uint32_t *list = neighbors_of(v, t, level, cap);
        for(uint32_t i = 0; i < cap; ++i)
            if(list[ i ] != EMPTY) { list[ i ] = EMPTY; any = true; }
    }
    if(any) atomicAdd(cleared, 1u);
}

static hipError_t launch_unlink_requests(int metric, const View &v, const uint64_t *labels, const uint2 *items, const uint64_t *off, uint32_t first,
                                         uint32_t count, LinkReq *reqs, int grid, hipStream_t stream)
{
    const size_t lds = unlink_lds_bytes(v.M0);
#define CALL(MM, GG) hipLaunchKernelGGL((k_unlink_requests<MM, GG>), dim3(grid), dim3(256), lds, stream, v, labels, items, off, first, count, reqs)
    LGPU_DISPATCH(metric, v.chunks, CALL);
#undef CALL
    return hipGetLastError();
}

static const char *kUnlinkFailed = "lantern_gpu: HIP failure while unlinking deleted rows";
constexpr size_t   kUnlinkRound = (size_t)4 << 20;  // requests produced and applied per round (64 MiB of requests, as much again sorted)

// The caller holds ix->mu and has flushed.  false -> ix->err.
static bool remove_labels_locked(Index *ix, const uint64_t *labels, size_t m, uint64_t &removed)
{
    removed = 0;
    if(m == 0 || ix->n == 0) return true;
    unsigned long long *d_removed = (unsigned long long *)scratch(ix, kScratchCallOut, 64);
    if(!d_removed) return false;
    if(!order_launch(ix, ix->stream)) return false;  // as an insertion batch: behind every search in flight
    uint64_t *d_in = nullptr, *d_sorted = nullptr;
    void     *temp = nullptr;
    size_t    temp_bytes = 0;
    unsigned long long h_removed = 0;
    bool ok = hipMalloc((void **)&d_in, m * 8) == hipSuccess && hipMalloc((void **)&d_sorted, m * 8) == hipSuccess &&
              hipMemcpyAsync(d_in, labels, m * 8, hipMemcpyHostToDevice, ix->stream) == hipSuccess &&
              hipMemsetAsync(d_removed, 0, 8, ix->stream) == hipSuccess &&
              rocprim::radix_sort_keys(nullptr, temp_bytes, (const uint64_t *)d_in, d_sorted, m, 0u, 64u, ix->stream) == hipSuccess &&
              hipMalloc(&temp, std::max<size_t>(temp_bytes, 16)) == hipSuccess &&
              rocprim::radix_sort_keys(temp, temp_bytes, (const uint64_t *)d_in, d_sorted, m, 0u, 64u, ix->stream) == hipSuccess;
    if(ok) {
        hipLaunchKernelGGL(k_remove_labels, dim3((unsigned)((ix->n + 255) / 256)), dim3(256), 0, ix->stream, ix->d_labels, ix->n, (const uint64_t *)d_sorted, m,
                           d_removed);
        ok = hipGetLastError() == hipSuccess && record_launch(ix, ix->stream) &&  // searches on other streams wait for it
             hipMemcpyAsync(&h_removed, d_removed, 8, hipMemcpyDeviceToHost, ix->stream) == hipSuccess &&
             hipMemcpyAsync(ix->labels.data(), ix->d_labels, ix->n * 8, hipMemcpyDeviceToHost, ix->stream) == hipSuccess;  // the host mirror
    }
    ok = hipStreamSynchronize(ix->stream) == hipSuccess && ok;
    if(d_in) (void)hipFree(d_in);
    if(d_sorted) (void)hipFree(d_sorted);
    if(temp) (void)hipFree(temp);
    if(!ok) {
        if(ix->err.empty()) set_err(ix, "lantern_gpu: HIP failure while removing labels");
        return false;
    }
    removed = h_removed;
    return true;
}

static size_t deleted_count_locked(const Index *ix) { return (size_t)std::count(ix->labels.begin(), ix->labels.begin() + (ptrdiff_t)ix->n, (uint64_t)0); }

// The caller holds ix->mu, has flushed and has refused the index forms the unlink does not serve.  false -> ix->err.
static bool unlink_locked(Index *ix, lantern_gpu_unlink_stats &st)
{
    const size_t n = ix->n, dead = deleted_count_locked(ix);
    if(dead == 0 || dead == n) return true;
    const size_t max_items = n + ix->upper_blocks;
    // items | offsets | counts | nitems, cleared
    const size_t at_off = max_items * 8, at_counts = at_off + (max_items + 1) * 8, at_ctr = at_counts + (max_items + 3) / 4 * 16;
    char *blk = (char *)scratch(ix, kScratchCallIn, at_ctr + 16);
    if(!blk) return false;
    uint2    *d_items = (uint2 *)blk;
    uint64_t *d_off = (uint64_t *)(blk + at_off);
    uint32_t *d_counts = (uint32_t *)(blk + at_counts), *d_ctr = (uint32_t *)(blk + at_ctr);
    if(!order_launch(ix, ix->stream)) return false;  // a graph mutation: ordered as an insertion batch
    const View v = ix->view();
    HIPCHK(ix, hipMemsetAsync(d_ctr, 0, 16, ix->stream));
    HIPCHK(ix, hipMemsetAsync(ix->d_totals + kTotUnlink, 0, 16, ix->stream));
    hipLaunchKernelGGL(k_unlink_flag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ix->stream, v, (const uint64_t *)ix->d_labels, d_items, d_ctr);
    HIPCHK(ix, hipGetLastError());
    uint32_t nitems = 0;
    HIPCHK(ix, hipMemcpyAsync(&nitems, d_ctr, 4, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(ix, hipStreamSynchronize(ix->stream));
    if(nitems > max_items) { set_err(ix, kUnlinkFailed); return false; }
    uint64_t offers = 0, cut_lists = 0;
    if(nitems) {
        const size_t lds = unlink_lds_bytes(ix->M0);
        const int    grid = (int)std::min<size_t>(nitems, (size_t)ix->num_cus * 32);
        hipLaunchKernelGGL(k_unlink_count, dim3(grid), dim3(256), lds, ix->stream, v, (const uint64_t *)ix->d_labels, (const uint2 *)d_items, nitems, d_counts);
        HIPCHK(ix, hipGetLastError());
        std::vector<uint32_t> counts(nitems);
        std::vector<uint2>    items(nitems);
        std::vector<uint64_t> off((size_t)nitems + 1, 0);
        HIPCHK(ix, hipMemcpyAsync(counts.data(), d_counts, (size_t)nitems * 4, hipMemcpyDeviceToHost, ix->stream));
        HIPCHK(ix, hipMemcpyAsync(items.data(), d_items, (size_t)nitems * 8, hipMemcpyDeviceToHost, ix->stream));
        HIPCHK(ix, hipStreamSynchronize(ix->stream));
        size_t round_max = 0;
        for(uint32_t i = 0; i < nitems; ++i) {
            off[ i + 1 ] = off[ i ] + counts[ i ];
            cut_lists += counts[ i ] == unlink_cut(items[ i ].y == 0 ? ix->M0 : ix->M);
        }
        offers = off[ nitems ];
        // the rounds: whole items, at most kUnlinkRound requests each (an item has at most cut(0) <= 4096)
        std::vector<uint32_t> bounds{ 0 };
        for(uint32_t a = 0; a < nitems;) {
            uint32_t b = a + 1;
            while(b < nitems && off[ b + 1 ] - off[ a ] <= kUnlinkRound) ++b;
            round_max = std::max<size_t>(round_max, (size_t)(off[ b ] - off[ a ]));
            bounds.push_back(b);
            a = b;
        }
        HIPCHK(ix, hipMemcpyAsync(d_off, off.data(), ((size_t)nitems + 1) * 8, hipMemcpyHostToDevice, ix->stream));
        const size_t R = std::max<size_t>(round_max, 1), temp_bytes = group_temp_bytes(R);
        LinkReq *d_links = (LinkReq *)scratch(ix, kScratchLinks, R * sizeof(LinkReq));
        LinkReq *d_reqs = (LinkReq *)scratch(ix, kScratchReqs, R * sizeof(LinkReq));
        char    *d_grp = (char *)scratch(ix, kScratchGroups, R * sizeof(uint2) + 16 + 4);
        void    *d_work = scratch(ix, kScratchWork, R * 8 + 16);
        char    *d_sort = (char *)scratch(ix, kScratchSort, R * 24 + temp_bytes + 64);
        if(!d_links || !d_reqs || !d_grp || !d_work || !d_sort) return false;
        GroupScratch gs;
        gs.keys_a = (uint64_t *)d_sort;
        gs.keys_b = gs.keys_a + R;
        gs.idx_a = (uint32_t *)(gs.keys_b + R);
        gs.idx_b = gs.idx_a + R;
        gs.temp = (void *)(((uintptr_t)(gs.idx_b + R) + 63) & ~(uintptr_t)63);
        gs.temp_bytes = temp_bytes;
        uint2    *d_groups = (uint2 *)d_grp;
        uint32_t *d_ngroups = (uint32_t *)(d_grp + R * sizeof(uint2));
        for(size_t r = 0; r + 1 < bounds.size(); ++r) {
            const uint32_t a = bounds[ r ], b = bounds[ r + 1 ];
            const uint32_t nreq = (uint32_t)(off[ b ] - off[ a ]);
            HIPCHK(ix, launch_unlink_requests(ix->mcode, v, ix->d_labels, d_items, d_off, a, b - a, d_links,
                                              (int)std::min<size_t>(b - a, (size_t)ix->num_cus * 32), ix->stream));
            if(nreq == 0) continue;
            // the build's own grouping pass and reverse-link kernels, on lists without holes
            HIPCHK(ix, launch_group_requests(d_links, nreq, gs, d_reqs, d_groups, d_ngroups, 1, 0, d_ngroups + 4, ix->stream, (uint32_t *)d_work));
            RevlinkArgs ra;
            ra.view = v;
            ra.ngroups = d_ngroups;
            ra.groups = d_groups;
            ra.max_groups = std::min<uint32_t>(nreq, b - a);
            ra.reqs = d_reqs;
            ra.totals = ix->d_totals + kTotUnlink;  // a range of its own: lantern_gpu_counters' build counters do not move
            ra.radius0 = ra.radius_upper = nullptr;  // no list here is as a re-prune left it; the state is reset before its next use
            HIPCHK(ix, launch_revlink(ix->mcode, ra, (char *)d_work + 16, (uint32_t *)d_work, ix->num_cus, ix->stream, true));
        }
    }
    ix->radius_stale = true;
    hipLaunchKernelGGL(k_unlink_clear, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ix->stream, v, (const uint64_t *)ix->d_labels, d_ctr + 1);
    HIPCHK(ix, hipGetLastError());
    if(!record_launch(ix, ix->stream)) return false;  // behind the last kernel that rewrites lists
    uint32_t           cleared = 0;
    unsigned long long tot[ 2 ] = {};
    HIPCHK(ix, hipMemcpyAsync(&cleared, d_ctr + 1, 4, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(ix, hipMemcpyAsync(tot, ix->d_totals + kTotUnlink, 16, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(ix, hipStreamSynchronize(ix->stream));
    st.tombstones_unlinked = cleared;
    st.lists_repaired = nitems;
    st.offers = offers;
    st.lists_cut = cut_lists;
    st.request_evals = offers;
    st.reprune_evals = tot[ 0 ];
    if(ix->entry < n && ix->labels[ ix->entry ] == 0) {  // the live node of the highest level, the lowest slot among those
        uint32_t best = EMPTY;
        int      best_level = -1;
        for(size_t i = 0; i < n; ++i)
            if(ix->labels[ i ] != 0 && (int)ix->levels[ i ] > best_level) best = (uint32_t)i, best_level = (int)ix->levels[ i ];
        ix->entry = best;
        ix->max_level = best_level;
        st.entry_moved = 1;
    }
    return true;
}

// ---- compaction (kernels: compact.hip) ------------------------------------------------------------------------------------------
// The arithmetic of the renumbering on the host: what lantern_gpu_plan_compact shows and what the device's two scans must agree with.
static void plan_compact_host(const uint64_t *labels, const uint8_t *levels, size_t n, uint32_t *slot_map, uint32_t *upper_off_new, uint64_t &live,
                              uint64_t &blocks)
{
    live = blocks = 0;
    for(size_t s = 0; s < n; ++s) {
        if(labels[ s ] == 0) {
            if(slot_map) slot_map[ s ] = EMPTY;
            continue;
        }
        if(slot_map) slot_map[ s ] = (uint32_t)live;
        if(upper_off_new) upper_off_new[ live ] = (uint32_t)blocks;
        ++live;
        blocks += levels[ s ];
    }
}

// the device arrays of an index that grow with its capacity, as reserve_locked sizes and fills them
struct CompactArrays
{
    uint4    *vec = nullptr, *screen = nullptr;
    float    *norm2 = nullptr, *radius0 = nullptr, *radius_upper = nullptr;
    float2   *screen_meta = nullptr;
    uint8_t  *codes = nullptr, *levels = nullptr;
    uint64_t *labels = nullptr;
    uint32_t *nbr0 = nullptr, *upper_off = nullptr, *upper_nbr = nullptr;
    void     *temp = nullptr;  // the map's block (CompactMap)
    void release()
    {
        void *all[] = { vec, screen, norm2, radius0, radius_upper, screen_meta, codes, levels, labels, nbr0, upper_off, upper_nbr, temp };
        for(void *p : all)
            if(p) (void)hipFree(p);
        *this = CompactArrays();
    }
};

static const char *kCompactFailed = "lantern_gpu: HIP failure while compacting the index";

// The caller holds ix->mu, has flushed, has refused the index forms the compaction does not serve and has unlinked.  `dead` > 0.
// false -> ix->err, and the index is exactly as it was: the new arrays are built beside the old ones and swapped in after the last
// kernel has succeeded (transient peak: old + new + 20 bytes per old slot for the map).
static bool compact_locked(Index *ix, size_t capacity, uint32_t *slot_map, lantern_gpu_compact_stats &st)
{
    const size_t n = ix->n;
    uint64_t     live = 0, blocks = 0;
    plan_compact_host(ix->labels.data(), ix->levels.data(), n, nullptr, nullptr, live, blocks);
    const size_t newcap = std::max<size_t>((size_t)live, capacity);
    if(newcap >= 0x7FFFFFFFull) { set_err(ix, "lantern_gpu: capacity above 2^31-1 slots is not supported"); return false; }
    const size_t row = (size_t)ix->chunks * 16, srow = ix->d_screen ? (size_t)screen_chunks_for(ix->chunks) * 16 : 0, codes = ix->pq ? ix->pq_S : 0;
    const size_t M0 = ix->M0, M = ix->M;
    const size_t temp_bytes = compact_temp_bytes(n), words = n + 1;
    const size_t map_bytes = 5 * words * 4 + ((temp_bytes + 63) & ~(size_t)63) + 64;
    // what one slot costs in the arrays sized by capacity (lantern_gpu_memory_usage's terms)
    const size_t per_slot = row + srow + (srow ? 8 : 0) + codes + M0 * 4 + 8 + 1 + 4 + 4 + (ix->d_norm2 ? 4 : 0);
    const size_t need = newcap * per_slot + (size_t)blocks * (M * 4 + 4) + map_bytes;
    size_t rb = 0, ob = 0;
    index_memory_bytes(ix, rb, ob);
    st.rows_before = n;
    st.upper_blocks_before = ix->upper_blocks;
    st.bytes_before = rb + ob;

    CompactArrays a;
    auto          take = [&](void **p, size_t bytes) { return hipMalloc(p, std::max<size_t>(bytes, 16)) == hipSuccess; };
    bool got = take(&a.temp, map_bytes) && take((void **)&a.labels, newcap * 8) && take((void **)&a.levels, newcap) && take((void **)&a.nbr0, newcap * M0 * 4) &&
               take((void **)&a.upper_off, newcap * 4) && take((void **)&a.radius0, newcap * 4) && take((void **)&a.upper_nbr, (size_t)blocks * M * 4) &&
               take((void **)&a.radius_upper, (size_t)blocks * 4) && take((void **)&a.vec, newcap * row);
    if(got && ix->d_norm2) got = take((void **)&a.norm2, newcap * 4);
    if(got && srow) got = take((void **)&a.screen, newcap * srow) && take((void **)&a.screen_meta, newcap * 8);
    if(got && codes) got = take((void **)&a.codes, newcap * codes);
    if(!got) {
        a.release();
        set_err(ix, "lantern_gpu: out of device memory: the compaction builds the new arrays beside the old ones and needs " + std::to_string(need) +
                        " bytes for them; the index is unchanged");
        return false;
    }
    auto fail = [&](const std::string &msg) {
        (void)hipStreamSynchronize(ix->stream);
        a.release();
        set_err(ix, msg);
        return false;
    };
    CompactMap m;
    m.flags = (uint32_t *)a.temp;
    m.lv = m.flags + words;
    m.map = m.lv + words;
    m.uoff = m.map + words;
    m.src_of = m.uoff + words;
    m.temp = (void *)(((uintptr_t)(m.src_of + words) + 63) & ~(uintptr_t)63);
    m.temp_bytes = temp_bytes;
    unsigned long long *d_dangling = (unsigned long long *)scratch(ix, kScratchCallOut, 64);
    if(!d_dangling || !order_launch(ix, ix->stream)) return fail(kCompactFailed);  // a graph mutation: ordered as an insertion batch
    hipStream_t q = ix->stream;
    // the tails beyond the live slots, as reserve_locked fills a grown array
    bool ok = hipMemsetAsync(d_dangling, 0, 8, q) == hipSuccess && hipMemsetAsync(a.levels, 0, std::max<size_t>(newcap, 16), q) == hipSuccess &&
              hipMemsetAsync(a.nbr0, 0xFF, std::max<size_t>(newcap * M0 * 4, 16), q) == hipSuccess &&
              hipMemsetAsync(a.upper_off, 0xFF, std::max<size_t>(newcap * 4, 16), q) == hipSuccess &&
              hipMemsetAsync(a.radius0, 0xFF, std::max<size_t>(newcap * 4, 16), q) == hipSuccess &&
              hipMemsetAsync(a.radius_upper, 0xFF, std::max<size_t>((size_t)blocks * 4, 16), q) == hipSuccess;
    if(ok && a.screen && newcap > live)
        ok = hipMemsetAsync((char *)a.screen + (size_t)live * srow, 0, (newcap - (size_t)live) * srow, q) == hipSuccess &&
             hipMemsetAsync(a.screen_meta + live, 0, (newcap - (size_t)live) * 8, q) == hipSuccess;
    if(ok && a.codes && newcap > live) ok = hipMemsetAsync(a.codes + (size_t)live * codes, 0, (newcap - (size_t)live) * codes, q) == hipSuccess;
    if(!ok) return fail(kCompactFailed);
    CompactMeta cm;
    cm.labels = ix->d_labels, cm.new_labels = a.labels;
    cm.levels = ix->d_levels, cm.new_levels = a.levels;
    cm.norm2 = ix->d_norm2, cm.new_norm2 = a.norm2;
    cm.screen_meta = ix->d_screen_meta, cm.new_screen_meta = a.screen_meta;
    cm.new_upper_off = a.upper_off;
    hipEvent_t ev[ 4 ] = {};  // all kernels: [0, 3]; the row kernel over the vector block: [1, 2] (lantern_gpu_last_compact_ms)
    for(hipEvent_t &x : ev) ok = ok && hipEventCreate(&x) == hipSuccess;
    auto drop_events = [&] {
        for(hipEvent_t x : ev)
            if(x) (void)hipEventDestroy(x);
    };
    ok = ok && hipEventRecord(ev[ 0 ], q) == hipSuccess && launch_compact_map(ix->d_labels, ix->d_levels, n, m, q) == hipSuccess &&
         hipEventRecord(ev[ 1 ], q) == hipSuccess && launch_compact_rows(ix->d_vec, a.vec, m.src_of, (size_t)live, row, ix->num_cus, q) == hipSuccess &&
         hipEventRecord(ev[ 2 ], q) == hipSuccess &&
         (!srow || launch_compact_rows(ix->d_screen, a.screen, m.src_of, (size_t)live, srow, ix->num_cus, q) == hipSuccess) &&
         (!codes || launch_compact_rows(ix->d_codes, a.codes, m.src_of, (size_t)live, codes, ix->num_cus, q) == hipSuccess) &&
         launch_compact_lists(ix->d_nbr0, a.nbr0, m, (uint32_t)n, (size_t)live, (uint32_t)M0, nullptr, nullptr, d_dangling, ix->num_cus, q) == hipSuccess &&
         (!blocks || launch_compact_lists(ix->d_upper_nbr, a.upper_nbr, m, (uint32_t)n, (size_t)live, (uint32_t)M, ix->d_levels, ix->d_upper_off, d_dangling,
                                          ix->num_cus, q) == hipSuccess) &&
         launch_compact_meta(cm, m, (size_t)live, q) == hipSuccess && hipEventRecord(ev[ 3 ], q) == hipSuccess;
    if(!ok) { drop_events(); return fail(kCompactFailed); }
    // the map, the totals of the two scans, the check and the host mirrors of the new slots
    std::vector<uint32_t> h_map(words), h_uoff((size_t)live);
    std::vector<uint64_t> h_labels((size_t)live);
    std::vector<uint8_t>  h_levels((size_t)live);
    unsigned long long    dangling = 0;
    uint32_t              d_blocks = 0;
    ok = hipMemcpyAsync(h_map.data(), m.map, words * 4, hipMemcpyDeviceToHost, q) == hipSuccess &&
         hipMemcpyAsync(&d_blocks, m.uoff + n, 4, hipMemcpyDeviceToHost, q) == hipSuccess &&
         hipMemcpyAsync(&dangling, d_dangling, 8, hipMemcpyDeviceToHost, q) == hipSuccess;
    if(ok && live)
        ok = hipMemcpyAsync(h_uoff.data(), a.upper_off, (size_t)live * 4, hipMemcpyDeviceToHost, q) == hipSuccess &&
             hipMemcpyAsync(h_labels.data(), a.labels, (size_t)live * 8, hipMemcpyDeviceToHost, q) == hipSuccess &&
             hipMemcpyAsync(h_levels.data(), a.levels, (size_t)live, hipMemcpyDeviceToHost, q) == hipSuccess;
    ok = ok && hipStreamSynchronize(q) == hipSuccess;
    float ms_all = 0.f, ms_rows = 0.f;
    if(ok) (void)hipEventElapsedTime(&ms_all, ev[ 0 ], ev[ 3 ]), (void)hipEventElapsedTime(&ms_rows, ev[ 1 ], ev[ 2 ]);
    drop_events();
    if(!ok) return fail(kCompactFailed);
    if(h_map[ n ] != live || d_blocks != blocks) return fail("lantern_gpu: the device's renumbering disagrees with the host's plan; the index is unchanged");
    if(dangling) return fail("lantern_gpu: " + std::to_string(dangling) + " entries of live lists name a deleted row after the unlink; the index is unchanged");
    if(live && (ix->entry >= n || h_map[ ix->entry ] == EMPTY)) return fail("lantern_gpu: the entry node is a deleted row after the unlink; the index is unchanged");
    if(!record_launch(ix, q)) return fail(kCompactFailed);

    // ---- the swap: nothing below can fail ----
    void *old[] = { ix->d_vec, ix->d_norm2, ix->d_screen, ix->d_screen_meta, ix->d_codes, ix->d_labels, ix->d_levels, ix->d_nbr0, ix->d_upper_off, ix->d_upper_nbr,
                    ix->d_radius0, ix->d_radius_upper, ix->d_bitmaps, ix->d_touched, a.temp };
    for(void *p : old)
        if(p) (void)hipFree(p);
    for(int sl = 1; sl < Index::kSearchSlots; ++sl)
        if(ix->slot_bitmaps[ sl ]) (void)hipFree(ix->slot_bitmaps[ sl ]);
    for(int sl = 0; sl < Index::kSearchSlots; ++sl) ix->slot_bitmaps[ sl ] = nullptr, ix->slot_rows[ sl ] = ix->slot_words[ sl ] = 0;
    ix->d_bitmaps = nullptr, ix->bitmap_slots = ix->bm_words = 0;  // sized by capacity: allocated again on first use
    ix->d_touched = nullptr, ix->touched_words = 0;
    ix->d_vec = a.vec, ix->d_norm2 = a.norm2, ix->d_screen = a.screen, ix->d_screen_meta = a.screen_meta, ix->d_codes = a.codes;
    ix->d_labels = a.labels, ix->d_levels = a.levels, ix->d_nbr0 = a.nbr0, ix->d_upper_off = a.upper_off, ix->d_upper_nbr = a.upper_nbr;
    ix->d_radius0 = a.radius0, ix->d_radius_upper = a.radius_upper;
    ix->radius_stale = true;  // the re-prune state is not moved
    ix->cap = newcap;
    ix->upper_cap = ix->upper_blocks = (size_t)blocks;
    ix->n = (size_t)live;
    ix->entry = live ? h_map[ ix->entry ] : EMPTY;
    if(!live) ix->max_level = -1;
    ix->labels.swap(h_labels);
    ix->levels.swap(h_levels);
    ix->upper_off.swap(h_uoff);
    std::unordered_set<uint32_t> seen;  // usearch_search_ef's own scan goes on: its slots through the map
    for(uint32_t s : ix->default_cursor.seen)
        if(s < n && h_map[ s ] != EMPTY) seen.insert(h_map[ s ]);
    ix->default_cursor.seen.swap(seen);
    ix->default_cursor.epoch = ++ix->epoch;
    ix->last_compact_ms[ 0 ] = ms_all, ix->last_compact_ms[ 1 ] = ms_rows;
    if(slot_map) std::memcpy(slot_map, h_map.data(), n * 4);
    index_memory_bytes(ix, rb, ob);
    st.rows_after = live;
    st.upper_blocks_after = blocks;
    st.bytes_after = rb + ob;
    st.bytes_moved = live * (uint64_t)(row + srow + (srow ? 8 : 0) + codes + M0 * 4 + 8 + 1 + 4 + (ix->d_norm2 ? 4 : 0)) + blocks * (uint64_t)(M * 4);
    return true;
}

}  // namespace lgpu

using namespace lgpu;

extern "C" {

void lantern_gpu_remove_labels(usearch_index_t h, const usearch_label_t *labels, size_t n, uint64_t *removed, usearch_error_t *e)
try {
    CLEAR(e);
    if(removed) *removed = 0;
    if(n && !labels) { FAIL(e, "lantern_gpu: null label array"); return; }
    Index *ix = H(h, e);
    if(!ix) return;
    std::lock_guard<std::mutex> g(ix->mu);
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return; }
    ix->err.clear();
    uint64_t r = 0;
    if(!remove_labels_locked(ix, labels, n, r)) { FAIL(e, ix->err.c_str()); return; }
    if(removed) *removed = r;
}
LANTERN_ABI_CATCH_VOID(e)

size_t lantern_gpu_deleted_count(usearch_index_t h, usearch_error_t *e)
try {
    CLEAR(e);
    Index *ix = H(h, e);
    if(!ix) return 0;
    std::lock_guard<std::mutex> g(ix->mu);
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return 0; }
    return deleted_count_locked(ix);
}
LANTERN_ABI_CATCH(e)

void lantern_gpu_unlink_deleted(usearch_index_t h, lantern_gpu_unlink_stats *out, usearch_error_t *e)
try {
    CLEAR(e);
    lantern_gpu_unlink_stats st;
    std::memset(&st, 0, sizeof(st));
    if(out) *out = st;
    Index *ix = H(h, e);
    if(!ix) return;
    std::lock_guard<std::mutex> g(ix->mu);
    if(ix->page_mode) {
        FAIL(e, set_err(ix, "lantern_gpu: unlink does not run on a page-attached index: its lists would have to go back through retriever_mut"));
        return;
    }
    if(ix->pq_compact) {
        FAIL(e, set_err(ix, "lantern_gpu: unlink does not run on a compact pq index: expand it first (lantern_gpu_pq_expand)"));
        return;
    }
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return; }
    ix->err.clear();
    if(!unlink_locked(ix, st)) {
        if(ix->err.empty()) set_err(ix, kUnlinkFailed);
        FAIL(e, ix->err.c_str());
        return;
    }
    if(out) *out = st;
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_compact_deleted(usearch_index_t h, size_t capacity, uint32_t *slot_map, lantern_gpu_compact_stats *out, usearch_error_t *e)
try {
    CLEAR(e);
    lantern_gpu_compact_stats st;
    std::memset(&st, 0, sizeof(st));
    if(out) *out = st;
    Index *ix = H(h, e);
    if(!ix) return;
    std::lock_guard<std::mutex> g(ix->mu);
    if(ix->page_mode) {
        FAIL(e, set_err(ix, "lantern_gpu: compaction does not run on a page-attached index: its rows and lists would have to go back through retriever_mut"));
        return;
    }
    if(ix->pq_compact) {
        FAIL(e, set_err(ix, "lantern_gpu: compaction does not run on a compact pq index: expand it first (lantern_gpu_pq_expand)"));
        return;
    }
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return; }
    ix->err.clear();
    if(!unlink_locked(ix, st.unlink)) {
        if(ix->err.empty()) set_err(ix, kUnlinkFailed);
        FAIL(e, ix->err.c_str());
        return;
    }
    if(deleted_count_locked(ix) == 0) {  // nothing to reclaim: no stat moves, `capacity` is ignored, the epoch stays
        if(slot_map)
            for(size_t s = 0; s < ix->n; ++s) slot_map[ s ] = (uint32_t)s;
        return;
    }
    lantern_gpu_compact_stats moved = st;
    if(!compact_locked(ix, capacity, slot_map, moved)) {
        if(ix->err.empty()) set_err(ix, kCompactFailed);
        FAIL(e, ix->err.c_str());
        if(out) *out = st;  // the unlink happened
        return;
    }
    if(out) *out = moved;
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_last_compact_ms(usearch_index_t h, float *out, usearch_error_t *e)
try {
    CLEAR(e);
    if(out) out[ 0 ] = out[ 1 ] = 0.f;
    Index *ix = H(h, e);
    if(!ix || !out) return;
    std::lock_guard<std::mutex> g(ix->mu);
    out[ 0 ] = ix->last_compact_ms[ 0 ], out[ 1 ] = ix->last_compact_ms[ 1 ];
}
LANTERN_ABI_CATCH_VOID(e)

void lantern_gpu_plan_compact(const uint64_t *labels, const uint8_t *levels, size_t n, uint32_t *slot_map, uint32_t *upper_off_new, uint64_t *live,
                              uint64_t *upper_blocks, usearch_error_t *e)
try {
    CLEAR(e);
    if(live) *live = 0;
    if(upper_blocks) *upper_blocks = 0;
    if(n && (!labels || !levels)) { FAIL(e, "lantern_gpu: null label or level array"); return; }
    if(n >= 0x7FFFFFFFull) { FAIL(e, "lantern_gpu: capacity above 2^31-1 slots is not supported"); return; }
    uint64_t l = 0, b = 0;
    plan_compact_host(labels, levels, n, slot_map, upper_off_new, l, b);
    if(live) *live = l;
    if(upper_blocks) *upper_blocks = b;
}
LANTERN_ABI_CATCH_VOID(e)

}  // extern "C"
