// host_trip.hpp -- the three trips a batched search takes through the host, each written once (index.hpp "HostBatch").
//
// An entry point (lantern_gpu_search_batch*: index.cpp, filter.hip) refuses what it refuses, looks its handles up and makes ONE of
// these calls with its launch as a callable: `bool(const HostBatch &b)` for the two host trips -- it reads b.d_q, b.out(b.d_out),
// b.stream and b.h_extra() -- and `bool()` for the device trip; false -> ix->err.  `failed` is the error text of a HIP failure that
// left nothing more specific in ix->err.
//
// `validate` is nullptr or a `bool(Index *)` (false -> ix->err) that runs under the mutex, after the flush and before anything is
// allocated: the per-query filtered forms' check that every filter is the index's.  Those forms alone reach a trip with an empty
// batch (nq == 0 or k == 0): its filters are checked all the same, then the trip returns silently.  (A params form's k == 0 is the
// width of its answer rows, not an empty batch: it is launched -- a `validate` of such a form says so with a member
// `static constexpr bool zero_width_rows = true`.)
#pragma once
#include <mutex>
#include <string>
#include <type_traits>

#include "abi_guard.hpp"
#include "index.hpp"

namespace lgpu {

template <class V, class = void> struct ZeroWidthRows : std::false_type {};
template <class V> struct ZeroWidthRows<V, std::void_t<decltype(V::zero_width_rows)>> : std::true_type {};
// a validating form's empty batch
template <class V> inline bool trip_is_empty(size_t nq, size_t k) { return nq == 0 || (k == 0 && !ZeroWidthRows<V>::value); }

// sync: the index's own page-locked block and stream, everything under ix->mu.
template <class Validate, class Launch>
void host_trip_sync(Index *ix, size_t nq, size_t k, size_t extra_bytes, const void *queries, int kind, const char *failed, Validate validate,
                    Launch launch, uint64_t *labels, float *distances, uint32_t *counts, const char **e)
{
    std::lock_guard<std::mutex> g(ix->mu);
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return; }
    ix->err.clear();
    if constexpr(!std::is_null_pointer<Validate>::value) {
        if(!validate(ix)) { FAIL(e, ix->err.c_str()); return; }
        if(trip_is_empty<Validate>(nq, k)) return;
    }
    HostBatch b = batch_layout(ix, Index::kLanes, nq, k, extra_bytes);
    if(!batch_stage(ix, b, queries, kind)) { FAIL(e, kNoStage); return; }
    if(!batch_device(ix, b)) { FAIL(e, ix->err.c_str()); return; }
    const bool ok = batch_upload(b) && launch(b);
    if(!batch_finish_locked(ix, b, ok, failed, labels, distances, counts)) FAIL(e, ix->err.c_str());
}

// A lane's error text belongs to the calling thread: ix->err is shared by every lane (and by every other entry point) and may be
// rewritten or cleared the moment the mutex is dropped, while the caller -- the scan service's dispatcher -- reads the message
// later and without the lock.
inline void lane_fail(const char **e, const std::string &text)
{
    static thread_local std::string msg;
    msg = text;
    FAIL(e, msg.c_str());
}

inline bool lane_ok(int lane, const char **e)
{
    if(lane >= 0 && lane < Index::kLanes) return true;
    FAIL(e, "lantern_gpu: lane must be in [0, 8)");
    return false;
}

// lane: for a caller that keeps SEVERAL batches in flight (the scan-side service: up to eight dispatchers, each executing a batch
// while another collects the next).  Each lane has its own stream, staging block and device buffers -- one caller at a time per lane
// -- so the queries are staged WITHOUT ix->mu; the mutex is held only while the lane's copies and its launch are queued; the wait for
// the answers, the long part, and their unpacking happen outside it.  That is what lets the lanes' launches overlap on the device
// (each in its own visited-bitmap slab: acquire_search_slot).
template <class Validate, class Launch>
void host_trip_lane(Index *ix, int lane, size_t nq, size_t k, size_t extra_bytes, const void *queries, int kind, const char *failed,
                    Validate validate, Launch launch, uint64_t *labels, float *distances, uint32_t *counts, const char **e)
{
    constexpr bool validates = !std::is_null_pointer<Validate>::value;
    const bool     empty = validates && trip_is_empty<Validate>(nq, k);
    HostBatch      b = batch_layout(ix, lane, nq, k, extra_bytes);
    if(!empty && !batch_stage(ix, b, queries, kind)) { FAIL(e, kNoLaneStage); return; }
    bool ok;
    {
        std::lock_guard<std::mutex> g(ix->mu);
        if(!flush_locked(ix)) { lane_fail(e, ix->err); return; }
        ix->err.clear();
        if constexpr(validates) {
            if(!validate(ix)) { lane_fail(e, ix->err); return; }
            if(empty) return;
        }
        if(!batch_device(ix, b)) { lane_fail(e, ix->err); return; }
        ok = batch_upload(b) && launch(b) && batch_download(b);
        if(!ok) lane_fail(e, ix->err.empty() ? failed : ix->err);
    }
    // whatever was queued is waited for even after a failure: the caller may free what the launch reads (its filters) once this returns
    if(hipStreamSynchronize(b.stream) != hipSuccess && ok) { ok = false; FAIL(e, failed); }
    if(ok) batch_unpack(b, 0, nq, labels, distances, counts);
}

// device: queries and answers are the caller's device memory, the launch is queued on the caller's stream and nothing is waited
// for.  `stride_rule(ix)` is NULL or the refusal of the caller's query row stride, read under the mutex and before the flush.
template <class Rule, class Launch>
void device_trip(Index *ix, Rule stride_rule, Launch launch, const char **e)
{
    std::lock_guard<std::mutex> g(ix->mu);
    if(const char *why = stride_rule(ix)) { FAIL(e, why); return; }
    if(!flush_locked(ix)) { FAIL(e, ix->err.c_str()); return; }
    ix->err.clear();
    if(!launch()) FAIL(e, ix->err.c_str());
}

// the stride rule of every form that states its stride
inline auto stride_is(size_t query_stride_bytes)
{
    return [ query_stride_bytes ](const Index *ix) { return query_stride_bytes == (size_t)ix->chunks * 16 ? nullptr : kStrideMismatch; };
}

}  // namespace lgpu
