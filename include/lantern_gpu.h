/*
 * lantern_gpu.h -- C ABI of the MI355X-native HNSW distance-evaluation path for Lantern.
 *
 * Two groups of entry points:
 *
 *  (1) The usearch C API exactly as Lantern calls it (boundary B1 of SURVEY.md section 8b).
 *      Lantern static-links usearch's c/lib.cpp into lantern.so (lantern_hnsw/CMakeLists.txt:89,
 *      115-120); usearch.h itself is NOT in the reference tree (un-vendored submodule), so the
 *      prototypes below are reconstructed from the call sites cited next to each one.  A
 *      maintainer links liblantern_gpu.so instead of c/lib.cpp and recompiles.
 *
 *  (2) lantern_gpu_* / lantern_scan_* / lantern_*_dist: batched and device-resident forms the
 *      reference lacks, the amgettuple paging shim (scan.c:167-338) and the SQL-callable
 *      distance functions' semantics (hnsw.c:296-405).
 *
 * Conventions (same as the reference's): errors are a `const char*` out-parameter, NULL on
 * success, pointing at a static or index-owned string on failure (hnsw.c:341-343, scan.c:100,
 * build.c:545-551); result arrays are caller-allocated (scan.c:207-212); vectors are borrowed
 * for the duration of the call.  There is NO CPU fallback: without a HIP device every compute
 * entry point fails with an error string.
 */
#ifndef LANTERN_GPU_H
#define LANTERN_GPU_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LANTERN_GPU_EXPORT __attribute__((visibility("default")))

/* ------------------------------------------------------------------------------------------ */
/* (1) usearch C API as used by Lantern                                                        */
/* ------------------------------------------------------------------------------------------ */

typedef void       *usearch_index_t;
typedef uint64_t    usearch_key_t;
typedef uint64_t    usearch_label_t; /* 6-byte heap TID packed in u64: utils.c:69-75 */
typedef float       usearch_distance_t;
typedef const char *usearch_error_t;

/* enum values pinned by lantern_cli/src/external_index/cli.rs:56-69 and server.rs:94-101 */
typedef enum usearch_metric_kind_t {
    usearch_metric_unknown_k = 0,
    usearch_metric_cos_k = 1,
    usearch_metric_l2sq_k = 3,
    usearch_metric_hamming_k = 8
} usearch_metric_kind_t;

typedef enum usearch_scalar_kind_t {
    usearch_scalar_unknown_k = 0,
    usearch_scalar_f32_k = 1,
    usearch_scalar_f64_k = 2,
    usearch_scalar_f16_k = 3,
    usearch_scalar_i8_k = 4,
    usearch_scalar_b1_k = 5
} usearch_scalar_kind_t;

/* external_index.c:613-697: slot -> pointer to the node tape */
typedef void *(*usearch_node_retriever_t)(void *ctx, uint64_t slot);

/* Fields are the ones Lantern sets: utils.c:57-67, scan.c:60-96, build.c:495-515, insert.c:116-132 */
typedef struct usearch_init_options_t
{
    usearch_metric_kind_t    metric_kind;
    void                    *metric; /* custom metric; Lantern always passes NULL (utils.c:63) */
    usearch_scalar_kind_t    quantization;
    size_t                   dimensions; /* f32 scalars, or BITS for hamming (scan.c:84-88) */
    size_t                   connectivity;
    size_t                   expansion_add;
    size_t                   expansion_search;
    size_t                   num_threads;
    bool                     pq;
    size_t                   num_centroids;
    size_t                   num_subvectors;
    void                    *retriever_ctx;
    usearch_node_retriever_t retriever;
    usearch_node_retriever_t retriever_mut;
} usearch_init_options_t;

/* usearch_storage.cpp:19-32,63-81 read these */
typedef struct metadata_t
{
    size_t                 neighbors_bytes;      /* 4 + M*6      (upper levels) */
    size_t                 neighbors_base_bytes; /* 4 + 2M*6     (level 0)      */
    double                 inverse_log_connectivity;
    size_t                 connectivity;
    size_t                 dimensions;
    usearch_init_options_t init_options;
} metadata_t;

#define USEARCH_SEARCH_EF_INVALID_VALUE 0 /* options.c:341: 0 = "use the index's ef" */
#define LANTERN_SLOT_SIZE 6               /* validate_index.c:39, hnsw.h:42-49 */
#define USEARCH_HEADER_SIZE 136           /* external_index.h:29-30 */
#define USEARCH_EMPTY_INDEX_SIZE USEARCH_HEADER_SIZE /* build.c:678 */

/* scan.c:99, build.c:517,675, insert.c:142.
 * quantization: f32 / f16 / i8 storage of real[] input (quant_bits 32 / 16 / 8), or b1 -- for hamming (integer[] input:
 *   bits) and for l2sq over real[] (quant_bits = 1, options.c:154-155: bit = (x > 0); the l2sq distance of {0,1} vectors
 *   is their Hamming distance).
 * pq = true (build.c:497-500, scan.c:75-81): pq_codebook = num_centroids rows of `dimensions` floats, row c = centroid c
 *   of every subvector, concatenated (pqtable.c:194-240); copied.  Every stored vector is replaced by its quantisation
 *   (per subvector the nearest centroid under the index metric, first minimum wins: product_quantization.c:80-124);
 *   all distances are distances to / between the DECODED vectors; the file and the pages carry num_subvectors code bytes
 *   per node (usearch_storage.cpp:29-31).  The device keeps the decodings resident in HBM next to the codes. */
LANTERN_GPU_EXPORT usearch_index_t usearch_init(usearch_init_options_t *, float *pq_codebook, usearch_error_t *);
/* scan.c:131, build.c:450,549,597,684, insert.c:237 */
LANTERN_GPU_EXPORT void usearch_free(usearch_index_t, usearch_error_t *);
/* build.c:124,543, insert.c:182 */
LANTERN_GPU_EXPORT void usearch_reserve(usearch_index_t, size_t capacity, usearch_error_t *);
/* scan.c:246, build.c:117,121,558,590, insert.c:148 */
LANTERN_GPU_EXPORT size_t usearch_size(usearch_index_t, usearch_error_t *);
/* build.c:116 */
LANTERN_GPU_EXPORT size_t usearch_capacity(usearch_index_t, usearch_error_t *);
/* server.rs:222-229 (Index::dimensions) */
LANTERN_GPU_EXPORT size_t usearch_dimensions(usearch_index_t, usearch_error_t *);
/* build.c:128; Rust add_raw server.rs:349.  Inserts are buffered and applied in batches on the
 * device (see lantern_gpu_set_add_batch); any reader (search/size/save) flushes first. */
LANTERN_GPU_EXPORT void usearch_add(usearch_index_t, usearch_label_t, const void *vector, usearch_scalar_kind_t,
                                    usearch_error_t *);
/* insert.c:209 (ldb_aminsert): one sequential insertion at the caller-drawn level (insert.c:32-46) of a node whose tape
 * the caller allocated inside a PostgreSQL page (`node_tape`, headed by usearch_init_node, usearch_storage.cpp:34-44)
 * at 48-bit page slot `slot`.  The node is linked into the HBM mirror; its own lists and stored vector are written into
 * `node_tape`, the re-written lists of the nodes it linked to into their tapes through init_options.retriever_mut
 * (external_index.c:673-697).  On an index that was not attached with usearch_view_mem_lazy the slots written are the
 * sequential ids of the file format. */
LANTERN_GPU_EXPORT void usearch_add_external(usearch_index_t, usearch_label_t, const void *vector, void *node_tape,
                                             usearch_scalar_kind_t, int16_t level, uint64_t slot, usearch_error_t *);
/* scan.c:220-228,273-281.  ef == 0 -> index default.  streaming == true returns the NEXT k results of
 * the same query: the index remembers what it handed out since the last non-streaming call, searches for
 * that many + k, and returns the first k that were not returned before (never a row twice). */
LANTERN_GPU_EXPORT size_t usearch_search_ef(usearch_index_t, const void *query, usearch_scalar_kind_t, size_t k,
                                            size_t ef, bool streaming, usearch_label_t *labels, float *distances,
                                            usearch_error_t *);
/* The per-scan half of the streaming contract.  In the reference every scan owns its own usearch handle (scan.c:99),
 * so usearch_search_ef's "what was handed out since the last non-streaming call" is per scan there.  When ONE resident
 * index serves many scans, each scan opens a cursor and searches through it; usearch_search_ef(h, ...) is the same call
 * on the index's built-in cursor.  Cursors must be closed before usearch_free. */
typedef struct lantern_gpu_cursor lantern_gpu_cursor_t;
LANTERN_GPU_EXPORT lantern_gpu_cursor_t *lantern_gpu_cursor_open(usearch_index_t, usearch_error_t *);
LANTERN_GPU_EXPORT size_t lantern_gpu_cursor_search(lantern_gpu_cursor_t *, const void *query, usearch_scalar_kind_t, size_t k,
                                                    size_t ef, bool streaming, usearch_label_t *labels, float *distances,
                                                    usearch_error_t *);
LANTERN_GPU_EXPORT size_t lantern_gpu_cursor_seen(lantern_gpu_cursor_t *); /* rows handed out since the last non-streaming call */
LANTERN_GPU_EXPORT void   lantern_gpu_cursor_close(lantern_gpu_cursor_t *);
/* lantern_gpu_cursor_search through a filter (lantern_gpu_filter_t: "Filtered search" below): streaming never hands out a row
 * twice, and every row it hands out is allowed */
struct lantern_gpu_filter;
LANTERN_GPU_EXPORT size_t lantern_gpu_cursor_search_filtered(lantern_gpu_cursor_t *, const struct lantern_gpu_filter *, const void *query,
                                                             usearch_scalar_kind_t, size_t k, size_t ef, bool streaming,
                                                             usearch_label_t *labels, float *distances, usearch_error_t *);
/* hnsw.c:317,326,340; product_quantization.c:102,185.  One pair, evaluated on the device. */
LANTERN_GPU_EXPORT float usearch_distance(const void *a, const void *b, usearch_scalar_kind_t, size_t dims,
                                          usearch_metric_kind_t, usearch_error_t *);
/* build.c:561, insert.c:160, utils.c:91 */
LANTERN_GPU_EXPORT metadata_t usearch_index_metadata(usearch_index_t, usearch_error_t *);
/* build.c:583: usearch-format file = 136-byte header + node tapes in slot order (App. B) */
LANTERN_GPU_EXPORT void usearch_save(usearch_index_t, const char *path, usearch_error_t *);
/* build.c:679 */
LANTERN_GPU_EXPORT void usearch_save_buffer(usearch_index_t, char *buffer, size_t length, usearch_error_t *);
/* Rust Index::load_from_buffer (external_index_server_test.rs:271-314) / usearch_load.  The file is untrusted: a header that does not
 * match the index options, a node count the length cannot hold, an entry slot, top level, neighbour count or neighbour slot out of
 * range, a truncated or corrupt node tape, an upper-level list naming a node that does not reach that level and -- on a pq index
 * with fewer than 256 centroids -- a code byte >= num_centroids ("a pq code names a centroid the codebook does not have") are refused
 * before anything reaches the device, and the index stays empty.  usearch_view_mem_lazy holds the pages to the same checks. */
LANTERN_GPU_EXPORT void usearch_load(usearch_index_t, const char *path, usearch_error_t *);
LANTERN_GPU_EXPORT void usearch_load_buffer(usearch_index_t, const char *buffer, size_t length, usearch_error_t *);
LANTERN_GPU_EXPORT size_t usearch_serialized_length(usearch_index_t, usearch_error_t *);
/* scan.c:110, insert.c:151: attach to an index that lives in PostgreSQL pages.  The reachable graph is
 * walked ONCE through init_options.retriever (slot -> node tape, external_index.c:613-671) from the
 * header's entry slot and mirrored into HBM; neighbour slots are the 6-byte ItemPointers of
 * external_index.c:380-409.  Searches then run on the mirror and return the nodes' labels. */
LANTERN_GPU_EXPORT void usearch_view_mem_lazy(usearch_index_t, char *header136, usearch_error_t *);
/* insert.c:214: refresh size / max_level / entry slot in the header copy (the entry slot in the form the index was
 * attached in: a 48-bit page slot after usearch_view_mem_lazy, a sequential id otherwise) */
LANTERN_GPU_EXPORT void usearch_update_header(usearch_index_t, char *header136, usearch_error_t *);
/* external_index.c:411,417 */
LANTERN_GPU_EXPORT uint64_t usearch_header_get_entry_slot(char *header136);
LANTERN_GPU_EXPORT void     usearch_header_set_entry_slot(char *header136, uint64_t slot);

/* Lantern's node-tape helpers (lantern_hnsw/src/hnsw/usearch_storage.hpp:9-23).  They are Lantern's own functions, but the
 * reference compiles them against usearch's C++ templates (usearch_storage.cpp:2-16: node_at<>), so whatever replaces usearch
 * brings them: same names, same signatures (`ldb_unaligned_slot_union_t *` = the 6-byte slots of hnsw.h:42-49, returned as
 * void * here; Lantern keeps its own declaration).  Host-only byte arithmetic over
 *   [key u64][level u16] { [count u32][slot 6 B x cap] } x (level + 1) [vector bytes]        (validate_index.c:105-226)
 * Callers: external_index.c:96-97,394-398,488, insert.c:207, delete.c:54-58, utils.c:93. */
#ifndef HNSW_USEARCH_STORAGE_H
LANTERN_GPU_EXPORT uint32_t UsearchNodeBytes(const metadata_t *metadata, int vector_bytes, int level);
LANTERN_GPU_EXPORT void usearch_init_node(metadata_t *meta, char *tape, usearch_key_t key, uint32_t level, uint64_t slot_id,
                                          void *vector, size_t vector_len);
LANTERN_GPU_EXPORT uint32_t node_tuple_size(char *node, uint32_t vector_dim, const metadata_t *meta);
LANTERN_GPU_EXPORT usearch_label_t label_from_node(char *node);
LANTERN_GPU_EXPORT unsigned long level_from_node(char *node);
LANTERN_GPU_EXPORT void reset_node_label(char *node);
LANTERN_GPU_EXPORT void *get_node_neighbors_mut(const metadata_t *meta, char *node, uint32_t level, uint32_t *neighbors_count);
#endif
/* reloption quant_bits -> scalar kind, as ldb_HnswGetScalarKind (options.c:137-158); *err carries the reference's text for a value the
 * enum reloption rejects (hnsw_sq.out:30-35) or one it has not implemented (4, 2: options.c:150-153).  unset = no reloption given. */
LANTERN_GPU_EXPORT usearch_scalar_kind_t lantern_quant_bits_scalar_kind(int quant_bits, bool unset, usearch_error_t *err);

/* ------------------------------------------------------------------------------------------ */
/* (2) batched / device-resident forms                                                         */
/* ------------------------------------------------------------------------------------------ */

LANTERN_GPU_EXPORT const char *lantern_gpu_version(void);
LANTERN_GPU_EXPORT int         lantern_gpu_device_count(void);

/* seed of the level draw (insert.c:32-46 uses PG's global PRNG; here levels are a stateless
 * hash of (seed, slot) so that builds are reproducible).  Call before the first add. */
LANTERN_GPU_EXPORT void lantern_gpu_set_seed(usearch_index_t, uint64_t seed, usearch_error_t *);
/* Insert batching: at most `max_batch` pending vectors are inserted per device pass and never
 * more than size/min_ratio (so early inserts are near-sequential).  max_batch = 1 reproduces
 * usearch_add's strictly sequential semantics.  Defaults: 8192, 16. */
LANTERN_GPU_EXPORT void lantern_gpu_set_add_batch(usearch_index_t, size_t max_batch, size_t min_ratio,
                                                  usearch_error_t *);
/* many inserts in one call (the external indexer's row stream, server.rs:214-267) */
LANTERN_GPU_EXPORT void lantern_gpu_add_many(usearch_index_t, const usearch_label_t *labels, const void *vectors,
                                             size_t n, usearch_scalar_kind_t, usearch_error_t *);
/* The two host-side rules that make a build reproducible by any builder (pure functions, no device):
 * the level of the node at `slot` -- floor(-ln(U) / ln(M)) as insert.c:32-46, U a hash of (seed, slot) -- and the
 * prefix of the pending vectors that forms the next device batch (<= max_batch, <= size / min_ratio, a vector that
 * raises the top level goes alone). */
LANTERN_GPU_EXPORT int    lantern_gpu_level_for(uint64_t seed, uint64_t slot, uint32_t connectivity);
LANTERN_GPU_EXPORT size_t lantern_gpu_plan_batch(size_t current_size, int max_level, const int *pending_levels, size_t pending,
                                                 size_t max_batch, size_t min_ratio);
/* apply all buffered inserts now */
LANTERN_GPU_EXPORT void lantern_gpu_flush(usearch_index_t, usearch_error_t *);
/* page-locked host memory for rows that are about to be handed to lantern_gpu_add_many / usearch_add: the upload runs at the
 * host link's rate instead of through the runtime's pageable staging (the indexing server's row chunks: 50 MB each).  NULL on
 * failure (callers fall back to ordinary memory). */
LANTERN_GPU_EXPORT void *lantern_gpu_host_alloc(size_t bytes);
LANTERN_GPU_EXPORT void  lantern_gpu_host_free(void *);
/* usearch_save_buffer without the buffer: the index file (the bytes usearch_save_buffer would produce) handed to `write` as a
 * sequence of spans, up to 1024 per call, in file order -- header, then per node its formatted prefix and its vector bytes
 * straight out of a page-locked staging buffer that the rows reach in ~64 MB chunks, the next chunk's copy overlapping this
 * one's consumption.  A span is layout-compatible with struct iovec: the indexing server passes them to writev(2)
 * (server.rs:388-422 sends the file it has just written to disk).  `write` returns 0 to go on, anything else aborts.  The index
 * stays locked until the last span has been consumed: other calls on it wait for a slow consumer. */
typedef struct lantern_gpu_span { const void *data; size_t size; } lantern_gpu_span;
typedef int (*lantern_gpu_write_fn)(void *ctx, const lantern_gpu_span *spans, size_t count);
LANTERN_GPU_EXPORT void lantern_gpu_save_stream(usearch_index_t, lantern_gpu_write_fn write, void *ctx, usearch_error_t *);
/* usearch_add with a caller-drawn level (insert.c:32-46); usearch_add_external is this plus the write-back to the pages */
LANTERN_GPU_EXPORT void lantern_gpu_add_with_level(usearch_index_t, usearch_label_t, const void *vector,
                                                   usearch_scalar_kind_t, int level, usearch_error_t *);

/* nq independent usearch_search_ef calls in one launch; host buffers.
 * labels/distances: nq x k (unused tail: label 0, +inf); counts: nq (may be NULL). */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch(usearch_index_t, const void *queries, size_t nq,
                                                 usearch_scalar_kind_t, size_t k, size_t ef, usearch_label_t *labels,
                                                 float *distances, uint32_t *counts, usearch_error_t *);
/* The same for a caller that keeps up to EIGHT batches in flight (`lane` 0 .. 7, one caller thread per lane): each lane has its
 * own stream and staging buffers inside the index, and the wait for the answers does not hold the index's lock, so the lanes'
 * launches overlap on the device (the scan-side service below runs one dispatcher per lane over this). */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_lane(usearch_index_t, int lane, const void *queries, size_t nq,
                                                      usearch_scalar_kind_t, size_t k, size_t ef, usearch_label_t *labels,
                                                      float *distances, uint32_t *counts, usearch_error_t *);
/* The same with every answer handed on AS ITS OWN WALK ENDS: `done(ctx, which, count)` is called from the calling thread for the
 * `count` queries (indices in `which`) that finished since the last call -- their rows of labels / distances / counts are filled in by
 * then -- until every query has been handed on; the function returns after the last call.  The walks of a launch differ in length by
 * 2x and more; a service that answers each client when ITS walk is over does not make it wait for the longest one of its batch. */
typedef void (*lantern_gpu_queries_done_fn)(void *ctx, const uint32_t *which, size_t count);
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_lane_notify(usearch_index_t, int lane, const void *queries, size_t nq,
                                                             usearch_scalar_kind_t, size_t k, size_t ef, usearch_label_t *labels,
                                                             float *distances, uint32_t *counts, lantern_gpu_queries_done_fn done, void *done_ctx,
                                                             usearch_error_t *);
/* Same, every buffer already in device memory, asynchronous on `stream` (a hipStream_t; NULL =
 * the default stream).  slots (u32 internal ids), counts, dist_evals (D) and expansions (E) may
 * be NULL.  `skip` drops that many leading results per query (streaming continuation).
 * Launches on DIFFERENT streams overlap, two at a time (each gets its own slab of visited bitmaps; a third queues behind
 * the slab it reuses): with independent batches -- a serving workload -- the second fills the machine while the first one's
 * longest walks drain (1M x 768 cosine, 1024-query batches: 0.68 -> 0.87 of the HBM peak).  Insert batches run behind every
 * search in flight, and searches queued on other streams behind them; no host synchronisation is involved. */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_device(usearch_index_t, const void *d_queries, size_t nq, size_t k,
                                                        size_t ef, size_t skip, uint64_t *d_labels, float *d_distances,
                                                        uint32_t *d_slots, uint32_t *d_counts, uint64_t *d_dist_evals,
                                                        uint64_t *d_expansions, void *stream, usearch_error_t *);
/* The same with the caller's query row stride stated: query i is read at d_queries + i * query_stride_bytes, which must equal
 * lantern_gpu_row_bytes() -- anything else is refused ("the query row stride does not match ...") instead of being read at
 * the wrong offsets and past the end of the caller's buffer.  lantern_gpu_search_batch_device (no stride argument) is accepted
 * only for indexes whose stored stride is the vector's own length rounded up to 16 bytes; for an index that widens its rows
 * (bit rows of 65 .. 127 bytes are stored at 128) it fails and names this entry point. */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_device_strided(usearch_index_t, const void *d_queries, size_t query_stride_bytes,
                                                                size_t nq, size_t k, size_t ef, size_t skip, uint64_t *d_labels,
                                                                float *d_distances, uint32_t *d_slots, uint32_t *d_counts,
                                                                uint64_t *d_dist_evals, uint64_t *d_expansions, void *stream,
                                                                usearch_error_t *);
/* PER-QUERY k, ef AND skip.  The entry points above take one k, one ef and one skip for the whole call; the four
 * below take them per query, params[i] for query i (ef 0 = the index's default; reserved must be 0), and serve the whole batch in at
 * most THREE launches whatever the parameters: the queries are split by where the walk keeps its candidate list -- expansion
 * (= max(ef, k + skip)) <= 64, <= 128, beyond -- and each non-empty class is one launch.
 * CONTRACT: for query i the ids, distance bits, count, D and E are exactly those of the uniform call with (k_i, ef_i, skip_i).
 * labels / distances (and slots) are nq x k_stride: row i holds query i's k_i answers, its tail label 0, +inf (slot ~0) as a uniform
 * row's unused tail; k_stride < max k_i is refused.  A query with k_i = 0 takes no walk: count 0, D = E = 0, and it is still handed on
 * by the notify form.  Every refusal -- a bad parameter, an expansion beyond the 160 KiB LDS budget -- is for the whole call, before
 * anything is launched or written, and names the first offending position: "... (params[i])".
 * The host and lane forms take `skip` too (the uniform host forms have none): a service that wants the device to drop the rows a scan
 * was already handed says so here.  Filtered searches take them per query through lantern_gpu_search_batch_filtered_each_params*. */
typedef struct lantern_gpu_query_params { uint32_t k, ef, skip, reserved; } lantern_gpu_query_params; /* ef 0 = index default; reserved must be 0 */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_params(usearch_index_t, const void *queries, size_t nq, usearch_scalar_kind_t,
                                                        const lantern_gpu_query_params *params, size_t k_stride, usearch_label_t *labels,
                                                        float *distances, uint32_t *counts, usearch_error_t *);
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_params_lane(usearch_index_t, int lane, const void *queries, size_t nq, usearch_scalar_kind_t,
                                                             const lantern_gpu_query_params *params, size_t k_stride, usearch_label_t *labels,
                                                             float *distances, uint32_t *counts, usearch_error_t *);
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_params_lane_notify(usearch_index_t, int lane, const void *queries, size_t nq,
                                                                    usearch_scalar_kind_t, const lantern_gpu_query_params *params, size_t k_stride,
                                                                    usearch_label_t *labels, float *distances, uint32_t *counts,
                                                                    lantern_gpu_queries_done_fn done, void *done_ctx, usearch_error_t *);
/* every buffer in device memory except `params`, a HOST array that is read during the call (it may be reused once the call returns) */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_params_device(usearch_index_t, const void *d_queries, size_t query_stride_bytes, size_t nq,
                                                               const lantern_gpu_query_params *params, size_t k_stride, uint64_t *d_labels,
                                                               float *d_distances, uint32_t *d_slots, uint32_t *d_counts, uint64_t *d_dist_evals,
                                                               uint64_t *d_expansions, void *stream, usearch_error_t *);
/* the last per-query-parameter call on this index that passed its checks (diagnostic; tests assert the regime): out[0] launches made
 * (0 .. 3), [1] [2] [3] queries in the classes expansion <= 64, <= 128, beyond, [4] the largest expansion, [5] 1 if any launch took a
 * latency-bound (spec) shape.  All zero before the first such call. */
LANTERN_GPU_EXPORT void lantern_gpu_last_params_launch(usearch_index_t, uint32_t out[6], usearch_error_t *);
/* Diagnostics (tests): the kernel instantiations of the unfiltered search launches THIS THREAD made since the last call, oldest first,
 * at most cap rows of 10 words (and at most the last four launches: a per-query-parameter call makes at most three):
 * [0] kernel (1 k_search, 2 k_search_adc)  [1] METRIC  [2] G  [3] PROF  [4] ROWS  [5] KPL  [6] SPEC  [7] EACH -- the template arguments
 * as the launch macro passed them (k_search_adc: G = 8, PROF = ROWS = 0, which are no parameters of it)  [8] the launch screens (its
 * view carries the int8 screen)  [9] queries of the launch.
 * Returns the number of launches since the last call (it may exceed cap, and four) and resets it.  No device is needed. */
LANTERN_GPU_EXPORT size_t lantern_gpu_last_search_cells(uint32_t *cells, size_t cap);
/* ------------------------------------------------------------------------------------------ */
/* Filtered search: k-NN limited to an allow-set of rows.                       */
/* PARITY UNPINNED BY THE REFERENCE: the reference's usearch fork is not in the tree; what follows */
/* is a definition of this library.                                                             */
/* ------------------------------------------------------------------------------------------ */
/* A filter is a set of allowed slots of ONE index at ONE size.  For a query, expansion = max(ef or the index's ef, k + skip):
 *  1. upper levels: greedy descent exactly as the unfiltered search; the filter does not apply on levels >= 1;
 *  2. base layer, WALK path: two lists ordered by (distance, slot): `top` (at most expansion entries, allowed slots only) and
 *     `next` (candidates still to expand, at most C entries, C >= expansion; a pop removes the entry).  Start: evaluate the start
 *     node (D += 1), push it to next, and to top if allowed.  While next is not empty: c = min(next); stop if |top| == expansion
 *     and worst(top) < c; else pop c (E += 1) and for each neighbour in list order: skip it if visited, else mark it visited and
 *     evaluate it (D += 1) as key x; if |top| < expansion or x < worst(top), push x to next (a full next keeps its C smallest: x
 *     replaces the worst entry when smaller and is dropped otherwise; a dropped node stays visited) and, if x's slot is allowed,
 *     insert x into top (at most expansion entries).  The answer is top[skip, skip + k); it may be shorter than k (the reachable
 *     part of the graph holds fewer allowed rows);
 *  3. EXACT path: every allowed slot evaluated, the (distance, slot)-smallest [skip, skip + k) returned; D = allowed count, E = 0;
 *  4. distances are the walk's per-pair reduction, bit for bit (usearch_distance): a row has the same bits on either path and in
 *     the unfiltered search.
 *  5. SEEDED WALK (lantern_gpu_set_filter_seeds > 0; off by default): the walk path of a query whose filter has count >= 1 allowed
 *     rows, S' = min(seeds, count), replaces "Start: ..." of 2 by
 *       seeding: for j = 0 .. S'-1 in order, x = the ((j * count) / S')-th allowed slot in ascending order (64-bit product, integer
 *         division); if x is unvisited, mark it visited, evaluate it (D += 1) and admit it by the rule of 2 (if |top| < expansion
 *         or x < worst(top): push x to next and insert it into top);
 *       allowed-only stage: the loop of 2 to its stop, except that only ALLOWED neighbours are considered -- a disallowed neighbour
 *         is neither marked, counted nor evaluated;
 *       hand-over: next := the keys of top (what the stage left in next lies beyond the radius and could never be popped); if the
 *         start node is unvisited, mark it visited, evaluate it (D += 1) and admit it (into top only if it is allowed);
 *     and then runs the loop of 2, unchanged, to its stop.  The exact path ignores the setting; seeds = 0 is the walk of 2 exactly;
 *     every row keeps the walk's distance bits and the order (distance, slot).
 * With an all-allowed filter, C >= expansion and seeds = 0 the walk path returns exactly the ids, distance bits, D and E of the
 * unfiltered search.  With seeds > 0 an all-allowed FILTER is no longer the unfiltered search (its walk starts from the seeds); a
 * NULL entry of the per-query form has no slot list, runs the walk of 2 and still is, bit for bit.  Deleted rows carry label 0 (hnsw.h:40); the reference skips them only after a search has returned them (scan.c:296-300)
 * and gives up streaming after 1000 rows (scan.c:249-252), so a selective predicate applied after the index scan returns fewer
 * than LIMIT rows -- a filter makes the walk itself look for allowed rows.
 * A filter is refused (an error naming both sizes) on another index, or once the index has grown: it is never extended implicitly:
 * lantern_gpu_filter_extend. */
typedef struct lantern_gpu_filter lantern_gpu_filter_t;
#define LANTERN_GPU_FILTER_SKIP_DELETED 1u /* also disallow every slot whose label is 0 */
/* allowed iff the slot's label is in labels[0..n) (any order, duplicates allowed): sorted and searched on the device -- the form a
 * backend feeds from a bitmap heap scan's TIDs, which are the labels */
LANTERN_GPU_EXPORT lantern_gpu_filter_t *lantern_gpu_filter_from_labels(usearch_index_t, const usearch_label_t *labels, size_t n,
                                                                        uint32_t flags, usearch_error_t *);
/* a host bitmap over slots: bit s of words[s / 32]; n_words must be ceil(size / 32) */
LANTERN_GPU_EXPORT lantern_gpu_filter_t *lantern_gpu_filter_from_slot_bitmap(usearch_index_t, const uint32_t *words, size_t n_words,
                                                                             uint32_t flags, usearch_error_t *);
LANTERN_GPU_EXPORT size_t lantern_gpu_filter_count(const lantern_gpu_filter_t *, usearch_error_t *); /* allowed slots */
LANTERN_GPU_EXPORT size_t lantern_gpu_filter_resident_bytes(const lantern_gpu_filter_t *, usearch_error_t *); /* device memory it holds */
LANTERN_GPU_EXPORT void   lantern_gpu_filter_free(lantern_gpu_filter_t *);
/* A FILTER'S LIFE CYCLE (DESIGN.md 4.9 "Filter life cycle").  Filters are immutable: each call below returns a NEW handle and only
 * reads its operands, which stay valid handles -- stale for searches as before -- until the caller frees them.  Nothing extends a
 * filter behind the caller's back: a search through a stale filter is refused as ever.  The argument checks (flags, op, NULLs, the
 * filter handles) are made before the device is used. */
#define LANTERN_GPU_FILTER_EXTEND_ALL 2u   /* extend only: every new slot is allowed (labels must be NULL, n 0) */
/* The filter `f` brought to the index's size after the flush every search performs: bits [0, f->n) as in f (a snapshot: rows
 * deleted since stay as f has them); a slot s in [f->n, size) is allowed iff its label is in labels[0..n) -- or, under EXTEND_ALL,
 * always -- and, under SKIP_DELETED, its label is not 0.  f->n == size gives an equal copy.  Refused: another index's filter, a
 * filter from before a compaction (the message a search gives: its slots name other rows now, and it is not remapped), unknown
 * flags, labels == NULL with n > 0. */
LANTERN_GPU_EXPORT lantern_gpu_filter_t *lantern_gpu_filter_extend(usearch_index_t, const lantern_gpu_filter_t *f, const usearch_label_t *labels,
                                                                   size_t n, uint32_t flags, usearch_error_t *);
#define LANTERN_GPU_FILTER_AND 0
#define LANTERN_GPU_FILTER_OR 1
#define LANTERN_GPU_FILTER_ANDNOT 2        /* a and not b */
/* Both operands must pass the check a search applies to a filter today (this index, its current size and epoch). */
LANTERN_GPU_EXPORT lantern_gpu_filter_t *lantern_gpu_filter_combine(usearch_index_t, const lantern_gpu_filter_t *a, const lantern_gpu_filter_t *b,
                                                                    int op, usearch_error_t *);
/* Diagnostics: the bitmap (n_words >= ceil(f->n / 32), else refused; words past the filter's own are written as zero) and / or the
 * first min(cap, count) allowed slots in list order; either pointer may be NULL.  Needs only a live handle: a stale filter can still
 * be read.  Returns the count. */
/* the index's size when the filter was built: its bitmap spans ceil(rows / 32) words (a stale filter answers too) */
LANTERN_GPU_EXPORT size_t lantern_gpu_filter_rows(const lantern_gpu_filter_t *f, usearch_error_t *);
LANTERN_GPU_EXPORT size_t lantern_gpu_filter_export(const lantern_gpu_filter_t *f, uint32_t *words, size_t n_words, uint32_t *slots, size_t cap,
                                                    usearch_error_t *);
/* path: 0 auto, 1 walk, 2 exact.  cand_cap = C (0: max(4 expansion, 256), capped by LDS; below expansion it is raised to it).
 * Auto takes the exact path when allowed^2 <= exact_factor * ef * n, ef the caller's or else the index's: a walk under a filter of
 * selectivity s evaluates about D / s rows, the exact path `allowed`.  The rule does not depend on k or skip, so it is stable
 * across a scan's pages.  Default exact_factor: 5.6, the measured crossover of the two paths (clustered 1M x 768 f32, ef = 64:
 * DESIGN.md 4.9).  An empty filter returns 0 results without a launch. */
LANTERN_GPU_EXPORT void lantern_gpu_set_filter_policy(usearch_index_t, int path, size_t cand_cap, double exact_factor, usearch_error_t *);
/* The seeded walk (5 above): the walk path of every later filtered search on this index -- single filter, per query, cursor, scan,
 * scan-side service -- starts from min(seeds, allowed) allowed rows.  0 = off (the default).  More than 4096 is refused.  For a
 * filter correlated with the data (the rows of one cluster, queries from all) the unseeded walk exhausts `next` among disallowed rows
 * before it meets an allowed one; a random filter pays the seeds' evaluations. */
LANTERN_GPU_EXPORT void lantern_gpu_set_filter_seeds(usearch_index_t, size_t seeds, usearch_error_t *);
/* diagnostic: out[0] the setting, [1] S' of the last single-filter walk launch (0 after an exact or empty one; per-query calls leave
 * it alone), [2] queries of the last filtered call that ran seeded, [3] walk-path queries of that call that did not (seeds = 0, or
 * NULL entries) */
LANTERN_GPU_EXPORT void lantern_gpu_last_filtered_seeds(usearch_index_t, uint32_t out[4], usearch_error_t *);
/* COMPACT PQ INDEXES (DESIGN.md 4.9 "Compact pq indexes").  A compact pq index (lantern_gpu_pq_compact) keeps only its code bytes in
 * HBM.  on = 0, THE DEFAULT: every filtered search on it is refused -- "filtered search does not run on a compact pq index: expand it
 * first (lantern_gpu_pq_expand)" -- as before this switch existed.  on = 1: every filtered entry point -- single filter, per query,
 * per-query (k, ef, skip), seeded walk, cursor, scan, scan-side service -- serves it, by the row routine the unfiltered search of that
 * index takes:
 *  - rows DECODED ON THE FLY (subvectors of whole 16-byte chunks, LANTERN_GPU_PQ_ADC unset or 0): the expanded index's arithmetic.
 *    With the same filter and policy every answer is the expanded index's: ids, distance bits, counts, D, E, and the launch shape
 *    lantern_gpu_last_filtered_launch reports;
 *  - ADC over the code rows (every other compact index): a row's distance is the unfiltered compact search's, bit for bit, on the walk
 *    and the exact path.  The per-query table (16 KiB per 16-byte chunk of a code row: 32 KiB at 32 subvectors, 128 KiB at 128 -- and
 *    at 96, whose rows sit at the 128-byte stride) lies in the launch's LDS in front of the raw query row, the walk's lists and the
 *    visited set, within the same 160 KiB: expansions and k + skip that no
 *    longer fit beside it are refused with the texts of the calls above, the visited set takes what is left (at most 2048 slots;
 *    below 4 M0 the HBM bitmap alone: its size changes no answer, D or E), and one workgroup runs per CU where two do not fit.
 *    The table is built anew for every query, and for none that evaluates no row (an empty filter, k_i == 0).
 * The path rule and its default exact_factor are unchanged: the f32 rows' 5.6, which also fits decoded rows; ADC's measured crossover is
 * far higher, and a caller who serves an ADC index may raise exact_factor through lantern_gpu_set_filter_policy.
 * on other than 0 or 1 is refused.  On an index that is not compact the setting changes nothing.  Default off until the path has
 * been measured on a device, as lantern_gpu_set_filter_seeds. */
LANTERN_GPU_EXPORT void lantern_gpu_set_filter_compact(usearch_index_t, int on, usearch_error_t *);
/* diagnostic: 0 the switch is off; else what a filtered search on the index as it stands now runs on: 1 stored rows (the index is
 * not compact), 2 rows decoded on the fly, 3 ADC */
LANTERN_GPU_EXPORT int lantern_gpu_filter_compact(usearch_index_t, usearch_error_t *);
/* launches of the two filtered kernels since the index was created */
LANTERN_GPU_EXPORT void lantern_gpu_filter_stats(usearch_index_t, uint64_t *walk_launches, uint64_t *exact_launches, usearch_error_t *);
/* the shape of the last filtered launch on this index (diagnostic; tests assert the regime a launch ran in):
 * out[0] path (1 walk, 2 exact), [1] workgroups, [2] expansion (walk: max(ef, k + skip); exact: k + skip), [3] candidate cap C of the walk
 * (0 on the exact path), [4] LDS visited-set slots of the walk (0 = HBM bitmap only; 0 on the exact path), [5] dynamic LDS bytes per
 * workgroup.  All zero before the first filtered launch and after a call that launched nothing (an empty filter).
 * A call answered by the dense route (lantern_gpu_set_filter_dense) reports out[0] = 3, out[2] = k + skip and 0 in every other field. */
LANTERN_GPU_EXPORT void lantern_gpu_last_filtered_launch(usearch_index_t, uint32_t out[6], usearch_error_t *);
/* THE EXACT PATH'S DENSE ROUTE (DESIGN.md 4.9 "Dense exact path"): a second implementation of the exact path for a batch of queries
 * behind ONE filter.  The exact pass reads every allowed row once per query; the dense route gathers the allowed rows into contiguous
 * chunks once per call and contracts them against all the queries on the matrix cores, as lantern_gpu_exact_search does with the whole
 * index -- top-(k + skip + 16) by the contraction, re-ranked with the walk's per-pair reduction, certified per query, and the queries the
 * certificate refuses answered by the exact pass itself.  Every output is the exact pass's: slots, distance bits, labels, counts,
 * D (= allowed), E (= 0), the tails of short rows and the cumulative counters; only the launches differ.  The path rule is untouched:
 * which filters go exact is still lantern_gpu_set_filter_policy's.
 * min_queries = 0, THE DEFAULT: off; every call issues the launches it issued before this switch existed.
 * min_queries = m > 0: a call of lantern_gpu_search_batch_filtered or lantern_gpu_search_batch_filtered_device takes the dense route
 *   when nq >= m, the path of its queries is exact (forced or by the rule), k + skip <= 240 (the exact k-NN's bound on k) and the index
 *   is not a compact pq index.  Every other call runs the kernels it runs today: none is refused because of this setting.
 * The per-query-filter calls, cursors, scans and the scan-side service never take it.
 * SYNCHRONISATION: a call on the dense route waits for its stream before it returns -- the certificate's flags cross to the host --
 * so lantern_gpu_search_batch_filtered_device, otherwise asynchronous, is synchronous for such a call (its answers are complete on
 * return).  The gathered copy is not kept: a filter reused by a later call is gathered again. */
LANTERN_GPU_EXPORT void lantern_gpu_set_filter_dense(usearch_index_t, size_t min_queries, usearch_error_t *);
LANTERN_GPU_EXPORT size_t lantern_gpu_filter_dense(usearch_index_t, usearch_error_t *); /* the setting */
/* since the index was created: out[0] calls answered by the dense route, [1] their queries, [2] of those the certificate passed,
 * [3] of those recomputed by the exact pass ([1] = [2] + [3]; a call with [3] > 0 also counts one exact launch in lantern_gpu_filter_stats) */
LANTERN_GPU_EXPORT void lantern_gpu_filter_dense_stats(usearch_index_t, uint64_t out[4], usearch_error_t *);
/* The dense route's decision and buffers without a device (a pure function; the call itself plans through it).
 * in[11]: [0] metric code (as lantern_gpu_plan_dense)  [1] 16-byte chunks per stored row  [2] allowed rows of the filter  [3] queries
 *   [4] k  [5] skip  [6] the min_queries setting  [7] the queries' path is exact (0 / 1)  [8] the index is a compact pq index (0 / 1)
 *   [9] LANTERN_GPU_DENSE_NATIVE (-1: unset)  [10] LANTERN_GPU_DENSE_FUSED (-1: unset)
 * out[8]: [0] 1: the call takes the dense route  [1] why not: 0 taken, 1 the setting is 0, 2 nq < min_queries, 3 the path is the walk,
 *   4 k + skip > 240, 5 a compact pq index, 6 nothing to launch (no allowed row, no query, k = 0)
 *   and, when taken (0 otherwise): [2] kk = k + skip + 16 survivors per query  [3] rows per gathered chunk
 *   [4] (low, high) bytes of the gather buffer: one chunk of rows as stored  [6] (low, high) bytes of the gathered rows' norm words
 *   (0 for bit rows, which carry none)
 * steps, cap, *n_steps: as lantern_gpu_plan_exact_knn's, and exactly its steps for (metric code, chunks, base rows = allowed, queries,
 *   k + skip); none when the route is not taken.  Returns NULL, or why the input is refused. */
LANTERN_GPU_EXPORT const char *lantern_gpu_plan_filtered_dense(const int64_t in[11], uint32_t out[8], uint32_t steps[][4], size_t cap, size_t *n_steps);
/* THE DENSE ROUTE FOR PER-QUERY-FILTER CALLS (DESIGN.md 4.9 "Dense exact path, per-query filters"): in a call of
 * lantern_gpu_search_batch_filtered_each or lantern_gpu_search_batch_filtered_each_device, the exact-path queries that name the same
 * filter HANDLE form a group, and the groups of at least min_group queries are answered by one segmented run of the exact k-NN: the
 * groups' slot lists are concatenated into one list (the call's own copy), the dense queries gathered into one block, and a tile of
 * one group's queries is contracted against that group's rows only -- top-(k + skip + 16) by the contraction, re-ranked with the
 * walk's per-pair reduction, certified per query.  Every output is what the call gives without the setting: slots, distance bits,
 * labels, counts, D (= that query's own filter's count), E (= 0), the tails of short rows and the cumulative counters.
 * A SEPARATE setting from lantern_gpu_set_filter_dense: neither switch turns the other's route on.
 * min_group = 0, THE DEFAULT: off; every call issues exactly the launches it issues without this switch.
 * min_group = m > 0: the path rule is untouched -- each query's path is still evaluated from its own filter's count.  Among the
 *   queries whose path is exact, those sharing a handle are a group (pointer identity, not set equality: two handles over one set are
 *   two groups).  A group is dense when it has >= m queries, k + skip <= 240, the index is not a compact pq index and the rows of all
 *   dense groups together fit 32 bits.  Everything else -- walk-path queries, NULL entries, empty filters, smaller groups -- runs
 *   exactly as without the setting, in the call's at most two per-query launches; the dense queries the certificate refuses join the
 *   exact launch's list, which answers them as it would have.  No call is refused because of the setting.
 * lantern_gpu_search_batch_filtered_each_lane, the three _each_params forms, cursors, scans and the scan-side service never take it.
 * COSINE: a row norm outside the certificate's range in ANY dense group refuses every dense query of the call (they are all
 *   recomputed by the exact launch): the flag is call-wide.
 * SYNCHRONISATION: a call with at least one dense group waits for its stream ONCE, after pending insert batches and the dense run and
 *   before its per-query launches are queued -- the certificate's flags cross to the host -- so
 *   lantern_gpu_search_batch_filtered_each_device, otherwise asynchronous, is synchronous for such a call up to that point: the dense
 *   groups' answers are complete on return, the per-query launches behind them are queued on `stream` as always.  The filters'
 *   lifetime rule is unchanged.
 * lantern_gpu_last_filtered_each keeps its meaning: [1] counts the dense queries (their path is exact), [5] the per-query kernels'
 * launches (0 .. 2: 0 when every query of the call was answered by the dense run).  lantern_gpu_filter_dense_stats counts such a call
 * once, and its dense queries as the single-filter route's. */
LANTERN_GPU_EXPORT void lantern_gpu_set_filter_dense_each(usearch_index_t, size_t min_group, usearch_error_t *);
LANTERN_GPU_EXPORT size_t lantern_gpu_filter_dense_each(usearch_index_t, usearch_error_t *); /* the setting */
/* the dense run of the last per-query-filter call on this index that passed its checks (all zero when it made none): out[0] dense
 * groups, [1] their queries, [2] of those certified, [3] recomputed by the exact launch, [4] rows gathered (the concatenated list's
 * length), [5] contraction steps */
LANTERN_GPU_EXPORT void lantern_gpu_last_filtered_each_dense(usearch_index_t, uint32_t out[6], usearch_error_t *);
/* That route's plan without a device (a pure function; the call itself plans through it).
 * in[7]: [0] metric code (as lantern_gpu_plan_dense)  [1] 16-byte chunks per stored row  [2] k  [3] skip  [4] the min_group setting
 *   [5] the index is a compact pq index (0 / 1)  [6] LANTERN_GPU_DENSE_NATIVE (-1: unset)
 * queries[nq][3]: per query [0] a filter id (-1: a NULL entry; equal ids for equal handles)  [1] that filter's allowed rows
 *   [2] the query's path is exact (0 / 1)
 * out[6]: [0] dense groups  [1] dense queries  [2] 0: at least one group is dense; else why none is: 1 the setting is 0,
 *   2 k + skip > 240, 3 a compact pq index, 4 the dense groups' rows do not fit 32 bits, 5 no handle stands behind min_group
 *   exact-path queries  [3] kk = k + skip + 16 survivors per query (0: nothing dense)  [4] rows per gathered chunk of the list
 *   [5] rows of the concatenated list
 * group[nq]: the dense group of each query, 0xFFFFFFFF: none.  order[nq]: its first out[1] entries are the dense queries as the run
 *   holds them (original query indices): groups by the first query that names them, a group's queries in call order.
 * seg[nq + 1]: its first out[0] + 1 entries are the groups' offsets into the concatenated list.
 * steps[i] = { first dense query, queries (<= 1024), first list position, positions }: one contraction launch -- a tile of ONE
 *   group's queries against that group's positions inside ONE chunk of 65 536 positions; chunk-major, then by group, then by tile.
 *   The first `cap` are written, *n_steps is their number.  Returns NULL, or why the input is refused. */
LANTERN_GPU_EXPORT const char *lantern_gpu_plan_filtered_each_dense(const int64_t in[7], const int64_t queries[][3], size_t nq, uint32_t out[6],
                                                                    uint32_t group[], uint32_t order[], uint32_t seg[], uint32_t steps[][4],
                                                                    size_t cap, size_t *n_steps);
/* lantern_gpu_search_batch through a filter (host buffers; the unused tail of a row is label 0 and +inf) */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_filtered(usearch_index_t, const lantern_gpu_filter_t *, const void *queries, size_t nq,
                                                          usearch_scalar_kind_t, size_t k, size_t ef, usearch_label_t *labels,
                                                          float *distances, uint32_t *counts, usearch_error_t *);
/* lantern_gpu_search_batch_device_strided through a filter */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_filtered_device(usearch_index_t, const lantern_gpu_filter_t *, const void *d_queries,
                                                                 size_t query_stride_bytes, size_t nq, size_t k, size_t ef, size_t skip,
                                                                 uint64_t *d_labels, float *d_distances, uint32_t *d_slots,
                                                                 uint32_t *d_counts, uint64_t *d_dist_evals, uint64_t *d_expansions,
                                                                 void *stream, usearch_error_t *);
/* PER-QUERY FILTERS: one call, filters[i] the filter of query i (a host array of nq handles).  Per query i:
 *  - filters[i] a filter: exactly what the single-filter call gives that query with that filter -- the same path rule
 *    (lantern_gpu_set_filter_policy: forced path, cand_cap, exact_factor, evaluated from THAT filter's count, n and ef), the same ids,
 *    distance bits, count, D and E;
 *  - filters[i] == NULL: every row allowed, walk path: by the all-allowed property the ids, bits, D and E of the unfiltered search;
 *  - an empty filter: count 0, rows of label 0 / +inf / EMPTY slot, D = E = 0.
 * The queries split into a walk group and an exact group; each group is ONE launch over its own list of queries (the exact group
 * longest first), whatever the filters are, and every answer lands in the row of its query.  Empty filters have no path: they ride
 * in the exact launch (in the walk launch when no query takes the exact path), where they touch no row; a call of empty filters
 * alone is one exact launch.  k, ef and skip -- hence expansion, C and the LDS carve -- are the call's, uniform over its queries.
 * An entry that is not a live filter handle, belongs to another index or is stale refuses the WHOLE call before anything is
 * launched or written: the single-filter message plus " (filters[i])", i the first offending position.  Compact pq indexes are
 * refused or served as by the single-filter calls (lantern_gpu_set_filter_compact).
 * Lifetime: a filter may be freed by its owner as soon as the call that used it has returned (the host and lane forms), or the
 * work queued on `stream` has completed (the device form).  The filters[] array itself is read only during the call.
 * lantern_gpu_filter_stats counts the launches; lantern_gpu_last_filtered_launch is not updated by these calls. */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_filtered_each(usearch_index_t, const lantern_gpu_filter_t *const *filters, const void *queries,
                                                               size_t nq, usearch_scalar_kind_t, size_t k, size_t ef, usearch_label_t *labels,
                                                               float *distances, uint32_t *counts, usearch_error_t *);
/* lantern_gpu_search_batch_filtered_device with a filter per query */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_filtered_each_device(usearch_index_t, const lantern_gpu_filter_t *const *filters,
                                                                      const void *d_queries, size_t query_stride_bytes, size_t nq, size_t k,
                                                                      size_t ef, size_t skip, uint64_t *d_labels, float *d_distances,
                                                                      uint32_t *d_slots, uint32_t *d_counts, uint64_t *d_dist_evals,
                                                                      uint64_t *d_expansions, void *stream, usearch_error_t *);
/* lantern_gpu_search_batch_lane with a filter per query: the lane's stream and page-locked staging block, the index mutex held only
 * while the copies and the launches are queued, the wait outside it (what a service that coalesces filtered queries calls) */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_filtered_each_lane(usearch_index_t, int lane, const lantern_gpu_filter_t *const *filters,
                                                                    const void *queries, size_t nq, usearch_scalar_kind_t, size_t k, size_t ef,
                                                                    usearch_label_t *labels, float *distances, uint32_t *counts,
                                                                    usearch_error_t *);
/* the last per-query call on this index that passed its checks (diagnostic; tests assert the regime): out[0] queries on the walk
 * path (the unfiltered ones included), [1] on the exact path, [2] unfiltered (NULL) entries, [3] empty filters, [4] distinct filter
 * handles in the array, [5] kernel launches made (0 .. 2).  All zero before the first such call. */
LANTERN_GPU_EXPORT void lantern_gpu_last_filtered_each(usearch_index_t, uint32_t out[6], usearch_error_t *);
/* PER-QUERY FILTERS WITH PER-QUERY k, ef AND skip: query i through filters[i] with params[i] = (k_i, ef_i,
 * skip_i) -- ef 0 = the index's default, reserved must be 0; `params` is a HOST array in all three forms, read during the call.
 * CONTRACT: for query i the ids, distance bits, count, D and E are exactly those of the single-filter call with filters[i] and
 * (k_i, ef_i, skip_i), with no tolerance.  filters[i] == NULL: the unfiltered search's answer for those parameters (the all-allowed
 * property above).  An empty filter: count 0, D = E = 0.  k_i == 0: no walk, count 0, D = E = 0, and the row is still written.
 * Answer rows are k_stride wide; the tail of row i beyond k_i is label 0 / +inf / EMPTY slot.
 * Per query, by the arithmetic of the uniform call: the path rule from that query's filter count and ef_i (or the index's default);
 * the walk's expansion max(ef_i, k_i + skip_i); the exact pass keeps k_i + skip_i keys; the candidate cap C_i is the policy's
 * cand_cap raised to the expansion, or max(4 expansion_i, 256), capped by the LDS left beside that query's own expansion.
 * lantern_gpu_set_filter_policy and lantern_gpu_set_filter_seeds apply as to lantern_gpu_search_batch_filtered_each.
 * LAUNCHES: at most two -- one walk launch over its list (expansion descending, stable) and one exact launch over its list (allowed
 * count descending, stable).  Queries without a path -- an empty filter, k_i == 0, an empty index -- ride in the exact launch (in the
 * walk launch when no query takes the exact path), where they touch no row; a call of such queries ALONE makes no launch: its rows
 * are written by memsets.  Each launch is carved once: the walk's from its largest expansion and its largest C_i, the exact one's from
 * its largest k_i + skip_i; vis_slots, the rows per round and the grid follow from that carve by the uniform call's rules.  The size
 * of the visited set changes no answer, D or E.
 * REFUSALS are for the whole call, before anything is queued or written, in this order:
 *  1. the handles, as lantern_gpu_search_batch_filtered_each: a null filter array, the index handle (an entry of filters[] that is no
 *     filter handle at all is named then, too);
 *  2. the parameter array, with lantern_gpu_search_batch_params' texts: NULL, reserved != 0, k_stride below a k_i -- each but the
 *     first with " (params[i])", i the first offender;
 *  (the scalar kind and NULL buffers of the host forms, the lane number before everything, the row stride of the device form)
 *  3. the filters: not a live handle / another index / stale, with " (filters[i])";
 *  4. a compact pq index, with the single-filter calls' text, unless lantern_gpu_set_filter_compact serves it;
 *  5. a query whose own shape exceeds the 160 KiB LDS budget, in batch order: the uniform call's text plus " (params[i])";
 *  6. "... the largest expansion and the largest candidate cap of the batch do not fit together: split the batch": every query fits
 *     alone, the walk launch's joint carve does not.  This needs the automatic cap (an explicit cand_cap gives the query of the largest
 *     expansion the largest C as well, and that query fits): with B(e) = 16 chunks + 2 ceil16(8 e) + 2 ceil16(8 M0) + ceil16(4 M0) +
 *     scalars + 16 bytes of walk LDS beside `next`, a query's C is min(max(4 e, 256), floor((163840 - B(e)) / 16)), and the call is
 *     refused iff B(e_max) + 16 C_max > 163840.  A query's own cap starts to bind at 80 e > 163840 - B(0): e > 2000 on 768-d f32
 *     rows with M = 16, 2032 at 128-d; below that, C_max = 4 e_max belongs to the largest expansion itself and the call fits.  So it
 *     takes a query of e > ~2000 whose room, floor((163840 - B(e)) / 16), is smaller than another query's C: a scan that has paged
 *     to 4900 rows leaves 5100 (768-d) and is refused beside any query of expansion 1276 or more; two long scans of different lengths
 *     (3300 and 3010) refuse each other.  A caller who meets it splits the batch.
 * Lifetime of the filters as for lantern_gpu_search_batch_filtered_each.  There is no notify form. */
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_filtered_each_params(usearch_index_t, const lantern_gpu_filter_t *const *filters,
                                                                      const void *queries, size_t nq, usearch_scalar_kind_t,
                                                                      const lantern_gpu_query_params *params, size_t k_stride,
                                                                      usearch_label_t *labels, float *distances, uint32_t *counts,
                                                                      usearch_error_t *);
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_filtered_each_params_lane(usearch_index_t, int lane, const lantern_gpu_filter_t *const *filters,
                                                                           const void *queries, size_t nq, usearch_scalar_kind_t,
                                                                           const lantern_gpu_query_params *params, size_t k_stride,
                                                                           usearch_label_t *labels, float *distances, uint32_t *counts,
                                                                           usearch_error_t *);
LANTERN_GPU_EXPORT void lantern_gpu_search_batch_filtered_each_params_device(usearch_index_t, const lantern_gpu_filter_t *const *filters,
                                                                             const void *d_queries, size_t query_stride_bytes, size_t nq,
                                                                             const lantern_gpu_query_params *params, size_t k_stride,
                                                                             uint64_t *d_labels, float *d_distances, uint32_t *d_slots,
                                                                             uint32_t *d_counts, uint64_t *d_dist_evals, uint64_t *d_expansions,
                                                                             void *stream, usearch_error_t *);
/* These calls update lantern_gpu_last_filtered_each (its fields mean the same; [3] counts every query without a path, k_i == 0
 * included) and fill this: out[0] the largest walk expansion, [1] the largest C_i, [2] the largest k_i + skip_i on the exact path,
 * [3] queries with k_i == 0.  All zero before the first such call. */
LANTERN_GPU_EXPORT void lantern_gpu_last_filtered_each_params(usearch_index_t, uint32_t out[4], usearch_error_t *);
/* The plan of such a call, without a device, an index or the environment (a pure function; the entry points plan through it).
 * in[8]: [0] chunks (16-byte chunks per stored row)  [1] M0  [2] n (rows)  [3] the index's default ef  [4] forced path (0 auto, 1 walk,
 *   2 exact)  [5] cand_cap (0: automatic)  [6] exact_factor, the BIT PATTERN of the double  [7] seeds (changes no shape).
 * counts[i]: the allowed count of query i's filter, -1 for a NULL entry.
 * per_query[i]: [0] path (0 none, 1 walk, 2 exact)  [1] expansion (exact: k + skip; 0 without a path)  [2] C (walk only)  [3] position
 *   in its launch's list (a query without a path: in the list it rides in; 0 when nothing is launched).
 * launch[0] the walk's, launch[1] the exact one's: [0] queries of its list, riders included (0: no such launch)  [1] largest expansion
 *   (exact: largest k + skip)  [2] largest C  [3] vis_slots (walk) / rows per round (exact)  [4] LDS bytes per workgroup
 *   [5] workgroups per CU.
 * Returns NULL, or the text the call is refused with (refusals 5 and 6 above). */
LANTERN_GPU_EXPORT const char *lantern_gpu_plan_filtered_params(const int64_t in[8], const int64_t counts[],
                                                                const lantern_gpu_query_params params[], size_t nq, uint32_t per_query[][4],
                                                                uint32_t launch[2][6]);
/* The same plan for a compact pq index served under lantern_gpu_set_filter_compact -- what the entry points plan such a call through;
 * pure as the one above.  in[9]: in[0..8) as above, [0] the chunks of a DECODED row (= of a raw f32 query row); [8] the 16-byte chunks
 * of a code row where the index is served by ADC (1..8: num_subvectors padded to 16, / 16), 0 where its rows are decoded on the fly.
 * With in[8] == 0 every field is lantern_gpu_plan_filtered_params' on the same in[0..8): the expanded index's shape.  With ADC the
 * carve is: table (in[8] x 16384 bytes) | raw query row | the lists | the visited set; 8 lanes per row; vis_slots what fits in the
 * workgroup's 160 KiB, at most 2048, 0 below 4 M0.  per_query as above.  launch[l]: [0..6) as above, [6] the table's bytes (0: no
 * table, or no such launch).  Returns NULL or the refusal, with the texts and " (params[i])" rules of refusals 5 and 6. */
LANTERN_GPU_EXPORT const char *lantern_gpu_plan_filtered_compact(const int64_t in[9], const int64_t counts[],
                                                                 const lantern_gpu_query_params params[], size_t nq, uint32_t per_query[][4],
                                                                 uint32_t launch[2][7]);
/* kernel shape of the search launch: waves per query (1..8; 0 = automatic: 4 when the batch fills the chip, up to 8 for
 * smaller batches) and resident workgroups (0 = auto) */
LANTERN_GPU_EXPORT void lantern_gpu_set_search_shape(usearch_index_t, int waves_per_query, int max_workgroups,
                                                     usearch_error_t *);

/* Exact k-NN over the index's vectors (the seq-scan `ORDER BY v <op> q LIMIT k`; ground truth
 * for recall, index_autotune/mod.rs:196-203).  Host buffers; slots: nq x k ascending by
 * (distance, slot).  Guarantee: per query the k smallest rows by (exact-order distance, slot) -- the distance in the pair
 * kernel's reduction order (usearch_distance's bits) -- identical to a brute force in that order.  The fp32-MFMA
 * pre-selection is certified per query and a query it cannot certify is recomputed in exact order (DESIGN.md 4.5;
 * lantern_gpu_exact_knn_stats).  k <= 240. */
LANTERN_GPU_EXPORT void lantern_gpu_exact_search(usearch_index_t, const void *queries, size_t nq, size_t k,
                                                 uint32_t *slots, float *distances, usearch_error_t *);

/* Diagnostic for the measurement harness: HIP events around every launch of the MFMA contraction (k_dense_f32; k_dense_native on
 * f16 / i8 indexes) inside
 * lantern_gpu_exact_search / _assign_to_clusters / _distance_matrix.  on != 0 starts recording; on == 0 stops and writes up to
 * `cap` records -- ms[i], rows[i] x cols[i] (queries x base rows of the launch), fused[i] (1: the launch with the fused top-k
 * epilogue) -- and returns how many launches were recorded.  Process-wide; any pointer may be NULL. */
LANTERN_GPU_EXPORT size_t lantern_gpu_dense_profile(int on, float *ms, uint32_t *rows, uint32_t *cols, uint32_t *fused, size_t cap);
/* Process-wide counters of the exact k-NN (lantern_gpu_exact_search, _assign_to_clusters, PQ encoding), cumulative: queries
 * answered, how many of them the MFMA pre-selection's certificate passed, and how many took the exact-order fallback
 * (queries = certified + fallback).  Any pointer may be NULL. */
LANTERN_GPU_EXPORT void lantern_gpu_exact_knn_stats(uint64_t *queries, uint64_t *certified, uint64_t *fallback);
/* Process-wide cumulative launches of the MFMA contraction by the type of its operands: launches[0] f32 rows (k_dense_f32; a
 * quantised index on the dequantised path counts here), [1] f16 rows, [2] i8 rows as stored (k_dense_native).  Counted inside
 * lantern_gpu_exact_search / _assign_to_clusters / PQ encoding and lantern_gpu_distance_matrix(exact_order = 0). */
LANTERN_GPU_EXPORT void lantern_gpu_dense_kind_stats(uint64_t launches[3]);
/* Which contraction an exact k-NN call runs -- host arithmetic only; the call itself takes its decisions from this function.
 * in:  [0] the index's internal metric code (metric, + 100 for f16 storage, + 200 for i8), [1] 16-byte chunks per stored row,
 *      [2] base rows, [3] the value of LANTERN_GPU_DENSE_NATIVE (-1: unset).
 * out: [0] operand kind 0 / 1 / 2 (f32, f16, i8); [1] bytes of the f32 copy of one chunk of base rows the call allocates (0
 *      when the rows are contracted as stored); [2] the `dims` handed to the certificate (0: the pre-selection ranks on the
 *      exact-order distance itself and is certified by construction: popcount metrics, native i8); [3] K steps (128 bytes per
 *      row each) per output tile (0: no MFMA contraction).  Returns NULL, or why the input is refused. */
LANTERN_GPU_EXPORT const char *lantern_gpu_plan_dense(const int64_t in[4], uint32_t out[4]);
/* Everything an exact k-NN call (lantern_gpu_exact_search, _assign_to_clusters, PQ encoding) decides before it touches the device,
 * without one (a pure function; lantern_gpu_plan_dense shows four of its numbers): the call plans with this function and then
 * launches what the plan lists.
 * in[7]: [0] metric code (as lantern_gpu_plan_dense)  [1] 16-byte chunks per stored row  [2] base rows  [3] queries  [4] k (1..240)
 *   [5] LANTERN_GPU_DENSE_NATIVE (-1: unset)  [6] LANTERN_GPU_DENSE_FUSED (-1: unset)
 * out[34]: [0] operand kind 0 / 1 / 2 (f32, f16, i8)  [1] the rows are dequantised to f32 for the contraction: 0 no, 1 from f16, 2 from i8
 *   [2] chunks of a row as the contraction reads it  [3] a popcount metric  [4] the pre-selection's keys are exact: nothing to certify
 *   [5] the dims the certificate is told  [6] K steps per output tile  [7] kk = k + 16 survivors per query  [8] base rows per launch
 *   [9] queries per launch  [10] seed columns  [11] candidate keys per query  [12] fused, after the rule: asked for, not a popcount
 *   metric, more base rows than seed columns  [13] leading dimension of the distance matrix
 *   then ten byte counts as (low word, high word): [14] the block of norms, best lists and flags  [16] the distance matrix
 *   [18] the candidate lists (0 unless fused)  [20] the queries' f32 copy  [22] one chunk of base rows' f32 copy (0: no copy)
 *   and offsets: [24] query norms, [26] base norms, [28] best lists (8-byte aligned), [30] flags inside [14]; [32] counters inside [18]
 * steps: the contraction launches in order (chunk of base rows by chunk, query tile by query tile, plain before fused), up to cap
 *   of them: [0] queries  [1] base rows  [2] 1: the fused epilogue (folded in by k_select over the candidate lists), 0: the matrix
 *   (k_select over its rows)  [3] the first base row.  *n_steps: how many there are, whatever cap is.
 * Returns NULL, or why the input is refused (a null array, a field out of range, rows that do not fit 32 bits). */
LANTERN_GPU_EXPORT const char *lantern_gpu_plan_exact_knn(const int64_t in[7], uint32_t out[34], uint32_t steps[][4], size_t cap, size_t *n_steps);

/* Diagnostic for the measurement harness: the memory objects every query of a launch asks for, in order (rows evaluated, adjacency
 * lists read) -- the input of the cache model behind bench.py's roofline.frac_dram_model (lantern_amd/tools/cache_model.c).
 * on = 1: allocate nq x per_query_cap entries and trace the following launches of at most nq queries (the instrumented walk:
 * f32 l2sq / cos, as lantern_gpu_search_unique_rows; same answers, D and E).  on = 0: copy the LAST traced launch's trace
 * (nq x per_query_cap u32) and counts (nq u32; above per_query_cap: the tail was dropped) out, free the buffers, switch it off.
 * Entry = slot (a row evaluation) | 0x80000000 (level-0 list of that node read) | 0xC0000000 (an upper-level list). */
LANTERN_GPU_EXPORT void lantern_gpu_search_row_trace(usearch_index_t, int on, size_t nq, size_t per_query_cap, uint32_t *trace,
                                                     uint32_t *counts, usearch_error_t *);

/* workgroups of the last unfiltered search launch, whatever path it took = walks resident on the device at a time (the cache
 * model's `walkers`) */
LANTERN_GPU_EXPORT int lantern_gpu_last_search_grid(usearch_index_t, usearch_error_t *);
/* The shape the library gives an unfiltered search launch, without a device (a pure function: tests of the shape rules, tuning).
 * in[31], by the names of the index's fields, the call and the environment switches:
 *   [0] chunks (16-byte chunks per stored row)  [1] M  [2] M0  [3] mcode (metric, +100 for f16 rows, +200 for i8)  [4] n (rows)
 *   [5] the index's default ef  [6] num_cus  [7] pq_compact  [8] pqd_inv (!= 0: rows can be decoded on the fly)  [9] pq_S16 (bytes
 *   per padded code row)  [10] search_vis_slots (-1: automatic)  [11] search_max_wg (0: none)  [12] phase_profile  [13] spec_profile
 *   [14] nq  [15] k  [16] ef  [17] skip  [18] waves (> 0: explicit; < 0: automatic, the classic fallback takes -waves)
 *   [19] 1: one class of a per-query-parameter call, shaped by [20] its largest expansion
 *   [21] LANTERN_GPU_SPEC is set, [22] its value  [23] LANTERN_GPU_ADC_SPEC is set, [24] != 0  [25] LANTERN_GPU_PQ_ADC != 0
 *   [26] LANTERN_GPU_SPEC_WAVES (0: unset)  [27] LANTERN_GPU_LDS_LIST != 0  [28] LANTERN_GPU_WIDE_ROWS (-1: unset)
 *   [29] reserved and ignored (the switch of a walk since removed; the slots after it keep their places)
 *   [30] LANTERN_GPU_WAVES_PER_CU (0: unset)
 * out[12]: [0] path (0 ADC over the code rows, 1 the f32 walk over rows decoded on the fly, 2 classic, 3 spec 1, 4 spec 2)
 *   [1] spec (the walk's shape; paths 0 and 1 take 0 / 2 and any)  [2] expansion  [3] waves per workgroup  [4] grid  [5] vis_slots  [6] LDS bytes per workgroup
 *   [7] spec_prefetch  [8] spec_cache  [9] wide_rows  [10] a latency-bound shape  [11] lds_list
 * Returns NULL, or the text the launch is refused with (then only out[2] is meaningful). */
LANTERN_GPU_EXPORT const char *lantern_gpu_plan_search(const int64_t in[31], uint32_t out[12]);
/* ... of an index that has ([31] != 0) or has not an int8 screen (f32 l2sq / cosine rows of >= 128 chunks; lantern_gpu_plan_search
 * plans the index without one): in[32], out[13].  out[12]: the bytes of the query's int8 planes in the workgroup's LDS, != 0 iff the
 * launch screens; they are part of out[6] and come out of out[5]. */
LANTERN_GPU_EXPORT const char *lantern_gpu_plan_search_screen(const int64_t in[32], uint32_t out[13]);
/* ... with the switch of the screened launches' list prefetch: in[33], [32] = LANTERN_GPU_SCREEN_LIST_PREFETCH (-1: unset, 0, 1; read
 * on every call); out[14], [13] != 0: the visit wave requests the front's level-0 list one hop ahead.  Only a launch that screens
 * (out[12] != 0) ever does; every other launch is planned as by lantern_gpu_plan_search. */
LANTERN_GPU_EXPORT const char *lantern_gpu_plan_search_screen_prefetch(const int64_t in[33], uint32_t out[14]);

/* Gathered distances: out[i] = metric(query, row(slots[i])) -- the kernel the graph walk is
 * made of, exposed for tests and profiling.  Host buffers. */
LANTERN_GPU_EXPORT void lantern_gpu_distance_gather(usearch_index_t, const void *query, const uint32_t *slots,
                                                    size_t n, float *out, usearch_error_t *);
/* kernel time (ms, HIP events on the index stream) of the last lantern_gpu_distance_gather launch of this index */
LANTERN_GPU_EXPORT float lantern_gpu_last_gather_ms(usearch_index_t, usearch_error_t *);
/* The int8 screen of the f32 l2sq and cosine walks: row evaluations of the searches that ran with it (logical,
 * cumulative) and how many of them read the f32 row (exact); the rest were rejected on the screen row.  Both 0 when the index has
 * no screen (another metric or storage, rows of fewer than 128 chunks, LANTERN_GPU_SCREEN=0). */
LANTERN_GPU_EXPORT void lantern_gpu_search_screen_stats(usearch_index_t, uint64_t *logical, uint64_t *exact, usearch_error_t *);
/* The int8 screen in the INSERTION walk: builds and batched inserts of an index that has a screen table test the
 * level-0 candidates of k_insert on the int8 row copy first, with the searches' exact bound -- the graph is edge for edge the one built
 * without it.  mode: 0 = off, 1 = on; any other value is refused.  On an index without a screen table mode 1 is accepted and has no
 * effect.  A launch is screened iff the mode is on, the index has the table, ef_construction <= 128, LANTERN_GPU_LDS_LIST is off, the
 * batch does not take the lone-insertion walk (more than 2 x CUs rows), it is not the row-sharded build, and the walk has two waves or
 * more.  The initial mode is LANTERN_GPU_INSERT_SCREEN (0 | 1) where set, on otherwise. */
LANTERN_GPU_EXPORT void lantern_gpu_set_insert_screen(usearch_index_t, int mode, usearch_error_t *);
/* ... counted since init, after buffered adds are flushed: out[0] screened k_insert launches, out[1] unscreened k_insert launches (the
 * lone-insertion walk is neither), out[2] rows put to the screen test, out[3] rows it rejected (their f32 rows were not read). */
LANTERN_GPU_EXPORT void lantern_gpu_insert_screen_stats(usearch_index_t, uint64_t out[4], usearch_error_t *);
/* The shape of a batch's k_insert launch, host arithmetic only (no device, no index, no environment).
 * in[13]: [0] metric code (1 cos, 3 l2sq, 8 hamming, +100 f16 rows, +200 i8 rows)  [1] 16-byte chunks per row  [2] M0
 *   [3] ef_construction  [4] rows the launch walks  [5] CUs  [6] waves per workgroup  [7] the index has a screen table
 *   [8] mode (lantern_gpu_set_insert_screen)  [9] LANTERN_GPU_LDS_LIST != 0  [10] row-sharded build (upper levels only)
 *   [11] the lone-insertion walk may be taken (one index, LANTERN_GPU_INSERT_SPEC != 0)  [12] LANTERN_GPU_INSERT_VIS_SLOTS, or -1
 * out[7]: [0] screened  [1] vis_slots  [2] LDS bytes per workgroup  [3] of which the query's int8 planes (!= 0 iff screened; they come
 *   out of [1])  [4] the lone-insertion walk  [5] spec_prefetch  [6] spec_cache
 * Returns NULL, or the text the launch is refused with. */
LANTERN_GPU_EXPORT const char *lantern_gpu_plan_insert(const int64_t in[13], uint32_t out[7]);
/* Diagnostics (tests): what the device STORED as the int8 screen of slots [first, first + count), copied out behind the index stream
 * after buffered single adds are flushed.  rows[count][row_bytes] int8 (16 per screen chunk, zero padded); meta[count][2] f32: l2sq
 * (s, r), cosine (s / norm, rho); norms[count] f32: a cosine index's cached rooted norms, the ones the fill divided by (an l2sq index
 * writes nothing there).  Any output pointer may be NULL.  Returns row_bytes = ceil(chunks / 4) * 16, or 0 for an index without a
 * screen (see lantern_gpu_search_screen_stats), which is not an error: nothing is written then.  A range that does not lie within
 * the index's size is refused. */
LANTERN_GPU_EXPORT size_t lantern_gpu_export_screen(usearch_index_t, size_t first, size_t count, int8_t *rows, float *meta, float *norms,
                                                    usearch_error_t *);
/* Diagnostics (tests): the screened hop's own decision (walk.hpp hop_distances_screened, called as the walk calls it) for one query,
 * n <= 64 slots (repeats allowed) and the radius `radius`, by one workgroup of `workgroup` = 256 or 512 threads:
 * rejected[i] = 1 where the screen rejects slots[i], else 0.  An index without a screen is refused. */
LANTERN_GPU_EXPORT void lantern_gpu_screen_probe(usearch_index_t, const void *query, const uint32_t *slots, size_t n, float radius,
                                                 int workgroup, uint8_t *rejected, usearch_error_t *);
/* Dense na x nb distance matrix between two host matrices (f32 rows of `dims` scalars, or u32
 * words for hamming with dims = bits; under cos / l2sq also usearch_scalar_f16_k -- rows of `dims` IEEE halves -- and
 * usearch_scalar_i8_k -- rows of `dims` int8 --, i.e. the values an index of that storage holds).  `exact_order` != 0 uses the
 * per-pair reduction order of the graph walk (bit-identical to usearch_distance); 0 uses the MFMA contraction of the operand
 * type: fp32 for f32 rows, f16 / i8 for rows of those kinds (i8: the same bits as exact_order != 0). */
LANTERN_GPU_EXPORT void lantern_gpu_distance_matrix(const void *a, size_t na, const void *b, size_t nb,
                                                    usearch_scalar_kind_t, size_t dims, usearch_metric_kind_t,
                                                    int exact_order, float *out, usearch_error_t *);

/* PQ k-means assignment, product_quantization.c:80-124 (assign_to_clusters): for every row i of `dataset`
 * (n rows of row_dims f32) the nearest of k centroids under `metric` over the subvector
 * [subvector_start, subvector_start + subvector_dim); the first minimum wins, as in the reference's
 * strict-< loop.  centers: k x subvector_dim f32.  out_distance may be NULL.  cos / l2sq only.
 * Guarantee: the smallest centroid by (exact-order distance, index), identical to that loop over usearch_distance -- the
 * exact k-NN with k = 1, certified or recomputed in exact order per row (lantern_gpu_exact_search). */
LANTERN_GPU_EXPORT void lantern_gpu_assign_to_clusters(const float *dataset, size_t n, size_t row_dims, size_t subvector_start,
                                                       size_t subvector_dim, const float *centers, size_t k,
                                                       usearch_metric_kind_t metric, uint32_t *out_cluster,
                                                       float *out_distance, usearch_error_t *);

/* flat graph exchange (tests, CPU-baseline timing on the identical graph, sharded serving) */
typedef struct lantern_gpu_graph_info
{
    size_t   size;
    size_t   upper_blocks; /* sum of node levels */
    uint32_t connectivity;
    uint32_t entry_slot;
    int32_t  max_level;
    uint32_t vector_words; /* 4-byte words per stored vector */
} lantern_gpu_graph_info;
LANTERN_GPU_EXPORT lantern_gpu_graph_info lantern_gpu_graph_info_get(usearch_index_t, usearch_error_t *);
/* any output pointer may be NULL.  levels[size] u8; nbr0[size][2M] u32 (0xFFFFFFFF = empty);
 * upper_off[size] u32; upper_nbr[upper_blocks][M] u32; labels[size] u64; vectors[size][words] */
LANTERN_GPU_EXPORT void lantern_gpu_export_graph(usearch_index_t, uint8_t *levels, uint32_t *nbr0, uint32_t *upper_off,
                                                 uint32_t *upper_nbr, uint64_t *labels, void *vectors,
                                                 usearch_error_t *);
/* pq indexes: the code bytes, codes[size][num_subvectors] (export_graph's `vectors` are the decoded f32 rows) */
LANTERN_GPU_EXPORT void lantern_gpu_export_codes(usearch_index_t, uint8_t *codes, usearch_error_t *);
/* pq = true indexes, COMPACT form.  A node of a PQ index carries num_subvectors code bytes (usearch_storage.cpp:29-31); the
 * device keeps every row's DECODING next to the codes because adding evaluates stored row against stored row.  A read-mostly
 * index -- the scan-side mirror of a built index (scan.c:75-110) -- gives the decodings up: lantern_gpu_pq_compact frees them
 * (10M x 768 at 96 subvectors: 0.96 GB of rows instead of 30.7 GB) and every search from then on evaluates rows by asymmetric
 * distance computation over the code bytes: a per-query table of partial sums (subvector x centroid) in LDS, num_subvectors
 * table entries added per row (lantern_amd/csrc/search_adc_kernel.hip; summation order defined there and restated by the
 * oracle -- distances agree with the decoded-row path to 1e-5 relative, not bit for bit: PARITY UNPINNED BY THE REFERENCE).
 * Anything that needs rows again (usearch_add, the exact search, an export with vectors) decodes them back first, as does
 * lantern_gpu_pq_expand.  LANTERN_GPU_PQ_COMPACT=1 compacts a pq index right after it is loaded or mirrored. */
LANTERN_GPU_EXPORT void lantern_gpu_pq_compact(usearch_index_t, usearch_error_t *);
LANTERN_GPU_EXPORT void lantern_gpu_pq_expand(usearch_index_t, usearch_error_t *);
/* HBM held by the index: the vector block (the code rows of a compact pq index) | adjacency, labels, levels, norms, codes */
/* bytes of one stored row in device memory = the row stride of `d_queries` in lantern_gpu_search_batch_device: the vector zero padded
 * to whole 16-byte chunks, and bit rows of 65 .. 127 bytes (768 bits: quant_bits = 1 at 768 dimensions, hamming over integer[24]) to 128 --
 * one cache line per row instead of a line and a piece of the next (usearch_storage.cpp:29-31 sizes the ON-TAPE vector; this is HBM only) */
LANTERN_GPU_EXPORT size_t lantern_gpu_row_bytes(usearch_index_t, usearch_error_t *);
LANTERN_GPU_EXPORT void lantern_gpu_memory_usage(usearch_index_t, size_t *row_bytes, size_t *other_bytes, usearch_error_t *);
LANTERN_GPU_EXPORT void lantern_gpu_import_graph(usearch_index_t, size_t size, const void *vectors,
                                                 const uint64_t *labels, const uint8_t *levels, const uint32_t *nbr0,
                                                 const uint32_t *upper_off, const uint32_t *upper_nbr,
                                                 uint32_t entry_slot, int32_t max_level, usearch_error_t *);
/* cumulative counters since init: distance evaluations and expanded nodes of searches, and the
 * same for the insert path */
typedef struct lantern_gpu_counters
{
    uint64_t search_dist_evals, search_expansions, search_queries;
    uint64_t add_dist_evals, add_expansions, add_vectors, add_batches;
    /* breakdown of add_dist_evals: walk / neighbour selection of the new node / reverse-link re-pruning.  The walk counts are
     * the reference algorithm's own (asserted equal to the oracle's).  The other two count what the DEVICE evaluates: a
     * candidate is tested against all kept rows at once (k_connect) and a full list's pair table is filled up front
     * (k_revlink_pairs), where sequential usearch stops at the first blocker -- they are >= the CPU path's counts and are the
     * right numerators for the device's rooflines, not for a CPU comparison. */
    uint64_t add_walk_evals, add_select_evals, add_revlink_evals, add_reprunes;
} lantern_gpu_counters;
LANTERN_GPU_EXPORT lantern_gpu_counters lantern_gpu_counters_get(usearch_index_t, usearch_error_t *);

/* Build profile: with profiling on, every insertion batch is bracketed by HIP events on the index stream (phase by phase);
 * the sums are milliseconds of device time per phase since init.  walk = k_insert (+ the batch layout), connect =
 * k_connect, group = the request grouping (+ exchange 1 of a sharded build), revlink = append + re-prune kernels,
 * exchange = exchange 2 of a sharded build (0 on one GPU). */
typedef struct lantern_gpu_build_profile
{
    double   walk_ms, connect_ms, group_ms, revlink_ms, exchange_ms;
    uint64_t batches;
} lantern_gpu_build_profile;
LANTERN_GPU_EXPORT void lantern_gpu_set_profiling(usearch_index_t, int on, usearch_error_t *);
LANTERN_GPU_EXPORT lantern_gpu_build_profile lantern_gpu_build_profile_get(usearch_index_t, usearch_error_t *);

/* Diagnostics of the walk kernel: while on, searches run an instrumented instantiation (f32 l2sq / cos rows of >= 128 or
 * 32..63 chunks only) whose thread 0 sums shader-clock cycles per phase of every hop.  out8 (may be NULL) receives and
 * clears the sums: visited filter + compaction | wait at the hop's first barrier | distances | merge | pop | arrival of the
 * neighbour list | upper-level descent | whole query.  When the walk splits a hop's bookkeeping over two waves (register
 * list, two or more waves per query: walk.hpp search_level_reg) thread 0 never merges: slot 3 ("merge") is then its pop
 * DECISION and slot 4 ("pop") the list wave's whole section (merge + pop + hand-off), which runs beside slots 3, 5 and 0. */
LANTERN_GPU_EXPORT void lantern_gpu_search_phase_profile(usearch_index_t, int on, unsigned long long *out8, usearch_error_t *);
/* Diagnostics: how many DISTINCT rows the searches between (on = 1) and the read (on = 0, rows != NULL) evaluated, over all their
 * queries: unique rows x row bytes is the cold-miss lower bound of a launch's DRAM traffic (every such row has to come from
 * HBM at least once), to put beside the algorithmic bytes (one row per evaluation) and the counters' fabric-side bytes.  Runs
 * the instrumented instantiation of the walk kernel (f32 l2sq / cos; same walk, same D and E; slower). */
LANTERN_GPU_EXPORT void lantern_gpu_search_unique_rows(usearch_index_t, int on, uint64_t *rows, usearch_error_t *);
/* the same for the latency-bound walk (lantern_amd/csrc/walk_spec.hpp): out32[8 * wave + i], waves 0..3 = visit | list | cache
 * fill | a row wave; i = 0 decision, 1 neighbour list, 2 issuing the row loads, 3 the wave's role section, 4 loads landing +
 * distances, 5 wait at the hop's barrier, 6 hops, 7 where lists came from (wave 0: staging area, wave 3: cache, wave 2: HBM) */
LANTERN_GPU_EXPORT void lantern_gpu_spec_profile(usearch_index_t, int on, unsigned long long *out32, usearch_error_t *);

/* order-independent-of-builder fingerprint of the graph (levels, labels, both adjacency arrays, entry point):
 * equal on two indexes iff they hold the same graph; used to check that replicas agree without moving them */
LANTERN_GPU_EXPORT uint64_t lantern_gpu_graph_checksum(usearch_index_t, usearch_error_t *);

/* ------------------------------------------------------------------------------------------ */
/* Deleting rows: tombstones, then unlinking them from the graph.              */
/* PARITY UNPINNED BY THE REFERENCE: its VACUUM resets the labels of the dead rows to 0         */
/* (delete.c:15-72, INVALID_ELEMENT_LABEL: hnsw.h:40), warns "deletes are currently not         */
/* implemented ... No memory will be reclaimed" (delete.c:24-25) and leaves the graph as it is;  */
/* scans drop label 0 after the search returned it (scan.c:296-300; hnsw_delete.out:28-55).      */
/* Beyond the label reset what follows is a definition of this library.                          */
/* ------------------------------------------------------------------------------------------ */
/* ldb_ambulkdelete for the resident copy.  After the flush every search performs, every slot whose label is in labels[0..n) gets
 * label 0.  The list may be in any order and may hold duplicates, labels no slot carries and 0: none of those counts.  *removed
 * (may be NULL) = the slots that changed from non-zero to zero; n == 0 is a no-op.  The list is sorted on the device and searched
 * once per slot.  The call is ordered against launches in flight as an insertion batch is: it waits for the searches in flight, and
 * searches on other streams wait for it.  Every index kind and form is served (f32, f16, i8, b1, pq expanded and compact,
 * page-attached mirrors): ONLY labels change -- graph, rows, screen rows and the size stay, so a tombstoned row is still evaluated,
 * expanded and returned (with label 0) until lantern_gpu_unlink_deleted.  Export, usearch_save* and lantern_gpu_save_stream write
 * label 0 and a load brings it back.  A filter built with LANTERN_GPU_FILTER_SKIP_DELETED is a snapshot of the labels at its build. */
LANTERN_GPU_EXPORT void lantern_gpu_remove_labels(usearch_index_t, const usearch_label_t *labels, size_t n, uint64_t *removed,
                                                  usearch_error_t *);
/* the slots whose label is 0, however they got it (this call, a file, a page, an import) */
LANTERN_GPU_EXPORT size_t lantern_gpu_deleted_count(usearch_index_t, usearch_error_t *);
/* lantern_gpu_unlink_deleted.  Notation: G the graph after the flush; T the slots with label 0; cap(l) = 2M at level 0 and M above;
 * cut(l) = max(256, 8 cap(l)).
 *  - If T is empty, or no live slot remains, nothing changes and every stat is 0.
 *  - Otherwise, for every live node p and every level l <= level(p), with L = p's list at l in stored order:
 *      if L has no entry in T it stays byte for byte; else
 *      keep   = the live entries of L in stored order;
 *      offers = walking L in stored order, every entry t in T contributes the live entries of G's list of t at level l, in stored
 *               order, skipping p, anything in keep and anything offered before; the walk stops when offers holds cut(l) slots;
 *      the new list starts as keep, compacted with no holes; every offer c, in that order, is then applied as ONE reverse-link
 *      request (close p, level l, new_slot c, d = metric(c, p)) exactly as an insertion's reverse link is (usearch
 *      reconnect_neighbor_nodes_): appended while the list has room, otherwise the cap(l) + 1 candidates are re-pruned by the
 *      neighbour-selection heuristic in (distance, per-centre tie order) order.
 *  - All reads are from G: the result does not depend on the order in which lists are processed.
 *  - Afterwards every list of every t in T is empty at every level.
 *  - If the entry node is in T, the new entry is the live node of the highest level, the lowest slot among those, and max_level
 *    becomes that level.
 *  - Rows, labels, levels, the size, slots, upper blocks, the screen copy and norms do not move: filters, cursors' `seen` sets and
 *    page maps stay valid.  The unlink itself reclaims no memory: lantern_gpu_compact_deleted (below) does.  A second call changes
 *    nothing and reports zeros.
 *  - It does not equal a rebuild of the live rows (DESIGN.md 4.11 says by how much).
 * The call is a graph mutation, ordered as an insertion batch.  The result is a pure function of the graph: the replicas of a
 * sharded build each call it and stay identical.  Refused: a page-attached index (its lists would have to go back through
 * retriever_mut) and a compact pq index (expand it first). */
typedef struct lantern_gpu_unlink_stats
{
    uint64_t tombstones_unlinked; /* slots of T that still had a neighbour of their own */
    uint64_t lists_repaired;      /* (p, l) lists that held an entry of T */
    uint64_t offers;              /* reverse-link requests made */
    uint64_t lists_cut;           /* lists whose offers reached cut(l) */
    uint64_t request_evals;       /* pair evaluations of the request kernel (one per offer) */
    uint64_t reprune_evals;       /* pair evaluations of the re-prunes, as the DEVICE counts them (lantern_gpu_counters: >= the sequential count) */
    uint64_t entry_moved;         /* 1 if the entry node was in T */
} lantern_gpu_unlink_stats;
LANTERN_GPU_EXPORT void lantern_gpu_unlink_deleted(usearch_index_t, lantern_gpu_unlink_stats *out /* or NULL */, usearch_error_t *);
/* lantern_gpu_compact_deleted: reclaims the tombstones' slots.  Notation as above; n the size after the flush.
 *  - After the flush the call does exactly what lantern_gpu_unlink_deleted does (its stats: `unlink`).  Then, with T the slots of
 *    label 0 and live = n - |T|: map[s] = the number of live slots below s for a live s, map[s] = 0xFFFFFFFF for s in T.  The
 *    renumbering is STABLE: live slots keep their relative order.
 *  - If T is empty nothing changes, every stat is 0, `capacity` is ignored and the epoch (below) does not move; slot_map receives
 *    the identity.
 *  - Otherwise, for every live s, slot map[s] of the new index carries what slot s carried: row, label, level, cached norm, the code
 *    bytes of an expanded pq index, the int8 screen row and its (s, r) metadata, all bit for bit.  Every list of s at every level
 *    keeps its stored order with every entry e replaced by map[e]; the 0xFFFFFFFF padding stays padding.  upper_off becomes the
 *    exclusive prefix sum of `level` over the new slots (a node of level 0 carries the running sum, which nothing dereferences;
 *    an insertion writes 0xFFFFFFFF there) and the upper blocks are copied from wherever they were.  entry = map[entry], max_level
 *    is unchanged, the size is live.
 *  - live == 0 (everything deleted: the case the unlink skips) leaves an empty index: size 0, no entry, max_level -1.
 *  - usearch_capacity becomes max(live, capacity).  The old arrays are FREED: lantern_gpu_memory_usage falls to what the new capacity
 *    costs (the upper blocks to exactly the live ones).  The arrays sized by capacity that are allocated on first use (visited bitmaps
 *    of every launch slot, the diagnostics bitmap of lantern_gpu_search_unique_rows) are dropped; the re-prune state is not moved but
 *    reset before its next use.
 *  - ALL OR NOTHING: the new arrays are built in fresh allocations beside the old ones and swapped in after the last kernel has
 *    succeeded, so the transient peak is old + new (+ 20 bytes per old slot for the map).  If an allocation fails the error names the
 *    bytes needed; if an entry of a live list maps to 0xFFFFFFFF (impossible after an unlink; the list kernel counts them) the error
 *    says how many.  Either way the index stays exactly as the unlink left it.
 *  - slot_map (may be NULL) receives map[0..n).
 *  - SLOTS CHANGE MEANING, so the index counts its compactions that moved something (the epoch).  A filter remembers the epoch of its
 *    build and is refused in another ("the index was compacted since the filter was built"), whatever the size has become since.  A
 *    cursor (lantern_gpu_cursor_*, lantern_scan) whose `seen` set is not empty and comes from another epoch is refused on a
 *    streaming continuation ("the index was compacted: rescan"); a non-streaming search starts it afresh.  usearch_search_ef's own
 *    continuation state is renumbered through map and goes on.  A scan-service connection remembers labels, not slots: it goes on too.
 *  - NOT A REBUILD: the result is the unlinked graph renumbered and nothing more; every search answers with the same labels, distance
 *    bits and counters as before the call (candidates are ordered by (distance, slot) and the order of the live slots is kept).
 *    Re-prunes and insertions that follow break exact distance ties by tie_mix(slot, centre) over the NEW slots, so from then on the
 *    graph may differ, among exactly tied candidates only, from what the uncompacted index would have grown into.
 * The call is a graph mutation, ordered as an insertion batch, and a pure function of the graph: the replicas of a sharded build each
 * call it and stay identical.  Refused: a page-attached index and a compact pq index (expand it first). */
typedef struct lantern_gpu_compact_stats
{
    lantern_gpu_unlink_stats unlink;   /* the unlink the call performs first (all zero if there was nothing to unlink) */
    uint64_t rows_before, rows_after;                 /* usearch_size before / after */
    uint64_t upper_blocks_before, upper_blocks_after;
    uint64_t bytes_before, bytes_after;               /* lantern_gpu_memory_usage row_bytes + other_bytes */
    uint64_t bytes_moved;                             /* bytes the compaction kernels wrote */
} lantern_gpu_compact_stats;
LANTERN_GPU_EXPORT void lantern_gpu_compact_deleted(usearch_index_t, size_t capacity, uint32_t *slot_map /* [rows_before] or NULL */,
                                                    lantern_gpu_compact_stats *out /* or NULL */, usearch_error_t *);
/* diagnostics: HIP-event times, in ms, of the last call that moved rows: out[0] all its kernels (map, rows, screen, codes, lists, metadata),
 * out[1] the row kernel over the vector block alone (what scripts/bench_compact.py holds against a device-to-device copy) */
LANTERN_GPU_EXPORT void lantern_gpu_last_compact_ms(usearch_index_t, float *out /* [2] */, usearch_error_t *);
/* the same arithmetic without a device (pure: no HIP call, no index): map as above, upper_off_new[j] = the levels of the live slots
 * below new slot j, *live and *upper_blocks their totals.  Every output may be NULL. */
LANTERN_GPU_EXPORT void lantern_gpu_plan_compact(const uint64_t *labels, const uint8_t *levels, size_t n, uint32_t *slot_map /* [n] */,
                                                 uint32_t *upper_off_new /* [live] */, uint64_t *live, uint64_t *upper_blocks, usearch_error_t *);

/* ------------------------------------------------------------------------------------------ */
/* Work-sharded index build over the GPUs of one node (the reference's     */
/* own parallel build is a thread pool on one shared index, server.rs:328-359).  One process or  */
/* thread per GPU, each with its own usearch_index_t replica.  lantern_gpu_add_sharded is a       */
/* COLLECTIVE: rank r passes shard r of the rows (global slot order = rank order); the shards are */
/* all-gathered into every replica's HBM, then every insertion batch is split across the ranks:   */
/* each walks and connects its share of the new nodes, the ranks all-gather the resulting top-M   */
/* neighbour lists, each applies the reverse links of the nodes it owns and the re-written        */
/* adjacency rows are all-gathered.  All replicas end up bit-identical to the graph one GPU       */
/* builds from the same rows with the same batch parameters.                                      */
/* ------------------------------------------------------------------------------------------ */
typedef struct lantern_gpu_comm lantern_gpu_comm_t;
#define LANTERN_GPU_COMM_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */
/* RCCL transport (xGMI, data stays in HBM): rank 0 draws the id and ships it to its peers by any means,
 * then every rank calls init_rccl with the HIP device it will build on current (hipSetDevice). */
LANTERN_GPU_EXPORT void lantern_gpu_comm_unique_id(char *id128, usearch_error_t *);
LANTERN_GPU_EXPORT lantern_gpu_comm_t *lantern_gpu_comm_init_rccl(int rank, int world, const char *id128, usearch_error_t *);
/* Host transport: the caller supplies an in-place all-gather over a HOST buffer (MPI, gloo, sockets):
 * on entry bytes [offsets[rank], +counts[rank]) are valid, on return (0 = success) every rank's segment is. */
typedef int (*lantern_gpu_allgatherv_fn)(void *ctx, void *host_buf, const size_t *offsets, const size_t *counts, int world,
                                         int rank);
LANTERN_GPU_EXPORT lantern_gpu_comm_t *lantern_gpu_comm_init_host(int rank, int world, lantern_gpu_allgatherv_fn, void *ctx,
                                                                  usearch_error_t *);
/* In-process world: `world` communicators for `world` threads of this process (one thread per GPU of a node,
 * or several ranks on one GPU in tests); out[world]. */
LANTERN_GPU_EXPORT void lantern_gpu_comm_init_local(int world, lantern_gpu_comm_t **out, usearch_error_t *);
LANTERN_GPU_EXPORT void lantern_gpu_comm_free(lantern_gpu_comm_t *);
LANTERN_GPU_EXPORT int  lantern_gpu_comm_rank(lantern_gpu_comm_t *);
LANTERN_GPU_EXPORT int  lantern_gpu_comm_world(lantern_gpu_comm_t *);
/* a collective that does not complete within `seconds` (default 180) fails instead of hanging */
LANTERN_GPU_EXPORT void lantern_gpu_comm_set_timeout(lantern_gpu_comm_t *, double seconds);
/* bytes this rank received and number of exchanges so far */
LANTERN_GPU_EXPORT void lantern_gpu_comm_stats(lantern_gpu_comm_t *, uint64_t *bytes_received, uint64_t *collectives);
/* the exchange primitive itself (in-place all-gather with per-rank sizes), host and device buffers */
LANTERN_GPU_EXPORT void lantern_gpu_comm_allgatherv_host(lantern_gpu_comm_t *, void *host_buf, const size_t *offsets,
                                                         const size_t *counts, usearch_error_t *);
LANTERN_GPU_EXPORT void lantern_gpu_comm_allgatherv_device(lantern_gpu_comm_t *, void *device_buf, const size_t *offsets,
                                                           const size_t *counts, void *stream, usearch_error_t *);
/* the balanced split used for batches and shards: rank r of `world` takes [n*r/world, n*(r+1)/world) */
LANTERN_GPU_EXPORT void lantern_gpu_shard_range(size_t n, int world, int rank, size_t *begin, size_t *end);
/* the collective insert described above; n_shard may be 0 */
LANTERN_GPU_EXPORT void lantern_gpu_add_sharded(usearch_index_t, lantern_gpu_comm_t *, const usearch_label_t *labels_shard,
                                                const void *vectors_shard, size_t n_shard, usearch_scalar_kind_t,
                                                usearch_error_t *);

/* Row-SHARDED build (SURVEY.md section 8e as written: "vectors sharded by row; each GPU generates candidates within its shard
 * for a tile of the rows; all-gather of the candidate lists; merge"): a COLLECTIVE on an EMPTY index (f32 / f16 / i8 / b1 rows,
 * not pq).  Rank r passes shard r of the rows.  Every rank keeps a graph over ITS rows only, grown in lock step with the global
 * one.  A batch of the global build (the usual plan, its members drawn from all shards in proportion): every rank inserts its
 * share into its own graph; the batch's rows are all-gathered (the only time a row crosses the fabric); every rank searches its
 * own graph for each row of the batch (k_search; K = max(2M + 1, 2 expansion_add / world) answers), the per-rank lists are
 * all-gathered in HBM (12 bytes per candidate) and merged on the device by (distance, slot) into the input of the neighbour
 * selection; selection and reverse links then run on every rank as in a one-GPU batch (the upper levels, ~1 / M of the rows, are
 * walked in the global graph as usual).  Every rank ends with the same graph and the same rows (lantern_gpu_graph_checksum).
 * The slots follow the batches, not the ranks: labels identify rows.  The graph is NOT the one usearch_add builds edge for edge
 * (a row's candidates are the union of `world` approximate searches instead of one): it equals, edge for edge, the CPU
 * restatement of THIS collective (oracle.row_sharded_build; tests/test_gpu_sharded_build.py), and is compared with the
 * one-GPU build by recall (profiles/r04_row_sharded_build.md: on par or better), where lantern_gpu_add_sharded above equals
 * the one-GPU build itself.  Cost: every rank searches ALL rows and links ALL rows; only the shard-graph insertions fall with
 * the world size (measured bound: 1.3x at 4-8 ranks) -- lantern_gpu_add_sharded is the build that scales.
 * LANTERN_GPU_ROW_SHARD_K / LANTERN_GPU_ROW_SHARD_EF override the candidates per shard / the expansion they are found with. */
LANTERN_GPU_EXPORT void lantern_gpu_add_row_sharded(usearch_index_t, lantern_gpu_comm_t *, const usearch_label_t *labels_shard,
                                                    const void *vectors_shard, size_t n_shard, usearch_scalar_kind_t,
                                                    usearch_error_t *);
/* the batches lantern_gpu_add_row_sharded runs for these shard sizes and where their rows come from (host arithmetic only, no
 * device): first[t] / count[t] = the batch's slots, share[t * world + r] = how many of its rows are shard r's (rank 0's take the
 * first slots of the batch).  Returns the number of batches; at most `capacity` are written. */
LANTERN_GPU_EXPORT size_t lantern_gpu_row_shard_plan(const uint64_t *shard_sizes, int world, uint64_t seed, uint32_t connectivity,
                                                     size_t max_batch, size_t min_ratio, size_t *first, size_t *count, size_t *share,
                                                     size_t capacity);

/* Row-PARTITIONED search (SURVEY.md section 8e as written: "vectors sharded by row; each GPU produces its best candidates
 * within its shard; all-gather; merge"), for indexes whose vectors do not fit one GPU's HBM: a COLLECTIVE over `comm`.  Every
 * rank holds its OWN index over a disjoint share of the rows -- built independently with usearch_add / lantern_gpu_add_many, no
 * exchange at build time, vector memory scales with the number of GPUs -- and passes the SAME queries.  Each searches its
 * share (usearch_search_ef semantics, ef per share), the per-rank top-k (label, distance) lists are all-gathered in place in
 * HBM (RCCL: xGMI; nq x k x 12 bytes per rank) and merged on the device by (distance, label).  Every rank returns the same
 * global top-k.  Labels must be unique across the shares.  (The work-sharded build above keeps ONE graph, bit-identical to
 * the single-GPU build, but needs every row in every GPU's HBM; this form trades that identity for capacity.) */
LANTERN_GPU_EXPORT void lantern_gpu_search_partitioned(usearch_index_t, lantern_gpu_comm_t *, const void *queries, size_t nq,
                                                       usearch_scalar_kind_t, size_t k, size_t ef, usearch_label_t *labels,
                                                       float *distances, uint32_t *counts, usearch_error_t *);

/* ------------------------------------------------------------------------------------------ */
/* amgettuple paging shim: ldb_ambeginscan / ldb_amgettuple / ldb_amendscan (scan.c:24-338)     */
/* ------------------------------------------------------------------------------------------ */
typedef struct lantern_scan lantern_scan_t;
/* init_k = GUC lantern_hnsw.init_k (options.h:44, default 10); ef = GUC lantern_hnsw.ef or 0 */
LANTERN_GPU_EXPORT lantern_scan_t *lantern_scan_begin(usearch_index_t, int init_k, int ef, usearch_error_t *);
/* the same scan driven through a scan-service connection (declared below) instead of a local index: what a PostgreSQL
 * backend runs when the mirror lives in the service process.  query_bytes = the size of one query vector. */
struct lantern_scan_client;
LANTERN_GPU_EXPORT lantern_scan_t *lantern_scan_begin_client(struct lantern_scan_client *, size_t query_bytes, int init_k, int ef,
                                                             usearch_error_t *);
/* ldb_amrescan: (re)arm the scan with an ORDER BY key; the vector is copied */
LANTERN_GPU_EXPORT void lantern_scan_rescan(lantern_scan_t *, const void *query, usearch_scalar_kind_t,
                                            usearch_error_t *);
/* ldb_amgettuple: true and *label set while tuples remain.  Skips label 0 (deleted, scan.c:296-300),
 * doubles k through the streaming continuation (scan.c:240-292), stops at 1000 rows (:249-252). */
LANTERN_GPU_EXPORT bool lantern_scan_gettuple(lantern_scan_t *, usearch_label_t *label, usearch_error_t *);
/* The k of every usearch_search_ef the scan has issued since its last rescan, in order -- the sequence the reference logs as
 * "LANTERN querying index for %d elements" (scan.c:219, :272; pinned by test/expected/hnsw_select.out:76-140: 10 | 4, 8, 8).
 * Writes min(n, cap) values to ks (may be NULL), returns n. */
LANTERN_GPU_EXPORT size_t lantern_scan_trace(lantern_scan_t *, int *ks, size_t cap);
LANTERN_GPU_EXPORT void lantern_scan_end(lantern_scan_t *);
/* Later rescans and gettuples of this scan go through the filter (lantern_gpu_cursor_search_filtered): every row it returns is
 * allowed, and the 1000-row cap counts allowed rows.  NULL clears it.  The filter must outlive the scan's use of it.
 * Refused on a scan of lantern_scan_begin_client: a filter handle is local to a process.  Such a scan inherits the filter of its
 * CONNECTION (lantern_scan_client_set_filter), with the same two properties. */
LANTERN_GPU_EXPORT void lantern_scan_set_filter(lantern_scan_t *, const struct lantern_gpu_filter *, usearch_error_t *);

/* ------------------------------------------------------------------------------------------ */
/* Lifecycle of the HBM mirrors of page-resident indexes.  The reference      */
/* attaches anew per scan and per insert (scan.c:99-110, insert.c:142-151: free for a lazy view);  */
/* a device mirror is a walk of the graph through the retriever, so a process keeps its mirrors in  */
/* this cache, keyed by (relation = relfilenode, version = LSN of the header page or num_vectors).   */
/* ------------------------------------------------------------------------------------------ */
typedef struct lantern_mirror lantern_mirror_t;
/* The resident mirror of (relation, version), or a fresh one: usearch_init(opts, pq_codebook) + usearch_view_mem_lazy(header).
 * A newer version replaces the relation's mirror (the stale one is freed when its last holder releases it).  Returns NULL
 * with *err == NULL when the header declares fewer than min_vectors nodes: the caller stays on the path it has. */
LANTERN_GPU_EXPORT lantern_mirror_t *lantern_mirror_acquire(uint64_t relation, uint64_t version, usearch_init_options_t *opts,
                                                            float *pq_codebook, char *header136, size_t min_vectors, usearch_error_t *);
LANTERN_GPU_EXPORT usearch_index_t lantern_mirror_index(lantern_mirror_t *);
LANTERN_GPU_EXPORT uint64_t        lantern_mirror_version(lantern_mirror_t *);
/* The mirror's retriever callbacks (init_options.retriever / retriever_mut / retriever_ctx -- the reference's per-scan,
 * per-insert RetrieverCtx: scan.c:34,132, insert.c:130,247) are kept PER HOLDER, a holder being a host thread (a PostgreSQL
 * backend is one; a threaded service runs one holder per thread): bound by that thread's acquire or rebind, dropped by that
 * thread's release -- no ctx pointer outlives the acquire / release pair that brought it, and one holder's release never takes
 * away another's.  usearch_add_external uses the calling thread's and fails with a message when it has none (a thread that
 * holds several handles of one mirror and released one of them binds its own again first). */
LANTERN_GPU_EXPORT void lantern_mirror_rebind(lantern_mirror_t *, const usearch_init_options_t *opts);
/* the holder applied a change itself (usearch_add_external + usearch_update_header): re-stamp instead of rebuilding */
LANTERN_GPU_EXPORT void lantern_mirror_advance(lantern_mirror_t *, uint64_t new_version);
LANTERN_GPU_EXPORT void lantern_mirror_release(lantern_mirror_t *);
/* DROP INDEX / REINDEX / VACUUM */
LANTERN_GPU_EXPORT void lantern_mirror_invalidate(uint64_t relation);
/* idle mirrors kept resident (default 8; least recently used goes first) */
LANTERN_GPU_EXPORT void lantern_mirror_set_capacity(size_t max_resident);
LANTERN_GPU_EXPORT void lantern_mirror_stats(uint64_t *hits, uint64_t *misses, uint64_t *rebuilds, uint64_t *resident);

/* ------------------------------------------------------------------------------------------ */
/* External indexing server (boundary B3): drop-in for `lantern-cli start-indexing-server`        */
/* (lantern_cli/src/external_index/server.rs:176-435,526-584); PostgreSQL side untouched           */
/* (lantern_hnsw/src/hnsw/external_index_socket.c:322-536).                                        */
/* ------------------------------------------------------------------------------------------ */
typedef struct lantern_index_server lantern_index_server_t;
/* Bind host:port (port 0 = ephemeral; default of the reference is 0.0.0.0:8998, cli.rs:126-151), start the
 * accept thread.  status_port: HTTP status endpoint {"status":0..3} (server.rs:586-597), -1 = none.
 * One connection is served at a time, as in the reference. */
LANTERN_GPU_EXPORT lantern_index_server_t *lantern_index_server_start(const char *host, int port, int status_port,
                                                                      const char *tmp_dir, usearch_error_t *);
/* The same over TLS (`start-indexing-server --cert C --key K`: cli.rs:146, server.rs:437-470,548): PEM files; every accepted
 * connection starts with the handshake (the PostgreSQL side: external_index_socket_ssl.c:6-62, TLS >= 1.2, no certificate
 * verification).  libssl is bound at run time; NULL, NULL = the plain server.  The router redirect of
 * external_index_socket.c:411-447 is the ROUTER's half of the protocol (server type 0x2), not this server's. */
LANTERN_GPU_EXPORT lantern_index_server_t *lantern_index_server_start_tls(const char *host, int port, int status_port, const char *tmp_dir,
                                                                          const char *cert_pem, const char *key_pem, usearch_error_t *);
LANTERN_GPU_EXPORT int      lantern_index_server_port(lantern_index_server_t *);
LANTERN_GPU_EXPORT int      lantern_index_server_status_port(lantern_index_server_t *);
/* 0 idle, 1 in progress, 2 failed, 3 succeeded (server.rs:44-49) */
LANTERN_GPU_EXPORT int      lantern_index_server_status(lantern_index_server_t *);
LANTERN_GPU_EXPORT uint64_t lantern_index_server_served(lantern_index_server_t *);
LANTERN_GPU_EXPORT void     lantern_index_server_stop(lantern_index_server_t *);

/* ------------------------------------------------------------------------------------------ */
/* Scan-side service: ONE HBM-resident index serves the k-NN queries of    */
/* many PostgreSQL backends, coalesced into batched launches.  A backend's ldb_amgettuple          */
/* (scan.c:167-338) calls lantern_scan_client_search where it calls usearch_search_ef today; the   */
/* server waits at most `max_wait_us` after the first queued query for company (at most            */
/* `max_batch` queries per launch; less if every connected backend is already accounted for or    */
/* a dispatcher's share of them is), searches them and routes the answers back: one call per    */
/* distinct (k, ef) of the batch.  LANTERN_SCAN_MIXED=1, on a device index: the unfiltered        */
/* requests of a batch go out in ONE per-query-parameter call whatever their (k, ef)              */
/* (lantern_gpu_search_batch_params_lane_notify: at most three launches), or -- when they all      */
/* share one (k, ef) -- in the uniform call.  (Off by default until its A/B is on record:         */
/* DESIGN.md 4.10.)  No thread per connection: a few epoll I/O threads                    */
/* (LANTERN_SCAN_IO_THREADS) carry all sockets.  Wire format: lantern_amd/csrc/scan_server.cpp.    */
/* ------------------------------------------------------------------------------------------ */
typedef struct lantern_scan_server lantern_scan_server_t;
typedef struct lantern_scan_client lantern_scan_client_t;
/* the batch search a server runs: nq queries of vec_bytes each -> labels/dists [nq][k], counts [nq]; 0 = ok,
 * otherwise *err points at a message that outlives the call */
typedef int (*lantern_batch_search_fn)(void *ctx, const void *queries, size_t nq, size_t vec_bytes, size_t k, size_t ef,
                                       uint64_t *labels, float *distances, uint32_t *counts, const char **err);
/* serve `index` (built, loaded or mirrored; it must outlive the server) on host:port (port 0 = ephemeral).  Two dispatcher
 * threads take turns -- one forms the next batch while the other's is being searched, each on its own lane of the index
 * (lantern_gpu_search_batch_lane) -- so consecutive launches overlap on the device.  A caller-supplied back end
 * (lantern_scan_server_start_fn) is entered by one thread only, unless LANTERN_SCAN_LANES=2 says it may be entered by two. */
LANTERN_GPU_EXPORT lantern_scan_server_t *lantern_scan_server_start(usearch_index_t index, const char *host, int port,
                                                                    size_t max_batch, unsigned max_wait_us, usearch_error_t *);
/* the same front end over any batch search function (tests; a host that shards queries over several GPUs) */
LANTERN_GPU_EXPORT lantern_scan_server_t *lantern_scan_server_start_fn(lantern_batch_search_fn, void *ctx, size_t vec_bytes,
                                                                       const char *host, int port, size_t max_batch,
                                                                       unsigned max_wait_us, usearch_error_t *);
/* FILTERS THROUGH THE SERVICE.  A connection may carry a filter (lantern_scan_client_set_filter: a list of labels, built on the
 * device by lantern_gpu_filter_from_labels and owned by the server); every later search of that connection goes through it.  Within a
 * batch's (k, ef) group the unfiltered requests take the path above; the filtered ones -- of whatever connections, with whatever
 * filters -- go out together in ONE lantern_gpu_search_batch_filtered_each_lane call.  Limits, errors and the wire message:
 * lantern_amd/csrc/scan_server.cpp.  LANTERN_SCAN_FILTER_BYTES: device memory the resident filters may take (default 1 GiB).
 * A back end of lantern_scan_server_start_fn has no filters (a filter message gets an error frame); the form below brings its own:
 * make -> an opaque filter (NULL and *err on failure) with its allowed rows and resident bytes; free; and the batch search with a
 * filter per query (never NULL entries: unfiltered requests go to the plain function). */
typedef void *(*lantern_scan_filter_make_fn)(void *ctx, const uint64_t *labels, size_t n, uint32_t flags, uint64_t *allowed,
                                             uint64_t *resident_bytes, const char **err);
typedef void (*lantern_scan_filter_free_fn)(void *ctx, void *filter);
typedef int (*lantern_batch_search_each_fn)(void *ctx, const void *const *filters, const void *queries, size_t nq, size_t vec_bytes, size_t k,
                                            size_t ef, uint64_t *labels, float *distances, uint32_t *counts, const char **err);
LANTERN_GPU_EXPORT lantern_scan_server_t *lantern_scan_server_start_filtered_fn(lantern_batch_search_fn, lantern_scan_filter_make_fn,
                                                                                lantern_scan_filter_free_fn, lantern_batch_search_each_fn,
                                                                                void *ctx, size_t vec_bytes, const char *host, int port,
                                                                                size_t max_batch, unsigned max_wait_us, usearch_error_t *);
/* filters set (clears not counted; an extension -- lantern_scan_client_extend_filter -- is not counted either: it rebuilds a filter
 * that was counted when it was set, and shows in resident_bytes only), requests searched through a filter, per-query-filter calls
 * made, the largest number of DISTINCT filters one such call carried, device bytes of the filters resident now */
/* MIXED BATCHES THROUGH AN INJECTED BACK END (tests of the dispatcher; a host that shards queries over several GPUs): the batch
 * search with (k, ef, skip) per query -- answer rows k_stride wide, as lantern_gpu_search_batch_params.  The unfiltered requests of a
 * batch that carry more than one distinct (k, ef) go to it in one call; a batch with one shared (k, ef) goes to the plain function. */
typedef int (*lantern_batch_search_params_fn)(void *ctx, const void *queries, size_t nq, size_t vec_bytes, const lantern_gpu_query_params *params,
                                              size_t k_stride, uint64_t *labels, float *distances, uint32_t *counts, const char **err);
LANTERN_GPU_EXPORT lantern_scan_server_t *lantern_scan_server_start_params_fn(lantern_batch_search_fn, lantern_batch_search_params_fn, void *ctx,
                                                                              size_t vec_bytes, const char *host, int port, size_t max_batch,
                                                                              unsigned max_wait_us, usearch_error_t *);
/* ... and for the FILTERED requests: the batch search with a filter and (k, ef, skip) per query, answer rows k_stride wide, as
 * lantern_gpu_search_batch_filtered_each_params.  The filtered requests of a batch that carry more than one distinct (k, ef) go to it
 * in ONE call; with one shared (k, ef) they take the each-function; a back end started without it keeps them grouped by (k, ef).  A call
 * it refuses is repeated one request at a time, so that only the offender sees the error.  The device index has it under
 * LANTERN_SCAN_MIXED=1 (off by default). */
typedef int (*lantern_batch_search_each_params_fn)(void *ctx, const void *const *filters, const void *queries, size_t nq, size_t vec_bytes,
                                                   const lantern_gpu_query_params *params, size_t k_stride, uint64_t *labels, float *distances,
                                                   uint32_t *counts, const char **err);
LANTERN_GPU_EXPORT lantern_scan_server_t *lantern_scan_server_start_filtered_params_fn(lantern_batch_search_fn, lantern_scan_filter_make_fn,
                                                                                       lantern_scan_filter_free_fn, lantern_batch_search_each_fn,
                                                                                       lantern_batch_search_each_params_fn, void *ctx, size_t vec_bytes,
                                                                                       const char *host, int port, size_t max_batch,
                                                                                       unsigned max_wait_us, usearch_error_t *);
LANTERN_GPU_EXPORT void lantern_scan_server_filter_stats(lantern_scan_server_t *, uint64_t *filters_set, uint64_t *filtered_requests,
                                                         uint64_t *each_calls, uint64_t *most_distinct_filters, uint64_t *resident_bytes);
LANTERN_GPU_EXPORT int  lantern_scan_server_port(lantern_scan_server_t *);
/* queries received, batches formed, back-end calls made (per batch: one per distinct (k, ef) -- or ONE for all its unfiltered requests
 * where the back end takes mixed batches -- plus one per (k, ef) of its filtered requests -- or ONE for all of them where the back end takes
 * a filter and (k, ef) per query; a mixed call is at most three kernel launches, a mixed filtered call at most two), largest batch so far */
LANTERN_GPU_EXPORT void lantern_scan_server_stats(lantern_scan_server_t *, uint64_t *requests, uint64_t *batches,
                                                  uint64_t *launches, uint64_t *largest_batch);
/* batches formed so far by size: bins[b] counts batches of 2^b .. 2^(b+1) - 1 requests (b < 16); returns the bins written */
/* mean microseconds of a request on the server by leg -- out4[0] read -> its batch closes, [1] batch closed -> its answer is known,
 * [2] answer known -> written to the socket -- and out4[3] the number of requests the means are over (cumulative since start) */
LANTERN_GPU_EXPORT void lantern_scan_server_timing(lantern_scan_server_t *, double *out4);
LANTERN_GPU_EXPORT size_t lantern_scan_server_batch_histogram(lantern_scan_server_t *, uint64_t *bins, size_t nbins);
LANTERN_GPU_EXPORT void lantern_scan_server_stop(lantern_scan_server_t *);
/* client: one connection per backend, one query at a time; returns the number of results (<= k), ascending */
LANTERN_GPU_EXPORT lantern_scan_client_t *lantern_scan_client_connect(const char *host, int port, usearch_error_t *);
LANTERN_GPU_EXPORT size_t lantern_scan_client_search(lantern_scan_client_t *, const void *query, size_t query_bytes, size_t k,
                                                     size_t ef, usearch_label_t *labels, float *distances, usearch_error_t *);
/* the streaming continuation (scan.c:273-281) through the service: the NEXT k rows of the scan this connection began with
 * its last lantern_scan_client_search; the state is the connection's, so concurrent backends never disturb each other */
LANTERN_GPU_EXPORT size_t lantern_scan_client_search_next(lantern_scan_client_t *, const void *query, size_t query_bytes, size_t k,
                                                          size_t ef, usearch_label_t *labels, float *distances, usearch_error_t *);
/* Set this connection's filter: allowed are the rows whose label is in labels[0 .. n) (n = 0: nothing is allowed; flags:
 * LANTERN_GPU_FILTER_SKIP_DELETED).  Returns the allowed rows.  It replaces the connection's previous filter and ends its current
 * scan; on an error the previous filter stays in force.  clear_filter: the connection is unfiltered again. */
LANTERN_GPU_EXPORT size_t lantern_scan_client_set_filter(lantern_scan_client_t *, const usearch_label_t *labels, size_t n, uint32_t flags,
                                                         usearch_error_t *);
LANTERN_GPU_EXPORT void   lantern_scan_client_clear_filter(lantern_scan_client_t *, usearch_error_t *);
/* Extend this connection's filter to the served index's present size (lantern_gpu_filter_extend on the server: the "LSRX" message):
 * the rows it has stay as they are, a row added since is allowed iff its label is in labels[0 .. n) -- or, under
 * LANTERN_GPU_FILTER_EXTEND_ALL (n must be 0), always; LANTERN_GPU_FILTER_SKIP_DELETED as above.  Returns the allowed rows.  Unlike
 * set_filter it KEEPS the connection's current scan: a continuation goes on where it stood.  On an error -- the connection has no
 * filter, the index was compacted since -- nothing changes.  Only lantern_scan_server_start serves the message: the injected back ends
 * of the *_fn forms have no extension hook and answer it with an error frame (the connection survives, its filter stays in force). */
LANTERN_GPU_EXPORT size_t lantern_scan_client_extend_filter(lantern_scan_client_t *, const usearch_label_t *labels, size_t n, uint32_t flags,
                                                            usearch_error_t *);
LANTERN_GPU_EXPORT void   lantern_scan_client_close(lantern_scan_client_t *);

/* ------------------------------------------------------------------------------------------ */
/* SQL-callable distance functions' semantics (hnsw.c:296-405): dimension checks + messages     */
/* ------------------------------------------------------------------------------------------ */
/* l2sq_dist(real[], real[]) -> float4; error text hnsw.c:301-303 */
LANTERN_GPU_EXPORT float lantern_l2sq_dist(const float *a, int a_dim, const float *b, int b_dim, usearch_error_t *);
LANTERN_GPU_EXPORT float lantern_cos_dist(const float *a, int a_dim, const float *b, int b_dim, usearch_error_t *);
/* hamming_dist(integer[], integer[]) -> int32 (hnsw.c:308-319,370-376): bits = dim*32 */
LANTERN_GPU_EXPORT int32_t lantern_hamming_dist(const int32_t *a, int a_dim, const int32_t *b, int b_dim,
                                                usearch_error_t *);

#ifdef __cplusplus
}
#endif
#endif /* LANTERN_GPU_H */
