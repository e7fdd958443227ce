/*
 * hiprag.h -- C-ABI of libhiprag.so, the MI355X (gfx950) hybrid-retrieval hot path.
 *
 * This is the drop-in boundary for batd-htplus/intool-rag's retrieval path.  The reference is pure
 * Python and reaches its native code through third-party wheels; each entry point below names the
 * reference call site (file:line under the reference repo) whose native work it replaces.  The Python
 * host side (intool-rag_amd/hiprag/_native.py) binds exactly these symbols with ctypes; INTEGRATION.md
 * shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - every function returns int32 status: 0 = OK, <0 = HIPRAG_E_*; hiprag_last_error() gives a
 *     thread-local message for the last failure on the calling thread.
 *   - handles are opaque uint64; the library owns all device memory behind a handle until *_destroy.
 *   - "_dev" variants take DEVICE pointers and a hipStream_t (as void*); they enqueue work and return
 *     without synchronising.  Non-"_dev" variants take HOST pointers, copy, run and synchronise.
 *   - callers may call from any thread (asyncio.to_thread workers, rag/providers/hf/embeddings.py:53,76):
 *     each handle serialises its own calls with an internal mutex and sets its device on entry.
 *   - no Python callbacks, no exceptions across the boundary, no torch types.
 */
#ifndef HIPRAG_H
#define HIPRAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPRAG_OK 0
#define HIPRAG_E_INVALID (-1)  /* bad argument */
#define HIPRAG_E_HIP (-2)      /* HIP runtime error (message has hipGetErrorString) */
#define HIPRAG_E_HANDLE (-3)   /* unknown / destroyed handle */
#define HIPRAG_E_IO (-4)       /* file error */
#define HIPRAG_E_NOMEM (-5)
#define HIPRAG_E_UNSUPPORTED (-6)

#define HIPRAG_METRIC_IP 0 /* larger score first  (faiss.IndexFlatIP order)  */
#define HIPRAG_METRIC_L2 1 /* smaller squared-L2 first (faiss.IndexFlatL2 order; rag/storage/faiss_index.py:123) */

/* ---- library ---------------------------------------------------------------------------------------- */
int32_t hiprag_version(void);
const char* hiprag_last_error(void);
int32_t hiprag_device_count(int32_t* out_count);
int32_t hiprag_device_sync(int32_t device);
/* The device's SCAN STREAM: one high-priority hipStream_t per device, owned by the library (valid until hiprag_shutdown).
 * The hybrid calls run their dense leg on it; hosts that chain scans themselves (hipidx_search_begin_dev,
 * hiphybrid_shard_begin_dev) pass it as scan_stream so that the kernels meant to run BESIDE a scan -- the finish of the
 * previous launch, a BM25 leg, an all-gather -- do not take the scan's CUs first: a scan workgroup needs an empty CU, the
 * others are many small workgroups, and the dispatcher serves the high-priority queue first (hipidx_set_spare_cus). */
int32_t hiprag_scan_stream(int32_t device, void** out_stream);
/* The device's two TAIL STREAMS (which = 0 / 1; normal priority, owned by the library): where the kernels that run beside a
 * scan belong -- the finish of the previous launch, an exchange, a merge.  One pair per device for the whole process: HIP
 * hands its four hardware queues per priority to streams in order of first use and lets later streams share them, and a
 * process that creates tail streams per index or per wrapper object slows its later pipelines down by that alone.  The
 * library's own pipeline (hipidx_search_dev) uses which = 0. */
int32_t hiprag_tail_stream(int32_t device, int32_t which, void** out_stream);
/* Optional process-level bracket: init checks that n_devices GPUs are visible (<= 0: at least one) and
 * creates their contexts up front; shutdown synchronises every device and drops every handle still registered (their
 * device memory goes with them) -- the reference has no counterpart, its indices live until the process exits
 * (`_INDEX_CACHE`, rag/storage/faiss_index.py:24). */
int32_t hiprag_init(int32_t n_devices);
int32_t hiprag_shutdown(void);

/* HIP-event timing on an arbitrary stream (bench.py measures kernels on the stream they run on). */
/* Calibration, not part of the path: GB/s this device sustains on a read-only stream with the dense scan's partition
 * (every wave its own contiguous range of 64 KiB blocks, non-temporal 16-byte loads) over a zeroed scratch buffer of
 * `bytes`, `reps` timed launches of four passes each.  bench.py reports it beside the scan's achieved rate. */
int32_t hiprag_probe_read_gbps(int32_t device, int64_t bytes, int32_t reps, double* out_gbps);

int32_t hiprag_event_create(uint64_t* out_event);
int32_t hiprag_event_record(uint64_t event, void* stream);
int32_t hiprag_event_elapsed_ms(uint64_t start, uint64_t stop, float* out_ms); /* synchronises on stop */
int32_t hiprag_event_destroy(uint64_t event);

/* ---- dense flat index (replaces faiss.IndexFlatL2 / IndexFlatIP) -------------------------------------
 * create   <- faiss.IndexFlatL2(d)                      rag/storage/faiss_index.py:123
 * add      <- index.add(float32[n,d])                   rag/storage/faiss_index.py:124
 * search   <- index.search(float32[nq,d], k)            rag/storage/faiss_index.py:83, rag/agent/search_engine.py:45
 * ntotal/d <- index.ntotal / index.d                    rag/storage/faiss_index.py:97,103
 * save/load<- faiss.write_index / faiss.read_index      rag/storage/faiss_index.py:133,54
 *
 * Results: exact top-k under (better score first, lower id first on ties), where the score of a row is the
 * fp64-accumulated inner product / squared L2 distance of the fp32 inputs; out_scores is that value rounded
 * to fp32.  Slots past ntotal are padded FAISS-style: id -1, score -FLT_MAX (IP) / FLT_MAX (L2).
 * Returned ids are row numbers in insertion order plus the index's id_base (row-sharded indices).
 * Inputs must be finite.
 */
/* One handle = one GPU's rows (`device`).  SURVEY 8b sketched a `n_shards` argument here; this library shards the way the
 * hardware is driven instead -- one process per GPU, each with its own handle over a contiguous row range
 * (`hipidx_set_id_base` makes its ids global), partial top-k merged after ONE all-gather by `hiprag_merge_topk_dev`
 * (hiprag/sharded.py).  The same holds for `hipbm25_create` (document-range shards, `hipbm25_set_id_base`). */
int32_t hipidx_create(int32_t d, int32_t metric, int32_t device, uint64_t* out_handle);
int32_t hipidx_destroy(uint64_t h);
int32_t hipidx_add(uint64_t h, const float* x_host, int64_t n);
/* `hipidx_add_dev` enqueues its re-tiling on `stream` and returns at once: `x_dev` must stay valid until that work has run.
 * The library orders everything that reads the rows behind it -- a later add that re-allocates, `hipidx_save`,
 * `hipidx_reconstruct` (host waits) and searches on any stream (device-side wait) -- so no caller-side synchronisation
 * is needed between an add and the next call on the same handle. */
int32_t hipidx_add_dev(uint64_t h, const float* x_dev, int64_t n, void* stream);
int32_t hipidx_ntotal(uint64_t h, int64_t* out_n);
int32_t hipidx_dim(uint64_t h, int32_t* out_d);
int32_t hipidx_metric(uint64_t h, int32_t* out_metric);
int32_t hipidx_set_id_base(uint64_t h, int64_t id_base);
int32_t hipidx_search(uint64_t h, const float* q_host, int32_t nq, int32_t k, float* out_scores, int64_t* out_ids);
/* device variant: out_scores64_dev [nq,k] double (exact, for cross-shard merges), out_scores_dev [nq,k]
 * float (may be NULL), out_ids_dev [nq,k] int64.  Enqueues and returns; q_dev and the outputs must stay valid until `stream`
 * has passed the call's work.  A batch of more queries than one launch takes (hipidx_launch_queries) is PIPELINED inside the
 * library: the scans run back to back on the device's scan stream (hiprag_scan_stream) with 48 CUs left out of their grids,
 * the finish of every launch but the last beside the next scan (hipidx_gate_tail_dev), `stream` ahead of the first scan
 * and behind the last finish -- 1M x 1024 rows, 16384 queries per call: 202 k queries/s; a 125 k-row shard: 1.32 M.  Such a
 * call uses every workspace slot: do not mix it with a begin / finish pipeline in flight on the same index. */
int32_t hipidx_search_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, double* out_scores64_dev,
                          float* out_scores_dev, int64_t* out_ids_dev, void* stream);
/* ---- scoped search: one collection index, per-query row-range scopes ---------------------------------
 * search_scoped <- search_by_vector(query_vector, limit, project)   rag/storage/faiss_index.py:140 -- `project` is accepted and
 *                  dropped there ("for future filtering", :150); rag/ingest/ingestion_pipeline.py:35 carries the same
 *                  argument through ingest.  Documents are appended whole, so a document is a contiguous row range of
 *                  the collection index and a project a handful of ranges: a SCOPE.
 * scopes in CSR form, HOST arrays, copied before the call returns:
 *   ranges_host         int64 [n_ranges][2]   half-open LOCAL row ranges [lo, hi) (rows in insertion order, before id_base)
 *   scope_offsets_host  int32 [n_scopes + 1]  scope s = ranges scope_offsets[s] .. scope_offsets[s + 1] - 1
 *   scope_of_query_host int32 [nq]            the scope query i searches, 0 .. n_scopes - 1
 * Result for query i: the top k of the rows that lie in a range of its scope under the flat index's own definition (the
 * block comment above: fp64-accumulated score of the fp32 values, better score then lower id, out_scores the fp32 rounding,
 * ids = local row + id_base, slots past the rows of the scope padded id -1, -FLT_MAX / -DBL_MAX (IP), FLT_MAX / DBL_MAX (L2)).
 * A row's score is THE SAME BITS hipidx_search_dev returns for it: the scope [0, ntotal) gives hipidx_search_dev's three
 * outputs bit for bit, the scope [lo, hi) those of an index that holds only rows lo..hi-1, ids + lo.
 * Only the rows of a scope are read (fp32, scope rows x d_pad x 4 bytes, once per group of up to 16 queries that name the
 * scope), never the scan's filter copy; ranges need no alignment.  Checks, all HIPRAG_E_INVALID before anything is enqueued:
 * nq >= 1; 1 <= k <= 256 (the partial list of a 256-row slice, merged by hiprag_merge_topk_dev, as in the IVF search);
 * n_scopes >= 1; q and the outputs non-null; then THE TABLE RULES, the same for every scoped entry of this header (one copy
 * of the code, csrc/scope_plan.h; hiprag_scope_plan below asks them without a handle).  With n the entry's count (ntotal
 * here; n, n_docs, documents elsewhere), in this order: scope_offsets_host non-null; scope_of_query_host non-null; the
 * offsets start at 0 and do not descend; ranges_host non-null unless there is no range; then for every range in turn, scope
 * by scope, 0 <= lo <= hi <= n, and after that lo >= the hi of the range before it IN ITS SCOPE (lo[j] >= hi[j-1]: touching
 * and empty ranges are allowed; ranges of different scopes may overlap and need not ascend); then every scope_of_query in
 * 0 .. n_scopes - 1.  The first rule broken is the one reported.
 * A scope without rows is valid and yields all padding.  out_scores_dev / out_scores may be NULL.  The _dev entry enqueues on
 * `stream` and returns without a host synchronisation (it waits device-side for pending hipidx_add_dev work; rows added
 * after a call are searchable by the next).  Workspace: (256-row slices of the largest scope) x k x 16 bytes per query; the
 * batch is cut into chunks of at most 16 384 queries whose partial lists stay within 512 MiB (a chunk is one query at least),
 * so a large scope costs chunks, never an error.
 * Which entry to call: the library does not choose.  A scoped call reads fp32 rows and scores in fp64; hipidx_search_dev
 * streams the bf16 filter copy through the MFMAs for 64 queries per pass.  The share of the rows
 * at which a batch that shares one scope stops being faster than the flat search has not been measured yet
 * (tools/bench_scoped.py reports it as break_even_share).
 * hipidx_scoped_info: out4 = { queries per work item (16), queries per chunk of the last scoped call, its chunks, rows_read =
 * the in-scope rows of its work items summed: for one chunk in which m_s queries name scope s of R_s rows,
 * sum_s ceil(m_s / 16) x R_s }; it synchronises the device. */
int32_t hipidx_search_scoped_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, const int64_t* ranges_host,
                                 const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                 double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream);
/* the same with q and the three outputs in HOST memory: copies, runs on the null stream, synchronises */
int32_t hipidx_search_scoped(uint64_t h, const float* q_host, int32_t nq, int32_t k, const int64_t* ranges_host,
                             const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                             double* out_scores64, float* out_scores, int64_t* out_ids);
int32_t hipidx_scoped_info(uint64_t h, int64_t* out4);
/* hiprag_scope_plan: the table rules above and the image of the tables a scoped search copies to the device, asked of the
 * library without a handle or a device -- arithmetic alone, like hiprag_scan_plan and hiprag_compaction_plan; the scoped
 * searches run the same code.  The tables are those of hipidx_search_scoped_dev over a structure of n entries (the
 * "is not within" message prints "n").  The image is int64 words in six sections,
 *   ranges [n_ranges][2] | slice_start [n_ranges + 1] | scope_off [n_scopes + 1] | scope_rows [n_scopes] |
 *   scope_slices [n_scopes] | scope of every query [nq]
 * where a range is cut into slices on ABSOLUTE multiples of slice_rows (a range with rows has (hi - 1) / slice_rows -
 * lo / slice_rows + 1 of them, an empty one none), slice_start[j] = slices of the ranges before j, and scope_rows /
 * scope_slices are the sums over a scope's ranges.  slice_rows = 0 gives the lean image ranges | scope_off | scope of every
 * query (hipivf_search_scoped_dev's): the other three sections are empty.  The flat search's image is that of slice_rows
 * 256 and group 16, the late-interaction search's that of 16 and 8.
 * out8 = { words of the image, smax = slices of the largest scope (0 when no scope has a row, and in the lean image),
 * bound = sum over the scopes of ceil(queries that name it / group) x its slices (the work items of a call in which up to
 * `group` queries of a scope share one), and the word at which each section but the first begins: slice_start, scope_off,
 * scope_rows, scope_slices, scope of every query }.  out_image in caller memory receives the image when image_cap (in words)
 * >= out8[0]; out_image NULL with image_cap 0 asks for out8 alone.  HIPRAG_E_INVALID, with nothing written: a null out8,
 * nq < 1, n_scopes < 1, n < 0, slice_rows < 0, group < 1, the table rules, a null out_image with image_cap != 0, an
 * image_cap below the image. */
int32_t hiprag_scope_plan(const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                          const int32_t* scope_of_query_host, int32_t nq, int64_t n, int32_t slice_rows, int32_t group,
                          int64_t* out8, int64_t* out_image, int64_t image_cap);
/* hiprag_slice_items: the WORK ITEMS of a sliced scoped search, asked of the library without a handle or a device, as
 * hiprag_scope_plan is.  hipidx_search_scoped_dev, hipmaxsim_search_scoped_dev and hipmaxsim_search_pruned_dev cut every scope
 * into slices of slice_rows entries on absolute multiples of slice_rows and give (scope, slice, group of up to `group` of
 * the queries that name the scope) to one workgroup; (slice_rows, group) = (256, 16), (16, 8), (256, 8) in that order, and
 * any other pair is refused.  The entry builds the image of hiprag_scope_plan, forms on the host the tables the device forms
 * (the queries sorted by scope, stably; items of a scope = its query groups x its slices, none for a scope no query names)
 * and runs the kernels' own decode (csrc/slice_items.h) for every item in turn.  An item is 8 int64 words:
 *   scope, slice of the scope, group, members (1..group), first = place of the group's first member among the queries
 *   sorted by scope, base = the slice's first entry (a multiple of slice_rows), p_lo, p_hi: the item covers entries
 *   [base + p_lo, base + p_hi) of the structure.
 * Items come in (scope, slice, group) order; for every scope and every group of it the windows of its items are disjoint
 * and their union is the scope's entries.  *out_count = the items (hiprag_scope_plan's bound); out_items receives them when
 * items_cap (in items) >= *out_count; out_items NULL with items_cap 0 asks for the count alone.  HIPRAG_E_INVALID, with
 * nothing written: a null out_count, nq < 1, n_scopes < 1, n < 0, another (slice_rows, group), the table rules, a null
 * out_items with items_cap != 0, an items_cap below the count. */
int32_t hiprag_slice_items(const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                           const int32_t* scope_of_query_host, int32_t nq, int64_t n, int32_t slice_rows, int32_t group,
                           int64_t* out_items, int64_t items_cap, int64_t* out_count);
/* ---- exact scores of given rows: faiss's compute_distance_subset for the flat index ------------------------------
 * score_ids <- "score": item.get("score", 0)                          rag/query/page_retriever.py:191 -- every chunk the
 *              reference hands to rank_pages carries the similarity index.search gave it (rag/storage/faiss_index.py:83).
 *              A fused candidate that only the BM25 leg found, or that lies outside the lists an IVF search probed, has
 *              none: a search scores a row only as a by-product of finding it.  This entry scores ANY rows.
 * ids int64 [nq][depth]: entry (i, j) = c names LOCAL row c - id_base.  It is VALID iff c >= 0 and 0 <= c - id_base < ntotal.
 * For a valid entry out_scores64[i][j] is the fp64-accumulated inner product / squared L2 distance of query i and the row's
 * fp32 values -- THE SAME BITS hipidx_search_dev, hipidx_search_scoped_dev and the hipivf_* entries return for that row and
 * query: it is rescore4 (csrc/dense_layout.h) on the row's quad (rows row & ~3 .. of its 32-row block), read from the lane
 * with lane & 3 == row & 3; there is no second accumulation loop.  out_scores[i][j] is its fp32 rounding; out_scores /
 * out_scores_dev may be NULL.  An invalid entry is PADDING: no row is read for it and its outputs are the search entries'
 * padding values, -DBL_MAX / -FLT_MAX (IP), DBL_MAX / FLT_MAX (L2).  The same id twice is two entries; no order of the ids
 * is assumed.  Read per valid entry: one 128-byte line of each of the row's pieces (its quad), d_pad x 16 bytes.
 * Checks, all HIPRAG_E_INVALID before anything is enqueued: null pointers (except out_scores); nq >= 1; depth >= 1;
 * nq x depth < 2^31.  An empty index is valid: everything is padding.
 * The _dev entry takes the handle, waits device-side for pending hipidx_add_dev work, enqueues on `stream` and returns
 * without a host synchronisation; it allocates nothing per call (an 8-byte counter word is made at the handle's first call).
 * The host entry copies, runs on the null stream and synchronises.
 * Kernel: a workgroup = one query x up to 64 consecutive entries (4, 8, .. 64: the smallest at which the grid is at most
 * 4096 workgroups, else 64), the query staged once in LDS as d_pad zero-padded floats, one wave per entry at a time.
 * hipidx_score_info: out4 = { valid entries, padding entries, workgroups launched, 0 } of the last call (zeros before the
 * first); integer counts, one integer atomic per workgroup, identical from run to run; it synchronises the device. */
int32_t hipidx_score_ids_dev(uint64_t h, const float* q_dev, int32_t nq, const int64_t* ids_dev, int32_t depth,
                             double* out_scores64_dev, float* out_scores_dev, void* stream);
int32_t hipidx_score_ids(uint64_t h, const float* q_host, int32_t nq, const int64_t* ids_host, int32_t depth,
                         double* out_scores64, float* out_scores);
int32_t hipidx_score_info(uint64_t h, int64_t* out4);
/* Removal: faiss.IndexFlat.remove_ids, on the class this index replaces, as STABLE COMPACTION -- the rows of `ranges_host`
 * (int64 [n_ranges][2], half-open LOCAL row ranges [lo, hi), ascending and not overlapping; touching and empty ranges are
 * allowed; 0 <= lo <= hi <= ntotal: the rules of one scope of hipidx_search_scoped) are removed, the survivors keep their
 * order and are renumbered densely.  It serves the reference's overwrite-on-re-ingest (rag/ingest/ingestion_pipeline.py:80-94
 * writes {doc_id}_faiss.index again, so a second ingest of a document replaces the first) for an index that holds many
 * documents.  Afterwards the index is indistinguishable from one built by one hipidx_add of the surviving rows in order
 * into a fresh handle of the same d, metric, scan mode and id_base: ntotal, the bytes hipidx_save writes,
 * hipidx_reconstruct, every output of every search entry, hipidx_row_bounds, hipidx_launch_queries and what a later
 * hipidx_add sees (rows past ntotal and vacated blocks are zero again; the two row maxima of the certificate are
 * recomputed over the survivors, so a removed outlier row does not leave the bound wide).  Capacity is not given back.
 * The rows move on the device, in place, in the blocked layout: rows before the first removed row are neither read nor
 * written, and the extra device memory of a call is at most 256 MiB whatever ntotal is.
 * Synchronous: takes the handle, waits for pending hipidx_add_dev work, runs on the null stream and synchronises before it
 * returns.  THE CALLER MUST HAVE NO SEARCH IN FLIGHT ON THE HANDLE (on any stream) -- as for a second pipelined search.
 * THE TABLE RULES, the same for every *_remove_ranges entry of this header and stated here alone (csrc/range_table.h holds
 * the one copy of the code).  With n the entry's count (ntotal here; rows, documents elsewhere), in this order: n_ranges >= 0;
 * ranges_host non-null unless n_ranges == 0; then for every range in turn 0 <= lo <= hi <= n, and after that lo >= the hi of
 * the range before it (an empty one included).  Touching and empty ranges are allowed; an empty table removes nothing.
 * Every check happens before anything is touched: a bad table returns HIPRAG_E_INVALID and leaves the index bit for bit
 * as it was.  An index that a live hipivf_* handle references (rows or centroids) is refused with HIPRAG_E_UNSUPPORTED:
 * the IVF list offsets would go stale.
 * hipidx_remove_info: out4 of the LAST removal = { rows removed, rows moved (the survivors behind the first removed row),
 * chunks of the move, extra device bytes it allocated (staging + range table) }.
 * hipidx_row_bounds (a test hook, like hipidx_reconstruct): out2 = { max |x|^2, max |x - bf16(x)|^2 } over the rows, rounded
 * up, as the certificate uses them. */
int32_t hipidx_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges);
int32_t hipidx_remove_info(uint64_t h, int64_t* out4);
int32_t hipidx_row_bounds(uint64_t h, float* out2);
/* hiprag_compaction_plan: what a removal does to a document CSR (the token store, the multi-vector store), asked of the
 * library without a handle or a device -- arithmetic alone, like hiprag_scan_plan; hiptok_remove_ranges and
 * hipmv_remove_ranges carry out the plan of the same code over their stored lengths.  lens int32 [n_docs] are the stored
 * lengths (>= 0), ranges_host a table over n = n_docs under the table rules above.  out6 = { the first removed document,
 * its offset (the item position where moving begins), documents afterwards, items afterwards, the longest document
 * afterwards, n_runs }; out_runs int64 [n_ranges + 1][3] in caller memory receives n_runs rows { src, dst, len } in items:
 * the surviving runs behind the first removed document, ascending, dst <= src, their destinations tiling [out6[1],
 * out6[3]).  A run is there when it holds an item (also with src == dst, when only empty documents went in front of it).
 * A table that removes nothing gives { n_docs, items, n_docs, items, longest, 0 }.  HIPRAG_E_INVALID: a null out6, lens or
 * out_runs that is needed, n_docs < 0, a negative length, the table rules. */
int32_t hiprag_compaction_plan(const int32_t* lens, int64_t n_docs, const int64_t* ranges_host, int32_t n_ranges, int64_t* out6,
                               int64_t* out_runs);
/* Queries one scan pass serves: 64.  HIPRAG_SCAN_MODE picks the scan's operands:
 *   bf16 (default)  the scan streams a bf16 FILTER COPY of the rows (2 B per element, kept beside the fp32 rows: 6 B per
 *                   element of HBM in all) against bf16 query tiles
 *   q64             streams the fp32 rows themselves, split on the fly into bf16 hi + lo, against bf16 query tiles (N*d*4
 *                   bytes per pass: the accounting of SURVEY 8(d)); no extra memory is read
 * Both return the same exact results -- the scan only nominates candidate groups (a per-query candidate list, filtered
 * inside the scan against a bound it maintains itself); every candidate the finish needs is re-scored in fp64 from the fp32
 * rows and a certificate (or, where it fails, the exhaustive path) proves nothing was missed.  The modes differ in how many
 * bytes a pass streams and how wide the certificate's error bound is.  Any other value is rejected by hipidx_create. */
int32_t hipidx_pass_queries(uint64_t h, int32_t* out_n);
/* Queries one scan LAUNCH takes (a multiple of the pass size): the scan kernel runs launch/pass passes back to back
 * inside one launch -- each pass streams the index once for its own query tile -- so that no kernel boundary (45-60 us
 * of idle GPU) separates them.  Sized by the index so that a launch lasts about 2.6 ms: in the default mode 8 passes
 * (512 queries) at 1M x 1024, 16 (the cap, 1024 queries) from half that down; it changes when rows are added.
 * HIPRAG_LAUNCH_QUERIES fixes it. */
int32_t hipidx_launch_queries(uint64_t h, int32_t* out_n);
/* Two-phase form of one launch (nq <= hipidx_launch_queries) for callers that pipeline: begin = index scan into
 * workspace `slot` (0..7, allocated on first use); finish = two kernels out of that slot (candidate ranking + fp64 re-score
 * + top-k + certificate in one; the exhaustive path for flagged queries).  k <= 128 takes this path; deeper k (to 1000) is
 * answered by the exhaustive path alone.  begin(slot s) of a later call must be ordered after finish(slot s) of the call that
 * used it (stream order or an event); the two phases may run on different streams if finish waits for begin.
 * search_dev == begin + finish on slot 0, repeated for every hipidx_launch_queries queries. */
int32_t hipidx_search_begin_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t slot, void* stream);
int32_t hipidx_search_finish_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t slot,
                                 double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream);
/* Leave n CUs out of the scan grid (default 0).  A scan workgroup takes a CU's whole LDS, so kernels of OTHER streams --
 * the finish of the previous launch, the BM25 leg of a hybrid call, at N > 1 the RCCL all-gather, whose ranks spin until
 * every peer has joined -- only run on CUs the scan leaves (or between scans).  The scan is HBM-bound and does not need
 * every CU: at 1M x 1024 rows a launch takes the same time on 192 workgroups as on 256 and 5 % longer on 160 (the wide
 * scan of launches of 256 queries and more is bound by its CUs instead: hipidx_pipe_spare_cus).  Takes
 * effect with the next launch, no synchronisation (the finish reads a launch's lists, never its partition).  The hybrid
 * calls and the row-sharded hosts set it themselves (hiphybrid_search*: 96 for the dense leg of the call). */
int32_t hipidx_set_spare_cus(uint64_t h, int32_t n);
int32_t hipidx_get_spare_cus(uint64_t h, int32_t* out_n);
/* How many CUs a host that pipelines launches (the finish of launch i beside scan i + 1) should leave out of the scan grid
 * for the index as it stands: what hipidx_search_dev's own pipeline leaves.  48, or 32 where a full launch takes the wide
 * scan and the 16 CUs save it a round of row tiles (1M x 1024: 19 -> 18 rounds).  Sets nothing: pass it to
 * hipidx_set_spare_cus; ask again after the index has grown or shrunk. */
int32_t hipidx_pipe_spare_cus(uint64_t h, int32_t* out_n);
/* The scan's launch policy, for tests and tools: which kernel a launch gets and in what shape is a pure function of a
 * shape, the launch's queries and depth, and the grid.  hipidx_scan_shape gives the shape a handle has as it stands (ask
 * again after the index has grown or shrunk); hiprag_scan_plan is arithmetic alone -- no handle, no device, callable on a
 * machine without a GPU.  cus = workgroups of the scan = CUs of the device - spare CUs.  (The two types end in _t because C
 * keeps functions and typedef names in one name space.) */
typedef struct hipidx_scan_shape_t {
    int64_t nblocks;     /* 32-row blocks of the index */
    int32_t P;           /* 1 KiB fp32 pieces per block: d_pad / 8, d_pad = d rounded up to 128 */
    int32_t mode;        /* HIPRAG_SCAN_MODE as read at creation: 3 = bf16, 2 = q64 */
    int32_t wide_env;    /* HIPRAG_SCAN_WIDE as read at creation: 0, 1, or -1 = unset */
    int32_t n_cu;        /* CUs of the device */
    int32_t launch_env;  /* HIPRAG_LAUNCH_QUERIES as read at creation (0 = launches sized by the index) */
} hipidx_scan_shape_t;
typedef struct hipidx_scan_plan_t {
    int32_t run;         /* 0: no scan is launched (no rows, or k beyond the finish: exhaustive path); then only `filter` and
                          * the four launch-independent fields at the end are set */
    int32_t wide;        /* the wide kernel (256 queries per read of the filter copy) */
    int32_t waves;       /* waves per scan workgroup: 4 or 8 */
    int32_t ring;        /* depth of the narrow kernels' load ring: 8 or 16 (0 for the wide kernel) */
    int32_t multi_pass;  /* more than 64 queries */
    int32_t filter;      /* the scan keeps a bound and lists only the groups that reach it */
    int32_t ncls;        /* bound classes in use */
    int32_t qtile_image; /* the query tiles are copied from images a small kernel makes ahead of the scan */
    int64_t lds_bytes;   /* dynamic LDS of the launch */
    int32_t launch_queries;     /* hipidx_launch_queries of the shape */
    int32_t pipe_spare_cus;     /* hipidx_pipe_spare_cus of the shape */
    int64_t bytes_per_pass_ip;  /* hipidx_stats.bytes_per_pass if launches of this plan's kind are what the index runs, */
    int64_t bytes_per_pass_l2;  /* for either metric */
} hipidx_scan_plan_t;
int32_t hiprag_scan_plan(const hipidx_scan_shape_t* shape, int32_t nq, int32_t k, int32_t cus, hipidx_scan_plan_t* out);
int32_t hipidx_scan_shape(uint64_t h, hipidx_scan_shape_t* out);
/* The WALK of the wide kernel, for tests and tools: the (row tile, column) pairs that workgroup `wg` of a grid of `cus`
 * computes, in the order it computes them, for an index of `nrt` row tiles of 256 rows and a launch of `ncol` columns of 256
 * queries.  The function the kernel itself calls -- arithmetic alone, no handle, no device.  The full rounds go by row tile
 * (row tile wg + i cus, all its columns in turn); the last, partial round is split by column over all the workgroups, so
 * no workgroup runs more than floor(nrt / cus) ncol + ceil((nrt mod cus) ncol / cus) pairs; with fewer row tiles than
 * workgroups, workgroup wg < nrt takes row tile wg and all its columns.  *out_pairs = the number of pairs of the
 * workgroup; the first min(cap, *out_pairs) of them are written to out_row_tile / out_column (both may be null with
 * cap = 0).  1 <= nrt < 2^28, 1 <= ncol <= 4, cus >= 1, 0 <= wg < cus. */
int32_t hiprag_wide_walk(int64_t nrt, int32_t ncol, int32_t cus, int32_t wg, int64_t cap, int64_t* out_row_tile,
                         int32_t* out_column, int64_t* out_pairs);
/* The FOLD SCHEDULE of the wide kernel, for tests and tools: out_fold[i] = 1 if wave `wave` (0..7: row half wave & 1, query
 * pair wave >> 1) of workgroup `wg` recomputes the bound of its 64-query unit behind pair number p0 + i of its walk, 0 if it
 * only reads the bound the launch has formed so far, for i < n.  The function the kernel itself calls -- arithmetic alone.
 * `every` = N, a power of two in 1..64: every pair below *out_first folds; from there a wave folds once in any N consecutive
 * pairs.  out_first / out_default (either may be null) receive that constant and the N an index uses when
 * HIPRAG_WIDE_FOLD_EVERY is not set; out_fold may be null with n = 0. */
int32_t hiprag_wide_fold(int64_t p0, int64_t n, int32_t wg, int32_t wave, int32_t every, uint8_t* out_fold, int32_t* out_first,
                         int32_t* out_default);
/* The START GATE: make `stream` (a tail stream) wait until the scan launched AFTER the one of `slot` has STARTED, i.e. until
 * every workgroup of that next scan holds its CU (the scan counts its workgroups in and raises a word; a one-wave kernel on
 * `stream` polls it).  Enqueued on the tail stream between the wait for the slot's own scan and hipidx_search_finish_dev, it
 * makes the finish (and whatever follows: an all-gather, a merge) be dispatched onto the CUs the next scan has left
 * (hipidx_set_spare_cus), beside it, instead of racing it for CUs: which of two queues that become ready at the same moment
 * is served first is not something a host can steer (measured: 0.89-1.23 M queries/s on a 125 k-row shard for one and the
 * same arrangement of streams, depending only on which hardware queues the streams happened to get).  The next scan must
 * have been LAUNCHED already (error otherwise) -- so a pipelined host enqueues the tails of step i right after it has launched
 * the scan of step i + 1, and without the gate when it needs step i's result before another scan is due (hiprag/sharded.py;
 * hipidx_search_dev does the same for a batch of several launches).  The wait is BOUNDED (1 ms: the gate opens ~30 us after
 * the previous scan has ended): where kernels are serialised -- counter collection, a debugger -- the awaited scan cannot
 * start while the wait runs, and the gate then simply times out. */
int32_t hipidx_gate_tail_dev(uint64_t h, int32_t slot, void* stream);
/* make sure slot 0's search workspace for k exists so that search / search_dev never allocate */
int32_t hipidx_reserve_search(uint64_t h, int32_t k);
/* Capacity for n_rows rows now (one allocation of each of the index's buffers; rows added later beyond it grow it by half
 * again as usual).  A caller that knows the size of the collection -- create_faiss_index's one add of all embeddings,
 * rag/storage/faiss_index.py:121-124, or a chunked ingest -- avoids the allocate / copy / free cycles of growth. */
int32_t hipidx_reserve_rows(uint64_t h, int64_t n_rows);
int32_t hipidx_reconstruct(uint64_t h, int64_t row, float* out_host); /* row as stored (tests, export) */
int32_t hipidx_save(uint64_t h, const char* path);
int32_t hipidx_load(const char* path, int32_t device, uint64_t* out_handle);

typedef struct hipidx_stats {
    int64_t passes;            /* scan passes so far (one per <= pass_queries queries; several per launch) */
    int64_t queries;           /* queries answered */
    int64_t fallback_queries;  /* queries that took the exhaustive path (certificate failed: massive ties, overflowing lists) */
    int64_t bytes_per_pass;    /* bytes of index the scan reads per pass, i.e. per 64 queries (algorithmic), by the kernel that a
                                * launch of launch_queries queries takes: the narrow kernels read the whole index per pass, the wide
                                * kernel once per 256 queries (filter copy and norms / 4) -- so bytes_per_pass x passes of a launch is
                                * what the launch really requests (two reads for 512 queries) */
    int64_t timed_passes;      /* scan LAUNCHES averaged into avg_scan_ms (at most the last 512) */
    float avg_scan_ms;         /* mean HIP-event duration of the scan kernel since timing was enabled, else -1 */
    float avg_scan_wall_ms;    /* same launches on the GPU wall clock, stamped inside the kernel: first wave in -> last wave out */
    float avg_scan_gap_ms;     /* mean idle time between consecutive timed scans (last wave out -> next first wave in) */
    int64_t launches;          /* scan kernel launches so far (each runs 1..launch_queries/pass_queries passes back to back) */
    int64_t roundb_queries;    /* queries whose re-scored prefix the finish had to extend once (more groups within eps of the k-th score) */
    int64_t list_entries;      /* candidate-list entries the scans wrote, summed over all queries answered by the finish */
    int64_t ranked_entries;    /* of those, entries at or above the final bound (what the finish ranks), summed */
    int64_t rescored_groups;   /* 16-row groups whose tagged quad was re-scored in fp64, summed */
    int64_t wide_launches;     /* of `launches`, those that ran the wide scan kernel (256 queries per read of the bf16 filter copy:
                                * bf16 mode, an index large enough for the filter, enough queries; HIPRAG_SCAN_WIDE=0|1 forces
                                * never / whenever eligible and is read when the index is created, any other value is rejected) */
    int64_t wide_theta_folds;  /* fold tiles the waves of the wide scans completed: (row tile, column) pairs behind which a wave
                                * recomputed its unit's bound from the class slots instead of only reading it (hiprag_wide_fold;
                                * HIPRAG_WIDE_FOLD_EVERY, a power of two in 1..64 read when the index is created, 1 = every pair) */
} hipidx_stats;
int32_t hipidx_get_stats(uint64_t h, hipidx_stats* out);
/* on = n > 0: HIP events (on the launch stream) around every n-th scan launch, in-kernel wall-clock stamps on every launch;
 * 0 = off.  Two event records cost ~20 us of dispatch bubble between chained launches, hence the sampling.  get_stats syncs. */
int32_t hipidx_enable_timing(uint64_t h, int32_t on);

/* ---- IVF-Flat (BASELINE north_star: "the flat-IP / IVF distance scan"; the reference builds faiss.IndexFlatL2 only,
 *      rag/storage/faiss_index.py:123 -- this is the approximate, low-latency one-query mode on top of the flat index) -------
 * rows_h       a flat index whose rows are stored PERMUTED by inverted list: list l = stored rows
 *              [list_offsets[l], list_offsets[l + 1]), every list starting on a 32-row block (pad with any rows);
 *              orig_ids_host[stored row] = the id results carry, -1 for padding rows
 * centroids_h  a flat index (same d, metric, device) over the nlist centroids, row l = centroid of list l
 * A search scores, exactly (fp64 from the fp32 rows, the flat index's own re-score), every row of the nprobe lists whose
 * centroids rank best for the query under the index's metric, and returns their top k in the canonical order.  It is
 * approximate unless nprobe >= nlist, where the result equals the flat index's bit for bit.  k <= 256, nprobe <= 1000.
 * The handle shares the two flat indexes (destroy it before them). */
int32_t hipivf_create(uint64_t rows_h, uint64_t centroids_h, const int64_t* list_offsets_host, const int64_t* orig_ids_host,
                      int32_t nlist, uint64_t* out_handle);
int32_t hipivf_destroy(uint64_t h);
int32_t hipivf_search_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t nprobe, double* out_scores64_dev,
                          float* out_scores_dev, int64_t* out_ids_dev, void* stream);
int32_t hipivf_info(uint64_t h, int32_t* out_nlist, int64_t* out_stored_rows, int64_t* out_longest_list);
/* hipivf_search_batch_dev: the LIST-MAJOR form of hipivf_search_dev for a batch of queries.  Same arguments, limits, checks and
 * error codes, and THE SAME RESULT, BIT FOR BIT (ids, scores64, scores32, padding included; hence the flat index's result at
 * nprobe >= nlist).  The probe table of the coarse step is inverted on the device, and every 256-row slice of a probed list is
 * read once per group of up to 16 of the queries that probe it instead of once per query; like every _dev entry it enqueues
 * on `stream` and returns without a host synchronisation.  Workspace: the partial lists take nprobe x (256-row slices of the
 * longest list) x k x 16 bytes per query; the batch is cut into chunks of at most 16 384 queries whose partial lists stay
 * within 512 MiB (a chunk is one query at least).  Which entry to call: hipivf_search_dev up to a few hundred queries (at 64
 * the two are level), this one from about 1024 queries on (2.1 x at 1024, 3.0 x at 16 384 queries, nprobe 8, on 1M x 1024
 * rows: profiles/ivf_batch_1m.json has all cells).
 * hipivf_batch_info: out4 = { the workspace budget in bytes, queries per chunk of the last batch call, its chunks, the
 * stored rows it read (rows of the lists that at least one query of a chunk probed, summed over the chunks) }; it
 * synchronises the device. */
int32_t hipivf_search_batch_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t nprobe,
                                double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream);
int32_t hipivf_batch_info(uint64_t h, int64_t* out4);
/* hipivf_search_scoped_dev: hipivf_search_batch_dev with a SCOPE per query -- the `project` argument of
 * rag/storage/faiss_index.py:140 for the IVF index.  Scopes in the CSR form of hipidx_search_scoped_dev (ranges_host int64
 * [n_ranges][2], scope_offsets_host int32 [n_scopes + 1], scope_of_query_host int32 [nq]; HOST arrays, copied before the call
 * returns); the ranges are half-open ranges of ORIGINAL IDS in [0, n), n = what hipivf_meta reports (a built, loaded or
 * updated index numbers its rows densely in insertion order, so these are the row ranges of a collection).
 * Probed lists: the coarse step is hipivf_search_dev's, unchanged -- the min(nprobe, nlist) lists whose centroids rank best
 * for the query, ties to the lower list, WHATEVER THE SCOPE (faiss's IDSelector behaviour): a probed list without an
 * in-scope row still counts against nprobe, and an in-scope row of a list that is not probed is not found.
 * Result for query i: the top k of the rows that are in a probed list and whose id lies in a range of its scope.  A row's
 * score is THE SAME BITS hipivf_search_dev and the flat index give for it; canonical order (better score, then lower id);
 * out_scores the fp32 rounding of out_scores64; padding id -1 with -DBL_MAX / -FLT_MAX (IP), DBL_MAX / FLT_MAX (L2).  Hence,
 * bit for bit on all three outputs: (A) the scope [0, n) gives hipivf_search_batch_dev's result at the same nprobe; (B) at
 * nprobe >= nlist the result is hipidx_search_scoped_dev's on a flat index of the same rows in id order, id_base 0.
 * Checks, all HIPRAG_E_INVALID before anything is enqueued: those of hipidx_search_scoped_dev with n for ntotal (null
 * pointers; nq >= 1; n_scopes >= 1; offsets start at 0 and do not descend; 0 <= lo <= hi <= n; the ranges of a scope ascend
 * and do not overlap, touching and empty ranges allowed; every scope_of_query in range), 1 <= k <= 256 and 1 <= nprobe <= 1000
 * as in hipivf_search_dev.  An empty scope and a scope that meets no probed list are valid and yield all padding;
 * out_scores_dev / out_scores may be NULL.  Works on every IVF handle (built, loaded, hipivf_from_centroids, hipivf_create)
 * and does not assume that ids ascend inside a list.  The _dev entry enqueues on `stream` and returns without a host
 * synchronisation (it waits device-side for pending adds, as hipivf_search_batch_dev does).  Workspace and chunking are
 * hipivf_search_batch_dev's (partial lists [nprobe x slices of the longest list][nq][k], 512 MiB, at most 16 384 queries per
 * chunk): a large call costs chunks, never an error.  Only the quads (aligned groups of 4 stored rows) that hold an in-scope
 * row are read, once per group of up to 16 of the (query, list) pairs that probe the list, whatever their scopes.  Rates: not
 * measured yet (tools/bench_ivf_scoped.py writes profiles/ivf_scoped_1m.json: each cell beside the two alternatives, the flat
 * scoped search and a deeper batch search filtered afterwards).
 * hipivf_scoped_info: out4 = { queries per work item (16), queries per chunk of the last scoped call, its chunks, rows_read =
 * 4 x the quads its kernel loaded, summed over work items and chunks: a quad is loaded if and only if at least one of its
 * rows is a member (not padding) in the scope of at least one query of the work item's group }; an integer counter, the
 * same from run to run; it synchronises the device. */
int32_t hipivf_search_scoped_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t nprobe,
                                 const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                 const int32_t* scope_of_query_host, double* out_scores64_dev, float* out_scores_dev,
                                 int64_t* out_ids_dev, void* stream);
/* the same with q and the three outputs in HOST memory: copies, runs on the null stream, synchronises */
int32_t hipivf_search_scoped(uint64_t h, const float* q_host, int32_t nq, int32_t k, int32_t nprobe,
                             const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                             const int32_t* scope_of_query_host, double* out_scores64, float* out_scores, int64_t* out_ids);
int32_t hipivf_scoped_info(uint64_t h, int64_t* out4);
/* hipivf_search_scoped_probe_dev: hipivf_search_scoped_dev with the rule that picks the probed lists as an argument.
 * A MEMBER LIST of scope s is a list with at least one stored row whose original id lies in a range of s (padding rows, id
 * -1, never count).  The COARSE ORDER of a query is the flat index's exact order of the centroids for it: the fp64 score of
 * the fp32 values, better first, ties to the lower list -- the bits hipidx_search on the centroid index gives.
 *   HIPIVF_PROBE_ANY    the min(nprobe, nlist) first lists of the coarse order, whatever the scope (faiss's IDSelector
 *                       behaviour): hipivf_search_scoped_dev, see there.
 *   HIPIVF_PROBE_SCOPE  query i probes the first min(nprobe, member lists of its scope) MEMBER lists of its coarse order:
 *                       a list without an in-scope row does not count against nprobe.  The result is the top k of the
 *                       in-scope rows of those lists; scores, canonical order, the fp32 rounding and the padding are exactly
 *                       those of hipivf_search_scoped_dev.
 * Properties, bit for bit on all three outputs:
 *   (P0) probe_mode = HIPIVF_PROBE_ANY is hipivf_search_scoped_dev.
 *   (P1) If every list is a member list of every scope used, PROBE_SCOPE equals PROBE_ANY at the same nprobe.
 *   (P2) At nprobe >= the member lists of the scope the result is hipidx_search_scoped_dev's on a flat index of the same
 *        rows in id order: the exact scoped search, reached with far fewer probes than nlist.
 *   (P3) For query i let p'_i be the smallest p such that the first p lists of its coarse order contain min(nprobe, members)
 *        member lists (nlist if the scope has none).  Row i of the PROBE_SCOPE result equals row i of
 *        hipivf_search_scoped_dev called with nprobe = p'_i: a list that is probed but is not a member contributes nothing.
 *        Hence at equal nprobe the rows PROBE_SCOPE examines are a superset of PROBE_ANY's for every query.
 * Checks: all those of hipivf_search_scoped_dev, and probe_mode must be 0 or 1 (HIPRAG_E_INVALID); all before anything is
 * enqueued.  PROBE_SCOPE needs the build's layout (ascending id within a list, padding only behind the members, less than a
 * block of it) -- what hipivf_build*, hipivf_from_centroids, the updates and a saved build give; a hipivf_create handle in
 * that layout is fine (searching moves no row), and a handle whose lists are not in it gets HIPRAG_E_UNSUPPORTED in this mode
 * and still answers in PROBE_ANY.  The FIRST PROBE_SCOPE call on a handle may synchronise once to establish the list
 * lengths; after it the _dev entry enqueues on `stream` and returns, like its siblings.
 * How: once per call, one thread per (scope, list) bisects the list's ascending ids for every range of the scope (cost:
 * ranges x lists x log2(list length)); per chunk, the centroids of the member lists are scored exactly, read once per group
 * of up to 16 queries (not once per query) and only the quads of centroids that hold a member list of a query of the group,
 * into a candidate table [queries][nlist rounded up to 4] (score, list; -1 for a list that is not a member), from which
 * hiprag_merge_topk_dev picks the probes in canonical order.  A scope with fewer member lists than nprobe leaves empty
 * probe slots, which name no list and cost nothing downstream.  The candidate table (16 bytes per query and list) counts
 * against the 512 MiB budget beside the partial lists: a large call costs chunks, never an error.  No float atomics: the
 * same bits from run to run.  Rates: not measured yet (tools/bench_ivf_scope_probe.py writes
 * profiles/ivf_scope_probe_1m.json).
 * hipivf_scope_probe_info: out4 of the last PROBE_SCOPE call on the handle (zeros before any) = { (scope, list) pairs that
 * are member pairs, over all n_scopes scopes of the call; (query, probe) slots actually probed = the sum over the queries
 * of min(nprobe, member lists of its scope); chunks; centroid rows read by the coarse step = 4 x the quads of centroids it
 * loaded, summed over the groups of 16 consecutive queries of every chunk: a quad is loaded if and only if one of its lists
 * is a member list of the scope of a query of the group }.  Integer counters, the same from run to run; it synchronises
 * the device. */
#define HIPIVF_PROBE_ANY   0   /* the nprobe best lists, whatever the scope: hipivf_search_scoped_dev */
#define HIPIVF_PROBE_SCOPE 1   /* the nprobe best lists AMONG THOSE THAT HOLD A ROW OF THE QUERY'S SCOPE */
int32_t hipivf_search_scoped_probe_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t nprobe, int32_t probe_mode,
                                       const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                       const int32_t* scope_of_query_host, double* out_scores64_dev, float* out_scores_dev,
                                       int64_t* out_ids_dev, void* stream);
/* the same with q and the three outputs in HOST memory, as hipivf_search_scoped */
int32_t hipivf_search_scoped_probe(uint64_t h, const float* q_host, int32_t nq, int32_t k, int32_t nprobe, int32_t probe_mode,
                                   const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                   const int32_t* scope_of_query_host, double* out_scores64, float* out_scores, int64_t* out_ids);
int32_t hipivf_scope_probe_info(uint64_t h, int64_t* out4);
/* ---- IVF-Flat build and files: the k-means of faiss.IndexIVFFlat.train + add as a library call (stands where the reference
 *      builds and writes its index, rag/storage/faiss_index.py:123 (IndexFlatL2), :133 (write_index), :54 (read_index)) --------
 * hipivf_build_dev  x_dev: [n, d] fp32 row-major on `device`, ordered on `stream`; returns once the index is built (it
 *                   synchronises `stream`).  The handle owns its rows index and its centroid index: hipivf_destroy and
 *                   hiprag_shutdown free them; no dense handle is created.  Algorithm, exactly:
 *   training rows   all n rows when max_train_rows is 0 or >= n; else m = max_train_rows rows, row i of the sample being
 *                   x[floor(i * n / m)], i = 0..m-1 (int64 arithmetic).
 *   initial centroids  centroid l = training row perm[l], l = 0..nlist-1, where perm starts as 0..m-1 and, for i = 0..nlist-1
 *                   in turn, perm[i] is swapped with perm[i + r % (m - i)], r the next output of splitmix64 whose state
 *                   starts at seed + 1 (the offset FAISS's Clustering gives the seed of its permutation); per output:
 *                   state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                   z = (z ^ z >> 27) * 0x94D049BB133111EB; r = z ^ z >> 31; all uint64.
 *   each of `iters` rounds
 *     assign        every training row to its nearest centroid under the metric: the flat index's exact k = 1 search over
 *                   the centroids (fp64 scores of the fp32 values), ties to the lower list id.
 *     update        a non-empty list's centroid = the mean of its members: fp64 sum in a fixed order (members ascending,
 *                   in chunks of 256, chunk sums added in chunk order), divided by the count in fp64; under IP the mean is
 *                   then divided by its fp64 norm (spherical k-means; a zero mean stays zero); rounded to fp32.  An empty
 *                   list keeps its previous centroid.
 *   layout          all n rows assigned to the final centroids as above, stored permuted by list, ascending original id
 *                   within a list, every list padded to whole 32-row blocks with zero rows of original id -1 (the layout
 *                   hipivf_create takes).
 * No float atomics: a build is bit-identical from run to run.  Checks: x and out_handle not null, 1 <= n < 2^31,
 * iters >= 0, 1 <= nlist <= the number of training rows, d and metric as for hipidx_create. */
int32_t hipivf_build_dev(const float* x_dev, int64_t n, int32_t d, int32_t metric, int32_t nlist, int32_t iters, uint64_t seed,
                         int64_t max_train_rows, int32_t device, void* stream, uint64_t* out_handle);
/* the same from host memory: copies x to the device, builds, synchronises */
int32_t hipivf_build(const float* x_host, int64_t n, int32_t d, int32_t metric, int32_t nlist, int32_t iters, uint64_t seed,
                     int64_t max_train_rows, int32_t device, void* stream, uint64_t* out_handle);
/* File format "HIPIVF01" (<- faiss.write_index, rag/storage/faiss_index.py:133): magic[8] "HIPIVF01", int32 version (1), d,
 * metric, nlist, int64 n, stored rows; then fp32 centroids [nlist][d], int64 list offsets [nlist + 1], int64 original ids
 * [stored rows], fp32 stored rows [stored rows][d] (padding included).  Little-endian, no gaps. */
int32_t hipivf_save(uint64_t h, const char* path);
/* (<- faiss.read_index, rag/storage/faiss_index.py:54) Rebuilds both flat indexes through the ordinary add path (the bf16
 * filter copy and row statistics are recomputed, as in hipidx_load).  The file is validated first: its size must be what
 * its header implies, offsets ascend on 32-row blocks from 0 to the stored row count, every original id lies in [-1, n)
 * and each of 0..n-1 appears exactly once; otherwise HIPRAG_E_IO / HIPRAG_E_INVALID.  A HIPIDX01 file is refused with a
 * message naming hipidx_load (and hipidx_load refuses this format by its magic). */
int32_t hipivf_load(const char* path, int32_t device, uint64_t* out_handle);
/* centroids as stored, fp32 [nlist][d] (<- index.quantizer.reconstruct_n) */
int32_t hipivf_get_centroids(uint64_t h, float* out_host);
/* list offsets [nlist + 1] and the original id of every stored row [stored rows] (-1 = padding), see hipivf_info */
int32_t hipivf_get_lists(uint64_t h, int64_t* offsets_host, int64_t* orig_ids_host);
/* dimension, metric and the number of original rows n */
int32_t hipivf_meta(uint64_t h, int32_t* out_d, int32_t* out_metric, int64_t* out_n);
/* where a hipivf_build* spent its time, ms of host wall clock: [0] assignment (the k = 1 searches, centroid indexes
 * included), [1] update (sort + sums), [2] final layout (sort, gather, add); zeros for a loaded index */
int32_t hipivf_build_times(uint64_t h, float* out_ms3);
/* ---- IVF-Flat updates: faiss.IndexIVFFlat.add and remove_ids under the trained centroids ---------------------------------------
 * The layout of hipivf_build (lists in list order, ascending original id within a list, every list padded to whole 32-row
 * blocks with zero rows of id -1, padding never ranked) is an INVARIANT of these calls: after any of them the handle is
 * indistinguishable from the layout step of hipivf_build applied to the current rows, in id order, under these centroids --
 * hipivf_get_lists, hipivf_info, hipivf_meta, the bytes of hipivf_save, all three outputs of both searches at any nprobe,
 * and what a later update sees.  The stored bytes of a row (fp32 pieces, bf16 filter copy, norm) are the bytes the ordinary
 * add path produced for it once; an update only moves them.  No float atomics: the same bits from run to run.
 * hipivf_from_centroids  an index of nlist EMPTY lists over the given centroids ([nlist][d] fp32, host): a trained
 *                   faiss.IndexIVFFlat with no rows.  n = 0, no stored rows, every search returns padding only; it saves and
 *                   loads.  The handle owns both flat indexes, as a built one does.  nlist >= 1; d, metric as hipidx_create.
 * hipivf_add_dev    stores n_add more rows (x_dev [n_add, d] fp32 row-major on the index's device, ordered on `stream`) under
 *                   the unchanged centroids.  They get the ids n .. n + n_add - 1 and are assigned as the build assigns: the
 *                   flat index's exact k = 1 search among the centroids, ties to the lower list.  Lists only grow, so every
 *                   stored row stays or moves up; rows before the first list that outgrows its padding are not touched.
 *                   Returns with the index usable (it synchronises `stream`, as the build does).  n_add == 0 is a no-op.
 *                   Batches above 128 MiB of rows are stored in several passes with the same result.
 * hipivf_add        the same from host memory.
 * hipivf_remove_ranges  removes the original ids of n_ranges half-open ranges [lo, hi), ranges_host = {lo0, hi0, lo1, hi1, ..}:
 *                   ascending and non-overlapping within [0, n), the table rules of hipidx_remove_ranges.  Survivors keep
 *                   their order and are renumbered densely (new id = old id minus the ids removed before it), the rule of the
 *                   flat removal, so the index still equals the flat index over the surviving rows at nprobe = nlist.  Lists
 *                   only shrink, every stored row stays or moves down.  Removing every row leaves the hipivf_from_centroids
 *                   state.  Allocations do not shrink.
 * Both updates are synchronous, hold the handle's mutex, and the caller has no search in flight (the contract of
 * hipidx_remove_ranges).  Every check precedes every write: a bad table, a null pointer or n + n_add >= 2^31 give
 * HIPRAG_E_INVALID and the handle is bit for bit what it was.  A handle made by hipivf_create is refused with
 * HIPRAG_E_UNSUPPORTED (the caller owns those rows), and so is a loaded file whose lists are not in the layout above.
 * Device memory beside the index: rows move through a staging buffer that, with the table of moves, stays within 256 MiB
 * whatever n is; a pass of an add also holds its batch sorted by list and tiled (2.5 x the batch, at most 128 MiB of rows).
 * A removal of many ranges runs in passes of about 2^20 / nlist ranges, the last ranges first.
 * hipivf_update_info  out5 = { rows added, rows removed, stored rows moved, staging chunks, extra device bytes (the largest
 *                   pass) } of the last hipivf_add* / hipivf_remove_ranges call; zeros before any. */
int32_t hipivf_from_centroids(const float* centroids_host, int32_t nlist, int32_t d, int32_t metric, int32_t device,
                              uint64_t* out_handle);
int32_t hipivf_add_dev(uint64_t h, const float* x_dev, int64_t n_add, void* stream);
int32_t hipivf_add(uint64_t h, const float* x_host, int64_t n_add);
int32_t hipivf_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges);
int32_t hipivf_update_info(uint64_t h, int64_t* out5);

/* ---- partial top-k merge (multi-GPU: after one all-gather of per-shard partial results) ---------------
 * in_scores64 / in_ids: n_parts blocks of [nq, k_in] (device), block p starting part_stride ELEMENTS after block
 * p-1 (0 = dense, nq*k_in) so both arrays can live interleaved in one all-gathered buffer.
 * Order: better score first (larger for IP, smaller for L2), then the LOWER id; scores compare numerically, so +0.0 and
 * -0.0 tie (the lower id wins) and a zero comes back as +0.0.  An entry with id < 0 is padding WHATEVER its score.  The
 * same (score, id) in two parts is two candidates: duplicates are kept, both are returned.  The place of a NaN score is
 * unspecified.  Ranks past the valid candidates: id -1, -DBL_MAX / -FLT_MAX (IP), DBL_MAX / FLT_MAX (L2).
 * out_scores_dev (the fp32 rounding of out_scores64_dev) may be NULL.  Limits, HIPRAG_E_INVALID otherwise: n_parts >= 1,
 * k_in >= 1, 1 <= k_out < 4096, part_stride 0 or >= nq*k_in, a known metric; nq = 0 returns OK and touches nothing.
 * Elements between the parts (part_stride > nq*k_in) are never read.
 * COST: up to 4096 candidates per query are selected in one pass of k_out rounds; beyond that every further pass takes in
 * only 4096 - k_out new candidates and again runs k_out rounds (~2 us each on an MI355X), so the time grows as
 * k_out * (n_parts*k_in - 4096) / (4096 - k_out).  The library's own callers stay at k_out <= 256 (a millisecond at most);
 * k_out near 4096 with more than 4096 candidates is legal and exact but slow: 9000 candidates at k_out = 4095 take ~40 s.  Tested at every kernel form and size boundary by
 * tests/test_selection_gpu.py.
 * New capability (the reference is single-process); correctness criterion: sharded == unsharded, bit for bit. */
int32_t hiprag_merge_topk_dev(const double* in_scores64_dev, const int64_t* in_ids_dev, int32_t n_parts, int32_t nq,
                              int32_t k_in, int32_t k_out, int64_t part_stride, int32_t metric,
                              double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream);

/* ---- BM25 term-at-a-time sparse scoring (named by the reference's README.md:54-58 and rag/config.py:43-45,
 *      implemented nowhere in it; spec in DESIGN.md) -------------------------------------------------------
 * Postings are CSR over term ids, doc ids ascending inside a list, impacts precomputed in fp32 by the host.
 * score(doc) = sum over query terms IN QUERY ORDER of impact (fp32 adds); docs with score <= 0 are excluded;
 * order (score desc, doc id asc); padding id -1 / score -FLT_MAX. */
int32_t hipbm25_create(int64_t n_docs, int64_t n_terms, const uint64_t* offsets_host, const uint32_t* doc_ids_host,
                       const float* impacts_host, int32_t device, uint64_t* out_handle);
int32_t hipbm25_destroy(uint64_t h);
int32_t hipbm25_set_id_base(uint64_t h, int64_t id_base);
int32_t hipbm25_search(uint64_t h, const uint32_t* term_ids_host, const int32_t* q_offsets_host, int32_t nq, int32_t k,
                       float* out_scores, int64_t* out_ids);
int32_t hipbm25_search_dev(uint64_t h, const uint32_t* term_ids_host, const int32_t* q_offsets_host, int32_t nq,
                           int32_t k, double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev,
                           void* stream);
/* ---- scoped BM25: the postings of the whole collection, per-query document-range scopes ------------------------
 * search_scoped <- the sparse leg of search_by_vector(query_vector, limit, project), rag/storage/faiss_index.py:140,150
 *                  (`project` is accepted and dropped there); hybrid search as README.md:54-58 / rag/config.py:43-45 name it.
 * Scopes in the CSR form of hipidx_search_scoped (ranges_host int64 [n_ranges][2] half-open LOCAL document ranges,
 * scope_offsets_host int32 [n_scopes + 1], scope_of_query_host int32 [nq]; HOST arrays, copied before the call returns).
 * Result for query i: the documents d in a range of its scope with score(d) > 0, ordered (score desc, id asc), first k, where
 * score(d) is the fp32 sum hipbm25_search forms for d -- the COLLECTION's impacts (its N, df and avgdl) in query order: a
 * scope masks documents, it does not change idf.  ids = local id + id_base; padding id -1, -FLT_MAX / -DBL_MAX.  Hence the scope
 * [0, n_docs) gives hipbm25_search_dev's three outputs bit for bit, the scope [lo, hi) those of a handle over the postings of
 * documents lo..hi-1 built with the collection's statistics (id_base lo).
 * Work follows the scope: one workgroup per (query, 9216-document tile that holds a document of its scope), whatever the
 * size of the collection; documents of such a tile outside the scope are masked before anything is selected.
 * Checks, all HIPRAG_E_INVALID before anything is enqueued: those of hipidx_search_scoped_dev with n_docs for ntotal (null
 * tables; nq >= 1; n_scopes >= 1; offsets start at 0 and do not descend; 0 <= lo <= hi <= n_docs; ranges of a scope ascend and
 * do not overlap, touching and empty ones allowed; every scope_of_query in range) and 1 <= k <= 64 (the tiled form's limit:
 * a deeper scoped list does not exist).  ANY number of terms per query; an empty query, unknown or duplicated terms and an
 * empty scope are valid (all padding / as unscoped).  out_scores64_dev and out_scores_dev may be NULL.  The _dev entry enqueues
 * on `stream` and returns without a host synchronisation.  Workspace: (tiles of the chunk's largest scope) x 4 x k x 16
 * bytes per query; the batch is cut into chunks of queries whose candidate lists stay within 512 MiB, a query whose own lists
 * pass 2^20 entries runs as a chunk of its own (a chunk is one query at least): a large scope costs chunks, never an error.
 * Which entry to call: the library does not choose (tools/bench_scoped_hybrid.py reports break_even_share).
 * hipbm25_scoped_info: out4 = { documents per tile (9216), work items (query x tile) of the last scoped call, tiles of its
 * largest scope, its chunks }; it synchronises the device. */
int32_t hipbm25_search_scoped_dev(uint64_t h, const uint32_t* term_ids_host, const int32_t* q_offsets_host, int32_t nq, int32_t k,
                                  const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                  const int32_t* scope_of_query_host, double* out_scores64_dev, float* out_scores_dev,
                                  int64_t* out_ids_dev, void* stream);
/* the same with the two outputs of hipbm25_search in HOST memory: runs on the null stream, synchronises */
int32_t hipbm25_search_scoped(uint64_t h, const uint32_t* term_ids_host, const int32_t* q_offsets_host, int32_t nq, int32_t k,
                              const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                              const int32_t* scope_of_query_host, float* out_scores, int64_t* out_ids);
int32_t hipbm25_scoped_info(uint64_t h, int64_t* out4);
/* ---- weighted sparse search: a weight per QUERY term (learned-sparse queries, BGE-M3's lexical weights) ------------------
 * search_weighted <- the sparse leg of the hybrid search EMBEDDING_MODEL = BAAI/bge-m3 was built for (rag/config.py:9), which
 *                    the reference names (HYBRID_SEARCH_ENABLED / BM25_WEIGHT / VECTOR_WEIGHT, rag/config.py:43-45) and does
 *                    not implement: score(q, d) = sum over shared token ids of qw[t] * dw[t], dw being the handle's impacts.
 * Each entry is the unweighted one plus term_weights_host, float [q_offsets[nq]] parallel to term_ids_host.
 * score(d) = the fp32 sum, IN QUERY-TERM ORDER, of fl32(w_t * impact[t, d]): the product is rounded to fp32, then added (two
 * roundings, never a fused multiply-add).  A term that occurs twice in a query is two slots, each with its own weight.
 * Everything else is the unweighted entry's: documents with score <= 0 excluded, order (score desc, id asc), padding,
 * id_base, the refusal of a dirty handle, the limits on k (1..1000, scoped 1..64), chunking and workspace; the tiled kernel
 * serves k <= 64 and queries of at most 64 terms, the global-accumulator form the rest.  With every weight 1.0f the three
 * outputs are those of the unweighted entry bit for bit.
 * Extra check, HIPRAG_E_INVALID before anything is enqueued: term_weights_host is not null and every weight is finite and
 * > 0 (the kernel's bounds rest on positive contributions; drop a term whose weight is zero). */
int32_t hipbm25_search_weighted(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host,
                                const int32_t* q_offsets_host, int32_t nq, int32_t k, float* out_scores, int64_t* out_ids);
int32_t hipbm25_search_weighted_dev(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host,
                                    const int32_t* q_offsets_host, int32_t nq, int32_t k, double* out_scores64_dev,
                                    float* out_scores_dev, int64_t* out_ids_dev, void* stream);
int32_t hipbm25_search_scoped_weighted(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host,
                                       const int32_t* q_offsets_host, int32_t nq, int32_t k, const int64_t* ranges_host,
                                       const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                       float* out_scores, int64_t* out_ids);
int32_t hipbm25_search_scoped_weighted_dev(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host,
                                           const int32_t* q_offsets_host, int32_t nq, int32_t k, const int64_t* ranges_host,
                                           const int32_t* scope_offsets_host, int32_t n_scopes,
                                           const int32_t* scope_of_query_host, double* out_scores64_dev, float* out_scores_dev,
                                           int64_t* out_ids_dev, void* stream);
/* ---- sparse scores of given documents: hipidx_score_ids for the postings (csrc/bm25_score_ids.hip) ----------------------
 * score_ids <- the "sparse" term of BGE-M3's compute_score (EMBEDDING_MODEL = BAAI/bge-m3, rag/config.py:9; BM25_WEIGHT /
 *              VECTOR_WEIGHT, rag/config.py:44-45): a search scores a document only as a by-product of finding it, so a
 *              candidate the dense leg found has no lexical score unless the top-k list happened to hold it.  This entry
 *              scores ANY (query, document) pair.
 * Queries as in hipbm25_search_weighted (term_ids_host, term_weights_host parallel to it, q_offsets_host int32 [nq + 1]; HOST
 * arrays, copied before the call returns); term_weights_host NULL = plain impacts (every weight 1.0f).
 * ids int64 [nq][depth]: entry (i, j) = c names LOCAL document c - id_base, id_base as set by hipbm25_set_id_base.  It is VALID
 * iff c >= 0 and 0 <= c - id_base < n_docs.  A valid entry gets the fp32 sum, IN QUERY-TERM ORDER, of fl32(w_t * impact[t, d])
 * over the query's slots whose list holds d: the product is rounded to fp32, then the add is rounded, never a fused
 * multiply-add -- THE SAME BITS every hipbm25_search* entry returns for that document and query (a slot whose list does not
 * hold d adds nothing there either), and 0.0f when no slot matches.  An invalid entry is PADDING: nothing is read for it and it
 * gets -FLT_MAX.  The same id twice is two entries; no order of the ids is assumed.  A repeated term is two slots, each with
 * its own weight; a term id >= n_terms matches nothing; an empty query scores 0.0f for every valid entry; a query may have any
 * number of terms.  With weights NULL or all 1.0f the result is the unweighted sum, bit for bit.
 * Checks, all HIPRAG_E_INVALID before anything is enqueued: null pointers (term_ids_host may be NULL when no query has a
 * term); nq >= 1; depth >= 1; nq x depth < 2^31; q_offsets start >= 0 and do not descend; given weights are finite and > 0; a
 * dirty handle (changed and not reweighed) is refused as by every search entry.  Every kind of handle: hipbm25_create,
 * hipbm25_create_tf after a reweigh, hipbm25_create_impacts.
 * The _dev entry stages its slot table (list start, list length, weight per slot) through the handle's pinned ring, enqueues on
 * `stream` and returns without a host synchronisation; it shares the handle's ordering with the searches (a call on another
 * stream than the previous one waits for it on the device).  The host entry copies, runs on the null stream and synchronises.
 * Kernel: a workgroup = one query x up to 64 consecutive entries (4, 8, .. 64 as hipidx_score_ids), the query's slots staged in
 * LDS in passes of 64; one wave per entry at a time, lane = slot: each lane bisects its list's ascending doc ids for d with
 * 4-byte loads and loads the impact on a hit, the wave folds the products of the lanes that hit in ascending lane order into
 * the entry's running sum, which is carried into the next pass.  No skip table is read.  No float atomics, one writer per
 * output, the same bits from run to run.
 * hipbm25_score_info: out4 = { valid entries, padding entries, workgroups launched, posting probes = bisections run = the sum
 * over valid entries of the query's slots with a non-empty list } of the last call (zeros before the first); integer counts,
 * two integer atomics per workgroup, identical from run to run; it synchronises the device. */
int32_t hipbm25_score_ids_dev(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host,
                              const int32_t* q_offsets_host, int32_t nq, const int64_t* ids_dev, int32_t depth,
                              float* out_scores_dev, void* stream);
int32_t hipbm25_score_ids(uint64_t h, const uint32_t* term_ids_host, const float* term_weights_host,
                          const int32_t* q_offsets_host, int32_t nq, const int64_t* ids_host, int32_t depth, float* out_scores);
int32_t hipbm25_score_info(uint64_t h, int64_t* out4);
typedef struct hipbm25_stats {
    int64_t queries;
    int64_t postings_touched; /* sum of df over all query terms so far */
    int64_t bytes_algorithmic; /* 8 B per posting + 2*4*N per query (zero + select read) */
} hipbm25_stats;
int32_t hipbm25_get_stats(uint64_t h, hipbm25_stats* out);

/* ---- updatable BM25 postings: append, remove and reweigh on the device (csrc/bm25_update.hip) ---------------------------
 * An append, a removal or a replacement of documents changes N, df and avgdl, hence EVERY impact.  A handle made by
 * hipbm25_create_tf keeps what impacts are made of -- tf per posting, the length of every document, df in the offsets --
 * and is updated in place; the search entries above go on reading doc_ids and impacts and do not change.
 * DEFINING PROPERTY: after any sequence of create_tf / append / remove_ranges, each followed by reweigh, the handle equals
 * hipbm25_create over hiprag.sparse.build_postings of the surviving documents in order (same term ids, same n_terms), bit
 * for bit: what hipbm25_export gives, and every output of every search and hybrid entry, padding included.
 *   create_tf      postings with term frequencies tf_host (>= 1) and doc_len_host [n_docs]; BM25 parameters k1 >= 0 and
 *                  0 <= b <= 1.  Reweighs itself (NULL-idf semantics, below).
 *   append         n_new_docs documents get the ids n_docs .. n_docs + n_new_docs - 1.  The batch is a CSR over
 *                  n_terms_after >= n_terms terms (new terms extend the vocabulary at the end; n_terms never shrinks) whose
 *                  doc ids are LOCAL to the batch, 0 .. n_new_docs - 1.  Every list becomes the old list followed by the
 *                  batch's.  Capacity grows by half again, so a run of small appends does not reallocate each time.
 *   remove_ranges  ranges_host int64 [n_ranges][2], half-open document ranges under the table rules of hipidx_remove_ranges
 *                  with n_docs for ntotal (0 <= lo <= hi <= n_docs, ascending, not overlapping, touching and empty ones
 *                  allowed).  Stable compaction: the survivors keep their order and are renumbered, a term whose every
 *                  posting went keeps its id with an empty list.  No document to remove: a no-op, the handle stays clean.
 *   reweigh        recomputes every impact and the skip tables: one pass over all postings, in fp64 in the operation order
 *                  of build_postings -- norm = k1*((1 - b) + (b*dl)/avgdl), impact = ((idf*tf)*(k1 + 1))/(tf + norm), rounded
 *                  once to fp32, never contracted into fused multiply-adds; avgdl = (double)(sum of doc_len)/(double)n_docs,
 *                  1.0 for an empty index.  idf_host = the caller's fp64 idf per term [n_terms] (hiprag.sparse passes
 *                  numpy's log(1 + (N - df + 0.5)/(df + 0.5)), which makes the defining property hold by construction); NULL:
 *                  the library evaluates the same expression with the C library's log, and an impact then equals numpy's or
 *                  is the adjacent fp32 value.
 * DIRTY STATE: append and remove_ranges change structure only and leave the handle dirty (a bulk ingest appends many
 * documents and pays for ONE reweigh); every search and hybrid entry on a dirty handle returns HIPRAG_E_INVALID with a
 * message that names hipbm25_reweigh, which clears the state.  id_base is untouched by all of them.
 * CHECKS, all before anything is touched (a refused call leaves the handle bit for bit as it was), HIPRAG_E_INVALID: null
 * pointers; offsets start at 0 and do not descend; every list strictly ascending by doc id; doc id < n_docs (create_tf) or
 * < n_new_docs (a batch); tf >= 1; documents afterwards < 2^32; a list that reaches 2048 postings stays below 2^32; the range
 * table rules; k1, b.  A handle made by plain hipbm25_create has no tf: append, remove_ranges and reweigh return
 * HIPRAG_E_UNSUPPORTED on it.
 * SYNCHRONISATION: the update entries are synchronous, like hipidx_remove_ranges: they take the handle's mutex, run on the
 * null stream and synchronise before they return.  THE CALLER MUST HAVE NO SEARCH IN FLIGHT ON THE HANDLE (a search enqueued
 * on a non-blocking stream reads the buffers an update swaps).  There are no asynchronous (_dev) update entries.
 * hipbm25_export: host copies of offsets [n_terms + 1], doc_ids / tf / impacts [postings] and doc_len [n_docs]; any pointer
 *   may be NULL (tf and doc_len need a create_tf handle); the impacts of a dirty handle are stale.  Test and save hook.
 * hipbm25_sizes: out4 = { n_docs, n_terms, postings, flags: 1 = holds tf, 2 = dirty, 4 = updatable impacts (below) }.
 * hipbm25_update_info: out8, for the last create_tf / append / remove_ranges = { kind (0 none, 1 create_tf, 2 append,
 *   3 remove_ranges), postings before, postings after, postings moved (append: those written at or behind the first
 *   inserted one; remove: the survivors behind the first removed one), documents before, documents after, extra device bytes
 *   the call allocated (temporaries included), 1 if the posting or doc_len buffers grew }.
 * hipbm25_impacts_host: the reweigh kernel's impact formula on the HOST for n postings with PER-POSTING idf, tf and dl: a
 *   test hook that needs no GPU (the operation order is checked against numpy there, the device against both on a GPU). */
int32_t hipbm25_create_tf(int64_t n_docs, int64_t n_terms, const uint64_t* offsets_host, const uint32_t* doc_ids_host,
                          const uint32_t* tf_host, const uint32_t* doc_len_host, double k1, double b, int32_t device,
                          uint64_t* out_handle);
int32_t hipbm25_append(uint64_t h, int64_t n_new_docs, int64_t n_terms_after, const uint64_t* batch_offsets_host,
                       const uint32_t* batch_doc_ids_host, const uint32_t* batch_tf_host, const uint32_t* batch_doc_len_host);
int32_t hipbm25_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges);
int32_t hipbm25_reweigh(uint64_t h, const double* idf_host);
int32_t hipbm25_export(uint64_t h, uint64_t* offsets, uint32_t* doc_ids, uint32_t* tf, float* impacts, uint32_t* doc_len);
int32_t hipbm25_sizes(uint64_t h, int64_t* out4);
int32_t hipbm25_update_info(uint64_t h, int64_t* out8);
int32_t hipbm25_impacts_host(const double* idf, const uint32_t* tf, const uint32_t* dl, int64_t n, double avgdl, double k1,
                             double b, float* out);

/* ---- updatable IMPACT postings: lexical weights that follow their collection on the device (csrc/bm25_impacts.hip) ------
 * Replaces, for BGE-M3's lexical weights (hipenc_forward_lexical), the two host steps a changed collection took: the lexsort
 * of hiprag.lexical.transpose_doc_weights over EVERY row and a new hipbm25_create.  An IMPACT HANDLE is a bm25 handle that
 * keeps impacts as given: no tf, no doc_len.  Such weights do not depend on N, df or avgdl, so an update needs no reweigh,
 * the handle is NEVER dirty and a search right after an append needs no other call; every hipbm25_search*, weighted or
 * scoped, and every hiphybrid_* entry serves it unchanged.
 * DEFINING PROPERTY: after any sequence of create_impacts / append_impacts / append_rows_dev / remove_ranges the handle
 * equals hipbm25_create over transpose_doc_weights of the surviving documents' rows in order (same n_terms), bit for bit:
 * what hipbm25_export gives, and every output of every search and hybrid entry, padding included; the same sequence gives the
 * same bytes from run to run (integer atomics only, and every list they fill is sorted by document afterwards).
 *   create_impacts   what hipbm25_create does, and the handle is updatable.
 *   append_impacts   hipbm25_append with float impacts in place of tf and doc_len: a term-major batch CSR over n_terms_after
 *                    >= n_terms terms with doc ids LOCAL to the batch; every list becomes the old list followed by the batch's.
 *   append_rows_dev  the batch is DOCUMENT-major DEVICE memory, exactly what hipenc_forward_lexical writes: terms_dev int32
 *                    [n_new_docs][row_stride], weights_dev float [n_new_docs][row_stride], counts_dev int32 [n_new_docs]; the
 *                    first counts[i] entries of row i are used, those behind them ignored.  The rows are transposed on the
 *                    device in slices of at most 8192 documents (count per term, scan, place through per-term integer cursors,
 *                    sort every list by document) and merged as append_impacts merges.
 *   hipbm25_remove_ranges  on an impact handle: the table rules and the stable compaction with renumbering of the tf handles;
 *                    the impacts travel with their postings.
 * After every change the skip tables are rebuilt on the device and the document-sized workspaces are dropped.
 * CHECKS, all before anything of the handle is touched (a refused call leaves it bit for bit as it was), HIPRAG_E_INVALID:
 * those of hipbm25_create_tf / hipbm25_append on sizes, offsets, lists and doc ids; every impact finite and > 0; for device
 * rows, in one validation kernel over the whole batch: 0 <= counts[i] <= row_stride, term ids strictly ascending within a row
 * and in [0, n_terms_after), weights finite and > 0 (the refusal names the first offending row and entry).  Documents and
 * list lengths stay below 2^32.  id_base is untouched by all of them.
 * CROSS-REFUSALS, HIPRAG_E_UNSUPPORTED: hipbm25_reweigh and hipbm25_append on an impact handle; append_impacts,
 * append_rows_dev (and, as before, remove_ranges) on a hipbm25_create handle, the two appends on a hipbm25_create_tf handle.
 * SYNCHRONISATION: as the update entries above -- the handle's mutex, the null stream, synchronised on return, NO SEARCH IN
 * FLIGHT ON THE HANDLE.  append_rows_dev first waits for the work already enqueued on `stream` (the forward that writes the
 * rows), as hipmv_append_dev does.
 * hipbm25_export gives offsets, doc_ids and impacts of an impact handle (tf and doc_len: HIPRAG_E_UNSUPPORTED).
 * hipbm25_sizes: flags gain 4 = updatable impacts.  hipbm25_update_info: kinds 4 create_impacts, 5 append_impacts,
 *   6 append_rows_dev (remove_ranges stays 3), the same eight fields; postings moved = those written at or behind the first
 *   inserted one, summed over the slices of a device append; extra bytes include the transposition's temporaries. */
int32_t hipbm25_create_impacts(int64_t n_docs, int64_t n_terms, const uint64_t* offsets_host, const uint32_t* doc_ids_host,
                               const float* impacts_host, int32_t device, uint64_t* out_handle);
int32_t hipbm25_append_impacts(uint64_t h, int64_t n_new_docs, int64_t n_terms_after, const uint64_t* batch_offsets_host,
                               const uint32_t* batch_doc_ids_host, const float* batch_impacts_host);
int32_t hipbm25_append_rows_dev(uint64_t h, const int32_t* terms_dev, const float* weights_dev, const int32_t* counts_dev,
                                int64_t n_new_docs, int64_t row_stride, int64_t n_terms_after, void* stream);

/* ---- reciprocal-rank fusion (README.md:54-58 "hybrid"; weights rag/config.py:44-45) ---------------------
 * s(d) = w_a/(c + rank_a(d)) + w_b/(c + rank_b(d)), ranks 1-based, a missing list contributes +0;
 * IEEE fp32 in exactly that order.  Order: larger s first, then the LOWER id (zeros of either sign tie).  ids < 0 in the
 * inputs are padding (holes anywhere in a list; the ranks of the entries behind a hole still count it).  An id repeated
 * inside a list is ONE document, ranked by its first occurrence; a document whose score is 0 or negative (zero or negative
 * weights) is still ranked.  Ranks past the documents: id -1, -FLT_MAX.  NaN weights or c: unspecified.
 * Limits, HIPRAG_E_INVALID otherwise: depth_a, depth_b >= 0 with depth_a + depth_b <= 4096 (a list of depth 0 may be a NULL
 * pointer), k >= 1 (any k; ranks past the union are padding), c + 1 > 0; nq = 0 returns OK.
 * Tested by tests/test_selection_gpu.py. */
int32_t hiprrf_fuse(const int64_t* ids_a_host, const int64_t* ids_b_host, int32_t nq, int32_t depth_a, int32_t depth_b,
                    int32_t k, float c, float w_a, float w_b, float* out_scores, int64_t* out_ids);
int32_t hiprrf_fuse_dev(const int64_t* ids_a_dev, const int64_t* ids_b_dev, int32_t nq, int32_t depth_a,
                        int32_t depth_b, int32_t k, float c, float w_a, float w_b, float* out_scores_dev,
                        int64_t* out_ids_dev, void* stream);

/* ---- hybrid fast path: one call = dense top-`depth` + BM25 top-`depth` + RRF -> top-k -------------------
 * What rag/query/retriever.py does per query batch with three calls, for hosts that bind the C-ABI directly: host
 * queries and term lists in, fused fp32 scores / ids out; the two result lists never leave the GPU.  Both handles must
 * live on the same device.  Row-sharded serving uses hiphybrid_shard_begin_dev / _end_dev below (the all-gather sits between
 * search and fusion -- ranks are global, so fusion has to follow the merge).
 * The two legs are independent and bound by different things (the dense scan by HBM, BM25 by LDS round trips), so they run
 * BESIDE each other: the dense leg on the device's scan stream (hiprag_scan_stream) with 96 CUs left out of its scan grid,
 * the BM25 leg on the caller's stream, its workgroups filling those CUs, RRF behind both (1M chunks, 256 queries per call:
 * 140-154 k hybrid queries/s against 123-137 k with the legs one after the other; identical results). */
int32_t hiphybrid_search(uint64_t dense_h, uint64_t bm25_h, const float* q_host, const uint32_t* term_ids_host,
                         const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, float c, float w_dense,
                         float w_sparse, float* out_scores, int64_t* out_ids);
/* The same with the queries, the two intermediate lists and the results in device memory, ordered on `stream` (the legs
 * start where `stream` is at the call; the fusion is enqueued on `stream` behind both legs; nothing synchronises).
 * lists_dev: int64 [4][nq][depth] the caller provides = dense fp64 score bits | dense ids | BM25 fp64 score bits | BM25 ids
 * (left there for callers that also want the per-leg lists, rag/query/retriever.py keeps both). */
int32_t hiphybrid_search_dev(uint64_t dense_h, uint64_t bm25_h, const float* q_dev, const uint32_t* term_ids_host,
                             const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, float c, float w_dense,
                             float w_sparse, int64_t* lists_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream);

/* ---- scoped hybrid: hiphybrid_search_dev over the rows / documents of each query's scope ------------------------------
 * What search_by_vector(query_vector, limit, project) (rag/storage/faiss_index.py:140,150) would do in the hybrid mode the
 * reference names (README.md:54-58, rag/config.py:43-45) if `project` were honoured: dense leg = hipidx_search_scoped_dev,
 * sparse leg = hipbm25_search_scoped_dev, RRF behind both.  Row == document: ONE set of scope tables serves both legs, and
 * the dense index's ntotal must equal the postings' n_docs.  Shape rules of hiphybrid_search_dev (depth > 0, k > 0) and
 * depth <= 64, the sparse leg's limit; every other check is that of the two scoped entries; all HIPRAG_E_INVALID before
 * anything is enqueued.  lists_dev as in hiphybrid_search_dev.  The legs run one after the other on `stream` (a scoped leg is
 * short: neither the scan stream nor the spare-CU setting is involved); no host synchronisation. */
int32_t hiphybrid_search_scoped_dev(uint64_t dense_h, uint64_t bm25_h, const float* q_dev, const uint32_t* term_ids_host,
                                    const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, float c, float w_dense,
                                    float w_sparse, const int64_t* ranges_host, const int32_t* scope_offsets_host,
                                    int32_t n_scopes, const int32_t* scope_of_query_host, int64_t* lists_dev,
                                    float* out_scores_dev, int64_t* out_ids_dev, void* stream);
/* the same with host arrays in and out; lists_host (int64 [4][nq][depth], may be NULL) receives the per-leg lists */
int32_t hiphybrid_search_scoped(uint64_t dense_h, uint64_t bm25_h, const float* q_host, const uint32_t* term_ids_host,
                                const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, float c, float w_dense,
                                float w_sparse, const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                const int32_t* scope_of_query_host, int64_t* lists_host, float* out_scores, int64_t* out_ids);
/* ---- scoped hybrid over the IVF index: hiphybrid_search_scoped* with the dense leg replaced by
 * hipivf_search_scoped_probe_dev(ivf_h, q, nq, depth, nprobe, probe_mode, ...) -- the approximate dense leg of a deployment
 * that serves its collection from the IVF companion.  The sparse leg, RRF, the depth <= 64 limit and lists_dev are
 * unchanged; hipivf_meta's n must equal the postings' n_docs (a row must be a document); every other check is that of the
 * two legs, all before anything is enqueued.  The legs run in stream order on `stream`; no host synchronisation (but see
 * the first PROBE_SCOPE call of a handle above).  At nprobe >= nlist (PROBE_SCOPE: >= the member lists of the scope) the
 * result is hiphybrid_search_scoped_dev's on a flat index of the same rows. */
int32_t hiphybrid_search_ivf_scoped_dev(uint64_t ivf_h, uint64_t bm25_h, const float* q_dev, const uint32_t* term_ids_host,
                                        const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, int32_t nprobe,
                                        int32_t probe_mode, float c, float w_dense, float w_sparse, const int64_t* ranges_host,
                                        const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                        int64_t* lists_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream);
/* the same with host arrays in and out; lists_host (int64 [4][nq][depth], may be NULL) receives the per-leg lists */
int32_t hiphybrid_search_ivf_scoped(uint64_t ivf_h, uint64_t bm25_h, const float* q_host, const uint32_t* term_ids_host,
                                    const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, int32_t nprobe,
                                    int32_t probe_mode, float c, float w_dense, float w_sparse, const int64_t* ranges_host,
                                    const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                    int64_t* lists_host, float* out_scores, int64_t* out_ids);

/* ---- row-sharded hybrid step: the two halves around the caller's ONE all-gather (SURVEY 8b `hiphybrid_search(...)`, 8e) ----
 * One process per GPU holds the rows AND the postings of one contiguous document range (hipidx_set_id_base /
 * hipbm25_set_id_base make the ids global).  A batch is
 *   hiphybrid_shard_begin_dev   local dense top-`depth` + local BM25 top-`depth` -> pack_dev, int64 [2 legs][2][nq][depth]
 *                               (leg 0 dense, leg 1 BM25; [0] = fp64 score bits, [1] = ids).  The index scan is enqueued on
 *                               scan_stream (callers chain their scans there), everything after it on tail_stream, ordered
 *                               behind the scan by a library-owned event; `slot` (0..7) as in hipidx_search_begin_dev.
 *                               scratch_f32_dev: 2 * nq * depth floats.  For the tails to run BESIDE the next scan, pass
 *                               the device's scan stream (hiprag_scan_stream) and leave the tails CUs
 *                               (hipidx_set_spare_cus(dense_h, 96)): see hipidx_set_spare_cus and hiphybrid_search.

 *   (caller)                    all-gather of pack_dev over the ranks -> gathered_dev [n_parts][2][2][nq][depth]: RCCL, MPI,
 *                               whatever the host has; 4 * nq * depth * 8 bytes per rank
 *   hiphybrid_shard_end_dev     each leg merged over the parts with the canonical comparator (better score, then lower id),
 *                               RRF over the two GLOBAL lists -> out_scores_dev / out_ids_dev [nq][k], identical on every rank.
 *                               scratch_dev: 4 * nq * depth int64.
 * hiprag/sharded.py (ShardedHybrid) is one client of these two calls; a host without Python needs nothing else.
 * The reference is a single CPU process (rag/storage/faiss_index.py:83, rag/Dockerfile:23-26): new capability. */
int32_t hiphybrid_shard_begin_dev(uint64_t dense_h, uint64_t bm25_h, const float* q_dev, const uint32_t* term_ids_host,
                                  const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t slot, int64_t* pack_dev,
                                  float* scratch_f32_dev, void* scan_stream, void* tail_stream);
int32_t hiphybrid_shard_end_dev(const int64_t* gathered_dev, int32_t n_parts, int32_t nq, int32_t depth, int32_t k,
                                int32_t dense_metric, float c, float w_dense, float w_sparse, int64_t* scratch_dev,
                                float* out_scores_dev, int64_t* out_ids_dev, void* stream);

/* ---- batch encoder: XLM-RoBERTa-large architecture (BGE-M3 embeddings, bge-reranker-v2-m3 cross-encoder) ---------
 * forward     <- HuggingFaceEmbeddings.embed_query / embed_documents (sentence-transformers encode, CLS pooling,
 *                normalize_embeddings=True)            rag/providers/hf/embeddings.py:32-35,54,77
 * score_pairs <- the cross-encoder the reference only configures (RERANKER_MODEL)      rag/config.py:25-27
 * Weights are DEVICE pointers owned by the caller (torch tensors) and must outlive the handle: matrices bf16 in
 * torch.nn.Linear layout [out, in]; biases and LayerNorm parameters fp32.  Token ids / lengths are HOST arrays
 * ([nseq, max_len] int32, right-padded; lengths include BOS/EOS).  Outputs are DEVICE fp32: forward -> [nseq, hidden]
 * L2-normalised CLS embeddings (zeros for length-0 rows); score_pairs -> [nseq] logits.
 * Batches of at most HIPENC_SMALL_ROWS (environment, read at create; default 384, 0 = never) padded token rows -- one
 * query through embed_single, a few short texts -- run the GEMMs as weight-streaming workgroups instead of 128 x 128
 * tiles (1.3 ms instead of 3.3 ms for one query on the 24-layer model); same arithmetic, fixed summation order. */
typedef struct hipenc_config {
    int32_t vocab, hidden, layers, heads, ffn, max_pos, pad_id;
    float ln_eps;
} hipenc_config;
typedef struct hipenc_layer_weights {
    const void *wqkv, *bqkv;     /* [3H, H] bf16 = cat(query, key, value).weight; [3H] f32 */
    const void *wo, *bo;         /* attention.output.dense */
    const void *ln1_g, *ln1_b;   /* attention.output.LayerNorm */
    const void *w1, *b1;         /* intermediate.dense [F, H] */
    const void *w2, *b2;         /* output.dense [H, F] */
    const void *ln2_g, *ln2_b;   /* output.LayerNorm */
} hipenc_layer_weights;
typedef struct hipenc_weights {
    const void *word_emb, *pos_emb, *type_emb;   /* [V,H], [max_pos,H], [H] (row 0 of token_type_embeddings) bf16 */
    const void *emb_ln_g, *emb_ln_b;             /* f32 */
    const hipenc_layer_weights* layers;          /* host array of `layers` entries */
    const void *cls_dense_w, *cls_dense_b, *cls_out_w, *cls_out_b; /* optional head: [H,H] bf16, [H] f32, [H] bf16, [1] f32 */
} hipenc_weights;
int32_t hipenc_create(const hipenc_config* cfg, const hipenc_weights* weights, int32_t device, uint64_t* out_handle);
int32_t hipenc_destroy(uint64_t h);
int32_t hipenc_forward(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq,
                       int32_t max_len, float* out_dev, void* stream);
int32_t hipenc_score_pairs(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq,
                           int32_t max_len, float* out_logits_dev, void* stream);
/* One linear layer of the encoder in isolation: C = A[M,K] * W[N,K]^T with the fused epilogue the encoder uses at that place
 * (0 = QKV: bias, q scaled by 1/8, head-major q / k into out / out_k and TRANSPOSED v into out_vt; 1 = bias + exact-erf GELU
 * -> bf16 [M,N]; 2 = bias + bf16 residual -> f32 [M,N]; 3 = the same sum rounded to bf16 [M,N], the pre-LayerNorm
 * form of the big-batch path).  All pointers are device memory.  impl 0 picks the kernel the way
 * hipenc_forward does, 1 forces 128 x 128 tiles, 2 the persistent 256 x 256 tiles.  For kernel tests and benchmarks
 * (tests/test_encoder_gpu.py, tools/bench_gemm.py): the nn.Linear calls inside sentence-transformers' forward
 * (rag/providers/hf/embeddings.py:54,77) are what it stands for. */
int32_t hipenc_linear(const void* a_dev, const void* w_dev, const float* bias_dev, int32_t M, int32_t N, int32_t K,
                      int32_t epilogue, const void* resid_dev, void* out_dev, void* out_k_dev, void* out_vt_dev, int32_t S,
                      int32_t heads, int32_t impl, void* stream);
/* hipenc_linear_ex: hipenc_linear (which is a thin call into it) plus what the kernel tests need.  Test hook only.
 *   epilogue 4   raw fp32 partial products, no bias: out = f32 [splits][m_valid][N], split s holding the product over
 *                K range [s K / splits, (s + 1) K / splits).  impl 1 takes `ksplit` in 1..4 (K a multiple of ksplit * 64);
 *                impl 3 picks splits = ceil(K / 1024) itself (pass ksplit 0).  *out_splits (may be NULL) receives the count.
 *   impl 3       the small-batch (weight-streaming) kernel, launched as hipenc_forward launches it; epilogues 0, 1 and 4.
 *                M a multiple of 64, N of 16, K / ceil(K / 1024) a multiple of 128; epilogues 0 and 1 need K <= 1024.
 *                Every row is a real row on this path: m_valid must equal M.
 *   m_valid      <= M, a multiple of 64: rows >= m_valid are GEMM padding (hipenc_forward's rows beyond nseq * S) and are
 *                NOT written; A, the residual and the outputs still have M rows.  The residual epilogues of the 256-tile
 *                kernel (2 and 3 under impl 2) never mask rows -- hipenc_forward gives them whole tiles -- and are refused
 *                unless m_valid = M.
 *   max_workgroups  impl 2 only: the persistent grid is min(tiles, CUs, max_workgroups); 0 = no cap.  The kernel's tile
 *                order puts no condition on the grid: a grid that is a multiple of 8 walks the XCD order, any other
 *                the plain order, and both visit every tile exactly once.
 * hipenc_layernorm runs one of the encoder's three LayerNorm kernels on the grid hipenc_forward uses:
 *   form 0  x f32 [M, H] -> y bf16 [M, H];
 *   form 1  x f32 [nsplit][M][H] partials (nsplit in 1..4), summed in split order, + bias f32 [H] + resid bf16 [M, H];
 *   form 2  x bf16 [M, H] (four rows per wave), H <= 1024.
 * H is a multiple of 128, at most 2048.  Rows >= M of y are not written. */
int32_t hipenc_linear_ex(const void* a_dev, const void* w_dev, const float* bias_dev, int32_t M, int32_t N, int32_t K,
                         int32_t epilogue, const void* resid_dev, void* out_dev, void* out_k_dev, void* out_vt_dev, int32_t S,
                         int32_t heads, int32_t impl, int32_t m_valid, int32_t ksplit, int32_t max_workgroups,
                         int32_t* out_splits, void* stream);
int32_t hipenc_layernorm(const void* x_dev, const float* gamma_dev, const float* beta_dev, void* y_dev, int32_t M, int32_t H,
                         float eps, int32_t form, int32_t nsplit, const float* bias_dev, const void* resid_dev, void* stream);
/* Test and bench hooks, like hipenc_linear; no product path calls them.
 * hipenc_attention runs the attention kernel alone, through the launch helper hipenc_forward uses.  All pointers are
 * device memory: q, k bf16 [nseq, heads, S, 64] (q already carries the 1/8 scale), vt bf16 [nseq, heads, 64, S] (V
 * transposed), lens int32 [nseq], ctx bf16 [nseq * S, heads * 64].  ctx is zero-filled on the stream first, as the
 * forward does: rows of 128-query tiles that lie wholly at or beyond a sequence's length stay zero; padding rows inside a
 * processed tile hold unspecified finite values.  Keys at positions >= len never contribute.  S is a positive multiple
 * of 64.  PRECONDITION, not checked (the lengths live on the device): 0 <= lens[i] <= S for every sequence.
 * hipenc_forward_hidden takes hipenc_forward's arguments and writes the last hidden state of EVERY token row instead
 * of the pooled CLS row: bf16 [nseq, S, hidden] with S = max_len rounded up to 64 -- the final activation buffer
 * copied out as the kernels left it (rows at positions >= len are unspecified). */
int32_t hipenc_attention(const void* q_dev, const void* k_dev, const void* vt_dev, const int32_t* lens_dev, void* ctx_dev,
                         int32_t nseq, int32_t S, int32_t heads, void* stream);
int32_t hipenc_forward_hidden(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq,
                              int32_t max_len, void* out_hidden_dev, void* stream);
int32_t hipenc_last_flops(uint64_t h, double* out_flops); /* algorithmic FLOPs of the last forward */
/* The forward's policy, for tests and tools (csrc/encoder_plan.h): which GEMM family a batch takes and how its N = hidden
 * products split K is a pure function of a shape and the batch's nseq x S rows (S = max_len rounded up to 64).  hipenc_shape
 * gives the shape a handle has; hipenc_forward_plan is arithmetic alone -- no handle, no device, callable on a machine
 * without a GPU -- and is what hipenc_forward itself asks.  Checks: hidden and ffn as hipenc_create wants them, n_cu, nseq
 * positive, S a positive multiple of 64.  (The two types end in _t because C keeps functions and typedef names in one
 * name space.) */
#define HIPENC_PATH_SMALL 0 /* weight-streaming GEMMs, fp32 partials summed by the LayerNorm */
#define HIPENC_PATH_BIG   1 /* persistent 256 x 256 tiles, bf16 pre-LayerNorm rows */
#define HIPENC_PATH_TILED 2 /* 128 x 128 tiles; a product whose split is > 1 writes partials the LayerNorm sums */
typedef struct hipenc_shape_t {
    int32_t hidden, ffn; /* of hipenc_config */
    int32_t n_cu;        /* CUs of the device */
    int32_t small_rows;  /* HIPENC_SMALL_ROWS as read at creation (default 384; <= 0: never the small-batch path) */
    int32_t use256;      /* HIPENC_GEMM256 as read at creation (default 1; 0: never the 256-tile path) */
} hipenc_shape_t;
typedef struct hipenc_plan_t {
    int32_t T;           /* token rows, nseq * S */
    int32_t M;           /* rows the GEMMs run over: T padded to whole tiles */
    int32_t path;        /* HIPENC_PATH_* */
    int32_t osplit;      /* tiled path: K split of the out-projection; 1 on the other paths */
    int32_t dsplit;      /* tiled path: K split of FFN-down; 1 on the other paths */
    int32_t fsplit;      /* ceil(ffn / 1024): the partials of the small path's FFN-down */
    int32_t head_split;  /* partials of the ColBERT head's product on this path */
    int64_t pre_bytes;   /* size of the pre-LayerNorm workspace */
} hipenc_plan_t;
int32_t hipenc_forward_plan(const hipenc_shape_t* shape, int32_t nseq, int32_t S, hipenc_plan_t* out);
int32_t hipenc_shape(uint64_t h, hipenc_shape_t* out);
/* ---- packed batches (csrc/encoder_packed.h): no GEMM row for a sequence's padding up to the batch's longest ------------
 * The padded entries above run every GEMM of every layer over nseq x S rows, S = the batch's longest rounded up to 64.  A
 * PACKED batch gives sequence i of length len_i only R_i = len_i rounded up to 64 rows (none if len_i = 0), starting at
 * row_off[i], the prefix sum of the R_i; Tp = row_off[nseq] rows in all.  Rows [len_i, R_i) are padding exactly as in the
 * padded layout (zeros from the embedding, keys masked).  The GEMM family depends on the row count alone:
 * hipenc_forward_plan(shape, 1, Tp) is the plan of a packed batch.
 * BATCH FORMAT: tokens_host holds the sequences one after another with no padding, sequence i = tokens[offsets[i] ..
 * offsets[i + 1]), offsets_host int32 [nseq + 1].
 *   hipenc_forward_packed         out_dev f32 [nseq][hidden]: L2-normalised CLS rows, zeros for empty sequences
 *   hipenc_score_pairs_packed     out_logits_dev f32 [nseq]; every sequence has at least one token
 *   hipenc_forward_hidden_packed  test hook: bf16 [offsets[nseq]][hidden], the REAL rows only, in order
 * THE CONTRACT: let P1 = hipenc_forward_plan(shape, nseq, S) be the plan of a padded batch that holds a sequence and P2 =
 * hipenc_forward_plan(shape, 1, Tp) that of a packed batch that holds it.  If P1 and P2 agree in path, osplit and dsplit,
 * the sequence's real hidden rows, its embedding and its logit are THE SAME BITS from both entries ("Packed
 * batches", has the argument); otherwise they differ by what two padded batches on different paths differ by.  A packed
 * result does not depend on which other sequences share the batch, as long as the plan is the same.
 * CHECKS, HIPRAG_E_INVALID before anything is enqueued: null pointers; nseq >= 0 (nseq = 0 returns HIPRAG_OK); offsets start
 * at 0 and do not descend; every id in [0, vocab); longest + pad_id + 1 < max_pos; Tp < 2^30; score_pairs_packed: every
 * length >= 1 and a classification head.  A batch whose sequences are all empty writes zeros and launches no GEMM.
 * Staging is hipenc_forward's (two asynchronous copies, one synchronise), the workspace is the handle's own, so the
 * caller-ordering rule of the padded entries holds unchanged.  hipenc_last_flops counts the real rows in the GEMM term and
 * the sum of 4 R_i^2 hidden per layer in the attention term.
 * THE LEXICAL AND ColBERT HEADS STAY PADDED-ONLY: hipenc_forward_lexical and hipenc_forward_colbert have no packed form.
 *   hipenc_packed_layout   arithmetic alone, like hipenc_forward_plan (no handle, no device): out_counts = { Tp, n_items };
 *                          out_row_off int32 [nseq + 1], out_gran_seq int32 [Tp / 64] (the sequence that owns each 64-row
 *                          granule) and out_items int32 [n_items][2] -- the attention work list (sequence, 128-query tile
 *                          j) for every 128 j < len, in sequence order -- may each be NULL (ask for the counts first).
 *   hipenc_packed_info     out4 = { Tp, real tokens, sequences, HIPENC_PATH_* (-1: no GEMM ran) } of the last packed forward.
 *   hipenc_attention_packed  test hook, the launch helper the packed forward uses: q, k bf16 [heads][Tp][64], vt bf16
 *                          [heads][64][Tp], row_off [nseq + 1], lens [nseq], items [n_items][2] as hipenc_packed_layout
 *                          gives them, all on the device; ctx bf16 [Tp][heads * 64] is zero-filled first.  A 128-query
 *                          tile of a sequence with 64 or 192 rows overhangs into the next sequence or past Tp: those
 *                          rows are never written by it.  PRECONDITION, not checked: the tables are a layout's. */
int32_t hipenc_forward_packed(uint64_t h, const int32_t* tokens_host, const int32_t* offsets_host, int32_t nseq, float* out_dev,
                              void* stream);
int32_t hipenc_score_pairs_packed(uint64_t h, const int32_t* tokens_host, const int32_t* offsets_host, int32_t nseq,
                                  float* out_logits_dev, void* stream);
int32_t hipenc_forward_hidden_packed(uint64_t h, const int32_t* tokens_host, const int32_t* offsets_host, int32_t nseq,
                                     void* out_hidden_dev, void* stream);
int32_t hipenc_packed_layout(const int32_t* lens_host, int32_t nseq, int32_t* out_row_off, int32_t* out_gran_seq,
                             int32_t* out_items, int32_t* out_counts);
int32_t hipenc_packed_info(uint64_t h, int64_t* out4);
int32_t hipenc_attention_packed(const void* q_dev, const void* k_dev, const void* vt_dev, const int32_t* row_off_dev,
                                const int32_t* lens_dev, const int32_t* items_dev, int32_t n_items, int32_t nseq, int32_t Tp,
                                int32_t heads, void* ctx_dev, void* stream);
/* ---- lexical head: BGE-M3's per-token lexical weights from the forward that makes the embedding ------------------------
 * forward_lexical <- the sparse output of EMBEDDING_MODEL = BAAI/bge-m3 (rag/config.py:9): relu(sparse_linear(last hidden
 *                    state)), kept per distinct token id as the maximum over its positions -- the model's side of the
 *                    hybrid search the reference names and does not implement (rag/config.py:43-45).
 * hipenc_set_lexical_head: w_dev bf16 [hidden] (sparse_linear.weight) and b_dev f32 [1] are the caller's DEVICE memory and
 * must outlive the handle, like every other weight; the n_unused (0..16) unused token ids -- BGE-M3's are bos, pad, eos and
 * unk -- are copied.  A second call replaces the head.  hipenc_create and hipenc_weights know nothing of it.
 * hipenc_forward_lexical runs ONE forward and writes
 *   out_dense_dev    [nseq][hidden], exactly what hipenc_forward writes for the same batch (the same kernel); may be NULL;
 *   out_terms_dev /  [nseq][max_len] (row stride max_len, not the padded length): the first out_counts_dev[i] entries of row
 *   out_weights_dev  i are the distinct token ids of sequence i that are not unused and whose weight is > 0, in ASCENDING id
 *                    order, each with the maximum of w_t over its positions; the entries behind are -1 / 0.0f;
 *   out_counts_dev   [nseq]; 0 for an empty sequence.
 * Token weight of position t < len: w_t = max(0, fl32(dot_t + b)), dot_t = the fp32 sum of the `hidden` products of the bf16
 * hidden row and the bf16 weight vector (each product is exact in fp32).  SUMMATION ORDER: lane l of a 64-lane wave adds
 * the products of columns l, l + 64, l + 128, .. in ascending order; the 64 partial sums are then combined by a butterfly
 * over lane distances 32, 16, 8, 4, 2, 1 (v[l] = v[l] + v[l ^ distance]); hiprag.lexical.lexical_reference is this in numpy.
 * No float atomics, the same bits from run to run, no host synchronisation beyond hipenc_forward's own (token staging).
 * Checks, HIPRAG_E_INVALID before anything is enqueued: those of hipenc_forward; null outputs (except out_dense_dev); no head
 * set; n_unused outside 0..16.  max_len > 2048 gives HIPRAG_E_UNSUPPORTED (ids and weights of a sequence live in LDS); the
 * drop-in provider caps sequences at 512 tokens. */
int32_t hipenc_set_lexical_head(uint64_t h, const void* w_dev, const float* b_dev, const int32_t* unused_ids_host,
                                int32_t n_unused);
int32_t hipenc_forward_lexical(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq,
                               int32_t max_len, float* out_dense_dev, int32_t* out_terms_dev, float* out_weights_dev,
                               int32_t* out_counts_dev, void* stream);

/* ---- BGE-M3 multi-vector (ColBERT) head (csrc/encoder_heads.h) ---------------------------------------------------------------
 * The third output of the reference's model (BAAI/bge-m3, rag/config.py:9): one unit vector per token, scored by late
 * interaction (hipmaxsim_* below), a second stage beside the cross-encoder of rag/config.py:25-27.
 *   hipenc_set_colbert_head  w_dev bf16 [hidden][hidden] in nn.Linear layout (colbert_linear.weight), b_dev f32 [hidden]:
 *                    caller-owned device memory that must outlive the handle.  A second call replaces the head;
 *                    hipenc_create knows nothing of it.
 *   hipenc_forward_colbert   ONE forward; it writes
 *     out_dense_dev   [nseq][hidden] f32, exactly what hipenc_forward writes for the same batch (the same kernel); may be NULL;
 *     out_counts_dev  [nseq] int32 = max(0, len_i - 1);
 *     out_vecs_dev    bf16 [nseq][max_len - 1][hidden]: row p < counts[i] of sequence i is the vector of token position
 *                     p + 1 -- CLS is skipped and EOS is kept, as FlagEmbedding's _colbert does with
 *                     last_hidden_state[:, 1:]; the rows at and behind counts[i] are zero.
 * ONE VECTOR: c[n] = the fp32 accumulation over hidden of the exact bf16 x bf16 products of the hidden row and W[n, :], in
 * the order of the GEMM kernel the batch size selects (the raw-partials form of the small-batch kernel or of the 128 x 128
 * tiles; a split K dimension is added in split order); v[n] = c[n] + b[n]; ss = the sum of v[n]^2, lane l of a 64-lane wave
 * adding columns l, l + 64, .. in ascending order (square and add rounded separately), then the butterfly of the lexical
 * head above; inv = 1.f / fmaxf(sqrtf(ss), 1e-12f); y[n] = bf16(v[n] * inv), round to nearest even.
 * hiprag.colbert.colbert_reference is this in numpy.  No float atomics, the same bits from run to run.
 * Checks, HIPRAG_E_INVALID before anything is enqueued: those of hipenc_forward; null out_vecs_dev or out_counts_dev; no head
 * set; max_len < 2.
 *   hipenc_colbert_rows      a test hook, as hipenc_attention and hipenc_layernorm are: the head alone (product and
 *                    normalisation through the launches the forward uses, on the path forward takes at nseq x S rows) on
 *                    rows x_dev bf16 [nseq x S][H] the caller supplies, S a multiple of 64, 1 <= row_stride <= S - 1,
 *                    out_vecs_dev bf16 [nseq][row_stride][H].  It synchronises `stream`. */
int32_t hipenc_set_colbert_head(uint64_t h, const void* w_dev, const float* b_dev);
int32_t hipenc_forward_colbert(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq,
                               int32_t max_len, float* out_dense_dev, void* out_vecs_dev, int32_t* out_counts_dev,
                               void* stream);
int32_t hipenc_colbert_rows(const void* x_dev, const int32_t* lens_dev, int32_t nseq, int32_t S, const void* w_dev,
                            const float* b_dev, int32_t H, void* out_vecs_dev, int32_t* out_counts_dev, int32_t row_stride,
                            void* stream);

/* ---- all three BGE-M3 outputs from ONE forward ----------------------------------------------------------------------------
 * forward_m3 <- FlagEmbedding's encode(return_dense, return_sparse, return_colbert_vecs) for EMBEDDING_MODEL = BAAI/bge-m3
 *               (rag/config.py:9): the three heads read the same last hidden state, so one 24-layer forward serves them.
 * CONTRACT: out_dense_dev (may be NULL), out_terms_dev / out_weights_dev / out_lex_counts_dev and out_vecs_dev /
 * out_col_counts_dev are, BIT FOR BIT, what hipenc_forward, hipenc_forward_lexical and hipenc_forward_colbert write for the
 * same batch, in their layouts ([nseq][hidden]; [nseq][max_len] x 2 and [nseq]; bf16 [nseq][max_len - 1][hidden] and [nseq]).
 * After the layers it runs the launches of the three entries one after the other on `stream`: every head reads the hidden
 * rows and none writes them, and the ColBERT head's partials go to the pre-LayerNorm buffer, which no other head touches.
 * Checks, HIPRAG_E_INVALID before anything is enqueued: the union of those entries' -- those of hipenc_forward; null outputs
 * (except out_dense_dev); BOTH heads set; max_len >= 2; max_len > 2048 gives HIPRAG_E_UNSUPPORTED.  Padded batches only. */
int32_t hipenc_forward_m3(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq, int32_t max_len,
                          float* out_dense_dev, int32_t* out_terms_dev, float* out_weights_dev, int32_t* out_lex_counts_dev,
                          void* out_vecs_dev, int32_t* out_col_counts_dev, void* stream);

/* ---- passage token store (csrc/token_store.hip): the token ids of every chunk of a collection, on the device -----------
 * Stands for the passage half of the cross-encoder input the reference only configures (rag/config.py:25-27): the ingest
 * tokenises every chunk once for its embedding (rag/providers/hf/embeddings.py:77), and the rerank call below reads those
 * ids instead of tokenising the candidates of every query again.  A CSR, document i = collection row i, BODIES only (no
 * bos / eos).  It is the fourth structure that follows a collection, after rows, IVF lists and postings, under the same rules.
 * Its offsets, growth and removal are the document CSR of csrc/doc_store.hip, which the multi-vector store shares.
 *   create         max_doc_tokens >= 1 is the cap per stored passage: a longer one keeps its first max_doc_tokens tokens (a
 *                  pair of at most 512 tokens never reads more than 508).  bos, eos, pad lie in [0, vocab).
 *   append         tokens_host int32, offsets_host int64 [n_docs + 1]; the new documents get the ids n .. n + n_docs - 1.
 *                  Empty documents are valid.  Capacity grows by half again.
 *   remove_ranges  stable compaction under the table rules of hipidx_remove_ranges.  The tokens move on the device through a
 *                  staging buffer of at most 128 MiB; tokens in front of the first removed document are neither read nor
 *                  written.  Afterwards hiptok_export equals that of a fresh store of the survivors, bit for bit.
 * CHECKS, all before anything is touched (a refused call leaves the handle bit for bit as it was), HIPRAG_E_INVALID: null
 * pointers; offsets start at 0 and do not descend; every id (those behind the cap included) lies in [0, vocab); the document
 * count afterwards is < 2^31; the range table rules.  HIPRAG_E_NOMEM (no room to grow) leaves the handle as it was too.
 * SYNCHRONISATION: append and remove_ranges are synchronous (null stream, the handle's mutex), and THE CALLER MUST HAVE NO
 * CALL IN FLIGHT ON THE HANDLE, as for hipidx_remove_ranges.
 *   export         host copies of offsets [n + 1] and tokens [stored tokens]; either may be NULL.  A test hook.
 *   sizes          out4 = { documents, stored tokens, max_doc_tokens, longest stored document }.
 * The lengths are kept on the host as well (4 bytes per document), so that the sequence length of a rerank call needs no
 * device read.  hiprag_shutdown drops live stores like every other handle. */
int32_t hiptok_create(int32_t vocab, int32_t bos, int32_t eos, int32_t pad, int32_t max_doc_tokens, int32_t device,
                      uint64_t* out_handle);
int32_t hiptok_destroy(uint64_t h);
int32_t hiptok_append(uint64_t h, const int32_t* tokens_host, const int64_t* offsets_host, int64_t n_docs);
int32_t hiptok_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges);
int32_t hiptok_export(uint64_t h, int64_t* offsets, int32_t* tokens);
int32_t hiptok_sizes(uint64_t h, int64_t* out4);

/* ---- rerank on the device (csrc/rerank.hip): the cross-encoder the reference only configures, rag/config.py:25-27 -------
 * (RERANKER_ENABLED, RERANKER_TOP_K, RERANKER_MODEL).  One call scores nq x depth (query, candidate) pairs with the
 * encoder's classification head and returns the best k of every query.  The candidate ids stay on the device, where
 * hiphybrid_search*_dev left them; the passages come from a token store.
 * THE PAIR RULE: q and p token bodies, L = max_len, room = max(0, L - 4):
 *     pair(q, p, L) = [bos] + q[:room] + [eos, eos] + p[:max(0, room - len(q[:room]))] + [eos]
 * CANDIDATES: c names stored document c - id_base.  c < 0 and every c outside [id_base, id_base + n_docs) is PADDING: its
 * row is never read, it is assembled as the 4-token pair of an empty query and an empty passage (no row of the encoder
 * batch is empty), its logit is reported as -FLT_MAX and it is counted (info).  The same document twice is two candidates.
 * SEQUENCE LENGTH: S = min(max_len, 4 + longest query of the call + longest stored document) rounded up to 64; the host
 * entry, which holds the ids, takes the longest document AMONG THE CALL'S VALID CANDIDATES instead.  One kernel writes
 * tokens [pairs][S] (pad behind each length) and lens [pairs] into the encoder's own buffers, in (query, position) order;
 * the forward runs from there with no host staging and no host synchronisation, max(1, max_batch_tokens / S) consecutive
 * pairs at a time (max_batch_tokens 0 = 131072), every sub-batch at the one S.
 * SELECTION: one kernel orders each query's valid candidates by (logit descending, position ascending) and writes the first
 * k: id, logit, position in the candidate list; ranks past the valid candidates get id -1, -FLT_MAX, position -1.  The
 * place of a NaN logit is unspecified.
 * CHECKS, HIPRAG_E_INVALID before anything is enqueued: null pointers (out_logits_dev and out_pos_dev may be NULL); nq >= 1;
 * 1 <= k <= depth <= 256; id_base >= 0; max_len >= 5 and max_len + pad_id + 1 < max_pos (hipenc_forward's rule);
 * q_offsets_host int32 [nq + 1] starts at 0 and does not descend, every query id lies in [0, the encoder's vocab); the
 * store's vocab <= the encoder's and its pad equals the encoder's pad_id; the encoder has a head; both handles live on one device.
 * ORDERING: the query arrays are copied before the call returns (as the scope tables of hipidx_search_scoped_dev are); the
 * call enqueues on `stream` and returns.  Lock order: encoder, then store.  CALLS ON ONE ENCODER HANDLE SHARE ITS
 * WORKSPACE -- these and hipenc_forward / hipenc_score_pairs alike -- AND MUST BE ORDERED BY THE CALLER (one stream, or
 * events between streams); so must calls on one store, whose query buffer they share.
 * There is no entry that takes token ids on the device: ids index the embedding table unchecked, and here every id was
 * range-checked by hiptok_append or, for the queries, by this call.
 *   hiprerank_host  candidates and outputs in HOST memory: copies, runs on the null stream, synchronises.
 *   hiprerank_info  out4 = { pairs assembled for valid candidates, candidates treated as padding, S, sub-batches } of the last
 *                   call on the store; it synchronises the device.
 *   hiprerank_assemble  a test hook: the assembly kernel alone, no encoder (query ids are checked against the store's
 *                   vocab).  S is the store-wide bound of hiprerank_dev and is returned in *out_S; out_tokens_host holds
 *                   [nq * depth][S] ints, which is at most nq * depth * (max_len rounded up to 64). */
int32_t hiprerank_dev(uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                      const int64_t* cand_ids_dev, int32_t depth, int64_t id_base, int32_t max_len, int32_t k,
                      int64_t max_batch_tokens, float* out_logits_dev, float* out_scores_dev, int64_t* out_ids_dev,
                      int32_t* out_pos_dev, void* stream);
int32_t hiprerank_host(uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                       const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t max_len, int32_t k,
                  int64_t max_batch_tokens, float* out_logits, float* out_scores, int64_t* out_ids, int32_t* out_pos);
int32_t hiprerank_info(uint64_t tok_h, int64_t* out4);
int32_t hiprerank_assemble(uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                           const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t max_len,
                           int32_t* out_tokens_host, int32_t* out_lens_host, int32_t* out_S);
/* ---- packed device rerank: every pair costs its OWN length rounded up to 64, not the store's longest document -----------
 * hiprerank_dev cannot sort its pairs by length (ids and lengths are on the device), so it pads every pair to the store-wide
 * S: one 500-token passage anywhere in a collection makes every pair of every later call cost 512 rows.  The packed entries
 * take the arguments of hiprerank_dev / hiprerank_host, apply the same checks and the same pair rule, run the same selection
 * kernel, and score the pairs through the encoder's packed forward (hipenc_score_pairs_packed's layout) instead:
 *   1. a kernel writes the length of every pair (the pair rule's arithmetic; a padding slot is the 4-token pair);
 *   2. ONE COPY TO PINNED HOST MEMORY AND ONE SYNCHRONISE OF `stream` FOLLOW: the packed entry trades hiprerank_dev's "no
 *      host synchronisation" for rows.  Everything enqueued on `stream` before the call has completed when it returns;
 *   3. the host lays the pairs out and cuts them, IN ORDER, GREEDILY into sub-batches: a sub-batch takes the next pair while
 *      its packed rows (every length rounded up to 64) stay <= max_batch_tokens (0 = 131072); it holds at least one pair;
 *   4. one upload of the tables; a kernel writes every pair's tokens at its rows, `pad` in the granule tails; the packed
 *      forward runs per sub-batch from those device tokens; the selection kernel of hiprerank_dev orders the candidates.
 * CONTRACT: the logits are the bits hipenc_score_pairs_packed gives for the pairs of each sub-batch.  Against hiprerank_dev
 * they differ as two padded batches on different paths do (the contract of the packed forward above).
 * One more check than hiprerank_dev: nq * depth * (max_len rounded up to 64) < 2^31.
 *   hiprerank_packed_host  candidates and outputs in HOST memory, as hiprerank_host; the same layout as the device entry (the
 *                   ids on the host give no tighter bound any more), so its results are the device entry's bit for bit.
 *   hiprerank_packed_info  out4 = { pairs of valid candidates, padding slots, packed rows of the call, sub-batches } of the
 *                   last packed call on the store; it synchronises the device.
 *   hiprerank_assemble_packed  a test hook: steps 1 to 4 without the encoder, ONE layout over all the pairs.  out_tokens_host
 *                   holds *out_Tp <= nq * depth * (max_len rounded up to 64) ints, out_row_off_host nq * depth + 1,
 *                   out_lens_host nq * depth. */
int32_t hiprerank_packed_dev(uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                             const int64_t* cand_ids_dev, int32_t depth, int64_t id_base, int32_t max_len, int32_t k,
                             int64_t max_batch_tokens, float* out_logits_dev, float* out_scores_dev, int64_t* out_ids_dev,
                             int32_t* out_pos_dev, void* stream);
int32_t hiprerank_packed_host(uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                              const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t max_len, int32_t k,
                              int64_t max_batch_tokens, float* out_logits, float* out_scores, int64_t* out_ids, int32_t* out_pos);
int32_t hiprerank_packed_info(uint64_t tok_h, int64_t* out4);
int32_t hiprerank_assemble_packed(uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                                  const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t max_len,
                                  int32_t* out_tokens_host, int32_t* out_row_off_host, int32_t* out_lens_host, int32_t* out_Tp);

/* ---- multi-vector store (csrc/multivec.hip): the per-token vectors of every chunk of a collection, on the device -------
 * The reference's model, BAAI/bge-m3 (rag/config.py:9), has three outputs; the third is one vector per token (the ColBERT
 * output), scored by late interaction below.  A CSR, document i = collection row i: offsets int64 [docs + 1], vecs bf16
 * [stored vectors][dim].  It is the sixth structure that follows a collection, after rows, IVF lists, postings, passage
 * tokens and pages, under the rules of the token store.
 * SIZE: 2 x dim bytes per stored token.  100 k passages of 120 tokens at 1024-d take 24.6 GB; 1 M passages take 245 GB and
 * do not fit beside the index; the fp8 format below stores dim + 4 bytes per token (12.3 GB and 123 GB), the MXFP4 format
 * below it dim / 2 + dim / 32 (544 bytes at 1024-d: 6.5 GB and 65 GB).
 *   create         dim is a multiple of 64 and at most 1024.  max_doc_vectors >= 1 is a cap: a longer document keeps its
 *                  first max_doc_vectors vectors.
 *   append_dev     vecs_dev bf16 [n_docs][row_stride][dim] in device memory (16-byte aligned), produced on `stream`;
 *                  counts_host int32 [n_docs], 0 <= count <= row_stride.  The call waits for `stream`, one kernel packs the
 *                  first min(count, cap) rows of every document behind the stored ones, and it returns with the store usable.
 *   append         the same from packed host memory: vecs_host bf16 [offsets_host[n_docs]][dim], offsets_host int64
 *                  [n_docs + 1].  Empty documents are valid in both forms.  Capacity grows by half again.
 *   remove_ranges  stable compaction under the table rules of hipidx_remove_ranges.  The vectors move on the device through
 *                  the bounded staging of hiptok_remove_ranges (one mover for both, a vector is dim / 2 of its words);
 *                  nothing in front of the first removed document is read or written.  Afterwards hipmv_export equals that
 *                  of a fresh store of the survivors, bit for bit.
 *   save / load    "HIPMV001", little-endian, no gaps: char magic[8], int32 version (1), int32 dim, int32 max_doc_vectors,
 *                  int64 documents, int64 stored vectors, the offsets, the vectors.  These vectors cannot be rebuilt without
 *                  encoding the collection again, which is why this store has a file and the token store has none.  The load
 *                  checks the header, the file's size and every offset (start at 0, no descent, no document above the cap,
 *                  end at the vector count) before it allocates; a bad file gives HIPRAG_E_IO.
 *   export         host copies of offsets [docs + 1] and vecs [stored vectors][dim]; either may be NULL.  A test hook.
 *   sizes          out4 = { documents, stored vectors, dim, longest stored document }.
 * CHECKS, all before anything is touched (a refused call leaves the handle bit for bit as it was), HIPRAG_E_INVALID: null
 * pointers; counts within [0, row_stride]; offsets start at 0 and do not descend; the document count afterwards is < 2^31;
 * the range table rules.  HIPRAG_E_NOMEM (no room to grow) leaves the handle as it was too.
 * SYNCHRONISATION: that of the token store -- updates are synchronous (null stream, the handle's mutex) and THE CALLER MUST
 * HAVE NO CALL IN FLIGHT ON THE HANDLE.  hiprag_shutdown drops live stores like every other handle. */
int32_t hipmv_create(int32_t dim, int32_t max_doc_vectors, int32_t device, uint64_t* out_handle);
int32_t hipmv_destroy(uint64_t h);
int32_t hipmv_append_dev(uint64_t h, const void* vecs_dev, int32_t row_stride, const int32_t* counts_host, int64_t n_docs,
                         void* stream);
int32_t hipmv_append(uint64_t h, const void* vecs_host, const int64_t* offsets_host, int64_t n_docs);
int32_t hipmv_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges);
int32_t hipmv_save(uint64_t h, const char* path);
int32_t hipmv_load(const char* path, int32_t device, uint64_t* out_handle);
int32_t hipmv_export(uint64_t h, int64_t* offsets, void* vecs);
int32_t hipmv_sizes(uint64_t h, int64_t* out4);

/* ---- the fp8 format of the multi-vector store (csrc/multivec.hip, the specification: csrc/multivec.h) ----------------
 * A store has one format, fixed at creation: 0 = bf16 (everything above, unchanged), 4 = MXFP4 (the next section) or 1 = fp8: OCP e4m3fn codes
 * uint8 [stored vectors][dim] and one power-of-two fp32 scale per vector, dim + 4 bytes per stored token instead of 2 x dim
 * (1 M passages of 120 tokens at 1024-d: 123 GB instead of 245 GB).  fp8 needs dim % 128 == 0, 128..1024.
 * QUANTISATION of a vector v (hiprag.colbert.fp8_quantize_reference restates it): amax = max |v_k|; amax == 0 gives codes
 * 0x00 and scale 1.0; a non-finite component or amax outside [2^-60, 2^60] stores the zero vector with scale 1.0 and is
 * counted; otherwise e = 7 - floor(log2 amax), code_k = e4m3fn(v_k * 2^e) rounded to nearest even (never saturating), a
 * -0 code stored as 0x00, scale = 2^-e.  code * scale is exact in bf16.
 * IDENTITY: hipmaxsim_* over an fp8 store gives, bit for bit, what it gives over a bf16 store holding the dequantised
 * vectors (hipmv_export of the fp8 store): the fp8 kernel feeds the same MFMA the same values in the same order.
 *   create_ex      hipmv_create with a format; hipmv_create is format 0.
 *   append_dev / append / remove_ranges / sizes / destroy   the same calls with the same bf16 inputs on either format; on an
 *                  fp8 store one kernel packs and quantises in one pass (both append forms give the same bytes), and a
 *                  removal moves codes (dim / 4 words a vector) and scales (one word) with the same run plan.
 *   export         on an fp8 store: the dequantised bf16 bits.
 *   export_fp8     host copies of offsets, codes [stored vectors][dim] and scales [stored vectors]; any may be NULL.
 *                  HIPRAG_E_INVALID on a bf16 store.
 *   format_info    out4 = { format, bytes per stored vector, vectors stored as zero by the domain guard since creation, 0 }.
 *   to_fp8         a NEW fp8 store from a bf16 one (same dim, cap and device), byte for byte a fresh fp8 store given the same
 *                  vectors; the source is untouched.  HIPRAG_E_INVALID on an fp8 store or a dim that fp8 does not take.
 *   save / load    an fp8 store's file is "HIPMVQ81": char magic[8], int32 version (1), int32 dim, int32 max_doc_vectors,
 *                  int32 format (1), int64 documents, int64 stored vectors, the offsets, the scales, the codes.  hipmv_load
 *                  tells the two kinds by their magic.  Before a handle exists it checks the header, the size, the offsets,
 *                  every scale (a positive power of two of the domain, or 1.0) and, in one streaming device pass, that no
 *                  code is a NaN pattern ((b & 0x7F) == 0x7F); a bad file gives HIPRAG_E_IO. */
int32_t hipmv_create_ex(int32_t dim, int32_t max_doc_vectors, int32_t device, int32_t format, uint64_t* out_handle);
int32_t hipmv_export_fp8(uint64_t h, int64_t* offsets, void* codes, float* scales);
int32_t hipmv_format_info(uint64_t h, int64_t* out4);
int32_t hipmv_to_fp8(uint64_t h, uint64_t* out_handle);

/* ---- the MXFP4 format of the multi-vector store (csrc/multivec.hip, the specification: csrc/multivec.h) --------------
 * Format 4 (bits per element; 2 and 3 are no formats): OCP microscaling FP4, e2m1 codes with one e8m0 scale per block of 32
 * consecutive components.  It needs dim % 128 == 0, 128..1024.  Per stored vector: codes uint8 [dim / 2], component 2i in
 * the low nibble of byte i and 2i + 1 in the high one, a nibble = sign | 2 exponent bits | 1 mantissa bit (magnitudes 0,
 * 0.5, 1, 1.5, 2, 3, 4, 6); scales uint8 [dim / 32], byte s meaning 2^(s - 127).  dim / 2 + dim / 32 bytes per stored token:
 * 544 at 1024-d, 0.266 of bf16 and 0.529 of fp8 (1 M passages of 120 tokens: 65 GB).
 * QUANTISATION of a vector v (hiprag.colbert.mxfp4_quantize_reference restates it): the vector guard of fp8 -- a non-finite
 * component or amax outside [2^-60, 2^60] stores the zero vector (codes 0x0, scale bytes 127) and is counted; amax == 0
 * gives the zero vector uncounted.  Otherwise per block: bmax == 0 gives codes 0 and scale byte 127; else
 * E = max(floor(log2 bmax) - 2, -100), read off bmax's exponent bits, scale byte = E + 127 (so 27..185), code_k =
 * e2m1(v_k * 2^-E) rounded to nearest, ties to the even mantissa, SATURATING at +-6 (the OCP MX rule: the scaled block
 * maximum lies in [4, 8)), a -0 code stored as 0x0.  code * 2^E is exact in bf16.  |v - deq| <= max(|v| / 4, 2^(E - 2)).
 * IDENTITY: hipmaxsim_* over an MXFP4 store gives, bit for bit, what it gives over a bf16 store of hipmv_export of it.
 *   append_dev / append / remove_ranges / sizes / destroy / export / format_info   as on an fp8 store: one kernel packs and
 *                  quantises, both append forms give the same bytes, a removal moves codes (dim / 8 words a vector) and
 *                  scales (dim / 128 words), export gives the dequantised bf16 bits, format_info { 4, dim / 2 + dim / 32,
 *                  guarded, 0 }.
 *   export_mxfp4   host copies of offsets, codes [stored vectors][dim / 2] and scales [stored vectors][dim / 32]; any may be
 *                  NULL.  HIPRAG_E_INVALID on another format, as hipmv_export_fp8 is on an MXFP4 store.
 *   to_mxfp4       a NEW MXFP4 store from a bf16 one, byte for byte a fresh MXFP4 store given the same vectors; the source is
 *                  untouched.  HIPRAG_E_INVALID on an fp8 or MXFP4 source (no second quantisation; hipmv_to_fp8 refuses an
 *                  MXFP4 source likewise) or a dim the format does not take.
 *   save / load    the file is "HIPMVQ41": HIPMVQ81's header with format = 4, then the offsets, the scales, the codes.
 *                  hipmv_load tells the three kinds by their magic; before a handle exists it checks the header, the size,
 *                  the offsets, that every scale byte is in [27, 185] and, in one streaming device pass, that no nibble is
 *                  0x8; a bad file gives HIPRAG_E_IO. */
int32_t hipmv_export_mxfp4(uint64_t h, int64_t* offsets, void* codes, void* scales);
int32_t hipmv_to_mxfp4(uint64_t h, uint64_t* out_handle);

/* ---- late interaction on the device (csrc/maxsim.hip): MaxSim over a multi-vector store -------------------------------
 * BGE-M3's colbert_score without a temperature: a second stage beside the cross-encoder the reference configures
 * (rag/config.py:25-27) that runs no forward per pair.  It mirrors hiprerank_dev: candidate ids still on the device, one
 * call, no host staging, the host waits for nothing.
 * INPUTS: q_vecs_dev bf16 [nq][q_stride][dim] (16-byte aligned) and q_counts_dev int32 [nq]; a count is clamped to
 * [0, q_stride] in the kernel.  dim is the store's.
 * CANDIDATES: c names stored document c - id_base.  c < 0, c - id_base outside [0, documents), a document with no stored
 * vector and every candidate of a query with no vector are PADDING: nothing of theirs is read, the pair score is -FLT_MAX
 * and they are counted (info).  The same id twice is two candidates.
 * SCORE of a valid pair, Lq query vectors q_i and Ld document vectors d_j:
 *     s_ij = the fp32 sum over dim of the bf16 products (exact in fp32), in one fixed order: k in chunks of 64 ascending,
 *            in a chunk one v_mfma_f32_32x32x16_bf16 step after the other, each step adding k = 64c + 32h + 8t .. + 7 for
 *            h = 0, 1 to the running value;
 *     m_i  = max_j s_ij;       score = (float)((the fp64 sum of m_i in ascending i) / (double)Lq).
 * The bits of a pair's score depend on its two vector sets alone: not on the candidate's position, on depth, nq or k, or on
 * what else is in the call.  No float atomics; the same bits from run to run.
 * OUTPUTS: out_pair_scores_dev [nq][depth] in candidate order (may be NULL); out_scores_dev, out_ids_dev, out_pos_dev
 * [nq][k] (out_pos_dev may be NULL): the valid candidates by (score descending, position ascending); ranks past them get
 * id -1, -FLT_MAX, position -1 -- hiprerank_dev's rules.
 * CHECKS, HIPRAG_E_INVALID before anything is enqueued: null pointers (except out_pair_scores_dev and out_pos_dev); nq >= 1;
 * 1 <= k <= depth <= 256; 1 <= q_stride <= 512; nq x depth < 2^31; id_base >= 0.
 * One workgroup per pair: up to 32 query vectors in LDS (64.5 KiB at 1024-d), four waves of 32 document vectors each against
 * them; a query of more than 32 vectors walks its tiles in turn and reads the document again.  Calls on one store share its
 * counters and, when out_pair_scores_dev is NULL, its score buffer: order them (one stream, or events between streams).
 *   hipmaxsim_host  every array in HOST memory: copies, runs on the null stream, synchronises.
 *   hipmaxsim_info  out4 = { valid pairs, padding candidates, document vectors read = the sum over valid pairs of
 *                   Ld x ceil(Lq / 32), 0 } of the last call on the store; it synchronises the device. */
int32_t hipmaxsim_dev(uint64_t mv_h, const void* q_vecs_dev, const int32_t* q_counts_dev, int32_t q_stride, int32_t nq,
                      const int64_t* cand_ids_dev, int32_t depth, int64_t id_base, int32_t k, float* out_pair_scores_dev,
                      float* out_scores_dev, int64_t* out_ids_dev, int32_t* out_pos_dev, void* stream);
int32_t hipmaxsim_host(uint64_t mv_h, const void* q_vecs_host, const int32_t* q_counts_host, int32_t q_stride, int32_t nq,
                       const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t k, float* out_pair_scores,
                       float* out_scores, int64_t* out_ids, int32_t* out_pos);
int32_t hipmaxsim_info(uint64_t mv_h, int64_t* out4);

/* ---- BGE-M3's combined score of candidate ids that are still on the device (csrc/lib.cpp, csrc/m3_score.hip) ------------
 * m3_score <- FlagEmbedding's compute_score "dense + sparse + colbert" for EMBEDDING_MODEL = BAAI/bge-m3 (rag/config.py:9);
 *             BM25_WEIGHT / VECTOR_WEIGHT (rag/config.py:44-45) are the reference's own hint at a weighted SCORE fusion, which
 *             it does not implement.  The hiphybrid_* entries fuse RANKS (RRF); this one fuses scores.
 * HANDLES: dense_h (a flat index) is always required: it defines the rows and the id_base.  bm25_h, when its leg runs, must
 * carry the same id_base and n_docs = ntotal; mv_h, when its leg runs, must hold ntotal documents (and id_base must be >= 0,
 * hipmaxsim_dev's rule); otherwise HIPRAG_E_INVALID.  A leg whose weight is 0 is NOT RUN: its handle and query arguments may
 * be 0 / NULL.  Weights (double) are finite and >= 0 and at least one is > 0.
 * COMPONENTS: candidate (i, j) = c is VALID iff it is valid for hipidx_score_ids (c >= 0, 0 <= c - id_base < ntotal).  The
 * components are exactly what the existing entries give the pair, because this call calls them, in stream order:
 * hipidx_score_ids_dev (q_dev f32 [nq][d]), hipbm25_score_ids_dev (term_ids_host / term_weights_host, may be NULL /
 * q_offsets_host) and hipmaxsim_dev's pair scores (q_vecs_dev bf16 [nq][q_stride][dim], q_counts_dev int32 [nq]).
 *   s_d = the fp64 dense score: on an IP index as it is; on an L2 index s_d = 1.0 - 0.5 * dist, the inner product of UNIT
 *         vectors -- which BGE-M3's embeddings are; on rows that are not unit vectors it is merely a decreasing map of dist;
 *   s_s = the fp32 sparse score widened to fp64;
 *   s_c = the fp32 MaxSim score widened to fp64; where the MaxSim pair is padding (a document or a query without vectors) the
 *         ColBERT term counts as 0.0, not as -FLT_MAX.
 * combined = (((w_d * s_d) + (w_s * s_s)) + (w_c * s_c)) / W in fp64, in that order, every operation rounded on its own (no
 * contraction); the terms of legs that were not run are left out, not multiplied by zero; W = (w_d + w_s) + w_c, formed on
 * the host.
 * OUTPUTS: out_parts_dev f32 [nq][depth][3] (may be NULL): per candidate the fp32 outputs of the three entries as they wrote
 * them -- hipidx_score_ids' out_scores (on an L2 index the squared distance, before the mapping above), the sparse score, the
 * MaxSim pair score; padding values included -- and 0.0f for a leg that was not run.  out_pair_scores_dev double [nq][depth]
 * (may be NULL): combined in candidate order, -DBL_MAX for an invalid candidate.  out_scores_dev double [nq][k], out_ids_dev
 * int64 [nq][k], out_pos_dev int32 [nq][k] (may be NULL): the valid candidates by (combined descending, position ascending);
 * ranks past them get id -1, -DBL_MAX, position -1 -- hiprerank_dev's rules.  The same id twice is two candidates.
 * CHECKS, HIPRAG_E_INVALID: nq >= 1; 1 <= k <= depth <= 256; the weights; null cand_ids / out_scores / out_ids; the query
 * arguments of every leg that runs; 1 <= q_stride <= 512; the handles' agreement above; then each leg's own checks as it is
 * reached (a leg that refuses leaves the outputs unspecified).
 * One small kernel behind the legs combines and ranks, one workgroup per query.  Workspace: one buffer per device,
 * nq x depth x 20 + nq x k x 12 bytes, grown on demand; calls on different streams are ordered on the device.  Lock order: the
 * workspace, then one handle at a time (dense, postings, store), never two handles at once -- as the hiphybrid_* entries.
 *   hipm3_score_host  every array in HOST memory: copies, runs on the null stream, synchronises. */
int32_t hipm3_score_dev(uint64_t dense_h, uint64_t bm25_h, uint64_t mv_h, const float* q_dev, const uint32_t* term_ids_host,
                        const float* term_weights_host, const int32_t* q_offsets_host, const void* q_vecs_dev,
                        const int32_t* q_counts_dev, int32_t q_stride, int32_t nq, const int64_t* cand_ids_dev, int32_t depth,
                        int32_t k, double w_dense, double w_sparse, double w_colbert, float* out_parts_dev,
                        double* out_pair_scores_dev, double* out_scores_dev, int64_t* out_ids_dev, int32_t* out_pos_dev,
                        void* stream);
int32_t hipm3_score_host(uint64_t dense_h, uint64_t bm25_h, uint64_t mv_h, const float* q_host, const uint32_t* term_ids_host,
                         const float* term_weights_host, const int32_t* q_offsets_host, const void* q_vecs_host,
                         const int32_t* q_counts_host, int32_t q_stride, int32_t nq, const int64_t* cand_ids_host, int32_t depth,
                         int32_t k, double w_dense, double w_sparse, double w_colbert, float* out_parts, double* out_pair_scores,
                         double* out_scores, int64_t* out_ids, int32_t* out_pos);

/* ---- late-interaction SEARCH (csrc/maxsim_search.hip): the exact MaxSim top k over every document of a scope -----------
 * search_scoped <- search_by_vector(query_vector, limit, project), rag/storage/faiss_index.py:140 (`project` is accepted and
 *                  dropped at :150), for the sixth structure of a collection: the multi-vector store as a FIRST stage.  A
 *                  passage whose pooled vector is mediocre never reaches a second stage; this entry ranks every document of
 *                  the project by its token vectors.  Brute force over the scope; hipmaxsim_search_pruned* below generates
 *                  candidates from centroid codes first.
 * INPUTS: the queries of hipmaxsim_dev (q_vecs_dev bf16 [nq][q_stride][dim], 16-byte aligned; q_counts_dev int32 [nq] on
 * the device, clamped to [0, q_stride] in the kernel; 1 <= q_stride <= 512).  Scopes in the CSR form of
 * hipidx_search_scoped_dev (ranges_host int64 [n_ranges][2] half-open LOCAL DOCUMENT ranges of the store, document i =
 * collection row i; scope_offsets_host int32 [n_scopes + 1]; scope_of_query_host int32 [nq]; HOST arrays, copied before the
 * call returns), under that entry's rules with the store's document count for ntotal.
 * RESULT for query i: the documents of its scope that hold at least one stored vector, by (MaxSim score descending, id
 * ascending), first k; out_ids = local document + id_base; ranks past them id -1 and -FLT_MAX; a query with no vector gets
 * all padding.  1 <= k <= 256.
 * BITS: the score of a (query, document) pair is THE SAME BITS hipmaxsim_dev gives that pair (SCORE above: the same MFMA,
 * the same k order per accumulator, max over j, the fp64 sum of the maxima in ascending i, divided by Lq, rounded to float),
 * and IDENTITY extends to this entry: on an fp8 store the result is that on a bf16 store of the dequantised vectors.  A
 * query's row does not depend on the other queries or scopes of the call, on nq, or on how the call is cut into chunks.
 * No float atomics; the same bytes from run to run.
 * CHECKS, all HIPRAG_E_INVALID before anything is enqueued: those of hipidx_search_scoped_dev (null pointers; nq >= 1;
 * n_scopes >= 1; offsets start at 0 and do not descend; 0 <= lo <= hi <= documents; the ranges of a scope ascend and do not
 * overlap, touching and empty ones allowed; every scope_of_query in range), 1 <= k <= 256, 1 <= q_stride <= 512, the
 * alignment of q_vecs, 0 <= id_base < 2^62.  The _dev entry enqueues on `stream` and returns without a host synchronisation.
 * WORK: one item = (scope, slice of 16 consecutive documents on absolute document boundaries, group of up to 8 of the
 * queries that name the scope); the group's query vectors are packed into R = 32 T rows of LDS (T = 2 at 1024-d, up to 4
 * below 640-d), a group of more rows passes over the slice ceil(rows / R) times; every slice leaves min(k, 16) entries per
 * query, merged by hiprag_merge_topk_dev.  Partial lists beyond 512 MiB cut the call into chunks of queries.  Calls on one
 * store share its workspace: order them (one stream, or events between streams).
 *   hipmaxsim_search_scoped  q_vecs, q_counts and both outputs in HOST memory: copies, runs on the null stream, synchronises.
 *   hipmaxsim_search_info    out8 = { valid pairs, padding pairs (a query without vectors or a document without vectors, in
 *                            scope), document vectors read = the sum over work items of passes x stored vectors of the
 *                            item's in-scope documents, R = query rows per pass, G = queries per work item, documents per
 *                            slice, chunks, work items } of the last search on the store; slots 3 to 5 are properties of
 *                            the build and the store's dim.  It synchronises the device. */
int32_t hipmaxsim_search_scoped_dev(uint64_t mv_h, const void* q_vecs_dev, const int32_t* q_counts_dev, int32_t q_stride,
                                    int32_t nq, int32_t k, const int64_t* ranges_host, const int32_t* scope_offsets_host,
                                    int32_t n_scopes, const int32_t* scope_of_query_host, int64_t id_base,
                                    float* out_scores_dev, int64_t* out_ids_dev, void* stream);
int32_t hipmaxsim_search_scoped(uint64_t mv_h, const void* q_vecs_host, const int32_t* q_counts_host, int32_t q_stride,
                                int32_t nq, int32_t k, const int64_t* ranges_host, const int32_t* scope_offsets_host,
                                int32_t n_scopes, const int32_t* scope_of_query_host, int64_t id_base, float* out_scores,
                                int64_t* out_ids);
int32_t hipmaxsim_search_info(uint64_t mv_h, int64_t* out8);

/* ---- centroid codes and the PRUNED late-interaction search (csrc/maxsim_codes.hip) ---------------------------------------
 * The candidate generation the brute-force entry above lacks, in the manner of PLAID (ColBERTv2's engine): every stored token
 * vector carries the id of its nearest centroid (its CODE), a query is scored against the centroids once, every document of
 * the scope is scored from its codes alone, and only the best ncand documents reach the exact kernel.  Opt-in: a store
 * without centroids, and every entry above, behaves exactly as before.
 * s(a, b): the fp32 value the MaxSim kernels form for a pair of vectors -- v_mfma_f32_32x32x16_bf16 with the k order of
 * csrc/maxsim_docs.h; a product does not care which vector is which operand.
 *   hipmv_attach_centroids  keeps a device copy of centroids_bf16_host, bf16 bits [ncent][dim], and computes the code of every
 *                           vector already stored; ncent % 32 == 0 and 32 <= ncent <= 65536, HIPRAG_E_INVALID otherwise with
 *                           the store as it was.  Attaching again replaces the table and codes every vector anew.
 *                           CODE: code(v) = the LOWEST c that maximises s(v, centroid_c), v the STORED vector (on an fp8 or
 *                           MXFP4 store the dequantised value).  ROLES in the kernel: the centroid table lies in LDS, 64 rows
 *                           at a time, and the stored vectors stream through the format's own operand path, a workgroup
 *                           keeping its 128 vectors while it walks the whole table: the store is read once whatever ncent is.
 *                           The codes are one more per-vector array of the store, int32 at the vectors' own offsets: they grow
 *                           and move with them.  hipmv_append and hipmv_append_dev code the new vectors in the same call, after
 *                           quantisation, so attaching after appending and appending after attaching give the same codes, and
 *                           after hipmv_remove_ranges the codes are those of a fresh store of the surviving documents.
 *                           hipmv_save / hipmv_load do not change: a loaded store is unattached (codes are recomputed from the
 *                           vectors and the table); hipmv_to_fp8 / hipmv_to_mxfp4 return an unattached store.
 *   hipmv_detach_centroids  drops table and codes; detaching an unattached store is no error.
 *   hipmv_export_centroids  out_bf16 [ncent][dim];   hipmv_export_codes  out_codes_i32 [stored vectors], in store order;
 *                           both HIPRAG_E_UNSUPPORTED on an unattached store.
 *   hipmv_centroid_info     out4 = { ncent (0: unattached), coded vectors, bytes of codes, 0 }.
 *   hipmv_gather_f32_dev    out_f32_dev [n][dim] (device) = the stored vectors item_idx_host[0 .. n) (host, GLOBAL vector
 *                           indices in store order, each in 0 .. stored - 1, checked before anything is written), dequantised
 *                           and widened to float: the sample centroid training takes of a store too large to export.  Runs on
 *                           the null stream and synchronises it.
 *
 * hipmaxsim_search_pruned_dev / hipmaxsim_search_pruned take the arguments of hipmaxsim_search_scoped[_dev] and ncand, and
 * optionally give the candidates: out_cand_ids int64 [nq][ncand] and out_cand_scores float [nq][ncand] (either may be NULL).
 * THREE STAGES on the caller's stream, the _dev form without a host synchronisation:
 *   table        T[q][c][i] = s(q_i, centroid_c) in fp32: the query's vectors in the LDS (query) role, the centroid table
 *                read as maxsim's kernel reads a document, hence the bits hipmaxsim_dev would give that pair.  Stored
 *                [c][q_stride rounded up to 32]: the Lq values of one code are contiguous.
 *   interaction  for every document of the query's scope that holds a vector: m_i = max_j T[code_j][i], approx =
 *                (float)((fp64 sum of m_i in ascending i) / Lq) -- hipmaxsim's reduction with every document vector replaced
 *                by its centroid.  Work items, scope tables, the counting sort of the queries by scope, partial lists and
 *                hiprag_merge_topk_dev are those of hipmaxsim_search_scoped_dev; one item = (scope, slice of 256 consecutive
 *                documents on absolute boundaries -- HIPRAG_MAXSIM_CODE_SLICE, a build constant -- group of up to 8 queries
 *                naming the scope), one wave per (query, document), lanes over i.  CANDIDATES: the in-scope documents that
 *                hold a vector by (approx descending, id ascending), first ncand; a document without vectors is never one; a
 *                query without vectors gets all padding (id -1, -FLT_MAX).  No float atomics, one writer per slot.
 *   exact        the candidates go to hipmaxsim_dev's kernel in ASCENDING ID order, padding last, so ties in the exact score
 *                break by id as in hipmaxsim_search_scoped.  RESULT: first k by (score descending, id ascending); ranks past
 *                them id -1 and -FLT_MAX.
 * Partial lists plus table beyond 512 MiB cut the call into chunks of queries (HIPRAG_PRUNED_BUDGET, bytes, read at every
 * call, overrides the 512 MiB: a test hook).
 * CONTRACT: (a) every returned score is the bits hipmaxsim_dev gives that pair.  (b) If ncand >= the number of in-scope
 * documents that hold a vector, the result equals hipmaxsim_search_scoped's bit for bit.  (c) out_cand_ids and
 * out_cand_scores equal hipmaxsim_search_scoped with k = ncand over a bf16 store whose every vector is replaced by its
 * centroid.  (d) A query's rows do not depend on the other queries or scopes of the call, on nq, or on the chunks.  (e) The
 * three store formats differ only through their stored values.  The same bytes from run to run.
 * CHECKS, all before anything is enqueued: those of hipmaxsim_search_scoped_dev, 1 <= k <= ncand <= 256, nq x ncand < 2^31
 * (HIPRAG_E_INVALID); a store without centroids is HIPRAG_E_UNSUPPORTED.  Calls on one store share its workspace: order them.
 *   hipmaxsim_pruned_info   out8 = { valid and padding (query, document) pairs of the interaction stage, codes read, bytes of
 *                           the query table of a chunk, chunks, work items (the bound of the call), pairs the exact stage
 *                           scored, documents per slice } of the last pruned search on the store.  It synchronises the device.
 * New capability (the reference ranks pooled vectors only). */
int32_t hipmv_attach_centroids(uint64_t mv_h, const void* centroids_bf16_host, int32_t ncent);
int32_t hipmv_detach_centroids(uint64_t mv_h);
int32_t hipmv_export_centroids(uint64_t mv_h, void* out_bf16);
int32_t hipmv_export_codes(uint64_t mv_h, int32_t* out_codes_i32);
int32_t hipmv_centroid_info(uint64_t mv_h, int64_t* out4);
int32_t hipmv_gather_f32_dev(uint64_t mv_h, const int64_t* item_idx_host, int64_t n, float* out_f32_dev);
int32_t hipmaxsim_search_pruned_dev(uint64_t mv_h, const void* q_vecs_dev, const int32_t* q_counts_dev, int32_t q_stride,
                                    int32_t nq, int32_t k, int32_t ncand, const int64_t* ranges_host,
                                    const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                    int64_t id_base, float* out_scores_dev, int64_t* out_ids_dev, int64_t* out_cand_ids_dev,
                                    float* out_cand_scores_dev, void* stream);
int32_t hipmaxsim_search_pruned(uint64_t mv_h, const void* q_vecs_host, const int32_t* q_counts_host, int32_t q_stride,
                                int32_t nq, int32_t k, int32_t ncand, const int64_t* ranges_host,
                                const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                int64_t id_base, float* out_scores, int64_t* out_ids, int64_t* out_cand_ids,
                                float* out_cand_scores);
int32_t hipmaxsim_pruned_info(uint64_t mv_h, int64_t* out8);

/* ---- page table and page ranking (csrc/page_table.hip): the last step of the reference's retriever on the device -------
 * rag/query/page_retriever.py:145-236 groups the retrieved chunks by page, scores every page (mean chunk score plus a boost
 * for the number of chunks) and returns the best few.  The table holds, for every collection row, page[row] and tag[row],
 * two int32 arrays on the device; it is the fifth structure that follows a collection, after rows, IVF lists, postings and
 * passage tokens, under the same rules.  A TAG names the document of a row: every document of an append gets the next
 * value of a counter of the handle, a value is never reused, and no caller interprets one.  Two rows lie on the same page
 * if and only if tag AND page are equal (the reference, which answers from one document's index, groups by page alone).
 *   append         pages_host int32 [n_rows], doc_offsets_host int64 [n_docs + 1]: document j is the rows doc_offsets[j] ..
 *                  doc_offsets[j + 1] - 1 of the batch; the rows get the next row numbers.  Empty documents (they take a tag
 *                  too) and an empty batch are valid.  Capacity grows by half again.
 *   remove_ranges  stable compaction under the table rules of hipidx_remove_ranges; a range may cut a document; survivors
 *                  keep page and tag.  The rows move on the device through the bounded staging of hiptok_remove_ranges
 *                  (one mover for both); rows in front of the first removed one are neither read nor written.
 *   export         host copies of page [rows] and tag [rows]; either may be NULL.  A test hook.
 *   sizes          out4 = { rows, tags issued, capacity in rows, 0 }.
 * CHECKS, all before anything is touched (a refused call leaves the handle bit for bit as it was), HIPRAG_E_INVALID: null
 * pointers; offsets start at 0 and do not descend; rows afterwards < 2^31; tags issued < 2^31; the range table rules.
 * HIPRAG_E_NOMEM (no room to grow) leaves the handle as it was too.
 * SYNCHRONISATION: that of the token store -- append and remove_ranges are synchronous (null stream, the handle's mutex) and
 * THE CALLER MUST HAVE NO CALL IN FLIGHT ON THE HANDLE.  hiprag_shutdown drops live tables like every other handle.
 *
 * hippage_rank_dev: every array is device memory; the call is enqueued on `stream`, stages nothing and synchronises nothing.
 * Per query, over cand_ids [depth] and the dense list (dense_ids, dense_scores64) [dense_depth]:
 *   VALID      candidate j with id c is valid iff c >= 0 and 0 <= c - id_base < rows; anything else is padding: skipped, its
 *              three per-candidate outputs are -1, -1, 0.0.  The same id twice is two candidates.
 *   SCORE      dense_pos[j] = the first position of the dense list whose id equals c (an id < 0 never matches), -1 if none:
 *              the candidate is then SPARSE-ONLY and s = 0.0.  Otherwise, v the dense value, in fp64: s = 1.0 - v / 2.0 for
 *              HIPRAG_METRIC_L2, s = v for IP, then s = max(0.0, min(1.0, s)) -- HipIndexReader.search's transform.  A
 *              dense-only caller passes its result list as cand_ids and as dense_ids.
 *   PAGES      form in first-seen order of the valid candidates by (tag, page) of their row; members stay in list order.
 *              score = acc / m + min(n * 0.05, 0.15): acc the fp64 sum of s over the members that are not sparse-only, added
 *              one after the other in list order, m their count, n the count of all members; m = 0: the boost alone.
 *              Nothing is contracted into a fused multiply-add.
 *   ORDER      score descending, ties to the page seen first (Python's stable sort(reverse=True)).  The place of a NaN is
 *              unspecified.
 *   OUTPUTS    out_n_pages [nq] = all pages of the query, before the cut.  Ranks r < min(n_pages, max_pages) of
 *              out_page_scores / _first / _members / _no [nq][max_pages] carry the page's score, the position of its first
 *              member, its member count and its page number; ranks past that carry -DBL_MAX, -1, 0, 0.
 *              out_cand_rank [nq][depth] = the 0-based rank of the candidate's page among ALL pages of the query (not cut at
 *              max_pages): the members of the page ranked r are the positions j with out_cand_rank[j] == r, ascending.
 *              out_cand_dense_pos, out_cand_scores [nq][depth] = dense_pos and s.
 * CHECKS, HIPRAG_E_INVALID before anything is enqueued: null pointers; nq >= 1; 1 <= depth <= 256; 1 <= dense_depth <= 256;
 * 1 <= max_pages <= depth; id_base >= 0; a known metric.
 * One kernel, one thread per candidate, a few KiB of LDS per query: depth <= 64 runs one wave per query and four queries per
 * workgroup, a deeper list one workgroup per query.  No float atomics; the same bits from run to run and in either form. */
int32_t hippage_create(int32_t device, uint64_t* out_handle);
int32_t hippage_destroy(uint64_t h);
int32_t hippage_append(uint64_t h, const int32_t* pages_host, const int64_t* doc_offsets_host, int64_t n_docs);
int32_t hippage_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges);
int32_t hippage_export(uint64_t h, int32_t* pages, int32_t* tags);
int32_t hippage_sizes(uint64_t h, int64_t* out4);
int32_t hippage_rank_dev(uint64_t h, const int64_t* cand_ids_dev, int32_t depth, const int64_t* dense_ids_dev,
                         const double* dense_scores64_dev, int32_t dense_depth, int32_t nq, int64_t id_base, int32_t metric,
                         int32_t max_pages, int32_t* out_n_pages_dev, double* out_page_scores_dev, int32_t* out_page_first_dev,
                         int32_t* out_page_members_dev, int32_t* out_page_no_dev, int32_t* out_cand_rank_dev,
                         int32_t* out_cand_dense_pos_dev, double* out_cand_scores_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPRAG_H */
