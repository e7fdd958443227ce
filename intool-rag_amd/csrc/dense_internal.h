// dense_internal.h -- what the translation units of the dense index share on the host side: struct DenseIndex (bodies in
// dense_index.hip, the removal in dense_remove.hip; its launch policy is dense_plan.h), its registry (dense_api.hip), and the
// workspace and host steps that the list-major searches have in common (group_partials.hip: IVF batch search in
// ivf_search.hip, scoped search in dense_scoped.hip), the upload of a scope image and the chunk driver of the sliced searches.
#pragma once
#include <atomic>
#include <vector>

#include "common.h"
#include "dense_layout.h"
#include "dense_plan.h"
#include "scope_plan.h"
#include "slice_items.h"

namespace hiprag {

// Workspace of a list-major search (group_partials.hip): the counting sort's tables, the sorted (query, entry) pairs, the
// work items of every entry, the rows-read counter and the partial lists the canonical merge reads.
struct GroupWorkspace {
    DevBuf tiles, len, offs, chunks, order, items, stat, ps, pi;
    i64 chunk = 0, chunks_n = 0;   // hipivf_batch_info / hipidx_scoped_info: queries per chunk and chunks of the last call
};

// What a scoped search keeps with its structure (flat index, IVF lists, multi-vector store): the call's scope tables go up
// to `meta` through a small ring of pinned staging buffers (an event per buffer: a buffer is rewritten only after the copy
// out of it has run), the rest is the list-major searches' workspace.
struct ScopeUpload {
    static constexpr int kRing = 4;
    PinBuf pin[kRing];
    hipEvent_t pin_ev[kRing] = {nullptr, nullptr, nullptr, nullptr};
    bool pin_used[kRing] = {false, false, false, false};
    int pin_next = 0;
    DevBuf meta;
    GroupWorkspace gw;
    ScopeUpload() = default;
    ScopeUpload(const ScopeUpload&) = delete;              // the events have one owner
    ScopeUpload& operator=(const ScopeUpload&) = delete;
    ~ScopeUpload() { for (hipEvent_t e : pin_ev) if (e) (void)hipEventDestroy(e); }
    // `words` int64 of a call's scope image (scope_plan.h) -> meta, through the next buffer of the ring, on `st`
    int32_t upload(const int64_t* img, size_t words, hipStream_t st);   // group_partials.hip
};

// Timing of the scan launches: a ring of event pairs around the scan kernel and in-kernel wall-clock stamps of the same
// launches, averaged by hipidx_get_stats (no sync inside the search path).
struct ScanTiming {
    static constexpr int kEvRing = 512;
    static constexpr int kMaxScanWaves = 12;   // stamp slots per scan workgroup
    bool on = false;               // hipidx_enable_timing
    int every = 1;                 // HIP events cost two barrier packets per launch on the scan's stream: they bracket every n-th
                                   // launch only (the in-kernel stamps cover every launch either way)
    int64_t count = 0;             // launches since timing was (re)enabled
    std::vector<hipEvent_t> evs;   // 2 * kEvRing once timing was enabled
    DevBuf stamps;                 // [kEvRing][n_cu * kMaxScanWaves][2] in-kernel wall-clock ticks
    int n_cu = 0, wall_khz = 100000;
    std::vector<char> ev_set;      // [kEvRing] whether the launch in that ring slot was bracketed by events
    std::vector<int> ev_waves;     // [kEvRing] waves of that launch (its stamps occupy the first 2 * waves words of the ring slot)

    ~ScanTiming() { for (hipEvent_t e : evs) (void)hipEventDestroy(e); }
    void enable(int n) { on = n != 0; every = std::max(1, n); count = 0; }
    int32_t ensure(int n_cu_, int device);   // events and stamp buffer, on first use
    // one launch: its ring slot, whether events bracket it, where its waves stamp (null: timing is off), and what is noted
    // behind the launch
    int slot() const { return (int)(count % kEvRing); }
    bool bracket() const { return on && count % every == 0; }
    unsigned long long* launch_stamps() const
    {
        return on ? stamps.as<unsigned long long>() + (size_t)slot() * n_cu * kMaxScanWaves * 2 : nullptr;
    }
    hipEvent_t edge(int which) const { return evs[2 * slot() + which]; }
    int note(bool bracketed, int waves);     // -> the ring slot it took, -1 with timing off
    int32_t summarise(bool have_rows, hipidx_stats* out) const;   // the three averages and timed_passes
};

struct DenseIndex {
    std::mutex mu;
    int device = 0;
    int d = 0, P = 0, metric = 0;
    int64_t ntotal = 0, cap_blocks = 0, id_base = 0;
    int n_cu = 256;
    int scan_cus = 256;       // workgroups of a scan launch (one per CU); hipidx_set_spare_cus leaves some CUs to other streams
    ScanMode scan_mode = kScanBf16;   // HIPRAG_SCAN_MODE: bf16 (bf16 filter copy; default) or q64 (fp32 rows split on the fly)
    int scan_wide = -1;       // HIPRAG_SCAN_WIDE: 0 = never the wide kernel, 1 = whenever a launch is eligible, unset (-1) = from kWideMinQ queries
    int wide_fold_every = kWideFoldEvery;   // HIPRAG_WIDE_FOLD_EVERY: N of the wide kernel's fold schedule (wide_fold), a power of two in 1..64
    DevBuf xb, xh, norms, scalars;  // xh: bf16 filter copy; scalars: [0] max |x|^2 bits (u32), [1] max |x - bf16(x)|^2 bits,
                                // [2..3] fallback counter (u64), [4..5] extended-prefix counter, [6..11] the finish's work
                                // counters, [12..13] fold tiles of the wide scans
    // search workspace of one launch in flight
    struct Workspace {
        DevBuf list, state, flags, ek, ei;   // state: count[Q] | thetac[Q] | slots[Q / 64][kClasses][64]
        DevBuf qtile;                        // bf16 mode: the query-tile images of a multi-pass launch (qtile_kernel)
        int k = 0, q = 0;
        int64_t blocks = 0;
        int ev_idx = -1;
        bool dirty = false;                  // a scan ran without its finish: the scan state is not clean
        int waves = 8;
        unsigned long long seq = 0;          // sequence number of the scan last launched into this slot (0: none)
    };
    static constexpr int kSlots = 8;   // launches in flight: the scan of step i+1 runs beside the tails of steps i, i-1, ...
    Workspace ws[kSlots];
    DevBuf qbuf, o64, o32, oid;
    ScopeUpload sc;   // scoped search (hipidx_search_scoped_dev, dense_scoped.hip)
    // hipidx_score_ids* (dense_score_ids.hip): the counter word of the last call (made at the first call) and its pairs
    DevBuf score_stat;
    i64 score_pairs = 0;
    // pinned host staging of hipidx_search's few-query path (device-visible under the same address): the query goes up with
    // an asynchronous copy, the finish writes scores, ids and flags straight into host memory
    PinBuf pin_q, pin_o32, pin_oid, pin_flags;
    // start gate: see ScanArgs (dense_index.hip).  `started` holds the workgroup counter and, on a line of its own, the gate
    // word; both only ever grow.
    unsigned long long* gate = nullptr;
    DevBuf started;
    unsigned long long scan_seq = 0, started_total = 0;
    static constexpr int kFewQueries = 16;
    int launch_q = 256;       // queries one begin/finish pair takes (a multiple of 64): update_launch_q
    int launch_env = 0;       // HIPRAG_LAUNCH_QUERIES (0 = size launches by the index)
    // stats
    int64_t passes = 0, queries = 0, launches = 0, wide_launches = 0;
    ScanTiming timing;

    int64_t nblocks() const { return (ntotal + kRowsPerBlock - 1) / kRowsPerBlock; }
    unsigned* max_norm2_bits() { return scalars.as<unsigned>(); }
    unsigned* max_dx2_bits() { return scalars.as<unsigned>() + 1; }
    unsigned long long* fallback_counter() { return reinterpret_cast<unsigned long long*>(scalars.as<unsigned>() + 2); }
    unsigned long long* extend_counter() { return reinterpret_cast<unsigned long long*>(scalars.as<unsigned>() + 4); }
    unsigned long long* work_counters() { return reinterpret_cast<unsigned long long*>(scalars.as<unsigned>() + 6); }
    unsigned long long* fold_counter() { return reinterpret_cast<unsigned long long*>(scalars.as<unsigned>() + 12); }

    // Ordering of `add` against everything else: add_dev enqueues its re-tiling kernels on the CALLER's stream, which may
    // be a non-blocking stream the null stream does not wait for.  `add_ev` marks the last add; grow / save / reconstruct
    // (null-stream copies) wait for it on the host, a search on another stream waits for it on the device.
    hipEvent_t add_ev = nullptr;
    bool add_pending = false;

    int32_t wait_adds_host()
    {
        if (add_pending) { HR_CHECK_HIP(hipEventSynchronize(add_ev)); add_pending = false; }
        return HIPRAG_OK;
    }
    int32_t wait_adds_stream(hipStream_t st)
    {
        if (add_pending) HR_CHECK_HIP(hipStreamWaitEvent(st, add_ev, 0));
        return HIPRAG_OK;
    }

    ~DenseIndex();
    int32_t init();
    int32_t grow(int64_t need_blocks);
    int32_t add_dev(const float* x_dev, int64_t n, hipStream_t st);   // x_dev: [n,d] row-major on this device
    int32_t add_host(const float* x, int64_t n);

    // removal (dense_remove.hip)
    static constexpr size_t kRemoveBudget = (size_t)256 << 20;   // the chunk size add_host uses
    i64 rm_info[4] = {0, 0, 0, 0};   // hipidx_remove_info: rows removed, rows moved, chunks, extra device bytes
    std::atomic<int> ivf_refs{0};    // live hipivf_* handles over this index: their list offsets pin the row numbers
    int32_t remove_ranges(const int64_t* ranges, int32_t n_ranges);
    int32_t finish_removal(i64 nb_old, i64 nb_new, i64 n_new, size_t xb_blk, size_t xh_blk, size_t n_blk);

    // The launch policy (dense_plan.h) of this index as it stands
    ScanShape shape() const { return {nblocks(), P, scan_mode, scan_wide, n_cu, launch_env}; }
    ScanPlan plan(int nq, int k, int cus) const { return plan_scan(shape(), nq, k, cus); }
    int scan_waves(int cus) const { return hiprag::scan_waves(shape(), cus); }
    bool wide_launch(int nq) const { return wide_launch_on(nq, scan_cus); }
    bool wide_launch_on(int nq, int cus) const { return hiprag::wide_launch_on(shape(), nq, cus); }   // ... if the scan had `cus` workgroups
    int pipe_spare_cus() const { return hiprag::pipe_spare_cus(shape(), launch_q); }
    void update_launch_q() { launch_q = launch_queries(shape()); }
    bool fast_k(int k) const { return k <= kMaxKFast; }
    int32_t reserve_slot(int slot, int k);
    static size_t state_words(size_t Q);
    static u32* st_count(const Workspace& w) { return w.state.as<u32>(); }
    static u32* st_thetac(const Workspace& w) { return w.state.as<u32>() + w.q; }
    static u32* st_slots(const Workspace& w) { return w.state.as<u32>() + 2 * (size_t)w.q; }

    // the two phases of a launch and the exhaustive path (dense_index.hip, which alone instantiates them); cus = workgroups
    // of the scan
    template <int METRIC>
    int32_t scan_pass(const float* q_dev, int nq, int k, int slot, int cus, hipStream_t st);
    template <int METRIC>
    int32_t finish_pass(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st,
                        int* host_flags = nullptr);
    template <int METRIC>
    int32_t exhaustive_pass(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st);

    int32_t prepare(int k, int slot);
    int32_t begin_dev(const float* q_dev, int nq, int k, int slot, int cus, hipStream_t st);
    int32_t finish_dev(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st,
                       int* host_flags = nullptr);
    int32_t exhaustive_dev(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st);
    int32_t search_few_host(const float* q_host, int nq, int k, float* out_scores, int64_t* out_ids);
    int32_t gate_tail(int slot, hipStream_t st);   // the start gate's wait (hipidx_gate_tail_dev)

    // Streams and events of search_dev's own pipeline (batches of more than one launch): created on first use
    hipStream_t pipe_tail = nullptr;
    hipEvent_t pipe_in = nullptr, pipe_scanned[kSlots] = {}, pipe_done[kSlots] = {};
    int32_t pipe_init();
    int32_t search_dev_pipelined(const float* q_dev, int nq, int k, double* o64p, float* o32p, int64_t* oidp, hipStream_t st);
    int32_t search_dev(const float* q_dev, int nq, int k, double* o64p, float* o32p, int64_t* oidp, hipStream_t st);
};

// dense_api.hip
Registry<DenseIndex>& reg();
int32_t create_dense(int32_t d, int32_t metric, int32_t device, std::shared_ptr<DenseIndex>& out);
// dense_index.hip
int32_t ensure_lds(const void* fn, size_t bytes);
int32_t read_rows_host(DenseIndex& ix, i64 o, i64 m, DevBuf& tmp, float* host);
size_t clear_ivf_registry();   // ivf_search.hip; clear_dense_registry drops the IVF handles first

#define GET_INDEX(h)                                                                           \
    HR_GET_HANDLE(ix, reg(), h, "unknown dense index handle %llu", (unsigned long long)(h));   \
    std::lock_guard<std::mutex> guard(ix->mu);                                                 \
    HR_CHECK_HIP(hipSetDevice(ix->device))

// group_partials.hip
constexpr int kSumRows = 256;            // members per chunk of the IVF build's segmented sum (the counting sort counts them)
int32_t ivf_counting_sort(const i64* a, i64 m, int nlist, int pad, DevBuf& tiles, DevBuf& len, DevBuf& offs, DevBuf& chunks,
                          i64* out, hipStream_t st);
int32_t group_item_scan(const i64* pair_len, const i64* slices, const i64* rows, int group, bool rows_per_group, int n,
                        i64* item_start, i64* rows_read, hipStream_t st);
int32_t fill_partials(int metric, double* ps, i64* pi, i64 n, hipStream_t st);
int queries_per_chunk(int nq, i64 parts, int k, i64 budget, int max_chunk, i64 extra_per_query = 0);

// The chunk driver of the sliced scoped searches (dense_scoped.hip, maxsim_search.hip, maxsim_codes.hip; work items:
// slice_items.h), in the three steps between which a driver does its own work.
struct SlicePlan {
    ScopeImage im;
    int n_scopes = 0, group = 0;
    i64 smax = 1, bound = 0;   // slices of the largest scope, 1 at least; work items of the whole call, no chunk has more
    int kp = 0;                // entries of a slice's partial list: min(depth, slice_rows)
};
// 1. the table rules, the image, the refusal of a scope beyond the merge (`depth`: k or ncand, as named).  Touches nothing.
int32_t slice_plan(const int64_t* ranges, const int32_t* scope_offsets, int n_scopes, const int32_t* scope_of_query, int nq, i64 n,
                   const char* name_of_n, int slice_rows, int group, int depth, const char* name_of_depth, SlicePlan& out);
// 2. room for chunks of qchunk queries, the image's upload and a zero rows-read counter, on `st`
int32_t slice_begin(ScopeUpload& S, const SlicePlan& P, int qchunk, hipStream_t st);
// 3. queries [o, o + m) of the call: sorted by scope, their work items counted, their partial lists [smax][m][kp] prefilled
int32_t slice_chunk(ScopeUpload& S, const SlicePlan& P, int metric, int o, int m, SliceTables& out, hipStream_t st);

}  // namespace hiprag
