// dense_internal.h -- what the translation units of the dense index share on the host side: struct DenseIndex (bodies in
// dense_index.hip, the removal in dense_remove.hip), its registry, and the workspace and host steps that the two list-major
// searches have in common (group_partials.hip: IVF batch search in ivf_search.hip, scoped search in dense_scoped.hip).
#pragma once
#include <atomic>
#include <vector>

#include "common.h"
#include "dense_layout.h"

namespace hiprag {

// Workspace of a list-major search (group_partials.hip): the counting sort's tables, the sorted (query, entry) pairs, the
// work items of every entry, the rows-read counter and the partial lists the canonical merge reads.
struct GroupWorkspace {
    DevBuf tiles, len, offs, chunks, order, items, stat, ps, pi;
    i64 chunk = 0, chunks_n = 0;   // hipivf_batch_info / hipidx_scoped_info: queries per chunk and chunks of the last call
};

struct DenseIndex {
    std::mutex mu;
    int device = 0;
    int d = 0, P = 0, metric = 0;
    int64_t ntotal = 0, cap_blocks = 0, id_base = 0;
    int n_cu = 256;
    int scan_cus = 256;       // workgroups of a scan launch (one per CU); hipidx_set_spare_cus leaves some CUs to other streams
    int scan_mode = 3;        // HIPRAG_SCAN_MODE: bf16 = 3 (bf16 filter copy; default), q64 = 2 (fp32 rows split on the fly)
    int scan_wide = -1;       // HIPRAG_SCAN_WIDE: 0 = never the wide kernel, 1 = whenever a launch is eligible, unset (-1) = from kWideMinQ queries
    DevBuf xb, xh, norms, scalars;  // xh: bf16 filter copy; scalars: [0] max |x|^2 bits (u32), [1] max |x - bf16(x)|^2 bits,
                                // [2..3] fallback counter (u64), [4..5] extended-prefix counter
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
    // scoped search (hipidx_search_scoped_dev, dense_scoped.hip): the call's scope tables go up through a small ring of pinned
    // staging buffers (an event per buffer: a buffer is rewritten only after the copy out of it has run), the rest is the
    // list-major searches' workspace
    struct Scoped {
        static constexpr int kRing = 4;
        PinBuf pin[kRing];
        hipEvent_t pin_ev[kRing] = {nullptr, nullptr, nullptr, nullptr};
        bool pin_used[kRing] = {false, false, false, false};
        int pin_next = 0;
        DevBuf meta;
        GroupWorkspace gw;
    } sc;
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
    // timing: a ring of event pairs around the scan kernel, averaged by get_stats (no sync inside the search path)
    static constexpr int kEvRing = 512;
    bool timing = false;
    std::vector<hipEvent_t> evs;   // 2*kEvRing once timing was enabled
    DevBuf stamps;                 // [kEvRing][n_cu * 8 waves][2] in-kernel wall-clock ticks of the same launches
    int wall_khz = 100000;
    int64_t ev_count = 0;          // launches since timing was (re)enabled
    int ev_every = 1;
    std::vector<char> ev_set;      // [kEvRing] whether the launch in that ring slot was bracketed by events
    std::vector<int> ev_waves;     // [kEvRing] waves of that launch (its stamps occupy the first 2 * waves words of the ring slot)

    int64_t nblocks() const { return (ntotal + kRowsPerBlock - 1) / kRowsPerBlock; }
    unsigned* max_norm2_bits() { return scalars.as<unsigned>(); }
    unsigned* max_dx2_bits() { return scalars.as<unsigned>() + 1; }
    unsigned long long* fallback_counter() { return reinterpret_cast<unsigned long long*>(scalars.as<unsigned>() + 2); }
    unsigned long long* extend_counter() { return reinterpret_cast<unsigned long long*>(scalars.as<unsigned>() + 4); }
    unsigned long long* work_counters() { return reinterpret_cast<unsigned long long*>(scalars.as<unsigned>() + 6); }

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

    static constexpr int kPassQ = 64;   // queries that share one read of the index
    // Small shards (an 8-GPU row split of 1M rows leaves 125 k per GPU): with 8 waves per workgroup a wave streams two or
    // three 32-row blocks per pass; 4-wave workgroups stream twice as many each and leave half of every SIMD's registers to
    // the tail kernels of earlier steps.  Measured in rounds 1-2 (1024 queries per launch, pipelined): 125 k rows 945 -> 902
    // us per step, 250 k 1640 -> 1590, 500 k about equal, 1M equal: 4 waves below 9 blocks per wave of the 8-wave partition.
    int scan_waves(int64_t nb) const { return (scan_mode == 3 && P % 32 == 0 && nb < (int64_t)scan_cus * 8 * 9) ? 4 : 8; }
    // Which launches take scan_wide_kernel (scan_wide.h): the bf16 copy, the filter on (more than 64 row tiles of 256 rows, so
    // that row tiles 0..31 publish all 64 classes), at least 32 workgroups (those row tiles all fall into the first round) and
    // enough queries.  Forced (HIPRAG_SCAN_WIDE=1): more than one 64-query pass.  Default: at least kWideMinQ queries --
    // measured one launch at a time, ms narrow / wide (profiles/wide_threshold_probe*.jsonl): at 1M x 1024 128 queries
    // 0.74 / 0.81, 192 queries 1.09 / 0.88, 256 queries 1.39 / 0.94; at 125 k x 1024 192 queries 0.210 / 0.234, 256 queries
    // 0.267 / 0.248: 256 is the smallest size at which the wide kernel wins on both -- and at least one row tile per
    // workgroup: on a smaller index part of the grid owns no tile while every narrow wave still streams its share (not
    // measured, so not taken).
    static constexpr int kWideMinQ = 256;
    bool wide_launch(int nq) const { return wide_launch_on(nq, scan_cus); }
    bool wide_launch_on(int nq, int cus) const;   // ... if the scan had `cus` workgroups
    bool fast_k(int k) const;
    void update_launch_q();
    int32_t reserve_slot(int slot, int k);
    static size_t state_words(size_t Q);
    static u32* st_count(const Workspace& w) { return w.state.as<u32>(); }
    static u32* st_thetac(const Workspace& w) { return w.state.as<u32>() + w.q; }
    static u32* st_slots(const Workspace& w) { return w.state.as<u32>() + 2 * (size_t)w.q; }

    // the two phases of a launch and the exhaustive path (dense_index.hip, which alone instantiates them)
    template <int METRIC>
    int32_t scan_pass(const float* q_dev, int nq, int k, int slot, hipStream_t st);
    template <int METRIC>
    int32_t finish_pass(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st,
                        int* host_flags = nullptr);
    template <int METRIC>
    int32_t exhaustive_pass(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st);

    int32_t prepare(int k, int slot);
    int32_t begin_dev(const float* q_dev, int nq, int k, int slot, hipStream_t st);
    int32_t finish_dev(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st,
                       int* host_flags = nullptr);
    int32_t search_few_host(const float* q_host, int nq, int k, float* out_scores, int64_t* out_ids);

    // Streams and events of search_dev's own pipeline (batches of more than one launch): created on first use
    hipStream_t pipe_tail = nullptr;
    hipEvent_t pipe_in = nullptr, pipe_scanned[kSlots] = {}, pipe_done[kSlots] = {};
    // CUs a pipelined scan leaves to the finish of the launch before it (search_dev's own pipeline, and hiprag/sharded.py
    // through hipidx_pipe_spare_cus).  The narrow scan is HBM-bound and 32-64 measure the same: 48.  The wide scan is bound by
    // its CUs: workgroup i walks row tiles i, i + G, ..., so a launch lasts ceil(row tiles / G) rounds, and CUs that save a
    // round are worth more to the scan than to the finish -- down to 32, below which the finish no longer fits beside the
    // scan (fin_kernel 0.38 ms at 32 spare CUs, 1.29 ms at 26).  1M x 1024, 512 queries: 19 rounds on 208
    // workgroups, 18 on 224, +2.4 %; 125 k x 1024, 1024 queries: 3 rounds either way, and 32 is 1.6 % SLOWER than 48.
    static constexpr int kPipeSpareCus = 48;
    static constexpr int kPipeSpareCusWide = 32;
    int pipe_spare_cus() const;

    int32_t pipe_init();
    int32_t search_dev_pipelined(const float* q_dev, int nq, int k, double* o64p, float* o32p, int64_t* oidp, hipStream_t st);
    int32_t search_dev(const float* q_dev, int nq, int k, double* o64p, float* o32p, int64_t* oidp, hipStream_t st);
};

// dense_index.hip
Registry<DenseIndex>& reg();
int32_t ensure_lds(const void* fn, size_t bytes);
int32_t create_dense(int32_t d, int32_t metric, int32_t device, std::shared_ptr<DenseIndex>& out);
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

}  // namespace hiprag
