// bm25_internal.h -- what the translation units of the BM25 index share on the host side: struct Bm25Index (search bodies in
// bm25.hip, the updates in bm25_update.hip, the impact handles in bm25_impacts.hip), its registry, and the one impact formula both the reweigh kernel and the host
// test hook evaluate.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"
#include "topk_device.h"

namespace hiprag {

constexpr int kBm25Batch = 32;       // queries scored concurrently by the global-accumulator form
constexpr int kTileDocs = 9216;      // documents per tile of the tiled TAAT kernel (bm25.hip)
constexpr u64 kSkipMinDf = 2048;     // lists from this length on carry a skip table

// One posting's impact: the arithmetic of hiprag.sparse.build_postings, fp64 in ITS operation order, rounded once to fp32.
// Contraction is off: hipcc fuses a*b + c into an FMA in device code by default, numpy never does, and one fused operation
// changes the last bit of some impacts.  fp64 division is correctly rounded on the host and on gfx950.
__host__ __device__ inline float bm25_impact(double idf, double tf, double dl, double avgdl, double k1, double b)
{
#pragma clang fp contract(off)
    const double norm = k1 * ((1.0 - b) + (b * dl) / avgdl);
    const double imp = ((idf * tf) * (k1 + 1.0)) / (tf + norm);
    return (float)imp;
}

// One search call, as the eight hipbm25_search* entries describe it to their one driver (run_search, bm25.hip).
struct Bm25Call {
    bool scoped, weighted, host;         // which of the eight: the driver's checks and messages follow the entry's
    const uint32_t* terms;
    const float* wts;                    // one weight per query-term slot, parallel to `terms`; null = plain impacts
    const int32_t* qoff;
    int nq, k;
    const int64_t* ranges;               // the scope tables of a scoped call (include/hiprag.h)
    const int32_t* scope_offsets;
    int n_scopes;
    const int32_t* scope_of_query;
    double* o64;                         // outputs: device pointers, o64 / o32 may be null.  A host call comes in with HOST
    float* o32;                          // pointers in o32 / oid and runs on the null stream into the handle's o32 / oid
    i64* oid;
    hipStream_t st;
};

struct Bm25Index {
    std::mutex mu;
    int device = 0;
    i64 n_docs = 0, n_terms = 0, n_postings = 0, id_base = 0;
    std::vector<uint64_t> offsets;  // host copy: planning happens on the host
    DevBuf doc_ids, impacts, acc, ranges, ck, ci, o64, o32, oid, skip_dev, slots_dev, nslots_dev, theta_dev, hist_dev;
    DevBuf wts_dev;                      // weighted searches: the slot weights, laid out like the slot table of the launch
    std::vector<i64> skip_index;         // per term: first entry of its skip table, or -1 (short lists)
    // Host staging of the query plans: a ring of pinned buffers, each with the event of its last copy.  A call fills the next
    // buffer and enqueues its copies without waiting for anything but THAT buffer's previous copy (kStages calls ago), so a
    // host that pipelines batches (ShardedHybrid: the BM25 leg of step i beside the scan of step i + 1) is not held until
    // the previous call's kernels have run -- with one pageable staging vector every call blocked on its predecessor.
    static constexpr int kStages = 4;
    struct Stage {
        PinBuf slots, nslots, scoped, wts;   // wts: slot weights of a weighted call; scoped: work items | tiles per query | range table of a scoped chunk
        hipEvent_t ev = nullptr;
        bool used = false;
    };
    Stage stages[kStages];
    unsigned stage_next = 0;
    bool force_global = false;           // HIPBM25_GLOBAL_ACC=1: the global-accumulator form for every k (A/B runs)
    DevBuf scoped_dev;                   // device image of Stage::scoped
    i64 scoped_budget = 512ll << 20;     // bytes of candidate lists per chunk of a scoped call (HIPBM25_SCOPED_BUDGET_MIB, tests)
    i64 sc_items = 0, sc_max_tiles = 0, sc_chunks = 0;   // hipbm25_scoped_info: the last scoped call
    int ws_k = 0;
    i64 queries = 0, postings_touched = 0, bytes_alg = 0;

    // ---- updatable handles (hipbm25_create_tf, bm25_update.hip): what impacts are made of, kept on the device -----------
    // tf is parallel to doc_ids, doc_len has one entry per document, offsets_dev mirrors `offsets`.  doc_ids2 / tf2 /
    // offsets2 are the destination of an append or a removal and are swapped with the live buffers behind it.  Capacities
    // are in entries and grow by half again (DenseIndex::grow), so a run of small appends does not reallocate each time.
    bool has_tf = false;                 // false: made by hipbm25_create, the update entries answer HIPRAG_E_UNSUPPORTED
    bool dirty = false;                  // structure changed since the last reweigh: every search entry refuses
    double k1 = 1.5, b = 0.75;
    i64 total_len = 0;                   // sum of doc_len: avgdl = total_len / n_docs
    i64 cap_postings = 0, cap_docs = 0;
    DevBuf tf, doc_len, offsets_dev, doc_ids2, tf2, offsets2, idf_dev, long_dev;
    i64 upd_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // hipbm25_update_info
    // ---- updatable IMPACT handles (hipbm25_create_impacts, bm25_impacts.hip): impacts as given, no tf, no doc_len -------
    // The impacts are the 32-bit stream that travels with doc_ids through the structure passes (tf2 is its destination), so
    // an update needs no reweigh and the handle is never dirty; the skip tables are rebuilt behind every change.
    bool has_impacts = false;
    // ---- hipbm25_score_ids* (bm25_score_ids.hip): the slot table of the call, its two counter words and its pairs ----------
    DevBuf sid_slots_dev, sid_qoff_dev, score_stat;
    i64 score_pairs = 0;

    i64 ntiles() const { return std::max<i64>(1, (n_docs + kTileDocs - 1) / kTileDocs); }
    i64 nchunks() const { return std::max<i64>(1, (n_docs + kTile - 1) / kTile); }
    i64 stride() const { return std::max<i64>(4, (n_docs + 3) / 4 * 4); }       // accumulator row stride (16-B aligned rows)
    i64 nlists() const { return (std::max<i64>(1, (n_docs + kSelPerWave - 1) / kSelPerWave) + 3) / 4 * 4; }

    // One workspace (ck / ci / theta / slots / acc) serves every call on this handle: a call on another stream than the
    // previous one is ordered behind it on the device, so that two streams never share the workspace in time.
    hipEvent_t prev_ev = nullptr;
    bool prev_ev_set = false;
    hipStream_t prev_stream = nullptr;

    struct ScopePlan {                      // the scopes of one call in tile terms, built while they are validated
        std::vector<uint32_t> rng;          // (lo, hi) of every range, the device's range table
        std::vector<int> tile, r0, r1;      // per scope, concatenated: its tiles ascending, each with the ranges [r0, r1) that meet it
        std::vector<i64> toff;              // [n_scopes + 1]: scope s owns entries toff[s] .. toff[s + 1] - 1
        i64 tiles_of(int s) const { return toff[(size_t)s + 1] - toff[(size_t)s]; }
    };

    ~Bm25Index();

    // search (bm25.hip): run_search checks a call and hands it to search(), which orders it behind the previous call's stream
    struct TileLaunch;                   // what plan_tiles hands to the launch: slots per query and the kernel
    int32_t reserve(int k);
    void launch_merge(i64 wave_cand, int nq, int k, double* o64p, float* o32p, i64* oidp, hipStream_t st);
    int32_t set_tile_lds();
    template <class FillImage>
    int32_t plan_tiles(const Bm25Call& c, int q0, int m, i64 lists, size_t image_words, FillImage fill_image, TileLaunch& tl);
    int32_t search(const Bm25Call& c, const ScopePlan& P);
    int32_t search_unscoped(const Bm25Call& c);
    int32_t search_tiled(const Bm25Call& c);
    int32_t plan_scopes(int nq, int k, const int64_t* ranges, const int32_t* scope_offsets, int n_scopes, const int32_t* scope_of_query,
                        ScopePlan& P) const;
    int chunk_queries(const ScopePlan& P, const int32_t* soq, int q0, int nq, int k, i64* max_tiles, i64* n_items) const;
    int32_t search_scoped(const Bm25Call& c, const ScopePlan& P);
    int32_t scoped_chunk(const Bm25Call& c, const ScopePlan& P, int q0, int m, int max_tiles, i64 n_items);
    void read_env();                     // HIPBM25_GLOBAL_ACC, HIPBM25_SCOPED_BUDGET_MIB
    // scores of given documents (bm25_score_ids.hip): ordered behind the previous call's stream as search() is
    int32_t score_ids(const uint32_t* terms, const float* wts, const int32_t* qoff, int nq, const int64_t* ids_dev, int depth, float* out_dev,
                      hipStream_t st);

    // updates (bm25_update.hip); all of them run on the null stream under the mutex and synchronise
    int32_t reserve_postings(i64 need, bool* grew, i64* extra);
    int32_t append(i64 n_new, i64 n_terms_after, const uint64_t* boff, const uint32_t* bids, const uint32_t* btf, const uint32_t* bdl);
    int32_t remove_ranges(const int64_t* ranges, int32_t n_ranges);
    int32_t reweigh(const double* idf_host);
    void drop_doc_workspaces();          // acc / ck / ci / ws_k depend on n_docs
    // The merge of an append, shared by the tf and the impact handles.  plan_merge: the offsets afterwards (old + batch,
    // elementwise) and the list-length check, nothing touched.  merge_batch: every list becomes the old list followed by the
    // batch's with ids + n_docs (append_kernel); `pay` is the live 32-bit stream parallel to doc_ids -- tf, or the impacts'
    // bits -- and the batch pointers are DEVICE memory (unused when the batch holds no posting).  Updates offsets, n_terms,
    // n_postings and skip_index; n_docs is the caller's.
    int32_t plan_merge(i64 n_terms_after, const uint64_t* boff_host, std::vector<uint64_t>& noff) const;
    int32_t merge_batch(DevBuf& pay, i64 n_terms_after, std::vector<uint64_t>& noff, const uint64_t* boff_host, const u64* boff_dev,
                        const u32* bids_dev, const u32* bpay_dev, bool* grew, i64* extra, i64* moved);
    int32_t rebuild_skips();             // skip tables of the lists that are long now (skip_kernel); synchronises

    // impact handles (bm25_impacts.hip)
    int32_t append_impacts(i64 n_new, i64 n_terms_after, const uint64_t* boff, const uint32_t* bids, const float* bimp);
    int32_t append_rows_dev(const int32_t* terms_dev, const float* weights_dev, const int32_t* counts_dev, i64 n_new, i64 row_stride,
                            i64 n_terms_after, hipStream_t stream);
};

// bm25_update.hip: host pieces the impact handles share with the tf path
void swap_buf(DevBuf& x, DevBuf& y);
inline i64 round4(i64 n) { return std::max<i64>(16, (n + 3) / 4 * 4); }   // capacities: whole 16-byte pieces, 16 entries at least
// base[i] = counts[0] + .. + counts[i - 1] for i in 0..n (rm_scan_kernel: one 1024-thread workgroup walks the counts), null stream
void launch_excl_scan(const u32* counts_dev, i64 n, u64* base_dev);

// bm25.hip
Registry<Bm25Index>& bm25_reg();

#define GET_BM25(h)                                                                          \
    std::shared_ptr<Bm25Index> ix = bm25_reg().get(h);                                       \
    if (!ix) { set_error("unknown bm25 handle %llu", (unsigned long long)(h)); return HIPRAG_E_HANDLE; } \
    std::lock_guard<std::mutex> guard(ix->mu);                                               \
    HR_CHECK_HIP(hipSetDevice(ix->device))

// a dirty handle (appended to or removed from, not reweighed yet) holds impacts of another collection: no search entry runs
#define BM25_REQUIRE_CLEAN(ix)                                                                                         \
    HR_REQUIRE(!(ix)->dirty, "this bm25 handle was changed by hipbm25_append / hipbm25_remove_ranges and its impacts are " \
                             "stale: call hipbm25_reweigh before searching")

}  // namespace hiprag
