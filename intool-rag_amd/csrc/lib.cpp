// lib.cpp -- library-level entry points of libhiprag.so: error state, device queries, HIP-event timing.
#include "common.h"
#include "dense_plan.h"
#include "scope_plan.h"
#include "slice_items.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <vector>

namespace hiprag {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

static Registry<hipEvent_t>& events()
{
    static Registry<hipEvent_t> r;
    return r;
}

// The device's SCAN STREAM: one high-priority stream per device, owned by the library (hiprag_scan_stream hands it to
// hosts that chain their own scans, hiprag/sharded.py).  A scan workgroup needs a whole CU (158 of 160 KiB of LDS) and a
// scan is launched on fewer workgroups than the chip has CUs (hipidx_set_spare_cus); the kernels that are to run beside
// it -- BM25 tiles, four to a CU, the finish of the previous launch -- are many small workgroups.  When a scan and such a
// kernel become ready together the dispatcher serves the high-priority queue first: the scan gets its CUs and the small
// workgroups fill the rest.  With equal priorities they take every CU first and the scan's workgroups start late, one by
// one, as CUs drain (the hybrid legs' times then simply add up: 123-137 k hybrid queries/s at 1M chunks, against 140-154 k
// beside each other on the same boxes).  Every dense leg of every hybrid call goes through this one stream, in the order
// the index's mutex admitted the calls (they share the index's workspace).
class ScanStreams {
public:
    int32_t get(int dev, hipStream_t& out)
    {
        std::lock_guard<std::mutex> g(mu_);
        auto it = hp_.find(dev);
        if (it == hp_.end()) {
            int least = 0, greatest = 0, cur = 0;
            hipStream_t hp = nullptr;
            HR_CHECK_HIP(hipGetDevice(&cur));
            HR_CHECK_HIP(hipSetDevice(dev));
            hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (e == hipSuccess) e = hipStreamCreateWithPriority(&hp, hipStreamNonBlocking, greatest);
            (void)hipSetDevice(cur);
            HR_CHECK_HIP(e);
            it = hp_.emplace(dev, hp).first;
        }
        out = it->second;
        return HIPRAG_OK;
    }
    // The device's TAIL STREAMS (two, normal priority): where the kernels that run beside a scan are enqueued -- the finish
    // of the previous launch, an exchange, a merge.  One pair per device for the whole process, not one per index or per
    // wrapper object: HIP has four hardware queues per priority and hands them out in order of first use, streams beyond
    // that SHARE queues, and a process that multiplied its tail streams (one pair per ShardedFlatIndex, a stream per index
    // for the library's own pipeline) slowed its later pipelines down by that alone.
    int32_t get_tail(int dev, int which, hipStream_t& out)
    {
        std::lock_guard<std::mutex> g(mu_);
        const long long key = (long long)dev * 2 + (which & 1);
        auto it = tail_.find(key);
        if (it == tail_.end()) {
            int cur = 0;
            hipStream_t st = nullptr;
            HR_CHECK_HIP(hipGetDevice(&cur));
            HR_CHECK_HIP(hipSetDevice(dev));
            const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
            (void)hipSetDevice(cur);
            HR_CHECK_HIP(e);
            it = tail_.emplace(key, st).first;
        }
        out = it->second;
        return HIPRAG_OK;
    }
    void clear()   // hiprag_shutdown, every device synchronised
    {
        std::lock_guard<std::mutex> g(mu_);
        for (auto& kv : hp_)
            if (hipSetDevice(kv.first) == hipSuccess) (void)hipStreamDestroy(kv.second);
        hp_.clear();
        for (auto& kv : tail_)
            if (hipSetDevice((int)(kv.first / 2)) == hipSuccess) (void)hipStreamDestroy(kv.second);
        tail_.clear();
    }

private:
    std::mutex mu_;
    std::unordered_map<int, hipStream_t> hp_;
    std::unordered_map<long long, hipStream_t> tail_;
};
static ScanStreams& scan_streams()
{
    static ScanStreams s;
    return s;
}
constexpr int kHybridSpareCus = 96;   // of 256: dense top-50 alone loses 0-7 % on 160 workgroups; 64-112 measure within the box-to-box spread (config 2)

// The two events of one hybrid call (legs start / dense leg done), pooled per device.
struct LegEvents {
    hipEvent_t in = nullptr, dense_done = nullptr;
    int dev = -1;
};
class LegEventPool {
public:
    int32_t acquire(int dev, LegEvents& out)
    {
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t i = 0; i < free_.size(); ++i)
                if (free_[i].dev == dev) { out = free_[i]; free_.erase(free_.begin() + (long)i); return HIPRAG_OK; }
        }
        LegEvents e;
        e.dev = dev;
        HR_CHECK_HIP(hipEventCreateWithFlags(&e.in, hipEventDisableTiming));
        hipError_t rc = hipEventCreateWithFlags(&e.dense_done, hipEventDisableTiming);
        if (rc != hipSuccess) { (void)hipEventDestroy(e.in); HR_CHECK_HIP(rc); }
        out = e;
        return HIPRAG_OK;
    }
    void release(const LegEvents& e)
    {
        std::lock_guard<std::mutex> g(mu_);
        free_.push_back(e);
    }
    void clear()
    {
        std::lock_guard<std::mutex> g(mu_);
        for (const LegEvents& e : free_) {
            if (hipSetDevice(e.dev) != hipSuccess) continue;
            (void)hipEventDestroy(e.in);
            (void)hipEventDestroy(e.dense_done);
        }
        free_.clear();
    }

private:
    std::mutex mu_;
    std::vector<LegEvents> free_;
};
static LegEventPool& leg_events()
{
    static LegEventPool p;
    return p;
}
// One lease per hybrid call.  While `busy` the scan stream may still write into buffers the call's frame owns: every way out
// of the frame (error returns included) first waits for it.
struct LegLease {
    LegEvents e;
    hipStream_t hp = nullptr;
    bool held = false, busy = false;
    ~LegLease()
    {
        if (busy && hp) (void)hipStreamSynchronize(hp);
        if (held) leg_events().release(e);
    }
};

// the dense leg of a hybrid call leaves CUs to the BM25 leg; the index's own setting comes back on every way out
struct SpareCusScope {
    uint64_t h = 0;
    int32_t before = -1;
    int32_t enter(uint64_t handle, int32_t spare)
    {
        int32_t rc = hipidx_get_spare_cus(handle, &before);
        if (rc) { before = -1; return rc; }
        h = handle;
        return before >= spare ? HIPRAG_OK : hipidx_set_spare_cus(handle, spare);
    }
    ~SpareCusScope() { if (before >= 0) (void)hipidx_set_spare_cus(h, before); }
};

struct StepEvents {    // one event per (device, slot): orders a step's tail stream behind its scan
    std::mutex mu;
    std::unordered_map<long long, hipEvent_t> ev;
    int32_t get(int dev, int slot, hipEvent_t& out)
    {
        std::lock_guard<std::mutex> g(mu);
        const long long key = (long long)dev * 64 + slot;
        auto it = ev.find(key);
        if (it == ev.end()) {
            hipEvent_t e = nullptr;
            HR_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            it = ev.emplace(key, e).first;
        }
        out = it->second;
        return HIPRAG_OK;
    }
    void clear()
    {
        std::lock_guard<std::mutex> g(mu);
        for (auto& kv : ev) {
            if (hipSetDevice((int)(kv.first / 64)) == hipSuccess) (void)hipEventDestroy(kv.second);
        }
        ev.clear();
    }
};
static StepEvents& step_events()
{
    static StepEvents s;
    return s;
}

namespace {
// hiprag_probe_read_gbps: what this device streams through a statically partitioned read (the dense scan's access
// pattern without its work): every wave reads its own contiguous range of 64 KiB blocks, 16 KiB in flight per wave,
// non-temporal 16-byte loads.
typedef float probe_f4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(512) void read_probe_kernel(const probe_f4* __restrict__ x, long long nblocks, int bpw, int passes,
                                                        float* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long gw = (long long)blockIdx.x * 8 + wave;
    probe_f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int pass = 0; pass < passes; ++pass) {
        for (int i = 0; i < bpw; ++i) {
            const long long b = gw * bpw + i;
            if (b >= nblocks) break;
            const probe_f4* src = x + b * 4096 + lane;   // a block = 64 KiB = 4096 x 16 B
            for (int p = 0; p < 64; p += 16) {
                probe_f4 r[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) r[u] = __builtin_nontemporal_load(src + (p + u) * 64);
#pragma unroll
                for (int u = 0; u < 16; ++u) acc += r[u];
            }
        }
    }
    if (acc[0] + acc[1] + acc[2] + acc[3] == 12345.678f) out[0] = 1.f;   // never true for a zeroed buffer: keeps the loads
}

// hiprag_slice_items: the items of a call decoded one by one into 8 int64 words each
template <int G, int S>
void decode_items(const SliceTables& t, int64_t n_items, int64_t* out)
{
    for (int64_t i = 0; i < n_items; ++i) {
        const SliceItem it = slice_item<G, S>(t, i);
        const int64_t w[8] = {it.scope, it.slice, it.group, it.members, it.first, it.base, it.p_lo, it.p_hi};
        std::copy(w, w + 8, out + 8 * i);
    }
}

}  // namespace

}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hiprag_version(void) { return 100; }

const char* hiprag_last_error(void) { return g_last_error.c_str(); }

int32_t hiprag_device_count(int32_t* out_count)
{
    HR_REQUIRE(out_count, "null out");
    int n = 0;
    HR_CHECK_HIP(hipGetDeviceCount(&n));
    *out_count = n;
    return HIPRAG_OK;
}

int32_t hiprag_init(int32_t n_devices)
{
    int n = 0;
    HR_CHECK_HIP(hipGetDeviceCount(&n));
    const int want = n_devices > 0 ? n_devices : 1;
    HR_REQUIRE(n >= want, "hiprag_init: %d device(s) requested, %d visible", want, n);
    for (int dev = 0; dev < want; ++dev) {   // create the contexts now, not inside the first search
        HR_CHECK_HIP(hipSetDevice(dev));
        HR_CHECK_HIP(hipFree(nullptr));
    }
    HR_CHECK_HIP(hipSetDevice(0));
    return HIPRAG_OK;
}

int32_t hiprag_shutdown(void)
{
    int n = 0;
    HR_CHECK_HIP(hipGetDeviceCount(&n));
    for (int dev = 0; dev < n; ++dev) {
        if (hipSetDevice(dev) == hipSuccess) (void)hipDeviceSynchronize();
    }
    clear_encoder_registry();
    clear_token_registry();
    clear_page_registry();
    clear_multivec_registry();
    clear_bm25_registry();
    clear_dense_registry();
    events().clear();
    leg_events().clear();
    scan_streams().clear();
    step_events().clear();
    return HIPRAG_OK;
}

// the walk of the wide kernel (dense_plan.h), pair by pair: what scan_wide_kernel's three cursors go through
int32_t hiprag_wide_walk(int64_t nrt, int32_t ncol, int32_t cus, int32_t wg, int64_t cap, int64_t* out_row_tile,
                         int32_t* out_column, int64_t* out_pairs)
{
    HR_REQUIRE(out_pairs, "null out");
    HR_REQUIRE(nrt >= 1 && nrt < ((int64_t)1 << 28) && ncol >= 1 && ncol <= kMaxQ / (kWideQTiles * 32) && cus >= 1 && wg >= 0 && wg < cus,
               "hiprag_wide_walk: 1 <= nrt < 2^28, 1 <= ncol <= %d, cus >= 1 and 0 <= wg < cus", kMaxQ / (kWideQTiles * 32));
    HR_REQUIRE(cap >= 0 && (cap == 0 || (out_row_tile && out_column)), "hiprag_wide_walk: cap > 0 needs both output arrays");
    const WideWalk W = wide_walk((uint32_t)nrt, (uint32_t)ncol, (uint32_t)cus, (uint32_t)wg);
    *out_pairs = W.npairs;
    for (uint32_t p = 0; p < W.npairs && (int64_t)p < cap; ++p) {
        const WidePair pr = wide_walk_pair(W, p);
        out_row_tile[p] = pr.rt;
        out_column[p] = (int32_t)pr.col;
    }
    return HIPRAG_OK;
}

// the work items of a sliced scoped search (slice_items.h), item by item: what the three kernels decode.  The tables behind
// the image are formed here as the device forms them: the counting sort is stable by scope, group_item_scan_kernel gives
// a scope with queries groups x slices items and a scope without queries none (group_partials.hip).
int32_t hiprag_slice_items(const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                           const int32_t* scope_of_query_host, int32_t nq, int64_t n, int32_t slice_rows, int32_t group,
                           int64_t* out_items, int64_t items_cap, int64_t* out_count)
{
    HR_REQUIRE(out_count, "out_count is null");
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(n_scopes >= 1, "n_scopes must be at least 1 (got %d)", n_scopes);
    HR_REQUIRE(n >= 0, "n must not be negative (got %lld)", (long long)n);
    const bool flat = slice_rows == 256 && group == 16, exact = slice_rows == 16 && group == 8, pruned = slice_rows == 256 && group == 8;
    HR_REQUIRE(flat || exact || pruned, "no sliced search has slices of %d entries and groups of %d queries: (256, 16), (16, 8) and (256, 8) "
               "are the three", slice_rows, group);
    int32_t rc;
    if ((rc = check_scope_tables(ranges_host, scope_offsets_host, n_scopes, scope_of_query_host, nq, n, "n"))) return rc;
    ScopeImage im;
    build_scope_image(ranges_host, scope_offsets_host, n_scopes, scope_of_query_host, nq, slice_rows, group, im);
    std::vector<i64> img(im.img.begin(), im.img.end()), pair_offs((size_t)n_scopes + 1, 0), item_start((size_t)n_scopes + 1, 0), order((size_t)nq);
    for (int i = 0; i < nq; ++i) ++pair_offs[(size_t)scope_of_query_host[i] + 1];
    for (int s = 0; s < n_scopes; ++s) {
        const i64 cnt = pair_offs[(size_t)s + 1];
        item_start[(size_t)s + 1] = item_start[(size_t)s] + (cnt + group - 1) / group * img[im.o_sl + s];
        pair_offs[(size_t)s + 1] += pair_offs[(size_t)s];
    }
    std::vector<i64> next(pair_offs.begin(), pair_offs.end() - 1);
    for (int i = 0; i < nq; ++i) order[(size_t)next[(size_t)scope_of_query_host[i]]++] = i;
    const int64_t n_items = item_start[(size_t)n_scopes];
    const bool count_only = !out_items && items_cap == 0;
    HR_REQUIRE(count_only || out_items, "out_items is null");
    HR_REQUIRE(count_only || items_cap >= n_items, "items_cap = %lld is below the call's %lld items", (long long)items_cap, (long long)n_items);
    *out_count = n_items;
    if (count_only) return HIPRAG_OK;
    const SliceTables t{img.data(), img.data() + im.o_slice, img.data() + im.o_off, pair_offs.data(), order.data(), item_start.data(), n_scopes};
    if (flat) decode_items<16, 256>(t, n_items, out_items);
    else if (exact) decode_items<8, 16>(t, n_items, out_items);
    else decode_items<8, 256>(t, n_items, out_items);
    return HIPRAG_OK;
}

// the fold schedule of the wide kernel (dense_plan.h): what wide_park asks for the tile it parks
int32_t hiprag_wide_fold(int64_t p0, int64_t n, int32_t wg, int32_t wave, int32_t every, uint8_t* out_fold, int32_t* out_first,
                         int32_t* out_default)
{
    HR_REQUIRE(p0 >= 0 && n >= 0 && p0 + n <= ((int64_t)1 << 31) && wg >= 0 && wg < (1 << 28) && wave >= 0 && wave < 8 && wide_fold_every_ok(every),
               "hiprag_wide_fold: 0 <= p0, p0 + n <= 2^31, 0 <= wg < 2^28, 0 <= wave < 8, every a power of two in 1..%d", kWideFoldMax);
    HR_REQUIRE(n == 0 || out_fold, "hiprag_wide_fold: n > 0 needs the output array");
    for (int64_t i = 0; i < n; ++i) out_fold[i] = wide_fold((uint32_t)(p0 + i), (uint32_t)wg, (uint32_t)wave, (uint32_t)every) ? 1 : 0;
    if (out_first) *out_first = kWideFoldFirst;
    if (out_default) *out_default = kWideFoldEvery;
    return HIPRAG_OK;
}

int32_t hiprag_probe_read_gbps(int32_t device, int64_t bytes, int32_t reps, double* out_gbps)
{
    HR_REQUIRE(out_gbps && bytes >= (1 << 20) && reps > 0, "bad probe arguments");
    HR_CHECK_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    HR_CHECK_HIP(hipGetDeviceProperties(&prop, device));
    const int ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const long long nblocks = bytes / 65536;
    const long long waves = (long long)ncu * 8;
    const int bpw = (int)((nblocks + waves - 1) / waves), passes = 4;
    void* x = nullptr;
    float* out = nullptr;
    HR_CHECK_HIP(hipMalloc(&x, (size_t)nblocks * 65536));
    hipError_t e = hipMalloc(&out, 64);
    if (e != hipSuccess) { (void)hipFree(x); HR_CHECK_HIP(e); }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.f;
    e = hipMemset(x, 0, (size_t)nblocks * 65536);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) {
        for (int it = 0; it < 2; ++it)
            hipLaunchKernelGGL(read_probe_kernel, dim3(ncu), dim3(512), 0, 0, (const probe_f4*)x, nblocks, bpw, passes, out);
        (void)hipEventRecord(e0, 0);
        for (int it = 0; it < reps; ++it)
            hipLaunchKernelGGL(read_probe_kernel, dim3(ncu), dim3(512), 0, 0, (const probe_f4*)x, nblocks, bpw, passes, out);
        (void)hipEventRecord(e1, 0);
        e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(out);
    (void)hipFree(x);
    HR_CHECK_HIP(e);
    *out_gbps = (double)nblocks * 65536.0 * passes * reps / ((double)ms * 1e-3) / 1e9;
    return HIPRAG_OK;
}

int32_t hiphybrid_search_dev(uint64_t dense_h, uint64_t bm25_h, const float* q_dev, const uint32_t* term_ids_host,
                             const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, float c, float w_dense,
                             float w_sparse, int64_t* lists_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    HR_REQUIRE(nq >= 0 && depth > 0 && k > 0, "bad hybrid shape");
    if (nq == 0) return HIPRAG_OK;
    HR_REQUIRE(q_dev && q_offsets_host && lists_dev && out_scores_dev && out_ids_dev, "null argument");
    int32_t rc;
    if ((rc = hipidx_reserve_search(dense_h, depth))) return rc;   // also makes the index's device current on this thread
    int cur_dev = 0;
    HR_CHECK_HIP(hipGetDevice(&cur_dev));
    const size_t nd = (size_t)nq * depth;      // lists_dev: int64 [4][nq][depth] = dense score bits | dense ids | BM25 score bits | BM25 ids
    hipStream_t main = (hipStream_t)stream;
    LegLease lease;
    if ((rc = scan_streams().get(cur_dev, lease.hp))) return rc;
    if ((rc = leg_events().acquire(cur_dev, lease.e))) return rc;
    lease.held = true;
    // the dense leg starts where the caller's stream is now (whatever produced q_dev is ahead of it), on the scan stream ...
    HR_CHECK_HIP(hipEventRecord(lease.e.in, main));
    HR_CHECK_HIP(hipStreamWaitEvent(lease.hp, lease.e.in, 0));
    lease.busy = true;
    {
        SpareCusScope spare;
        if ((rc = spare.enter(dense_h, kHybridSpareCus))) return rc;
        if ((rc = hipidx_search_dev(dense_h, q_dev, nq, depth, reinterpret_cast<double*>(lists_dev), nullptr, lists_dev + nd, lease.hp)))
            return rc;
    }
    HR_CHECK_HIP(hipEventRecord(lease.e.dense_done, lease.hp));
    // ... the BM25 leg beside it on the caller's stream, on the CUs the scan leaves (and on all of them once it is done) ...
    if ((rc = hipbm25_search_dev(bm25_h, term_ids_host, q_offsets_host, nq, depth, reinterpret_cast<double*>(lists_dev + 2 * nd), nullptr,
                                 lists_dev + 3 * nd, stream))) return rc;
    // ... and the fusion behind both
    HR_CHECK_HIP(hipStreamWaitEvent(main, lease.e.dense_done, 0));
    lease.busy = false;   // from here the caller's stream orders everything that touches the caller's buffers
    return hiprrf_fuse_dev(lists_dev + nd, lists_dev + 3 * nd, nq, depth, depth, k, c, w_dense, w_sparse, out_scores_dev, out_ids_dev, stream);
}

int32_t hiphybrid_search(uint64_t dense_h, uint64_t bm25_h, const float* q_host, const uint32_t* term_ids_host,
                         const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, float c, float w_dense,
                         float w_sparse, float* out_scores, int64_t* out_ids)
{
    HR_REQUIRE(nq >= 0 && depth > 0 && k > 0, "bad hybrid shape");
    if (nq == 0) return HIPRAG_OK;
    HR_REQUIRE(q_host && q_offsets_host && out_scores && out_ids, "null argument");
    int32_t d = 0, rc;
    if ((rc = hipidx_dim(dense_h, &d))) return rc;
    if ((rc = hipidx_reserve_search(dense_h, depth))) return rc;   // also makes the index's device current on this thread
    DevBuf q, lists, os, oi;
    if ((rc = q.reserve((size_t)nq * d * sizeof(float)))) return rc;
    if ((rc = lists.reserve((size_t)4 * nq * depth * 8))) return rc;
    if ((rc = os.reserve((size_t)nq * k * sizeof(float)))) return rc;
    if ((rc = oi.reserve((size_t)nq * k * 8))) return rc;
    HR_CHECK_HIP(hipMemcpy(q.p, q_host, (size_t)nq * d * sizeof(float), hipMemcpyHostToDevice));
    rc = hiphybrid_search_dev(dense_h, bm25_h, q.as<float>(), term_ids_host, q_offsets_host, nq, depth, k, c, w_dense, w_sparse,
                              lists.as<int64_t>(), os.as<float>(), oi.as<int64_t>(), nullptr);
    // whatever the call enqueued (helper streams included: the null stream waits for them, or the call drained them on its
    // error path) is done before the frame's buffers go
    if (rc) { (void)hipDeviceSynchronize(); return rc; }
    HR_CHECK_HIP(hipMemcpy(out_scores, os.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_ids, oi.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

// ---- scoped hybrid: both legs over the rows / documents of the query's scope, RRF behind them -------------------------------
static int32_t check_scoped_hybrid(uint64_t dense_h, uint64_t bm25_h, const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k)
{
    HR_REQUIRE(nq >= 0 && depth > 0 && k > 0, "bad hybrid shape");
    HR_REQUIRE(depth <= 64, "depth must be in 1..64 for a scoped hybrid search (got %d): the limit of the scoped BM25 leg", depth);
    if (nq == 0) return HIPRAG_OK;
    HR_REQUIRE(q_offsets_host, "null argument");
    HR_REQUIRE(q_offsets_host[0] >= 0, "q_offsets must start >= 0");
    for (int b = 0; b < nq; ++b) HR_REQUIRE(q_offsets_host[b] <= q_offsets_host[b + 1], "q_offsets must be non-decreasing");
    int64_t ntotal = 0, n_docs = 0;
    int32_t rc;
    if ((rc = hipidx_ntotal(dense_h, &ntotal))) return rc;
    if ((rc = bm25_n_docs(bm25_h, &n_docs))) return rc;
    HR_REQUIRE(ntotal == n_docs, "scoped hybrid search: the dense index holds %lld rows, the postings %lld documents (a row must be a document)",
               (long long)ntotal, (long long)n_docs);
    return HIPRAG_OK;
}

int32_t hiphybrid_search_scoped_dev(uint64_t dense_h, uint64_t bm25_h, const float* q_dev, const uint32_t* term_ids_host,
                                    const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, float c, float w_dense,
                                    float w_sparse, const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                    const int32_t* scope_of_query_host, int64_t* lists_dev, float* out_scores_dev, int64_t* out_ids_dev,
                                    void* stream)
{
    int32_t rc;
    if ((rc = check_scoped_hybrid(dense_h, bm25_h, q_offsets_host, nq, depth, k)) || nq == 0) return rc;
    HR_REQUIRE(q_dev && lists_dev && out_scores_dev && out_ids_dev, "null argument");
    HR_REQUIRE(term_ids_host || q_offsets_host[nq] == q_offsets_host[0], "null term ids");
    const size_t nd = (size_t)nq * depth;      // lists_dev as in hiphybrid_search_dev
    // the legs in stream order: the dense leg checks the scope tables (the sparse leg runs the same check_scope_tables,
    // scope_plan.h, over the same number of documents), so nothing is enqueued before every check has passed
    if ((rc = hipidx_search_scoped_dev(dense_h, q_dev, nq, depth, ranges_host, scope_offsets_host, n_scopes, scope_of_query_host,
                                       reinterpret_cast<double*>(lists_dev), nullptr, lists_dev + nd, stream)))
        return rc;
    if ((rc = hipbm25_search_scoped_dev(bm25_h, term_ids_host, q_offsets_host, nq, depth, ranges_host, scope_offsets_host, n_scopes,
                                        scope_of_query_host, reinterpret_cast<double*>(lists_dev + 2 * nd), nullptr, lists_dev + 3 * nd, stream)))
        return rc;
    return hiprrf_fuse_dev(lists_dev + nd, lists_dev + 3 * nd, nq, depth, depth, k, c, w_dense, w_sparse, out_scores_dev, out_ids_dev, stream);
}

int32_t hiphybrid_search_scoped(uint64_t dense_h, uint64_t bm25_h, const float* q_host, const uint32_t* term_ids_host,
                                const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, float c, float w_dense,
                                float w_sparse, const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                const int32_t* scope_of_query_host, int64_t* lists_host, float* out_scores, int64_t* out_ids)
{
    int32_t d = 0, rc;
    if ((rc = check_scoped_hybrid(dense_h, bm25_h, q_offsets_host, nq, depth, k)) || nq == 0) return rc;
    HR_REQUIRE(q_host && out_scores && out_ids, "null argument");
    if ((rc = hipidx_dim(dense_h, &d))) return rc;
    if ((rc = hipidx_reserve_search(dense_h, depth))) return rc;   // makes the index's device current on this thread
    DevBuf q, lists, os, oi;
    if ((rc = q.reserve((size_t)nq * d * sizeof(float)))) return rc;
    if ((rc = lists.reserve((size_t)4 * nq * depth * 8))) return rc;
    if ((rc = os.reserve((size_t)nq * k * sizeof(float)))) return rc;
    if ((rc = oi.reserve((size_t)nq * k * 8))) return rc;
    HR_CHECK_HIP(hipMemcpy(q.p, q_host, (size_t)nq * d * sizeof(float), hipMemcpyHostToDevice));
    rc = hiphybrid_search_scoped_dev(dense_h, bm25_h, q.as<float>(), term_ids_host, q_offsets_host, nq, depth, k, c, w_dense, w_sparse,
                                     ranges_host, scope_offsets_host, n_scopes, scope_of_query_host, lists.as<int64_t>(), os.as<float>(),
                                     oi.as<int64_t>(), nullptr);
    if (rc) { (void)hipDeviceSynchronize(); return rc; }   // whatever was enqueued is done before the frame's buffers go
    HR_CHECK_HIP(hipMemcpy(out_scores, os.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_ids, oi.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    if (lists_host) HR_CHECK_HIP(hipMemcpy(lists_host, lists.p, (size_t)4 * nq * depth * 8, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

// ---- scoped hybrid over the IVF index: the dense leg is hipivf_search_scoped_probe_dev at depth `depth` ---------------------
static int32_t check_ivf_scoped_hybrid(uint64_t ivf_h, uint64_t bm25_h, const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k,
                                       int32_t* out_d)
{
    HR_REQUIRE(nq >= 0 && depth > 0 && k > 0, "bad hybrid shape");
    HR_REQUIRE(depth <= 64, "depth must be in 1..64 for a scoped hybrid search (got %d): the limit of the scoped BM25 leg", depth);
    if (nq == 0) return HIPRAG_OK;
    HR_REQUIRE(q_offsets_host, "null argument");
    HR_REQUIRE(q_offsets_host[0] >= 0, "q_offsets must start >= 0");
    for (int b = 0; b < nq; ++b) HR_REQUIRE(q_offsets_host[b] <= q_offsets_host[b + 1], "q_offsets must be non-decreasing");
    int64_t n = 0, n_docs = 0;
    int32_t rc, metric = 0;
    if ((rc = hipivf_meta(ivf_h, out_d, &metric, &n))) return rc;
    if ((rc = bm25_n_docs(bm25_h, &n_docs))) return rc;
    HR_REQUIRE(n == n_docs, "scoped IVF hybrid search: the IVF index holds %lld rows, the postings %lld documents (a row must be a document)",
               (long long)n, (long long)n_docs);
    return HIPRAG_OK;
}

int32_t hiphybrid_search_ivf_scoped_dev(uint64_t ivf_h, uint64_t bm25_h, const float* q_dev, const uint32_t* term_ids_host,
                                        const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, int32_t nprobe,
                                        int32_t probe_mode, float c, float w_dense, float w_sparse, const int64_t* ranges_host,
                                        const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                        int64_t* lists_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    int32_t rc, d = 0;
    if ((rc = check_ivf_scoped_hybrid(ivf_h, bm25_h, q_offsets_host, nq, depth, k, &d)) || nq == 0) return rc;
    HR_REQUIRE(q_dev && lists_dev && out_scores_dev && out_ids_dev, "null argument");
    HR_REQUIRE(term_ids_host || q_offsets_host[nq] == q_offsets_host[0], "null term ids");
    const size_t nd = (size_t)nq * depth;      // lists_dev as in hiphybrid_search_dev
    // the legs in stream order, as in hiphybrid_search_scoped_dev: the dense leg checks the scope tables for both (one
    // check_scope_tables, the same n)
    if ((rc = hipivf_search_scoped_probe_dev(ivf_h, q_dev, nq, depth, nprobe, probe_mode, ranges_host, scope_offsets_host, n_scopes,
                                             scope_of_query_host, reinterpret_cast<double*>(lists_dev), nullptr, lists_dev + nd, stream)))
        return rc;
    if ((rc = hipbm25_search_scoped_dev(bm25_h, term_ids_host, q_offsets_host, nq, depth, ranges_host, scope_offsets_host, n_scopes,
                                        scope_of_query_host, reinterpret_cast<double*>(lists_dev + 2 * nd), nullptr, lists_dev + 3 * nd, stream)))
        return rc;
    return hiprrf_fuse_dev(lists_dev + nd, lists_dev + 3 * nd, nq, depth, depth, k, c, w_dense, w_sparse, out_scores_dev, out_ids_dev, stream);
}

int32_t hiphybrid_search_ivf_scoped(uint64_t ivf_h, uint64_t bm25_h, const float* q_host, const uint32_t* term_ids_host,
                                    const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t k, int32_t nprobe,
                                    int32_t probe_mode, float c, float w_dense, float w_sparse, const int64_t* ranges_host,
                                    const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                    int64_t* lists_host, float* out_scores, int64_t* out_ids)
{
    int32_t d = 0, rc;
    if ((rc = check_ivf_scoped_hybrid(ivf_h, bm25_h, q_offsets_host, nq, depth, k, &d)) || nq == 0) return rc;
    HR_REQUIRE(q_host && out_scores && out_ids, "null argument");
    if ((rc = ivf_make_device_current(ivf_h))) return rc;
    DevBuf q, lists, os, oi;
    if ((rc = q.reserve((size_t)nq * d * sizeof(float)))) return rc;
    if ((rc = lists.reserve((size_t)4 * nq * depth * 8))) return rc;
    if ((rc = os.reserve((size_t)nq * k * sizeof(float)))) return rc;
    if ((rc = oi.reserve((size_t)nq * k * 8))) return rc;
    HR_CHECK_HIP(hipMemcpy(q.p, q_host, (size_t)nq * d * sizeof(float), hipMemcpyHostToDevice));
    rc = hiphybrid_search_ivf_scoped_dev(ivf_h, bm25_h, q.as<float>(), term_ids_host, q_offsets_host, nq, depth, k, nprobe, probe_mode, c,
                                         w_dense, w_sparse, ranges_host, scope_offsets_host, n_scopes, scope_of_query_host,
                                         lists.as<int64_t>(), os.as<float>(), oi.as<int64_t>(), nullptr);
    if (rc) { (void)hipDeviceSynchronize(); return rc; }   // whatever was enqueued is done before the frame's buffers go
    HR_CHECK_HIP(hipMemcpy(out_scores, os.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_ids, oi.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    if (lists_host) HR_CHECK_HIP(hipMemcpy(lists_host, lists.p, (size_t)4 * nq * depth * 8, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

// ---- BGE-M3's combined score of candidate ids (include/hiprag.h): the three component entries, then m3_score.hip ------------
extern "C++" {
namespace {
// Workspace of hipm3_score_dev: the components of the call ([nq][depth] fp64 + 3 x fp32) and the ranked outputs hipmaxsim_dev
// insists on writing ([nq][k] fp32 + int64).  One per device for the process; a call holds `mu` while it enqueues and waits
// device-side for the previous call on another stream, so two streams never share the buffer in time.
struct M3Work {
    std::mutex mu;
    DevBuf buf;
    hipEvent_t prev = nullptr;
    hipStream_t prev_stream = nullptr;
    bool prev_set = false;
};
M3Work& m3_work(int dev)
{
    static std::mutex mu;
    static std::map<int, std::unique_ptr<M3Work>> works;
    std::lock_guard<std::mutex> g(mu);
    std::unique_ptr<M3Work>& w = works[dev];
    if (!w) w.reset(new M3Work());
    return *w;
}
}  // namespace
}  // extern "C++"

int32_t hipm3_score_dev(uint64_t dense_h, uint64_t bm25_h, uint64_t mv_h, const float* q_dev, const uint32_t* term_ids_host,
                        const float* term_weights_host, const int32_t* q_offsets_host, const void* q_vecs_dev, const int32_t* q_counts_dev,
                        int32_t q_stride, int32_t nq, const int64_t* cand_ids_dev, int32_t depth, int32_t k, double w_dense, double w_sparse,
                        double w_colbert, float* out_parts_dev, double* out_pair_scores_dev, double* out_scores_dev, int64_t* out_ids_dev,
                        int32_t* out_pos_dev, void* stream)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(1 <= k && k <= depth && depth <= 256, "1 <= k <= depth <= 256 does not hold (k = %d, depth = %d)", k, depth);
    HR_REQUIRE(std::isfinite(w_dense) && std::isfinite(w_sparse) && std::isfinite(w_colbert) && w_dense >= 0.0 && w_sparse >= 0.0 &&
                   w_colbert >= 0.0, "the weights must be finite and >= 0 (got %g, %g, %g)", w_dense, w_sparse, w_colbert);
    HR_REQUIRE(w_dense > 0.0 || w_sparse > 0.0 || w_colbert > 0.0, "at least one weight must be > 0");
    HR_REQUIRE(cand_ids_dev && out_scores_dev && out_ids_dev, "null argument");
    const bool use_d = w_dense > 0.0, use_s = w_sparse > 0.0, use_c = w_colbert > 0.0;
    HR_REQUIRE(!use_d || q_dev, "q is null and w_dense > 0");
    HR_REQUIRE(!use_s || q_offsets_host, "q_offsets is null and w_sparse > 0");
    HR_REQUIRE(!use_c || (q_vecs_dev && q_counts_dev), "q_vecs / q_counts is null and w_colbert > 0");
    HR_REQUIRE(!use_c || (1 <= q_stride && q_stride <= 512), "q_stride must be in 1..512 (got %d)", q_stride);
    int32_t rc, metric = 0;
    int64_t ntotal = 0, id_base = 0;
    if ((rc = hipidx_ntotal(dense_h, &ntotal)) || (rc = hipidx_metric(dense_h, &metric)) || (rc = dense_id_base(dense_h, &id_base))) return rc;
    if (use_s) {
        int64_t n_docs = 0, sb = 0;
        if ((rc = bm25_n_docs(bm25_h, &n_docs)) || (rc = bm25_id_base(bm25_h, &sb))) return rc;
        HR_REQUIRE(n_docs == ntotal, "the dense index holds %lld rows, the postings %lld documents (a row must be a document)",
                   (long long)ntotal, (long long)n_docs);
        HR_REQUIRE(sb == id_base, "the dense index has id_base %lld, the postings %lld", (long long)id_base, (long long)sb);
    }
    if (use_c) {
        int64_t sz[4];
        if ((rc = hipmv_sizes(mv_h, sz))) return rc;
        HR_REQUIRE(sz[0] == ntotal, "the dense index holds %lld rows, the multi-vector store %lld documents (a row must be a document)",
                   (long long)ntotal, (long long)sz[0]);
        HR_REQUIRE(id_base >= 0, "id_base must not be negative for the ColBERT leg (got %lld)", (long long)id_base);
    }
    int dev = 0;
    HR_CHECK_HIP(hipGetDevice(&dev));   // the dense getters made the index's device current
    hipStream_t st = (hipStream_t)stream;
    M3Work& W = m3_work(dev);
    std::lock_guard<std::mutex> guard(W.mu);
    const size_t pairs = (size_t)nq * depth, nk = (size_t)nq * k;
    // fp64 first, then int64, then the 4-byte arrays: every piece stays aligned
    const size_t bytes = pairs * 8 + nk * 8 + (3 * pairs + nk) * 4;
    if ((rc = W.buf.reserve(bytes))) return rc;
    double* d64 = W.buf.as<double>();
    int64_t* mid = reinterpret_cast<int64_t*>(d64 + pairs);
    float* d32 = reinterpret_cast<float*>(mid + nk);
    float* s32 = d32 + pairs;
    float* c32 = s32 + pairs;
    float* msc = c32 + pairs;
    if (W.prev_set && W.prev_stream != st) HR_CHECK_HIP(hipStreamWaitEvent(st, W.prev, 0));
    // the legs in stream order, each through its own entry (its checks, its lock, its bits)
    if (use_d && (rc = hipidx_score_ids_dev(dense_h, q_dev, nq, cand_ids_dev, depth, d64, d32, stream))) return rc;
    if (use_s && (rc = hipbm25_score_ids_dev(bm25_h, term_ids_host, term_weights_host, q_offsets_host, nq, cand_ids_dev, depth, s32, stream)))
        return rc;
    if (use_c && (rc = hipmaxsim_dev(mv_h, q_vecs_dev, q_counts_dev, q_stride, nq, cand_ids_dev, depth, id_base, k, c32, msc, mid, nullptr, stream)))
        return rc;
    M3Combine a;
    a.cand = cand_ids_dev;
    a.dense64 = use_d ? d64 : nullptr; a.dense32 = use_d ? d32 : nullptr;
    a.sparse32 = use_s ? s32 : nullptr; a.maxsim32 = use_c ? c32 : nullptr;
    a.w_dense = w_dense; a.w_sparse = w_sparse; a.w_colbert = w_colbert;
    a.w_sum = (w_dense + w_sparse) + w_colbert;
    a.id_base = id_base; a.ntotal = ntotal;
    a.depth = depth; a.k = k; a.l2 = metric == HIPRAG_METRIC_L2;
    a.out_parts = out_parts_dev; a.out_pairs = out_pair_scores_dev; a.out_scores = out_scores_dev; a.out_ids = out_ids_dev; a.out_pos = out_pos_dev;
    if ((rc = launch_m3_combine(a, nq, st))) return rc;
    if (!W.prev) HR_CHECK_HIP(hipEventCreateWithFlags(&W.prev, hipEventDisableTiming));
    HR_CHECK_HIP(hipEventRecord(W.prev, st));
    W.prev_set = true;
    W.prev_stream = st;
    return HIPRAG_OK;
}

int32_t hipm3_score_host(uint64_t dense_h, uint64_t bm25_h, uint64_t mv_h, const float* q_host, const uint32_t* term_ids_host,
                         const float* term_weights_host, const int32_t* q_offsets_host, const void* q_vecs_host, const int32_t* q_counts_host,
                         int32_t q_stride, int32_t nq, const int64_t* cand_ids_host, int32_t depth, int32_t k, double w_dense, double w_sparse,
                         double w_colbert, float* out_parts, double* out_pair_scores, double* out_scores, int64_t* out_ids, int32_t* out_pos)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(1 <= k && k <= depth && depth <= 256, "1 <= k <= depth <= 256 does not hold (k = %d, depth = %d)", k, depth);
    HR_REQUIRE(cand_ids_host && out_scores && out_ids, "null argument");
    const bool use_d = w_dense > 0.0, use_c = w_colbert > 0.0;
    HR_REQUIRE(!use_d || q_host, "q is null and w_dense > 0");
    HR_REQUIRE(!use_c || (q_vecs_host && q_counts_host), "q_vecs / q_counts is null and w_colbert > 0");
    HR_REQUIRE(!use_c || (1 <= q_stride && q_stride <= 512), "q_stride must be in 1..512 (got %d)", q_stride);
    int32_t rc, d = 0;
    int64_t sz[4] = {0, 0, 0, 0};
    if ((rc = hipidx_dim(dense_h, &d))) return rc;   // makes the index's device current on this thread
    if (use_c && (rc = hipmv_sizes(mv_h, sz))) return rc;
    const size_t pairs = (size_t)nq * depth, nk = (size_t)nq * k;
    const size_t qb = use_d ? (size_t)nq * d * 4 : 0, vb = use_c ? (size_t)nq * q_stride * (size_t)sz[2] * 2 : 0;
    DevBuf q, qv, qc, cand, parts, ps, os, oi, op;
    if ((rc = q.reserve(std::max<size_t>(qb, 16))) || (rc = qv.reserve(std::max<size_t>(vb, 16))) || (rc = qc.reserve((size_t)nq * 4)) ||
        (rc = cand.reserve(pairs * 8)) || (rc = parts.reserve(pairs * 12)) || (rc = ps.reserve(pairs * 8)) || (rc = os.reserve(nk * 8)) ||
        (rc = oi.reserve(nk * 8)) || (rc = op.reserve(nk * 4)))
        return rc;
    if (use_d) HR_CHECK_HIP(hipMemcpy(q.p, q_host, qb, hipMemcpyHostToDevice));
    if (use_c) {
        HR_CHECK_HIP(hipMemcpy(qv.p, q_vecs_host, vb, hipMemcpyHostToDevice));
        HR_CHECK_HIP(hipMemcpy(qc.p, q_counts_host, (size_t)nq * 4, hipMemcpyHostToDevice));
    }
    HR_CHECK_HIP(hipMemcpy(cand.p, cand_ids_host, pairs * 8, hipMemcpyHostToDevice));
    rc = hipm3_score_dev(dense_h, bm25_h, mv_h, use_d ? q.as<float>() : nullptr, term_ids_host, term_weights_host, q_offsets_host,
                         use_c ? qv.p : nullptr, use_c ? qc.as<int32_t>() : nullptr, q_stride, nq, cand.as<int64_t>(), depth, k, w_dense, w_sparse,
                         w_colbert, parts.as<float>(), ps.as<double>(), os.as<double>(), oi.as<int64_t>(), op.as<int32_t>(), nullptr);
    if (rc) { (void)hipDeviceSynchronize(); return rc; }   // whatever was enqueued is done before the frame's buffers go
    if (out_parts) HR_CHECK_HIP(hipMemcpy(out_parts, parts.p, pairs * 12, hipMemcpyDeviceToHost));
    if (out_pair_scores) HR_CHECK_HIP(hipMemcpy(out_pair_scores, ps.p, pairs * 8, hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_scores, os.p, nk * 8, hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_ids, oi.p, nk * 8, hipMemcpyDeviceToHost));
    if (out_pos) HR_CHECK_HIP(hipMemcpy(out_pos, op.p, nk * 4, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

// ---- row-sharded hybrid step: the library's two halves around the caller's ONE all-gather ----------------

int32_t hiphybrid_shard_begin_dev(uint64_t dense_h, uint64_t bm25_h, const float* q_dev, const uint32_t* term_ids_host,
                                  const int32_t* q_offsets_host, int32_t nq, int32_t depth, int32_t slot, int64_t* pack_dev,
                                  float* scratch_f32_dev, void* scan_stream, void* tail_stream)
{
    HR_REQUIRE(nq > 0 && depth > 0, "bad hybrid shape");
    HR_REQUIRE(q_dev && q_offsets_host && pack_dev && scratch_f32_dev, "null argument");
    int32_t rc;
    // the HBM-heavy part stays on the caller's scan stream (scans chained one after the other) ...
    if ((rc = hipidx_search_begin_dev(dense_h, q_dev, nq, depth, slot, scan_stream))) return rc;   // makes the device current
    int dev = 0;
    HR_CHECK_HIP(hipGetDevice(&dev));
    hipEvent_t scanned = nullptr;
    if ((rc = step_events().get(dev, slot, scanned))) return rc;
    if (tail_stream != scan_stream) {
        HR_CHECK_HIP(hipEventRecord(scanned, (hipStream_t)scan_stream));
        HR_CHECK_HIP(hipStreamWaitEvent((hipStream_t)tail_stream, scanned, 0));
    }
    // ... everything latency-bound on the tail stream, beside later scans: the dense finish and the BM25 leg fill the two
    // halves of the pack, [leg][score bits | ids][nq][depth]
    const size_t leg = (size_t)2 * nq * depth;
    if ((rc = hipidx_search_finish_dev(dense_h, q_dev, nq, depth, slot, reinterpret_cast<double*>(pack_dev), scratch_f32_dev,
                                       pack_dev + (size_t)nq * depth, tail_stream)))
        return rc;
    return hipbm25_search_dev(bm25_h, term_ids_host, q_offsets_host, nq, depth, reinterpret_cast<double*>(pack_dev + leg),
                              scratch_f32_dev + (size_t)nq * depth, pack_dev + leg + (size_t)nq * depth, tail_stream);
}

int32_t hiphybrid_shard_end_dev(const int64_t* gathered_dev, int32_t n_parts, int32_t nq, int32_t depth, int32_t k,
                                int32_t dense_metric, float c, float w_dense, float w_sparse, int64_t* scratch_dev,
                                float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    HR_REQUIRE(n_parts > 0 && nq > 0 && depth > 0 && k > 0, "bad hybrid shape");
    HR_REQUIRE(gathered_dev && scratch_dev && out_scores_dev && out_ids_dev, "null argument");
    const size_t nd = (size_t)nq * depth, part = 4 * nd;      // one rank's pack: 2 legs x {scores, ids} x nq x depth
    int64_t* dl_s = scratch_dev;                              // merged dense leg: score bits | ids, then the sparse leg
    int64_t* dl_i = scratch_dev + nd;
    int64_t* sl_s = scratch_dev + 2 * nd;
    int64_t* sl_i = scratch_dev + 3 * nd;
    int32_t rc;
    // each leg merged GLOBALLY with the canonical comparator, then RRF over the two global lists (ranks are global: fusing
    // per shard and merging afterwards would be a different function)
    if ((rc = hiprag_merge_topk_dev(reinterpret_cast<const double*>(gathered_dev), gathered_dev + nd, n_parts, nq, depth, depth,
                                    (int64_t)part, dense_metric, reinterpret_cast<double*>(dl_s), nullptr, dl_i, stream)))
        return rc;
    if ((rc = hiprag_merge_topk_dev(reinterpret_cast<const double*>(gathered_dev + 2 * nd), gathered_dev + 3 * nd, n_parts, nq, depth,
                                    depth, (int64_t)part, HIPRAG_METRIC_IP, reinterpret_cast<double*>(sl_s), nullptr, sl_i, stream)))
        return rc;
    return hiprrf_fuse_dev(dl_i, sl_i, nq, depth, depth, k, c, w_dense, w_sparse, out_scores_dev, out_ids_dev, stream);
}

int32_t hiprag_scan_stream(int32_t device, void** out_stream)
{
    HR_REQUIRE(out_stream, "null out");
    hipStream_t st = nullptr;
    int32_t rc = scan_streams().get(device, st);
    if (rc) return rc;
    *out_stream = (void*)st;
    return HIPRAG_OK;
}

int32_t hiprag_tail_stream(int32_t device, int32_t which, void** out_stream)
{
    HR_REQUIRE(out_stream && (which == 0 || which == 1), "which must be 0 or 1");
    hipStream_t st = nullptr;
    int32_t rc = scan_streams().get_tail(device, which, st);
    if (rc) return rc;
    *out_stream = (void*)st;
    return HIPRAG_OK;
}

int32_t hiprag_device_sync(int32_t device)
{
    HR_CHECK_HIP(hipSetDevice(device));
    HR_CHECK_HIP(hipDeviceSynchronize());
    return HIPRAG_OK;
}

int32_t hiprag_event_create(uint64_t* out_event)
{
    HR_REQUIRE(out_event, "null out");
    auto ev = std::make_shared<hipEvent_t>();
    HR_CHECK_HIP(hipEventCreate(ev.get()));
    *out_event = events().put(ev);
    return HIPRAG_OK;
}

int32_t hiprag_event_record(uint64_t event, void* stream)
{
    auto ev = events().get(event);
    if (!ev) { set_error("unknown event handle"); return HIPRAG_E_HANDLE; }
    HR_CHECK_HIP(hipEventRecord(*ev, (hipStream_t)stream));
    return HIPRAG_OK;
}

int32_t hiprag_event_elapsed_ms(uint64_t start, uint64_t stop, float* out_ms)
{
    HR_REQUIRE(out_ms, "null out");
    auto a = events().get(start);
    auto b = events().get(stop);
    if (!a || !b) { set_error("unknown event handle"); return HIPRAG_E_HANDLE; }
    HR_CHECK_HIP(hipEventSynchronize(*b));
    HR_CHECK_HIP(hipEventElapsedTime(out_ms, *a, *b));
    return HIPRAG_OK;
}

int32_t hiprag_event_destroy(uint64_t event)
{
    auto ev = events().get(event);
    if (!ev) { set_error("unknown event handle"); return HIPRAG_E_HANDLE; }
    (void)hipEventDestroy(*ev);
    events().erase(event);
    return HIPRAG_OK;
}

}  // extern "C"
