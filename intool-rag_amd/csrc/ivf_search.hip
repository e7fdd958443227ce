// ivf_search.hip -- IVF-Flat search on top of the flat index: the query-major probe kernel, the list-major batch kernel,
// the hipivf_* handle and its accessors.  The k-means build and save / load are ivf_build.hip.
#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

#include "ivf_internal.h"

namespace hiprag {
namespace {

// ------------------------------------------------------------------------------------------------------
// IVF-Flat on top of the flat index (BASELINE north_star: "the flat-IP / IVF distance scan"; the reference itself builds
// faiss.IndexFlatL2 only, rag/storage/faiss_index.py:123).  The rows are stored PERMUTED by inverted list in an ordinary
// flat index (every list starts on a 32-row block; padding rows carry the original id -1), the nlist centroids in a second
// one.  A search is: exact top-nprobe of the query among the centroids (the flat search, dense_index.hip) -> every probed list is cut
// into slices of kIvfRows rows, one workgroup per (query, list, slice) re-scores its rows in fp64 straight from the fp32
// rows (the same rescore4 as the flat finish, dense_layout.h: a row's score is the same bits in both indexes) and keeps its best k ->
// the canonical merge of the partial lists (hiprag_merge_topk_dev).  Approximate by construction unless nprobe = nlist,
// where every row is scored and the result equals the flat index's bit for bit (tests/test_ivf_gpu.py).
// Bound: HBM -- rows probed x d_pad x 4 bytes per query.  This QUERY-MAJOR order (ivf_probe_kernel, hipivf_search_dev) is the
// low-latency path for one query or a few: every workgroup streams its rows for a single query, so a list that many queries
// of a batch probe is read once per query.  The LIST-MAJOR order (ivf_batch_kernel, hipivf_search_batch_dev, below) reads a
// slice once for up to kIvfBatchG queries and gives the same bits (DESIGN 8 has the measured rates of both).
// ------------------------------------------------------------------------------------------------------
constexpr int kIvfRows = 256;   // rows per workgroup of the probe kernel
struct IvfArgs {
    const float4* xb;
    const float* q;        // [nq, d]
    const i64* probe;      // [nq, nprobe] list ids from the centroid search (-1 = no such list)
    const i64* offs;       // [nlist + 1] first stored row of every list (multiples of 32)
    const i64* orig;       // [stored rows] original id, -1 for padding
    double* ps;            // [nprobe * smax][nq][k] partial scores
    i64* pi;               //                         partial ids
    int d, P, k, nq, nprobe, smax;
};

template <int METRIC>
__global__ __launch_bounds__(256) void ivf_probe_kernel(IvfArgs a)
{
    __shared__ u64 keys[kIvfRows];
    __shared__ i64 ids[kIvfRows];
    __shared__ KeyId red[2 * 4];
    __shared__ float qv[kMaxDPad];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y, part = blockIdx.x;
    const int j = part / a.smax, sl = part - j * a.smax;
    const int dpad = a.P * 8;
    const i64 list = a.probe[(i64)q * a.nprobe + j];
    i64 lo = 0, hi = 0;
    if (list >= 0) {
        lo = a.offs[list] + (i64)sl * kIvfRows;
        hi = min(a.offs[list + 1], lo + kIvfRows);
    }
    const int n = hi > lo ? (int)(hi - lo) : 0;     // workgroup-uniform
    double* ps = a.ps + ((i64)part * a.nq + q) * a.k;
    i64* pi = a.pi + ((i64)part * a.nq + q) * a.k;
    if (n == 0) {
        for (int r = tid; r < a.k; r += 256) { ps[r] = METRIC == HIPRAG_METRIC_IP ? -DBL_MAX : DBL_MAX; pi[r] = -1; }
        return;
    }
    for (int c = tid; c < dpad; c += 256) qv[c] = c < a.d ? a.q[(i64)q * a.d + c] : 0.f;
    for (int c = tid; c < kIvfRows; c += 256) { keys[c] = 0; ids[c] = -1; }
    __syncthreads();
    for (int g = wave; g * 4 < n; g += 4) {
        const i64 row0 = lo + (i64)g * 4;               // lists start on 32-row blocks and slices on 256 rows: quad-aligned
        const double s = rescore4<METRIC>(a.xb, a.P, row0 / kRowsPerBlock, (int)(row0 % kRowsPerBlock), qv);
        const i64 row = row0 + (lane & 3);
        if (lane < 4) {
            const i64 oid = row < hi ? a.orig[row] : -1;
            keys[g * 4 + lane] = oid >= 0 ? ord64(METRIC == HIPRAG_METRIC_IP ? s : -s) : 0ull;
            ids[g * 4 + lane] = oid;
        }
    }
    __syncthreads();
    wg_topk_rounds<256>(keys, ids, (n + 3) & ~3, a.k, red, [&](int r, u64 kk, i64 id) {
        ps[r] = kk ? (METRIC == HIPRAG_METRIC_IP ? unord64(kk) : -unord64(kk)) : (METRIC == HIPRAG_METRIC_IP ? -DBL_MAX : DBL_MAX);
        pi[r] = kk ? id : -1;
    });
}

// ------------------------------------------------------------------------------------------------------
// List-major batch search (hipivf_search_batch_dev).  The probe table [nq][nprobe] of the coarse step is inverted by the
// build's counting sort (pair (q, j) -> list), and the work is cut into ITEMS = (list, slice of kIvfRows stored rows, group
// of up to kIvfBatchG of the (q, j) pairs that probe the list).  The number of items depends on the data and stays on the
// device: group_item_scan_kernel (group_partials.hip) writes item_start[l] = items of the lists before l, a fixed grid strides over
// item_start[nlist], and an item finds its list by bisection (items of one slice are consecutive, so the workgroups that
// run side by side share the slice's rows in L2 / MALL).
//
// ivf_batch_kernel: 512 threads = 8 waves.  A wave takes a quad group (4 rows) of the slice, loads its 16 pieces per lane
// ONCE (rescore_load8 x 2: 16 float4 = 64 VGPRs, the register shape of rescore4) and scores them against every query of the
// group, whose vectors sit in LDS, with rescore4's own accumulate and butterfly (rescore_acc8, rescore_reduce16): a score
// is the bits hipivf_search_dev and the flat finish give.  Then wave w selects, for members w, w + 8, ... of the group, the
// best k of the slice's <= 256 keys (4 per lane in registers, k rounds of one wave-wide xor-shuffle reduction, no barrier)
// and writes partial (j, slice) of query q where ivf_probe_kernel writes it, so the canonical merge is reused untouched.
// Every slot has exactly one writer and there are no float atomics: the same bits from run to run.  Slots nobody writes
// (slices past the end of a list, -1 probes, ranks past the rows of a slice) are prefilled (fill_partials, group_partials.hip).
// LDS: G queries of d_pad floats + G x 256 keys + 256 ids = 98.1 KiB at d = 1024 (G = 16): one workgroup = 8 waves per CU,
// 2 per SIMD (one loads while the other computes); G = 32 would need 164 KiB.  Resource usage
// (-Rpass-analysis=kernel-resource-usage, gfx950), both metrics: 207 VGPRs (the 64 row floats are also kept converted to
// fp64 across the query loop), no scratch, no VGPR spill, occupancy 2 waves / SIMD -- the same one workgroup per CU that the
// LDS allows at d = 1024, so the registers cost nothing there; at small d they, not the LDS, hold it at one workgroup.
// Bound: this kernel, and in it the fp64 pipe and the LDS reads of the queries (16 ds_read_b128 per 64 fma per lane), not
// HBM: a slice of 1 MiB is read once per 16 queries.  Measured (profiles/ivf_batch_1m.json, 1M x 1024, nlist 1024, k = 10):
// 16 384 queries at nprobe 8 take 29.5 ms = 555 k queries/s against 187 k for hipivf_search_dev and 197 k for the flat
// search; the kernel is 26.4 ms of the call, the merge 0.6 ms, the inversion 0.2 ms (profiles/ivf_batch_1m_kernel_stats.csv).
// From 1024 queries on this is the entry to call; at 64 queries the two are level (nprobe <= 8) and neither beats the flat
// search beyond nprobe 8.
// ------------------------------------------------------------------------------------------------------
constexpr int kIvfBatchG = 16;           // queries per work item
constexpr int kIvfBatchThreads = 512;
constexpr i64 kIvfBatchBudget = 512ll << 20;   // bytes of partial lists per chunk of queries (include/hiprag.h)
constexpr int kIvfBatchMaxChunk = 16384;       // queries per chunk at most

struct IvfBatchArgs {
    const float4* xb;
    const float* q;          // [nq, d]
    const i64* offs;         // [nlist + 1] first stored row of every list
    const i64* orig;         // [stored rows] original id, -1 for padding
    const i64* pair_offs;    // [nlist + 1] first entry of every list in `order`
    const i64* order;        // the pairs q * nprobe + j, sorted by probed list (stable)
    const i64* item_start;   // [nlist + 1] work items of the lists before l; [nlist] = the item count
    double* ps;              // [nprobe * smax][nq][k] partial scores (ivf_probe_kernel's layout)
    i64* pi;
    int d, P, k, nq, nprobe, smax, nlist;
};

template <int METRIC>
__global__ __launch_bounds__(kIvfBatchThreads) void ivf_batch_kernel(IvfBatchArgs a)
{
    constexpr int G = kIvfBatchG, S = kIvfRows, NW = kIvfBatchThreads / 64;
    extern __shared__ unsigned char ivf_smem[];
    const int dpad = a.P * 8;
    float* qv = reinterpret_cast<float*>(ivf_smem);            // [G][dpad]
    u64* keys = reinterpret_cast<u64*>(qv + (size_t)G * dpad); // [G][S]
    i64* ids = reinterpret_cast<i64*>(keys + G * S);           // [S]
    int* mq = reinterpret_cast<int*>(ids + S);                 // [G] query of a group member
    int* mj = mq + G;                                          // [G] its probe rank j
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rr = lane & 3, hh = (lane >> 2) & 1, pq = lane >> 3;
    const i64 nitems = a.item_start[a.nlist];
    for (i64 item = blockIdx.x; item < nitems; item += gridDim.x) {
        int l = 0, lh = a.nlist;                 // item_start[l] <= item < item_start[lh]
        while (lh - l > 1) {
            const int mid = (l + lh) >> 1;
            if (a.item_start[mid] <= item) l = mid; else lh = mid;
        }
        const i64 p0 = a.pair_offs[l], cnt = a.pair_offs[l + 1] - p0;
        const int ngroups = (int)((cnt + G - 1) / G);
        const i64 within = item - a.item_start[l];
        const int sl = (int)(within / ngroups), grp = (int)(within - (i64)sl * ngroups);
        const int gn = (int)min((i64)G, cnt - (i64)grp * G);          // 1..G members
        const i64 lo = a.offs[l] + (i64)sl * S, hi = min(a.offs[l + 1], lo + S);
        const int n = (int)(hi - lo);                                 // 1..S rows (lists start on 32-row blocks: quad-aligned)
        const int n4 = (n + 3) & ~3;
        if (tid < gn) {
            const i64 pair = a.order[p0 + (i64)grp * G + tid];
            mq[tid] = (int)(pair / a.nprobe);
            mj[tid] = (int)(pair % a.nprobe);
        }
        for (int c = tid; c < S; c += kIvfBatchThreads) ids[c] = c < n ? a.orig[lo + c] : -1;
        __syncthreads();
        for (int g = 0; g < gn; ++g) {
            const float* src = a.q + (i64)mq[g] * a.d;
            for (int c = tid; c < dpad; c += kIvfBatchThreads) qv[g * dpad + c] = c < a.d ? src[c] : 0.f;
        }
        __syncthreads();
        for (int g4 = wave; g4 * 4 < n; g4 += NW) {
            const i64 row0 = lo + (i64)g4 * 4;
            const float4* src = a.xb + (row0 / kRowsPerBlock) * a.P * kPieceVec4 + piece_slot(hh, (int)(row0 % kRowsPerBlock) + rr);
            float4 x0[8], x1[8];
            rescore_load8<0>(x0, src, pq, a.P);
            rescore_load8<1>(x1, src, pq, a.P);
            const i64 oid = ids[g4 * 4 + rr];
            for (int g = 0; g < gn; ++g) {
                double acc = 0.0;
                rescore_acc8<METRIC, 0>(acc, x0, pq, hh, a.P, qv + g * dpad);
                rescore_acc8<METRIC, 1>(acc, x1, pq, hh, a.P, qv + g * dpad);
                const double s = rescore_reduce16(acc);
                if (lane < 4) keys[g * S + g4 * 4 + lane] = oid >= 0 ? ord64(METRIC == HIPRAG_METRIC_IP ? s : -s) : 0ull;
            }
        }
        __syncthreads();
        for (int g = wave; g < gn; g += NW) {
            u64 kk[S / 64];
            i64 ii[S / 64];
#pragma unroll
            for (int t = 0; t < S / 64; ++t) {
                const int pos = t * 64 + lane;
                kk[t] = pos < n4 ? keys[g * S + pos] : 0ull;
                ii[t] = ids[pos];
            }
            const i64 o = ((i64)(mj[g] * a.smax + sl) * a.nq + mq[g]) * a.k;
            for (int r = 0; r < a.k; ++r) {
                KeyId best;
                best.key = 0;
                best.id = 0x7FFFFFFFFFFFFFFFll;
                best.pos = -1;
#pragma unroll
                for (int t = 0; t < S / 64; ++t)
                    if (kk[t] != 0 && key_before(kk[t], ii[t], best.key, best.id)) { best.key = kk[t]; best.id = ii[t]; best.pos = t * 64 + lane; }
                const KeyId w = wave_best(best);
                if (w.key == 0) break;            // exhausted (wave-uniform); the remaining ranks keep their padding
                if (lane == 0) {
                    a.ps[o + r] = METRIC == HIPRAG_METRIC_IP ? unord64(w.key) : -unord64(w.key);
                    a.pi[o + r] = w.id;
                }
#pragma unroll
                for (int t = 0; t < S / 64; ++t)
                    if (w.pos == t * 64 + lane) kk[t] = 0;
            }
        }
        __syncthreads();                          // the next item overwrites the LDS
    }
}

}  // namespace

Registry<IvfIndex>& ivf_reg()
{
    static Registry<IvfIndex> r;
    return r;
}

size_t clear_ivf_registry() { return ivf_reg().clear(); }

// iv.list_tab, made on first use and after an update has released it: per list its slices and its stored rows -- what
// group_item_scan takes per entry
int32_t ensure_list_tab(IvfIndex& iv)
{
    if (iv.list_tab.p) return HIPRAG_OK;
    const int nlist = iv.nlist;
    std::vector<i64> tab((size_t)2 * nlist);
    for (int l = 0; l < nlist; ++l) {
        const i64 rows = iv.offs_host[(size_t)l + 1] - iv.offs_host[(size_t)l];
        tab[(size_t)l] = (rows + kIvfRows - 1) / kIvfRows;
        tab[(size_t)nlist + l] = rows;
    }
    int32_t rc;
    if ((rc = iv.list_tab.reserve(tab.size() * 8))) return rc;
    HR_CHECK_HIP(hipMemcpy(iv.list_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    return HIPRAG_OK;
}
}  // namespace hiprag

using namespace hiprag;

extern "C" {

// ---- IVF-Flat ----------------------------------------------------------------------------------------------------------
int32_t hipivf_create(uint64_t rows_h, uint64_t centroids_h, const int64_t* list_offsets_host, const int64_t* orig_ids_host,
                      int32_t nlist, uint64_t* out_handle)
{
    HR_REQUIRE(out_handle && list_offsets_host && orig_ids_host && nlist > 0, "bad hipivf_create arguments");
    HR_GET_HANDLE(rows, reg(), rows_h, "unknown dense index handle");
    HR_GET_HANDLE(cents, reg(), centroids_h, "unknown dense index handle");
    HR_REQUIRE(rows->d == cents->d && rows->metric == cents->metric && rows->device == cents->device,
               "rows and centroids must agree in dimension, metric and device");
    HR_REQUIRE(cents->ntotal == nlist, "the centroid index holds %lld rows, nlist is %d", (long long)cents->ntotal, nlist);
    HR_REQUIRE(list_offsets_host[0] == 0 && list_offsets_host[nlist] == rows->ntotal, "list offsets must cover the stored rows [0, %lld)",
               (long long)rows->ntotal);
    auto iv = std::make_shared<IvfIndex>();
    iv->attach(rows, cents);
    iv->nlist = nlist;
    iv->offs_host.assign(list_offsets_host, list_offsets_host + nlist + 1);
    for (i64 r = 0; r < rows->ntotal; ++r) iv->n_rows += orig_ids_host[r] >= 0;
    for (int l = 0; l < nlist; ++l) {
        const i64 len = list_offsets_host[l + 1] - list_offsets_host[l];
        HR_REQUIRE(len >= 0 && list_offsets_host[l] % kRowsPerBlock == 0, "list %d must start on a 32-row block and not be negative", l);
        iv->maxlen = std::max(iv->maxlen, len);
    }
    HR_CHECK_HIP(hipSetDevice(rows->device));
    int32_t rc;
    if ((rc = iv->offs.reserve((size_t)(nlist + 1) * 8))) return rc;
    if ((rc = iv->orig.reserve((size_t)std::max<i64>(rows->ntotal, 1) * 8))) return rc;
    HR_CHECK_HIP(hipMemcpy(iv->offs.p, list_offsets_host, (size_t)(nlist + 1) * 8, hipMemcpyHostToDevice));
    HR_CHECK_HIP(hipMemcpy(iv->orig.p, orig_ids_host, (size_t)rows->ntotal * 8, hipMemcpyHostToDevice));
    *out_handle = ivf_reg().put(iv);
    return HIPRAG_OK;
}

int32_t hipivf_destroy(uint64_t h)
{
    GET_IVF(h);
    {
        std::lock_guard<std::mutex> guard(iv->mu);
        (void)hipSetDevice(iv->rows->device);
        (void)hipDeviceSynchronize();
    }
    ivf_reg().erase(h);
    return HIPRAG_OK;
}

int32_t hipivf_search_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t nprobe, double* out_scores64_dev,
                          float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    HR_REQUIRE(nq >= 0 && k > 0 && k <= kIvfRows, "k must be in 1..%d (got %d)", kIvfRows, k);
    HR_REQUIRE(nprobe > 0 && nprobe <= kMaxK, "nprobe must be in 1..%d (got %d)", kMaxK, nprobe);
    if (nq == 0) return HIPRAG_OK;
    HR_REQUIRE(q_dev && out_scores64_dev && out_ids_dev, "null device pointer");
    DenseIndex& R = *iv->rows;
    DenseIndex& C = *iv->cents;
    HR_CHECK_HIP(hipSetDevice(R.device));
    hipStream_t st = (hipStream_t)stream;
    const int np = std::min(nprobe, iv->nlist);
    const int smax = (int)std::max<i64>(1, (iv->maxlen + kIvfRows - 1) / kIvfRows);
    const int parts = np * smax;
    const int qchunk = std::max(1, std::min(nq, 1024));
    int32_t rc;
    if ((rc = iv->probe64.reserve((size_t)qchunk * np * 8))) return rc;
    if ((rc = iv->probe_ids.reserve((size_t)qchunk * np * 8))) return rc;
    if ((rc = iv->gw.ps.reserve((size_t)parts * qchunk * k * 8))) return rc;
    if ((rc = iv->gw.pi.reserve((size_t)parts * qchunk * k * 8))) return rc;
    {
        std::lock_guard<std::mutex> gr(R.mu);
        if ((rc = R.wait_adds_stream(st))) return rc;
    }
    for (int o = 0; o < nq; o += qchunk) {
        const int m = std::min(qchunk, nq - o);
        const float* qo = q_dev + (i64)o * R.d;
        {   // coarse quantiser: the exact flat search of the query among the centroids
            std::lock_guard<std::mutex> gc(C.mu);
            if ((rc = C.search_dev(qo, m, np, iv->probe64.as<double>(), nullptr, iv->probe_ids.as<int64_t>(), st))) return rc;
        }
        IvfArgs a;
        a.xb = R.xb.as<float4>(); a.q = qo; a.probe = iv->probe_ids.as<i64>(); a.offs = iv->offs.as<i64>(); a.orig = iv->orig.as<i64>();
        a.ps = iv->gw.ps.as<double>(); a.pi = iv->gw.pi.as<i64>(); a.d = R.d; a.P = R.P; a.k = k; a.nq = m; a.nprobe = np; a.smax = smax;
        if (R.metric == HIPRAG_METRIC_IP) hipLaunchKernelGGL(ivf_probe_kernel<HIPRAG_METRIC_IP>, dim3(parts, m), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(ivf_probe_kernel<HIPRAG_METRIC_L2>, dim3(parts, m), dim3(256), 0, st, a);
        HR_CHECK_HIP(hipGetLastError());
        if ((rc = hiprag_merge_topk_dev(iv->gw.ps.as<double>(), iv->gw.pi.as<int64_t>(), parts, m, k, k, (int64_t)m * k, R.metric,
                                        out_scores64_dev + (i64)o * k, out_scores_dev ? out_scores_dev + (i64)o * k : nullptr,
                                        out_ids_dev + (i64)o * k, stream)))
            return rc;
    }
    iv->searches += nq;
    return HIPRAG_OK;
}

// List-major batch search: the same result as hipivf_search_dev, bit for bit (include/hiprag.h).
int32_t hipivf_search_batch_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, int32_t nprobe, double* out_scores64_dev,
                                float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    HR_REQUIRE(nq >= 0 && k > 0 && k <= kIvfRows, "k must be in 1..%d (got %d)", kIvfRows, k);
    HR_REQUIRE(nprobe > 0 && nprobe <= kMaxK, "nprobe must be in 1..%d (got %d)", kMaxK, nprobe);
    if (nq == 0) return HIPRAG_OK;
    HR_REQUIRE(q_dev && out_scores64_dev && out_ids_dev, "null device pointer");
    DenseIndex& R = *iv->rows;
    DenseIndex& C = *iv->cents;
    HR_CHECK_HIP(hipSetDevice(R.device));
    hipStream_t st = (hipStream_t)stream;
    const int nlist = iv->nlist;
    const int np = std::min(nprobe, nlist);
    const int smax = (int)std::max<i64>(1, (iv->maxlen + kIvfRows - 1) / kIvfRows);
    const int parts = np * smax;
    const int qchunk = queries_per_chunk(nq, parts, k, kIvfBatchBudget, kIvfBatchMaxChunk);
    int32_t rc;
    if ((rc = iv->probe64.reserve((size_t)qchunk * np * 8))) return rc;
    if ((rc = iv->probe_ids.reserve((size_t)qchunk * np * 8))) return rc;
    if ((rc = iv->gw.ps.reserve((size_t)parts * qchunk * k * 8))) return rc;
    if ((rc = iv->gw.pi.reserve((size_t)parts * qchunk * k * 8))) return rc;
    if ((rc = iv->gw.order.reserve((size_t)qchunk * np * 8))) return rc;
    if ((rc = iv->gw.items.reserve((size_t)(nlist + 1) * 8))) return rc;
    if ((rc = iv->gw.stat.reserve(8))) return rc;
    if ((rc = ensure_list_tab(*iv))) return rc;
    HR_CHECK_HIP(hipMemsetAsync(iv->gw.stat.p, 0, 8, st));
    {
        std::lock_guard<std::mutex> gr(R.mu);
        if ((rc = R.wait_adds_stream(st))) return rc;
    }
    const bool ip = R.metric == HIPRAG_METRIC_IP;
    const size_t lds = (size_t)kIvfBatchG * R.P * 8 * 4 + (size_t)kIvfBatchG * kIvfRows * 8 + (size_t)kIvfRows * 8 + 2 * kIvfBatchG * 4;
    const void* bk = ip ? reinterpret_cast<const void*>(ivf_batch_kernel<HIPRAG_METRIC_IP>)
                        : reinterpret_cast<const void*>(ivf_batch_kernel<HIPRAG_METRIC_L2>);
    if ((rc = ensure_lds(bk, lds))) return rc;
    for (int o = 0; o < nq; o += qchunk) {
        const int m = std::min(qchunk, nq - o);
        const float* qo = q_dev + (i64)o * R.d;
        {   // coarse quantiser: the exact flat search of the query among the centroids
            std::lock_guard<std::mutex> gc(C.mu);
            if ((rc = C.search_dev(qo, m, np, iv->probe64.as<double>(), nullptr, iv->probe_ids.as<int64_t>(), st))) return rc;
        }
        // (q, j) pairs by probed list, then the work items of every list
        const i64 pairs = (i64)m * np;
        if ((rc = ivf_counting_sort(iv->probe_ids.as<i64>(), pairs, nlist, 1, iv->gw.tiles, iv->gw.len, iv->gw.offs, iv->gw.chunks,
                                    iv->gw.order.as<i64>(), st)))
            return rc;
        if ((rc = group_item_scan(iv->gw.len.as<i64>(), iv->list_tab.as<i64>(), iv->list_tab.as<i64>() + nlist, kIvfBatchG, false, nlist,
                                  iv->gw.items.as<i64>(), iv->gw.stat.as<i64>(), st)))
            return rc;
        if ((rc = fill_partials(R.metric, iv->gw.ps.as<double>(), iv->gw.pi.as<i64>(), (i64)parts * m * k, st))) return rc;
        IvfBatchArgs a;
        a.xb = R.xb.as<float4>(); a.q = qo; a.offs = iv->offs.as<i64>(); a.orig = iv->orig.as<i64>();
        a.pair_offs = iv->gw.offs.as<i64>(); a.order = iv->gw.order.as<i64>(); a.item_start = iv->gw.items.as<i64>();
        a.ps = iv->gw.ps.as<double>(); a.pi = iv->gw.pi.as<i64>();
        a.d = R.d; a.P = R.P; a.k = k; a.nq = m; a.nprobe = np; a.smax = smax; a.nlist = nlist;
        // items <= (pairs / G + lists with a pair) x slices of the longest list; the grid strides over the device-side count
        const i64 bound = (pairs / kIvfBatchG + std::min<i64>(nlist, pairs)) * smax;
        const unsigned grid = (unsigned)std::max<i64>(1, std::min<i64>(bound, (i64)R.n_cu));   // one resident workgroup per CU
        if (ip) hipLaunchKernelGGL(ivf_batch_kernel<HIPRAG_METRIC_IP>, dim3(grid), dim3(kIvfBatchThreads), lds, st, a);
        else hipLaunchKernelGGL(ivf_batch_kernel<HIPRAG_METRIC_L2>, dim3(grid), dim3(kIvfBatchThreads), lds, st, a);
        HR_CHECK_HIP(hipGetLastError());
        if ((rc = hiprag_merge_topk_dev(iv->gw.ps.as<double>(), iv->gw.pi.as<int64_t>(), parts, m, k, k, (int64_t)m * k, R.metric,
                                        out_scores64_dev + (i64)o * k, out_scores_dev ? out_scores_dev + (i64)o * k : nullptr,
                                        out_ids_dev + (i64)o * k, stream)))
            return rc;
    }
    iv->searches += nq;
    iv->gw.chunk = qchunk;
    iv->gw.chunks_n = (nq + qchunk - 1) / qchunk;
    return HIPRAG_OK;
}

int32_t hipivf_batch_info(uint64_t h, int64_t* out4)
{
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    HR_REQUIRE(out4, "null out");
    out4[0] = kIvfBatchBudget;
    out4[1] = iv->gw.chunk;
    out4[2] = iv->gw.chunks_n;
    out4[3] = 0;
    if (iv->gw.stat.p) {
        HR_CHECK_HIP(hipSetDevice(iv->rows->device));
        HR_CHECK_HIP(hipDeviceSynchronize());
        HR_CHECK_HIP(hipMemcpy(&out4[3], iv->gw.stat.p, 8, hipMemcpyDeviceToHost));
    }
    return HIPRAG_OK;
}

int32_t hipivf_info(uint64_t h, int32_t* out_nlist, int64_t* out_stored_rows, int64_t* out_longest_list)
{
    GET_IVF(h);
    HR_REQUIRE(out_nlist && out_stored_rows && out_longest_list, "null out");
    *out_nlist = iv->nlist;
    *out_stored_rows = iv->rows->ntotal;
    *out_longest_list = iv->maxlen;
    return HIPRAG_OK;
}

int32_t hipivf_get_centroids(uint64_t h, float* out_host)
{
    GET_IVF(h);
    HR_REQUIRE(out_host, "null out");
    std::lock_guard<std::mutex> guard(iv->mu);
    std::lock_guard<std::mutex> gc(iv->cents->mu);
    HR_CHECK_HIP(hipSetDevice(iv->cents->device));
    DevBuf tmp;
    return read_rows_host(*iv->cents, 0, iv->nlist, tmp, out_host);
}

int32_t hipivf_get_lists(uint64_t h, int64_t* offsets_host, int64_t* orig_ids_host)
{
    GET_IVF(h);
    HR_REQUIRE(offsets_host && orig_ids_host, "null out");
    std::lock_guard<std::mutex> guard(iv->mu);
    HR_CHECK_HIP(hipSetDevice(iv->rows->device));
    memcpy(offsets_host, iv->offs_host.data(), iv->offs_host.size() * 8);
    HR_CHECK_HIP(hipMemcpy(orig_ids_host, iv->orig.p, (size_t)iv->rows->ntotal * 8, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hipivf_meta(uint64_t h, int32_t* out_d, int32_t* out_metric, int64_t* out_n)
{
    GET_IVF(h);
    HR_REQUIRE(out_d && out_metric && out_n, "null out");
    *out_d = iv->rows->d;
    *out_metric = iv->rows->metric;
    *out_n = iv->n_rows;
    return HIPRAG_OK;
}

}  // extern "C"
