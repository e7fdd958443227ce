// dense_scoped.hip -- scoped search over the flat index (hipidx_search_scoped*): the exact top k of a query's row-range
// scope.  The rows and the re-score are dense_layout.h's; the work items are slice_items.h's; the upload of the scope tables
// and the chunk driver (sort of the queries by scope, item count, prefill of the partial lists) are group_partials.hip's.
#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

#include "dense_internal.h"

namespace hiprag {
namespace {

// ------------------------------------------------------------------------------------------------------
// Scoped search (hipidx_search_scoped_dev): the exact top k of the rows of a SCOPE -- a few half-open row ranges, e.g. the
// documents of one project in a collection index (the `project` argument the reference carries to rag/storage/
// faiss_index.py:140 and drops at :150).  Only the rows of the scope are read, in fp32, and scored in fp64 by rescore4's
// arithmetic (dense_layout.h): a row's score is the bits the flat search gives for it.  The bf16 scan is not used: it streams the whole
// index by construction, and its certificate speaks about all rows.
//
// The list-major IVF search (ivf_search.hip) with ranges where that has lists.  Every range is cut on ABSOLUTE 256-row boundaries into
// slices, so a slice starts on a quad of a 32-row block whatever lo is, and the rows of its first and last quad that lie
// outside [lo, hi) are masked (key 0: they are read, never ranked).  A work ITEM = (scope, slice, group of up to kScopedG
// of the queries that name the scope).  The queries are sorted by scope with the IVF build's counting sort,
// group_item_scan_kernel (group_partials.hip) writes item_start[s] = items of the scopes before s, a fixed grid strides over item_start[n_scopes],
// and an item finds its scope, then its range, by bisection (items of one slice are consecutive: the workgroups that run
// side by side share the slice in L2 / MALL).  Slice t of a scope is part t of its queries' partial lists [smax][nq][k];
// parts nobody writes are prefilled (fill_partials, group_partials.hip) and the canonical merge (hiprag_merge_topk_dev) finishes.
// One writer per slot, no float atomics: the same bits from run to run.
//
// scoped_kernel is ivf_batch_kernel (ivf_search.hip) with the mask: 512 threads = 8 waves, a wave loads a quad's 16 pieces
// per lane once and scores it against every query of the group from LDS, then wave w selects for members w, w + 8, ... of the group.  A row
// past ntotal is never ranked (hi <= ntotal) and a block past nblocks never read: a quad that is loaded holds a row of the
// range.  LDS: G x (d_pad floats + 256 keys) + G ints = 96.1 KiB at d = 1024.  Resource usage
// (-Rpass-analysis=kernel-resource-usage, gfx950), both metrics: 197 VGPRs, no scratch, no VGPR spill (15 SGPRs are parked in
// VGPR lanes, 13 in ivf_batch_kernel), occupancy 2 waves / SIMD = one workgroup per CU, as ivf_batch_kernel.
// Bound: one query -- HBM (scope rows x d_pad x 4 bytes); a full group -- the fp64 pipe, as in ivf_batch_kernel.
// ------------------------------------------------------------------------------------------------------
constexpr int kScopedG = 16;              // queries per work item
constexpr int kScopedRows = 256;          // rows per slice
constexpr int kScopedThreads = 512;
constexpr int kScopedMaxK = 256;          // the partial list of a slice holds its best k <= rows of a slice
constexpr i64 kScopedBudget = 512ll << 20;   // bytes of partial lists per chunk of queries
constexpr int kScopedMaxChunk = 16384;

struct ScopedArgs {
    const float4* xb;
    const float* q;          // [nq, d]
    SliceTables t;           // the chunk's work items (slice_items.h)
    double* ps;              // [smax][nq][k] partial scores
    i64* pi;                 //               partial ids (local rows)
    int d, P, k, nq;
};

__global__ __launch_bounds__(256) void scoped_id_base_kernel(i64* __restrict__ ids, i64 n, i64 id_base)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256)
        if (ids[i] >= 0) ids[i] += id_base;
}

template <int METRIC>
__global__ __launch_bounds__(kScopedThreads) void scoped_kernel(ScopedArgs a)
{
    constexpr int G = kScopedG, S = kScopedRows, NW = kScopedThreads / 64;
    extern __shared__ unsigned char scoped_smem[];
    const int dpad = a.P * 8;
    float* qv = reinterpret_cast<float*>(scoped_smem);         // [G][dpad]
    u64* keys = reinterpret_cast<u64*>(qv + (size_t)G * dpad); // [G][S]
    int* mq = reinterpret_cast<int*>(keys + G * S);            // [G] query of a group member
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rr = lane & 3, hh = (lane >> 2) & 1, pq = lane >> 3;
    const i64 nitems = a.t.item_start[a.t.n_scopes];
    for (i64 item = blockIdx.x; item < nitems; item += gridDim.x) {
        const SliceItem it = slice_item<G, S>(a.t, item);
        const i64 sl = it.slice, base = it.base;
        const int gn = it.members, p_lo = it.p_lo, p_hi = it.p_hi;   // rows of the range: positions [p_lo, p_hi)
        const int g_lo = p_lo >> 2, g_hi = (p_hi + 3) >> 2;           // its quads
        if (tid < gn) mq[tid] = (int)a.t.order[it.first + tid];
        __syncthreads();
        for (int g = 0; g < gn; ++g) {
            const float* src = a.q + (i64)mq[g] * a.d;
            for (int c = tid; c < dpad; c += kScopedThreads) qv[g * dpad + c] = c < a.d ? src[c] : 0.f;
        }
        __syncthreads();
        for (int g4 = g_lo + wave; g4 < g_hi; g4 += NW) {
            const i64 row0 = base + (i64)g4 * 4;
            const float4* src = a.xb + (row0 / kRowsPerBlock) * a.P * kPieceVec4 + piece_slot(hh, (int)(row0 % kRowsPerBlock) + rr);
            float4 x0[8], x1[8];
            rescore_load8<0>(x0, src, pq, a.P);
            rescore_load8<1>(x1, src, pq, a.P);
            const int pos = g4 * 4 + rr;
            const bool in = pos >= p_lo && pos < p_hi;                // rows of the quad outside [lo, hi): key 0
            for (int g = 0; g < gn; ++g) {
                double acc = 0.0;
                rescore_acc8<METRIC, 0>(acc, x0, pq, hh, a.P, qv + g * dpad);
                rescore_acc8<METRIC, 1>(acc, x1, pq, hh, a.P, qv + g * dpad);
                const double sc = rescore_reduce16(acc);
                if (lane < 4) keys[g * S + pos] = in ? ord64(METRIC == HIPRAG_METRIC_IP ? sc : -sc) : 0ull;
            }
        }
        __syncthreads();
        for (int g = wave; g < gn; g += NW) {
            u64 kk[S / 64];
            i64 ii[S / 64];
#pragma unroll
            for (int t = 0; t < S / 64; ++t) {
                const int pos = t * 64 + lane;
                kk[t] = pos >= g_lo * 4 && pos < g_hi * 4 ? keys[g * S + pos] : 0ull;
                ii[t] = base + pos;
            }
            const i64 o = (sl * a.nq + mq[g]) * a.k;
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

// hipidx_search_scoped_dev under the index mutex (include/hiprag.h).  Every check runs before anything is enqueued.
int32_t scoped_search_dev(DenseIndex& X, const float* q_dev, int nq, int k, const int64_t* ranges, const int32_t* scope_offsets,
                          int n_scopes, const int32_t* scope_of_query, double* out64, float* out32, int64_t* out_ids, hipStream_t st)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(k >= 1 && k <= kScopedMaxK, "k must be in 1..%d for a scoped search (got %d)", kScopedMaxK, k);
    HR_REQUIRE(n_scopes >= 1, "n_scopes must be at least 1 (got %d)", n_scopes);
    HR_REQUIRE(q_dev, "q is null");
    HR_REQUIRE(out64, "out_scores64 is null");
    HR_REQUIRE(out_ids, "out_ids is null");
    int32_t rc;
    SlicePlan P;
    if ((rc = slice_plan(ranges, scope_offsets, n_scopes, scope_of_query, nq, X.ntotal, "ntotal", kScopedRows, kScopedG, k, "k", P))) return rc;

    ScopeUpload& S = X.sc;
    GroupWorkspace& W = S.gw;
    const int qchunk = queries_per_chunk(nq, P.smax, k, kScopedBudget, kScopedMaxChunk);
    if ((rc = slice_begin(S, P, qchunk, st))) return rc;
    if ((rc = X.wait_adds_stream(st))) return rc;

    const bool ip = X.metric == HIPRAG_METRIC_IP;
    const size_t lds = (size_t)kScopedG * X.P * 8 * 4 + (size_t)kScopedG * kScopedRows * 8 + kScopedG * 4;
    const void* sk = ip ? reinterpret_cast<const void*>(scoped_kernel<HIPRAG_METRIC_IP>)
                        : reinterpret_cast<const void*>(scoped_kernel<HIPRAG_METRIC_L2>);
    if ((rc = ensure_lds(sk, lds))) return rc;
    const unsigned grid = (unsigned)std::max<i64>(1, std::min<i64>(P.bound, (i64)X.n_cu));   // one resident workgroup per CU
    for (int o = 0; o < nq; o += qchunk) {
        const int m = std::min(qchunk, nq - o);
        ScopedArgs a;
        if ((rc = slice_chunk(S, P, X.metric, o, m, a.t, st))) return rc;
        a.xb = X.xb.as<float4>(); a.q = q_dev + (i64)o * X.d;
        a.ps = W.ps.as<double>(); a.pi = W.pi.as<i64>();
        a.d = X.d; a.P = X.P; a.k = k; a.nq = m;
        if (ip) hipLaunchKernelGGL(scoped_kernel<HIPRAG_METRIC_IP>, dim3(grid), dim3(kScopedThreads), lds, st, a);
        else hipLaunchKernelGGL(scoped_kernel<HIPRAG_METRIC_L2>, dim3(grid), dim3(kScopedThreads), lds, st, a);
        HR_CHECK_HIP(hipGetLastError());
        if ((rc = hiprag_merge_topk_dev(W.ps.as<double>(), W.pi.as<int64_t>(), (int32_t)P.smax, m, k, k, (int64_t)m * k, X.metric,
                                        out64 + (i64)o * k, out32 ? out32 + (i64)o * k : nullptr, out_ids + (i64)o * k, st)))
            return rc;
    }
    if (X.id_base != 0) {
        const i64 n = (i64)nq * k;
        hipLaunchKernelGGL(scoped_id_base_kernel, dim3((unsigned)std::min<i64>((n + 255) / 256, 4096)), dim3(256), 0, st,
                           reinterpret_cast<i64*>(out_ids), n, (i64)X.id_base);
        HR_CHECK_HIP(hipGetLastError());
    }
    W.chunk = qchunk;
    W.chunks_n = (nq + qchunk - 1) / qchunk;
    return HIPRAG_OK;
}

}  // namespace hiprag

using namespace hiprag;

extern "C" {

// The scope tables' rules and image without a handle or a device (include/hiprag.h).  Nothing is written on refusal.
int32_t hiprag_scope_plan(const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                          const int32_t* scope_of_query_host, int32_t nq, int64_t n, int32_t slice_rows, int32_t group,
                          int64_t* out8, int64_t* out_image, int64_t image_cap)
{
    HR_REQUIRE(out8, "out8 is null");
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(n_scopes >= 1, "n_scopes must be at least 1 (got %d)", n_scopes);
    HR_REQUIRE(n >= 0, "n must not be negative (got %lld)", (long long)n);
    HR_REQUIRE(slice_rows >= 0, "slice_rows must not be negative (got %d)", slice_rows);
    HR_REQUIRE(group >= 1, "group must be at least 1 (got %d)", group);
    int32_t rc;
    if ((rc = check_scope_tables(ranges_host, scope_offsets_host, n_scopes, scope_of_query_host, nq, n, "n"))) return rc;
    ScopeImage im;
    build_scope_image(ranges_host, scope_offsets_host, n_scopes, scope_of_query_host, nq, slice_rows, group, im);
    const bool sizes_only = !out_image && image_cap == 0;
    HR_REQUIRE(sizes_only || out_image, "out_image is null");
    HR_REQUIRE(sizes_only || image_cap >= (int64_t)im.words, "image_cap = %lld is below the image's %lld words", (long long)image_cap,
               (long long)im.words);
    const int64_t out[8] = {(int64_t)im.words, im.smax, im.bound, (int64_t)im.o_slice, (int64_t)im.o_off, (int64_t)im.o_rows,
                            (int64_t)im.o_sl, (int64_t)im.o_soq};
    std::copy(out, out + 8, out8);
    if (!sizes_only) std::copy(im.img.begin(), im.img.end(), out_image);
    return HIPRAG_OK;
}

// Scoped search: the top k of the rows in the ranges of the query's scope (include/hiprag.h).
int32_t hipidx_search_scoped_dev(uint64_t h, const float* q_dev, int32_t nq, int32_t k, const int64_t* ranges_host,
                                 const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                                 double* out_scores64_dev, float* out_scores_dev, int64_t* out_ids_dev, void* stream)
{
    GET_INDEX(h);
    return scoped_search_dev(*ix, q_dev, nq, k, ranges_host, scope_offsets_host, n_scopes, scope_of_query_host, out_scores64_dev,
                             out_scores_dev, out_ids_dev, (hipStream_t)stream);
}

int32_t hipidx_search_scoped(uint64_t h, const float* q_host, int32_t nq, int32_t k, const int64_t* ranges_host,
                             const int32_t* scope_offsets_host, int32_t n_scopes, const int32_t* scope_of_query_host,
                             double* out_scores64, float* out_scores, int64_t* out_ids)
{
    GET_INDEX(h);
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(k >= 1 && k <= kScopedMaxK, "k must be in 1..%d for a scoped search (got %d)", kScopedMaxK, k);
    HR_REQUIRE(q_host, "q is null");
    HR_REQUIRE(out_scores64, "out_scores64 is null");
    HR_REQUIRE(out_ids, "out_ids is null");
    int32_t rc;
    if ((rc = ix->qbuf.reserve((size_t)nq * ix->d * sizeof(float)))) return rc;
    if ((rc = ix->o64.reserve((size_t)nq * k * sizeof(double)))) return rc;
    if ((rc = ix->o32.reserve((size_t)nq * k * sizeof(float)))) return rc;
    if ((rc = ix->oid.reserve((size_t)nq * k * sizeof(int64_t)))) return rc;
    HR_CHECK_HIP(hipMemcpy(ix->qbuf.p, q_host, (size_t)nq * ix->d * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = scoped_search_dev(*ix, ix->qbuf.as<float>(), nq, k, ranges_host, scope_offsets_host, n_scopes, scope_of_query_host,
                                ix->o64.as<double>(), ix->o32.as<float>(), ix->oid.as<int64_t>(), nullptr)))
        return rc;
    HR_CHECK_HIP(hipMemcpy(out_scores64, ix->o64.p, (size_t)nq * k * sizeof(double), hipMemcpyDeviceToHost));
    if (out_scores) HR_CHECK_HIP(hipMemcpy(out_scores, ix->o32.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_ids, ix->oid.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

// { queries per work item, queries per chunk of the last scoped call, its chunks, rows its work items read }; synchronises
int32_t hipidx_scoped_info(uint64_t h, int64_t* out4)
{
    GET_INDEX(h);
    HR_REQUIRE(out4, "out4 is null");
    out4[0] = kScopedG;
    out4[1] = ix->sc.gw.chunk;
    out4[2] = ix->sc.gw.chunks_n;
    out4[3] = 0;
    if (ix->sc.gw.stat.p) {
        HR_CHECK_HIP(hipDeviceSynchronize());
        HR_CHECK_HIP(hipMemcpy(&out4[3], ix->sc.gw.stat.p, 8, hipMemcpyDeviceToHost));
    }
    return HIPRAG_OK;
}

}  // extern "C"
