// maxsim_search.hip -- late-interaction SEARCH (hipmaxsim_search_scoped*, include/hiprag.h): the exact MaxSim top k over
// every document of a query's scope, the scoped entry of the multi-vector store beside those of the flat index, the IVF
// lists and the postings.  Brute force: a project's token vectors are a few hundred MB, contiguous in the store, and one
// read of them serves a whole group of queries.
//
// The host side is the chunk driver of group_partials.hip (slice_plan / slice_begin / slice_chunk): the scope tables and
// checks of scope_plan.h, the queries sorted by scope, work ITEMS (slice_items.h) = (scope, slice of kSliceDocs consecutive
// documents cut on ABSOLUTE document boundaries, group of up to kSearchG queries that name the scope), partial lists
// [slices][queries][min(k, kSliceDocs)] prefilled by fill_partials and finished by hiprag_merge_topk_dev (a float is exact
// as a double, so the merge's fp64 order is the float order).  One writer per slot, no float atomics.
//
// maxsim_scope_kernel<Docs, T>: 512 threads = 8 waves, document-major.  The group's query vectors are PACKED row after row
// into LDS (maxsim_kernel's row pitch of 2 dim + 16 bytes; the clamped counts are read here, a prefix over at most kSearchG
// values says where a query's rows lie), R = 32 T rows at a time: T = the 32-row tiles that fit beside the tables, at most 4
// (2 at 1024-d).  An MFMA output element depends on one document row and one query row alone, so two short queries share a
// tile without changing a bit; a group of more than R rows runs ceil(rows / R) passes over the slice.  A wave owns whole
// documents: it walks one in 32-vector tiles (the last tile clamped to the document's last row: nothing is masked, nothing
// behind the document is read), loads each k-chunk of its rows from global memory ONCE (Docs::load_chunk, with the chunk
// after the one being multiplied already in flight) and multiplies it against each of the T LDS tiles into T accumulators
// (Docs::mul_chunk: dot_tile's products in dot_tile's order).  max_j stays in the lane; lane g of the wave then adds the
// maxima of query g's rows in ascending i to the fp64 sum of (query g, document), which lives in LDS across the passes:
// the additions of hipmaxsim_dev in its order, hence its bits.  At the end of an item the workgroup selects every query's
// best min(k, kSliceDocs) documents with wg_topk_rounds and writes part `slice` of its partial lists.  Documents of the
// first and last slice of a range outside [lo, hi) are never read; a document without vectors is never ranked.
#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

#include "dense_internal.h"
#include "maxsim_docs.h"
#include "multivec.h"

#ifndef HIPRAG_MAXSIM_SLICE
#define HIPRAG_MAXSIM_SLICE 16   // documents per slice: a build constant (DESIGN 5.5 has the reasoning)
#endif

namespace hiprag {

// What hipmaxsim_search_scoped* keeps with the store (multivec.h), and the shape of the last search.
struct MaxsimSearchWs : MaxsimWsBase {
    i64 tiles = 0, chunks = 0, items = 0;   // of the last search: T, chunks, the bound on its work items
};

int32_t MaxsimWsBase::begin(int device, const SlicePlan& P, int qchunk, hipStream_t st)
{
    int32_t rc;
    if (!n_cu) {
        int n = 0;
        HR_CHECK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device));
        n_cu = std::max(n, 1);
    }
    if ((rc = counters.reserve(3 * sizeof(u64))) || (rc = slice_begin(sc, P, qchunk, st))) return rc;
    HR_CHECK_HIP(hipMemsetAsync(counters.p, 0, 3 * sizeof(u64), st));
    return HIPRAG_OK;
}

int32_t MaxsimWsBase::stage(const void* q_vecs_host, const int32_t* q_counts_host, int32_t q_stride, int32_t nq, int32_t k, int32_t dim)
{
    const size_t nk = (size_t)nq * k, qb = (size_t)nq * q_stride * dim * 2;
    int32_t rc;
    if ((rc = hq.reserve(qb)) || (rc = hc.reserve((size_t)nq * 4)) || (rc = hos.reserve(nk * 4)) || (rc = hoi.reserve(nk * 8))) return rc;
    HR_CHECK_HIP(hipMemcpy(hq.p, q_vecs_host, qb, hipMemcpyHostToDevice));
    HR_CHECK_HIP(hipMemcpy(hc.p, q_counts_host, (size_t)nq * 4, hipMemcpyHostToDevice));
    return HIPRAG_OK;
}

int32_t MaxsimWsBase::give_back(int32_t rc, int32_t nq, int32_t k, float* out_scores, int64_t* out_ids)
{
    if (rc) { (void)hipDeviceSynchronize(); return rc; }
    HR_CHECK_HIP(hipMemcpy(out_scores, hos.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_ids, hoi.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t check_maxsim_shape(int32_t q_stride, int32_t n_scopes, int64_t id_base)
{
    HR_REQUIRE(1 <= q_stride && q_stride <= kMaxsimMaxQStride, "q_stride must be in 1..%d (got %d)", kMaxsimMaxQStride, q_stride);
    HR_REQUIRE(n_scopes >= 1, "n_scopes must be at least 1 (got %d)", n_scopes);
    HR_REQUIRE(id_base >= 0 && id_base < (1ll << 62), "id_base must be in 0..2^62 (got %lld)", (long long)id_base);
    return HIPRAG_OK;
}

namespace {

using namespace mvk;

constexpr int kQTile = 32;                        // query rows per LDS tile = per MFMA
constexpr int kSearchG = 8;                       // queries per work item
constexpr int kSliceDocs = HIPRAG_MAXSIM_SLICE;   // documents per slice
constexpr int kSearchThreads = 512, kSearchWaves = kSearchThreads / 64;
constexpr int kSearchMaxK = 256, kMaxTiles = 4;
constexpr size_t kLdsBudget = 160 * 1024 - 4096;  // a CU's LDS less the static tables below
constexpr i64 kSearchBudget = 512ll << 20;        // bytes of partial lists per chunk of queries
constexpr int kSearchMaxChunk = 16384;
static_assert(kSliceDocs >= 1 && kSliceDocs <= 64, "documents per slice");

struct SearchArgs {
    const uint16_t* q;       // [nq][q_stride][dim] of the chunk
    const int32_t* q_counts; // [nq]
    SliceTables t;           // the chunk's work items (slice_items.h)
    const i64* doc_off;      // the store's CSR
    double* ps;              // [smax][nq][kp] partial scores
    i64* pi;                 //                partial ids (local document + id_base)
    u64* counters;
    i64 id_base;
    int q_stride, dim, kp, nq;
};

template <class Docs, int T>
__global__ __launch_bounds__(kSearchThreads) void maxsim_scope_kernel(SearchArgs a, Docs docs)
{
    constexpr int G = kSearchG, S = kSliceDocs, NW = kSearchWaves, R = T * kQTile;
    extern __shared__ __align__(16) unsigned char q_lds[];   // [R][dim * 2 + kRowPad]
    __shared__ double sums[G][S];      // the fp64 sum of (member, document) so far
    __shared__ u64 keys[S];
    __shared__ i64 ids[S];
    __shared__ i64 d_first[S];         // first stored vector of a document of the slice
    __shared__ int d_len[S];           // its vectors; 0 outside [lo, hi)
    __shared__ int mq[G], mc[G];       // query and clamped count of a member
    __shared__ int mpre[G + 1];        // packed rows before member g; [gn .. G] = the group's rows
    __shared__ KeyId red[2 * NW];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pieces = a.dim >> 3;                // 16-byte pieces of a vector
    const int pitch = a.dim * 2 + kRowPad, tile_bytes = kQTile * pitch;
    const int n_ch = Docs::n_chunks(a.dim);
    const unsigned char* my_q = q_lds + r * pitch + h * 64;
    const i64 nitems = a.t.item_start[a.t.n_scopes];
    for (i64 item = blockIdx.x; item < nitems; item += gridDim.x) {
        const SliceItem it = slice_item<G, S>(a.t, item);
        const i64 sl = it.slice, base = it.base;
        const int gn = it.members, p_lo = it.p_lo, p_hi = it.p_hi;   // documents of the range: positions [p_lo, p_hi)
        item_members(it, a.t.order, a.q_counts, a.q_stride, tid, mq, mc);
        item_docs<S>(it, a.doc_off, tid, d_first, d_len);
        for (int i = tid; i < G * S; i += kSearchThreads) (&sums[0][0])[i] = 0.0;
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int g = 0; g < G; ++g) {
                mpre[g] = run;
                if (g < gn) run += mc[g];
            }
            mpre[G] = run;
        }
        __syncthreads();
        const int rows_total = mpre[G];
        const int passes = (rows_total + R - 1) / R;
        for (int pass = 0; pass < passes; ++pass) {
            const int row0 = pass * R, nrows = min(R, rows_total - row0);
            if (pass) __syncthreads();           // the rows of the pass before this one have been read
            for (int row = wave; row < R; row += NW) {
                const int prow = row0 + row;
                uint4* dst = reinterpret_cast<uint4*>(q_lds + row * pitch);
                if (prow < rows_total) {         // wave-uniform
                    int g = 0;
                    while (mpre[g + 1] <= prow) ++g;   // the member that owns packed row prow (prow < mpre[gn]: g < gn)
                    const uint4* src = reinterpret_cast<const uint4*>(a.q) + ((i64)mq[g] * a.q_stride + (prow - mpre[g])) * pieces;
                    for (int p = lane; p < pieces; p += 64) dst[p] = src[p];
                } else {
                    for (int p = lane; p < pieces; p += 64) dst[p] = make_uint4(0u, 0u, 0u, 0u);
                }
            }
            __syncthreads();
            for (int dd = wave; dd < S; dd += NW) {
                const int ld = d_len[dd];
                if (ld <= 0) continue;           // outside the range, or no stored vector: nothing of it is read
                const i64 d0 = d_first[dd];
                const int n_doc_tiles = (ld + kQTile - 1) / kQTile;
                float m[T];
                f32x16 acc[T];
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    m[t] = -INFINITY;
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
                }
                i64 row = d0 + min(r, ld - 1);
                typename Docs::Chunk cur = docs.load_chunk(row, h, 0, a.dim);
                for (int dt = 0; dt < n_doc_tiles; ++dt) {
                    // the tile after this one, clamped like every row: behind the last tile it names the document's last row
                    const i64 next_row = d0 + min((dt + 1) * kQTile + r, ld - 1);
                    for (int c = 0; c < n_ch; ++c) {
                        const bool last = c + 1 == n_ch;
                        const typename Docs::Chunk nxt = docs.load_chunk(last ? next_row : row, h, last ? 0 : c + 1, a.dim);
                        docs.template mul_chunk<T>(acc, cur, c, my_q, tile_bytes);
                        cur = nxt;
                    }
                    row = next_row;
#pragma unroll
                    for (int t = 0; t < T; ++t) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) {   // 16 of the tile's 32 documents; the other lane half has the rest
                            m[t] = fmaxf(m[t], acc[t][i]);
                            acc[t][i] = 0.f;
                        }
                    }
                }
                // lane g adds the maxima of member g's rows of this pass, ascending, to the pair's fp64 sum
                const bool member = lane < gn;
                const int lo_g = member ? mpre[lane] - row0 : 0, hi_g = member ? mpre[lane + 1] - row0 : 0;
                double sum = member ? sums[lane][dd] : 0.0;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const float mt = fmaxf(m[t], __shfl_xor(m[t], 32));
#pragma nounroll   // unrolled, the 32 T lane reads pile up in SGPRs and spill
                    for (int i = 0; i < kQTile && t * kQTile + i < nrows; ++i) {
                        const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mt), i));
                        const int prow = t * kQTile + i;
                        if (prow >= lo_g && prow < hi_g) sum += (double)v;
                    }
                }
                if (member) sums[lane][dd] = sum;
            }
        }
        __syncthreads();
        if (tid == 0) {
            u64 n_docs = 0, vecs = 0, n_q = 0;
            for (int p = p_lo; p < p_hi; ++p) {
                n_docs += d_len[p] > 0 ? 1 : 0;
                vecs += (u64)d_len[p];
            }
            for (int g = 0; g < gn; ++g) n_q += mc[g] > 0 ? 1 : 0;
            atomicAdd(a.counters + 0, n_q * n_docs);
            atomicAdd(a.counters + 1, (u64)gn * (u64)(p_hi - p_lo) - n_q * n_docs);
            atomicAdd(a.counters + 2, (u64)passes * vecs);
        }
        for (int g = 0; g < gn; ++g) {
            const int lq = mc[g];
            if (lq <= 0) continue;               // uniform: a query with no vector keeps its padding
            if (tid < S) {
                keys[tid] = d_len[tid] > 0 ? ord64((double)(float)(sums[g][tid] / (double)lq)) : 0ull;
                ids[tid] = base + tid + a.id_base;
            }
            __syncthreads();
            const i64 o = (sl * a.nq + mq[g]) * a.kp;
            wg_topk_rounds<kSearchThreads>(keys, ids, S, a.kp, red, [&](int rank, u64 key, i64 id) {
                if (key != 0) {                  // exhausted ranks keep their padding
                    a.ps[o + rank] = unord64(key);
                    a.pi[o + rank] = id;
                }
            });
        }
        __syncthreads();                          // the next item overwrites the LDS
    }
}

int tiles_of(int dim) { return (int)std::min<size_t>(kMaxTiles, kLdsBudget / ((size_t)kQTile * ((size_t)dim * 2 + kRowPad))); }

template <class Docs>
int32_t launch_scope(int T, unsigned grid, size_t lds, hipStream_t st, const SearchArgs& a, Docs docs)
{
    int32_t rc;
#define HR_SCOPE_CASE(TT)                                                                                               \
    case TT:                                                                                                            \
        if ((rc = ensure_lds(reinterpret_cast<const void*>(maxsim_scope_kernel<Docs, TT>), lds))) return rc;            \
        hipLaunchKernelGGL((maxsim_scope_kernel<Docs, TT>), dim3(grid), dim3(kSearchThreads), lds, st, a, docs);        \
        break
    switch (T) {
        HR_SCOPE_CASE(2);
        HR_SCOPE_CASE(3);
        HR_SCOPE_CASE(4);
    default:
        set_error("no MaxSim search kernel for %d query tiles", T);
        return HIPRAG_E_INVALID;
    }
#undef HR_SCOPE_CASE
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

// the checks both entries make before they touch anything
int32_t check_search_shape(int32_t nq, int32_t k, int32_t q_stride, int32_t n_scopes, int64_t id_base)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(k >= 1 && k <= kSearchMaxK, "k must be in 1..%d for a MaxSim search (got %d)", kSearchMaxK, k);
    return check_maxsim_shape(q_stride, n_scopes, id_base);
}

// hipmaxsim_search_scoped_dev under the store's mutex.  Every check runs before anything is enqueued.
int32_t search_scoped_impl(MultiVecStore& X, const void* q_dev, const int32_t* q_counts_dev, int32_t q_stride, int nq, int k,
                           const int64_t* ranges, const int32_t* scope_offsets, int n_scopes, const int32_t* scope_of_query,
                           int64_t id_base, float* out_scores, int64_t* out_ids, hipStream_t st)
{
    int32_t rc;
    if ((rc = check_search_shape(nq, k, q_stride, n_scopes, id_base))) return rc;
    HR_REQUIRE(q_dev, "q_vecs is null");
    HR_REQUIRE(q_counts_dev, "q_counts is null");
    HR_REQUIRE(out_scores, "out_scores is null");
    HR_REQUIRE(out_ids, "out_ids is null");
    HR_REQUIRE(((uintptr_t)q_dev & 15) == 0, "q_vecs must be aligned to 16 bytes");
    SlicePlan P;
    if ((rc = slice_plan(ranges, scope_offsets, n_scopes, scope_of_query, nq, X.csr.n_docs, "documents", kSliceDocs, kSearchG, k, "k", P))) return rc;
    const int kp = P.kp;   // entries of a slice's partial list
    const int T = tiles_of(X.dim);
    HR_REQUIRE(T >= 2, "dim = %d leaves no room for two query tiles", X.dim);
    // ---- every check has passed: from here the call allocates and enqueues ---------------------------------------------
    if (!X.search_ws) X.search_ws = std::make_shared<MaxsimSearchWs>();
    MaxsimSearchWs& M = *X.search_ws;
    GroupWorkspace& W = M.sc.gw;
    const int qchunk = queries_per_chunk(nq, P.smax, kp, kSearchBudget, kSearchMaxChunk);
    if ((rc = M.o64.reserve((size_t)nq * k * 8))) return rc;
    if ((rc = M.begin(X.device, P, qchunk, st))) return rc;

    const size_t lds = (size_t)T * kQTile * ((size_t)X.dim * 2 + kRowPad);
    const bool fp8 = X.format == kMvFp8;
    const unsigned grid = (unsigned)std::max<i64>(1, std::min<i64>(P.bound, (i64)M.n_cu * 4));   // the items loop takes the rest
    for (int o = 0; o < nq; o += qchunk) {
        const int m = std::min(qchunk, nq - o);
        SearchArgs a;
        if ((rc = slice_chunk(M.sc, P, HIPRAG_METRIC_IP, o, m, a.t, st))) return rc;
        a.q = reinterpret_cast<const uint16_t*>(q_dev) + (i64)o * q_stride * X.dim; a.q_counts = q_counts_dev + o;
        a.doc_off = X.csr.offsets.as<i64>();
        a.ps = W.ps.as<double>(); a.pi = W.pi.as<i64>(); a.counters = M.counters.as<u64>();
        a.id_base = id_base; a.q_stride = q_stride; a.dim = X.dim; a.kp = kp; a.nq = m;
        if (X.format == kMvMxfp4) rc = launch_scope(T, grid, lds, st, a, DocsMxfp4{X.codes.as<unsigned char>(), X.scales.as<unsigned char>()});
        else if (fp8) rc = launch_scope(T, grid, lds, st, a, DocsFp8{X.codes.as<unsigned char>(), X.scales.as<float>()});
        else rc = launch_scope(T, grid, lds, st, a, DocsBf16{X.vecs.as<uint16_t>()});
        if (rc) return rc;
        if ((rc = hiprag_merge_topk_dev(W.ps.as<double>(), W.pi.as<int64_t>(), (int32_t)P.smax, m, kp, k, (int64_t)m * kp, HIPRAG_METRIC_IP,
                                        M.o64.as<double>() + (i64)o * k, out_scores + (i64)o * k, out_ids + (i64)o * k, st)))
            return rc;
    }
    M.tiles = T;
    M.chunks = (nq + qchunk - 1) / qchunk;
    M.items = P.bound;
    return HIPRAG_OK;
}

}  // namespace
}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipmaxsim_search_scoped_dev(uint64_t mv_h, const void* q_vecs_dev, const int32_t* q_counts_dev, int32_t q_stride, int32_t nq,
                                    int32_t k, const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                    const int32_t* scope_of_query_host, int64_t id_base, float* out_scores_dev, int64_t* out_ids_dev,
                                    void* stream)
{
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    return search_scoped_impl(*s, q_vecs_dev, q_counts_dev, q_stride, nq, k, ranges_host, scope_offsets_host, n_scopes, scope_of_query_host,
                              id_base, out_scores_dev, out_ids_dev, (hipStream_t)stream);
}

int32_t hipmaxsim_search_scoped(uint64_t mv_h, const void* q_vecs_host, const int32_t* q_counts_host, int32_t q_stride, int32_t nq,
                                int32_t k, const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                const int32_t* scope_of_query_host, int64_t id_base, float* out_scores, int64_t* out_ids)
{
    int32_t rc;
    if ((rc = check_search_shape(nq, k, q_stride, n_scopes, id_base))) return rc;
    HR_REQUIRE(q_vecs_host && q_counts_host && out_scores && out_ids, "null argument");
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    if (!s->search_ws) s->search_ws = std::make_shared<MaxsimSearchWs>();
    MaxsimSearchWs& M = *s->search_ws;
    if ((rc = M.stage(q_vecs_host, q_counts_host, q_stride, nq, k, s->dim))) return rc;
    rc = search_scoped_impl(*s, M.hq.p, M.hc.as<int32_t>(), q_stride, nq, k, ranges_host, scope_offsets_host, n_scopes, scope_of_query_host,
                            id_base, M.hos.as<float>(), M.hoi.as<int64_t>(), nullptr);
    return M.give_back(rc, nq, k, out_scores, out_ids);
}

int32_t hipmaxsim_search_info(uint64_t mv_h, int64_t* out8)
{
    HR_REQUIRE(out8, "null out");
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_CHECK_HIP(hipDeviceSynchronize());
    unsigned long long c[3] = {0, 0, 0};
    const MaxsimSearchWs* M = s->search_ws.get();
    if (M && M->counters.p) HR_CHECK_HIP(hipMemcpy(c, M->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    const int T = tiles_of(s->dim);
    out8[0] = (int64_t)c[0];
    out8[1] = (int64_t)c[1];
    out8[2] = (int64_t)c[2];
    out8[3] = (int64_t)T * kQTile;
    out8[4] = kSearchG;
    out8[5] = kSliceDocs;
    out8[6] = M ? M->chunks : 0;
    out8[7] = M ? M->items : 0;
    return HIPRAG_OK;
}

}  // extern "C"
