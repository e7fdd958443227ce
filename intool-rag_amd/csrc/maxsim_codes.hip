// maxsim_codes.hip -- centroid codes on the multi-vector store and the PRUNED late-interaction search built on them
// (hipmv_attach_centroids .. hipmv_centroid_info, hipmaxsim_search_pruned*, include/hiprag.h): the PLAID-style middle between
// the scope tables of the scoped searches and the exact MaxSim of up to 256 candidates (maxsim.hip).  Every stored vector
// carries the id of its nearest centroid; a query is scored against the centroids once; every document of the scope is
// scored from its codes alone, 4 bytes per token and a table lookup instead of 2 x dim bytes and a dot product; only the best
// ncand documents reach the exact kernel.
//
// s(a, b), the one product everything here is made of: the fp32 value v_mfma_f32_32x32x16_bf16 forms for a pair of rows with
// the k order of maxsim_docs.h (chunks of 64 ascending, lane half h its 32 of them).  An output element depends on its two
// rows alone, and a * b == b * a exactly, so it does not matter which row is the A operand.
//
// rows_kernel<Docs, kArgmax>: ONE body, two uses.  Rows of one side lie in LDS, kRowTiles tiles of 32 per trip (maxsim_kernel's
// row pitch of 2 dim + 16 bytes); the other side streams from global memory through Docs::load_chunk / mul_chunk, each of the
// four waves 32 rows of it at a time, loaded once per trip for all the LDS tiles.  The accumulator has the LDS row on the lane
// and 16 streamed rows in its registers.
//   kArgmax   the CODES.  LDS side = the centroid table, streamed side = the STORED vectors through the store's own Docs
//             struct, so the value is that of the dequantised vector on an fp8 or MXFP4 store and the three formats need no
//             code of their own.  A workgroup keeps its 128 vectors and walks the whole table, trip by trip: the store is
//             read from HBM once, whatever ncent is.  A lane keeps a running (max, argmax) per register over the centroids
//             it sees (r, r + 32, ..: ascending, and only a greater value replaces, so the lowest wins); one butterfly over the
//             32 lanes of a half at the end, ties to the lower centroid.
//   !kArgmax  the query TABLE T[q][c][i] = s(q_i, centroid_c).  LDS side = the query's vectors, streamed side = the centroid
//             table through DocsBf16, exactly as maxsim_kernel reads a document: the bits hipmaxsim_dev gives that pair.
//             Stored [c][P], P = q_stride rounded up to 32, so the Lq values of one code are contiguous.
//
// interaction_kernel: the hot kernel of a search.  Work items, scope image, counting sort of the queries by scope, partial
// lists and the canonical merge are the scoped search's (scope_plan.h, group_partials.hip); a slice is kCodeSlice documents.
// One wave per (query, document), lanes over i: m_i = max_j T[code_j][i] (the document's codes go through the wave 64 at a
// time; at Lq <= 32 the lane halves take alternate codes), then the fp64 sum of m_i in ascending i, divided by Lq, rounded
// to float -- hipmaxsim's own reduction with every document vector replaced by its centroid.  A slice's best min(ncand,
// kCodeSlice) documents are ranked by counting under (score descending, id ascending): one writer per slot, no float atomics.
// order_candidates_kernel puts a query's candidates into ascending id order, padding last, for the exact stage.
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dense_internal.h"
#include "maxsim_docs.h"
#include "multivec.h"
#include "topk_device.h"

#ifndef HIPRAG_MAXSIM_CODE_SLICE
#define HIPRAG_MAXSIM_CODE_SLICE 256   // documents per slice of the interaction stage: a build constant
#endif

namespace hiprag {

// What hipmaxsim_search_pruned* keeps with the store (multivec.h), and beside it the query table of a chunk, the candidates,
// and the shape of the last call.
struct MaxsimPrunedWs : MaxsimWsBase {
    DevBuf table;                    // float [queries of a chunk][ncent][P]
    DevBuf cs, ci, cand;             // candidates by approximate score (scores, ids); candidates by id
    i64 table_bytes = 0, chunks = 0, items = 0;
};

namespace {

using namespace mvk;

constexpr int kRowTile = 32;                        // rows per LDS tile = per MFMA
constexpr int kRowTiles = 2;                     // LDS tiles per trip: 132 KB at 1024-d
constexpr int kRowThreads = 256, kRowWaves = kRowThreads / 64;
constexpr int kRowBlock = kRowWaves * kRowTile;     // streamed rows per workgroup
constexpr int kMinCent = 32, kMaxCent = 65536;

constexpr int kCodeSlice = HIPRAG_MAXSIM_CODE_SLICE;
constexpr int kPrunedG = 8;                      // queries per work item
constexpr int kPrunedThreads = 512, kPrunedWaves = kPrunedThreads / 64;
constexpr int kMaxCand = 256;
constexpr i64 kPrunedBudget = 512ll << 20;       // bytes of partial lists and query table per chunk of queries
constexpr int kPrunedMaxChunk = 16384;
static_assert(kCodeSlice >= 1 && kCodeSlice <= kPrunedThreads, "documents per slice: one thread each");

struct RowsArgs {
    const uint16_t* lds_rows;   // bf16 [groups][group_rows][dim]: the LDS side (one group: the centroids | a query's vectors)
    int group_rows;             // ncent | q_stride
    int n_trips;                // trips of kRowTiles tiles over a group's rows
    int dim;
    i64 s0, s1;                 // the streamed rows [s0, s1): stored vectors | centroids
    int32_t* codes;             // kArgmax: [stored] the code of a streamed row
    float* table;               // !kArgmax: [groups][s1][P]
    int P;
};

template <class Docs, bool kArgmax>
__global__ __launch_bounds__(kRowThreads) void rows_kernel(RowsArgs a, Docs docs)
{
    extern __shared__ __align__(16) unsigned char l_lds[];   // [kRowTiles * kRowTile][dim * 2 + kRowPad]
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pieces = a.dim >> 3;                // 16-byte pieces of a row
    const int pitch = a.dim * 2 + kRowPad, tile_bytes = kRowTile * pitch;
    const int n_ch = Docs::n_chunks(a.dim);
    const unsigned char* my_l = l_lds + r * pitch + h * 64;
    // codes: a workgroup per block of streamed rows, every trip.  Table: x = (group, trip), y = block of streamed rows.
    const i64 sblock = kArgmax ? (i64)blockIdx.x : (i64)blockIdx.y;
    const int group = kArgmax ? 0 : (int)(blockIdx.x / (unsigned)a.n_trips);
    const int trip0 = kArgmax ? 0 : (int)(blockIdx.x % (unsigned)a.n_trips);
    const int trip1 = kArgmax ? a.n_trips : trip0 + 1;
    const i64 srow0 = a.s0 + sblock * kRowBlock + (i64)wave * kRowTile;
    const bool active = srow0 < a.s1;             // wave-uniform; an idle wave still stages and meets the barriers
    const i64 my_s = min(srow0 + r, a.s1 - 1);    // behind the end the last row again: nothing outside [s0, s1) is read
    const uint4* lsrc = reinterpret_cast<const uint4*>(a.lds_rows) + (i64)group * a.group_rows * pieces;
    float bestv[16];
    int bestc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        bestv[i] = -INFINITY;
        bestc[i] = r;                             // a code is a centroid whatever the values are
    }
    for (int trip = trip0; trip < trip1; ++trip) {
        const int row0 = trip * kRowTiles * kRowTile;
        if (trip != trip0) __syncthreads();       // the rows of the trip before this one have been read
        for (int p = tid; p < kRowTiles * kRowTile * pieces; p += kRowThreads) {
            const int row = p / pieces, piece = p - row * pieces;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row0 + row < a.group_rows) v = lsrc[(i64)(row0 + row) * pieces + piece];
            *reinterpret_cast<uint4*>(l_lds + row * pitch + piece * 16) = v;
        }
        __syncthreads();
        if (!active) continue;
        f32x16 acc[kRowTiles];
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
        }
        for (int c = 0; c < n_ch; ++c) docs.template mul_chunk<kRowTiles>(acc, docs.load_chunk(my_s, h, c, a.dim), c, my_l, tile_bytes);
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t) {
            const int lrow = row0 + t * kRowTile + r;   // the lane's LDS row; register i holds streamed row 8 (i / 4) + 4 h + i % 4
            if (kArgmax) {
                if (lrow < a.group_rows) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        if (acc[t][i] > bestv[i]) {
                            bestv[i] = acc[t][i];
                            bestc[i] = lrow;
                        }
                    }
                }
            } else if (lrow < a.P) {               // rows q_stride .. P - 1 are zero rows: their values are 0
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const i64 srow = srow0 + (i >> 2) * 8 + h * 4 + (i & 3);
                    if (srow < a.s1) a.table[((i64)group * a.s1 + srow) * a.P + lrow] = acc[t][i];
                }
            }
        }
    }
    if (kArgmax && active) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float v = bestv[i];
            int c = bestc[i];
#pragma unroll
            for (int dist = 16; dist; dist >>= 1) {   // within the lane half: the 32 lanes that hold this streamed row
                const float ov = __shfl_xor(v, dist);
                const int oc = __shfl_xor(c, dist);
                if (ov > v || (ov == v && oc < c)) {
                    v = ov;
                    c = oc;
                }
            }
            const i64 srow = srow0 + (i >> 2) * 8 + h * 4 + (i & 3);
            if (r == 0 && srow < a.s1) a.codes[srow] = c;
        }
    }
}

template <class Docs, bool kArgmax>
int32_t launch_rows(dim3 grid, hipStream_t st, const RowsArgs& a, Docs docs)
{
    const size_t lds = (size_t)kRowTiles * kRowTile * ((size_t)a.dim * 2 + kRowPad);
    int32_t rc;
    if ((rc = ensure_lds(reinterpret_cast<const void*>(rows_kernel<Docs, kArgmax>), lds))) return rc;
    hipLaunchKernelGGL((rows_kernel<Docs, kArgmax>), grid, dim3(kRowThreads), lds, st, a, docs);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

// codes[v] of stored vectors [v0, v1) against `ncent` centroids
int32_t code_range(MultiVecStore& s, const uint16_t* cent, int ncent, int32_t* codes, i64 v0, i64 v1, hipStream_t st)
{
    constexpr i64 kMaxGrid = 1ll << 30;
    for (i64 b0 = v0; b0 < v1; b0 += kMaxGrid * kRowBlock) {
        const i64 b1 = std::min(v1, b0 + kMaxGrid * kRowBlock);
        RowsArgs a;
        a.lds_rows = cent; a.group_rows = ncent; a.n_trips = (ncent + kRowTiles * kRowTile - 1) / (kRowTiles * kRowTile); a.dim = s.dim;
        a.s0 = b0; a.s1 = b1; a.codes = codes; a.table = nullptr; a.P = 0;
        const dim3 grid((unsigned)((b1 - b0 + kRowBlock - 1) / kRowBlock));
        int32_t rc;
        if (s.format == kMvMxfp4) rc = launch_rows<DocsMxfp4, true>(grid, st, a, DocsMxfp4{s.codes.as<unsigned char>(), s.scales.as<unsigned char>()});
        else if (s.format == kMvFp8) rc = launch_rows<DocsFp8, true>(grid, st, a, DocsFp8{s.codes.as<unsigned char>(), s.scales.as<float>()});
        else rc = launch_rows<DocsBf16, true>(grid, st, a, DocsBf16{s.vecs.as<uint16_t>()});
        if (rc) return rc;
    }
    return HIPRAG_OK;
}

struct PrunedArgs {
    const int32_t* q_counts; // [nq] of the chunk
    SliceTables t;           // the chunk's work items (slice_items.h)
    const i64* doc_off;      // the store's CSR
    const int32_t* codes;    // [stored]
    const float* table;      // [nq][ncent][P] of the chunk
    double* ps;              // [smax][nq][kp] partial scores
    i64* pi;                 //                partial ids (local document + id_base)
    u64* counters;
    i64 id_base;
    int q_stride, P, ncent, kp, nq;
};

__global__ __launch_bounds__(kPrunedThreads) void interaction_kernel(PrunedArgs a)
{
    constexpr int G = kPrunedG, S = kCodeSlice, NW = kPrunedWaves;
    __shared__ float score[G][S];      // the approximate score of (member, document)
    __shared__ i64 d_first[S];         // first stored vector of a document of the slice
    __shared__ int d_len[S];           // its vectors; 0 outside [lo, hi)
    __shared__ int mq[G], mc[G];       // query and clamped count of a member
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const i64 nitems = a.t.item_start[a.t.n_scopes];
    for (i64 item = blockIdx.x; item < nitems; item += gridDim.x) {
        const SliceItem it = slice_item<G, S>(a.t, item);
        const i64 sl = it.slice, base = it.base;
        const int gn = it.members, p_lo = it.p_lo, p_hi = it.p_hi;   // documents of the range: positions [p_lo, p_hi)
        item_members(it, a.t.order, a.q_counts, a.q_stride, tid, mq, mc);
        item_docs<S>(it, a.doc_off, tid, d_first, d_len);
        __syncthreads();
        for (int dd = wave; dd < S; dd += NW) {
            const int ld = d_len[dd];
            if (ld <= 0) continue;               // outside the range, or no stored vector: nothing of it is read
            const int32_t* dc = a.codes + d_first[dd];
            for (int g = 0; g < gn; ++g) {
                const int lq = mc[g];
                if (lq <= 0) continue;           // uniform
                const float* T = a.table + (i64)mq[g] * a.ncent * a.P;
                const int parts = lq <= 32 ? 2 : 1;          // lane halves take alternate codes of a short query
                const int il = parts == 2 ? (lane & 31) : lane, sub = parts == 2 ? (lane >> 5) : 0;
                const int rows = 64 / parts;
                double sum = 0.0;
                for (int i0 = 0; i0 < lq; i0 += rows) {
                    const int i = min(i0 + il, lq - 1);      // behind the query's end its last row again: a value nobody adds
                    float m = -INFINITY;
                    for (int j0 = 0; j0 < ld; j0 += 64) {
                        const int n = min(64, ld - j0);
                        const int cj = dc[j0 + min(lane, n - 1)];
                        for (int jj = 0; jj < n; jj += parts) {
                            const int c = __shfl(cj, min(jj + sub, n - 1));   // an odd n: the last code twice, which no maximum notices
                            m = fmaxf(m, T[(i64)c * a.P + i]);
                        }
                    }
                    if (parts == 2) m = fmaxf(m, __shfl_xor(m, 32));
                    const int cntr = min(rows, lq - i0);
                    for (int ii = 0; ii < cntr; ++ii)        // ascending i, in fp64: hipmaxsim's sum
                        sum += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), ii));
                }
                if (lane == 0) score[g][dd] = (float)(sum / (double)lq);
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
            atomicAdd(a.counters + 2, n_q * vecs);
        }
        // every member's best kp documents of the slice, ranked by counting: (score descending, id ascending)
        for (int g = 0; g < gn; ++g) {
            if (mc[g] <= 0) continue;            // uniform: a query with no vector keeps its padding
            if (tid < S && d_len[tid] > 0) {
                const u64 key = ord64((double)score[g][tid]);
                int rank = 0;
                for (int o = 0; o < S; ++o) {
                    if (d_len[o] <= 0) continue;
                    const u64 ko = ord64((double)score[g][o]);
                    rank += (ko > key || (ko == key && o < tid)) ? 1 : 0;
                }
                if (rank < a.kp) {
                    const i64 at = (sl * a.nq + mq[g]) * a.kp + rank;
                    a.ps[at] = (double)score[g][tid];
                    a.pi[at] = base + tid + a.id_base;
                }
            }
        }
        __syncthreads();                          // the next item overwrites the LDS
    }
}

// One workgroup per query: its candidates (by approximate score, padding id -1 last) into ascending id order, padding last.
__global__ __launch_bounds__(kMaxCand) void order_candidates_kernel(const i64* __restrict__ by_score, int ncand, i64* __restrict__ by_id)
{
    __shared__ i64 ids[kMaxCand];
    const int t = threadIdx.x;
    const i64 base = (i64)blockIdx.x * ncand;
    const i64 id = t < ncand ? by_score[base + t] : -1;
    ids[t] = id;
    __syncthreads();
    if (t >= ncand) return;
    int rank = 0;
    for (int o = 0; o < ncand; ++o) {
        const i64 other = ids[o];
        if (id >= 0) rank += (other >= 0 && other < id) ? 1 : 0;
        else rank += (other >= 0 || o < t) ? 1 : 0;
    }
    by_id[base + rank] = id >= 0 ? id : -1;
}

// the checks both entries make before they touch anything
int32_t check_pruned_shape(int32_t nq, int32_t k, int32_t ncand, int32_t q_stride, int32_t n_scopes, int64_t id_base)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(1 <= k && k <= ncand && ncand <= kMaxCand, "1 <= k <= ncand <= %d does not hold (k = %d, ncand = %d)", kMaxCand, k, ncand);
    int32_t rc;
    if ((rc = check_maxsim_shape(q_stride, n_scopes, id_base))) return rc;
    HR_REQUIRE((int64_t)nq * ncand < (1ll << 31), "nq x ncand = %lld must be below 2^31", (long long)nq * ncand);
    return HIPRAG_OK;
}

int32_t require_attached(const MultiVecStore& X)
{
    if (X.ncent == 0) {
        set_error("the store has no centroids: hipmv_attach_centroids comes before a pruned search");
        return HIPRAG_E_UNSUPPORTED;
    }
    return HIPRAG_OK;
}

// bytes of partial lists and query table a chunk of queries may take: kPrunedBudget, or HIPRAG_PRUNED_BUDGET (read at every
// call: the tests force a call into many chunks with it)
i64 pruned_budget()
{
    const char* e = getenv("HIPRAG_PRUNED_BUDGET");
    if (e && *e) {
        const long long v = atoll(e);
        if (v > 0) return (i64)v;
    }
    return kPrunedBudget;
}

// hipmaxsim_search_pruned_dev under the store's mutex.  Every check runs before anything is enqueued.
int32_t search_pruned_impl(MultiVecStore& X, const void* q_dev, const int32_t* q_counts_dev, int32_t q_stride, int nq, int k, int ncand,
                           const int64_t* ranges, const int32_t* scope_offsets, int n_scopes, const int32_t* scope_of_query,
                           int64_t id_base, float* out_scores, int64_t* out_ids, int64_t* out_cand_ids, float* out_cand_scores,
                           hipStream_t st)
{
    int32_t rc;
    if ((rc = check_pruned_shape(nq, k, ncand, q_stride, n_scopes, id_base))) return rc;
    if ((rc = require_attached(X))) return rc;
    HR_REQUIRE(q_dev, "q_vecs is null");
    HR_REQUIRE(q_counts_dev, "q_counts is null");
    HR_REQUIRE(out_scores, "out_scores is null");
    HR_REQUIRE(out_ids, "out_ids is null");
    HR_REQUIRE(((uintptr_t)q_dev & 15) == 0, "q_vecs must be aligned to 16 bytes");
    SlicePlan L;
    if ((rc = slice_plan(ranges, scope_offsets, n_scopes, scope_of_query, nq, X.csr.n_docs, "documents", kCodeSlice, kPrunedG, ncand, "ncand", L))) return rc;
    const int kp = L.kp;   // entries of a slice's partial list
    // ---- every check has passed: from here the call allocates and enqueues ---------------------------------------------
    if (!X.pruned_ws) X.pruned_ws = std::make_shared<MaxsimPrunedWs>();
    MaxsimPrunedWs& M = *X.pruned_ws;
    GroupWorkspace& W = M.sc.gw;
    const int P = (q_stride + kRowTile - 1) / kRowTile * kRowTile;
    const i64 table_per_query = (i64)X.ncent * P * (i64)sizeof(float);
    const int qchunk = queries_per_chunk(nq, L.smax, kp, pruned_budget(), kPrunedMaxChunk, table_per_query);
    if ((rc = M.table.reserve((size_t)qchunk * (size_t)table_per_query))) return rc;
    if ((rc = M.o64.reserve((size_t)nq * ncand * 8))) return rc;
    if ((rc = M.cand.reserve((size_t)nq * ncand * 8))) return rc;
    if (!out_cand_ids && (rc = M.ci.reserve((size_t)nq * ncand * 8))) return rc;
    if (!out_cand_scores && (rc = M.cs.reserve((size_t)nq * ncand * 4))) return rc;
    int64_t* cand_by_score = out_cand_ids ? out_cand_ids : M.ci.as<int64_t>();
    float* cand_scores = out_cand_scores ? out_cand_scores : M.cs.as<float>();
    if ((rc = M.begin(X.device, L, qchunk, st))) return rc;

    const unsigned grid = (unsigned)std::max<i64>(1, std::min<i64>(L.bound, (i64)M.n_cu * 4));   // the items loop takes the rest
    const int n_trips = (P + kRowTiles * kRowTile - 1) / (kRowTiles * kRowTile);
    for (int o = 0; o < nq; o += qchunk) {
        const int m = std::min(qchunk, nq - o);
        // the table of the chunk's queries: x = (query, trip over its rows), y = blocks of centroids
        RowsArgs t;
        t.lds_rows = reinterpret_cast<const uint16_t*>(q_dev) + (i64)o * q_stride * X.dim; t.group_rows = q_stride; t.n_trips = n_trips;
        t.dim = X.dim; t.s0 = 0; t.s1 = X.ncent; t.codes = nullptr; t.table = M.table.as<float>(); t.P = P;
        if ((rc = launch_rows<DocsBf16, false>(dim3((unsigned)(m * n_trips), (unsigned)((X.ncent + kRowBlock - 1) / kRowBlock)), st, t,
                                               DocsBf16{X.centroids.as<uint16_t>()})))
            return rc;
        PrunedArgs a;
        if ((rc = slice_chunk(M.sc, L, HIPRAG_METRIC_IP, o, m, a.t, st))) return rc;
        a.q_counts = q_counts_dev + o;
        a.doc_off = X.csr.offsets.as<i64>(); a.codes = X.cent_codes.as<int32_t>(); a.table = M.table.as<float>();
        a.ps = W.ps.as<double>(); a.pi = W.pi.as<i64>(); a.counters = M.counters.as<u64>();
        a.id_base = id_base; a.q_stride = q_stride; a.P = P; a.ncent = X.ncent; a.kp = kp; a.nq = m;
        hipLaunchKernelGGL(interaction_kernel, dim3(grid), dim3(kPrunedThreads), 0, st, a);
        HR_CHECK_HIP(hipGetLastError());
        if ((rc = hiprag_merge_topk_dev(W.ps.as<double>(), W.pi.as<int64_t>(), (int32_t)L.smax, m, kp, ncand, (int64_t)m * kp, HIPRAG_METRIC_IP,
                                        M.o64.as<double>() + (i64)o * ncand, cand_scores + (i64)o * ncand, cand_by_score + (i64)o * ncand, st)))
            return rc;
    }
    hipLaunchKernelGGL(order_candidates_kernel, dim3((unsigned)nq), dim3(kMaxCand), 0, st, reinterpret_cast<const i64*>(cand_by_score), ncand, M.cand.as<i64>());
    HR_CHECK_HIP(hipGetLastError());
    M.table_bytes = (i64)std::min(qchunk, nq) * table_per_query;
    M.chunks = (nq + qchunk - 1) / qchunk;
    M.items = L.bound;
    // the exact stage: hipmaxsim_dev's kernel over the candidates in ascending id order, so that ties break by id
    return maxsim_candidates(X, q_dev, q_counts_dev, q_stride, nq, M.cand.as<int64_t>(), ncand, id_base, k, out_scores, out_ids, st);
}

}  // namespace

int32_t mv_code_range(MultiVecStore& s, int64_t v0, int64_t v1, hipStream_t st)
{
    if (s.ncent == 0 || v1 <= v0) return HIPRAG_OK;
    return code_range(s, s.centroids.as<uint16_t>(), s.ncent, s.cent_codes.as<int32_t>(), v0, v1, st);
}

}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipmv_attach_centroids(uint64_t mv_h, const void* centroids_bf16_host, int32_t ncent)
{
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_REQUIRE(centroids_bf16_host, "centroids is null");
    HR_REQUIRE(ncent >= kMinCent && ncent <= kMaxCent && ncent % kRowTile == 0, "ncent must be a multiple of %d in %d..%d (got %d)", kRowTile,
               kMinCent, kMaxCent, ncent);
    // the new table and the new codes are made beside the old ones: a failure leaves the store as it was
    DevBuf cent, codes;
    int32_t rc;
    const size_t cb = (size_t)ncent * s->dim * 2;
    if ((rc = cent.reserve(cb))) return rc;
    if ((rc = codes.reserve((size_t)std::max<int64_t>(s->csr.cap_items, 1) * sizeof(int32_t)))) return rc;
    HR_CHECK_HIP(hipDeviceSynchronize());   // whatever reads the old table or writes the vectors has finished
    HR_CHECK_HIP(hipMemcpy(cent.p, centroids_bf16_host, cb, hipMemcpyHostToDevice));
    if ((rc = code_range(*s, cent.as<uint16_t>(), ncent, codes.as<int32_t>(), 0, s->csr.n_items, nullptr))) return rc;
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    std::swap(s->centroids.p, cent.p);
    std::swap(s->centroids.bytes, cent.bytes);
    std::swap(s->cent_codes.p, codes.p);
    std::swap(s->cent_codes.bytes, codes.bytes);
    s->ncent = ncent;
    return HIPRAG_OK;
}

int32_t hipmv_detach_centroids(uint64_t mv_h)
{
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_CHECK_HIP(hipDeviceSynchronize());
    s->ncent = 0;
    s->centroids.release();
    s->cent_codes.release();
    return HIPRAG_OK;
}

int32_t hipmv_export_centroids(uint64_t mv_h, void* out_bf16)
{
    HR_REQUIRE(out_bf16, "null out");
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    int32_t rc;
    if ((rc = require_attached(*s))) return rc;
    HR_CHECK_HIP(hipMemcpy(out_bf16, s->centroids.p, (size_t)s->ncent * s->dim * 2, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hipmv_export_codes(uint64_t mv_h, int32_t* out_codes_i32)
{
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    int32_t rc;
    if ((rc = require_attached(*s))) return rc;
    HR_REQUIRE(out_codes_i32 || s->csr.n_items == 0, "null out");
    if (s->csr.n_items) HR_CHECK_HIP(hipMemcpy(out_codes_i32, s->cent_codes.p, (size_t)s->csr.n_items * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hipmv_centroid_info(uint64_t mv_h, int64_t* out4)
{
    HR_REQUIRE(out4, "null out");
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    out4[0] = s->ncent;
    out4[1] = s->ncent ? s->csr.n_items : 0;
    out4[2] = s->ncent ? s->csr.n_items * (int64_t)sizeof(int32_t) : 0;
    out4[3] = 0;
    return HIPRAG_OK;
}

int32_t hipmaxsim_search_pruned_dev(uint64_t mv_h, const void* q_vecs_dev, const int32_t* q_counts_dev, int32_t q_stride, int32_t nq,
                                    int32_t k, int32_t ncand, const int64_t* ranges_host, const int32_t* scope_offsets_host,
                                    int32_t n_scopes, const int32_t* scope_of_query_host, int64_t id_base, float* out_scores_dev,
                                    int64_t* out_ids_dev, int64_t* out_cand_ids_dev, float* out_cand_scores_dev, void* stream)
{
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    return search_pruned_impl(*s, q_vecs_dev, q_counts_dev, q_stride, nq, k, ncand, ranges_host, scope_offsets_host, n_scopes,
                              scope_of_query_host, id_base, out_scores_dev, out_ids_dev, out_cand_ids_dev, out_cand_scores_dev,
                              (hipStream_t)stream);
}

int32_t hipmaxsim_search_pruned(uint64_t mv_h, const void* q_vecs_host, const int32_t* q_counts_host, int32_t q_stride, int32_t nq,
                                int32_t k, int32_t ncand, const int64_t* ranges_host, const int32_t* scope_offsets_host, int32_t n_scopes,
                                const int32_t* scope_of_query_host, int64_t id_base, float* out_scores, int64_t* out_ids,
                                int64_t* out_cand_ids, float* out_cand_scores)
{
    int32_t rc;
    if ((rc = check_pruned_shape(nq, k, ncand, q_stride, n_scopes, id_base))) return rc;
    HR_REQUIRE(q_vecs_host && q_counts_host && out_scores && out_ids, "null argument");
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    if ((rc = require_attached(*s))) return rc;
    if (!s->pruned_ws) s->pruned_ws = std::make_shared<MaxsimPrunedWs>();
    MaxsimPrunedWs& M = *s->pruned_ws;
    const size_t nc = (size_t)nq * ncand;
    if ((rc = M.ci.reserve(nc * 8)) || (rc = M.cs.reserve(nc * 4))) return rc;
    if ((rc = M.stage(q_vecs_host, q_counts_host, q_stride, nq, k, s->dim))) return rc;
    rc = search_pruned_impl(*s, M.hq.p, M.hc.as<int32_t>(), q_stride, nq, k, ncand, ranges_host, scope_offsets_host, n_scopes,
                            scope_of_query_host, id_base, M.hos.as<float>(), M.hoi.as<int64_t>(), nullptr, nullptr, nullptr);
    if ((rc = M.give_back(rc, nq, k, out_scores, out_ids))) return rc;
    if (out_cand_ids) HR_CHECK_HIP(hipMemcpy(out_cand_ids, M.ci.p, nc * 8, hipMemcpyDeviceToHost));
    if (out_cand_scores) HR_CHECK_HIP(hipMemcpy(out_cand_scores, M.cs.p, nc * 4, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hipmaxsim_pruned_info(uint64_t mv_h, int64_t* out8)
{
    HR_REQUIRE(out8, "null out");
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_CHECK_HIP(hipDeviceSynchronize());
    unsigned long long c[3] = {0, 0, 0}, exact[3] = {0, 0, 0};
    const MaxsimPrunedWs* M = s->pruned_ws.get();
    if (M && M->counters.p) HR_CHECK_HIP(hipMemcpy(c, M->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    if (M && M->chunks && s->counters.p) HR_CHECK_HIP(hipMemcpy(exact, s->counters.p, sizeof(exact), hipMemcpyDeviceToHost));
    out8[0] = (int64_t)c[0];
    out8[1] = (int64_t)c[1];
    out8[2] = (int64_t)c[2];
    out8[3] = M ? M->table_bytes : 0;
    out8[4] = M ? M->chunks : 0;
    out8[5] = M ? M->items : 0;
    out8[6] = (int64_t)exact[0];
    out8[7] = kCodeSlice;
    return HIPRAG_OK;
}

}  // extern "C"
