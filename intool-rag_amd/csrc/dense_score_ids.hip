// dense_score_ids.hip -- exact scores of GIVEN rows of the flat index (hipidx_score_ids*): faiss's compute_distance_subset.
// The rows and the re-score are dense_layout.h's, so a row's score is the bits every search entry gives for it.
#include <cfloat>

#include "dense_internal.h"

namespace hiprag {
namespace {

// ------------------------------------------------------------------------------------------------------
// Every chunk the reference hands to rank_pages carries the similarity its search returned (rag/query/page_retriever.py:191,
// rag/storage/faiss_index.py:83).  A search scores a row as a by-product of finding it; a fused candidate that only the BM25
// leg found, or a row outside the probed IVF lists, has no score.  This call scores ANY (query, row id) pairs.
//
// ids int64 [nq][depth].  Entry (i, j) = c names local row c - id_base; valid iff c >= 0 and 0 <= c - id_base < ntotal.  A
// valid entry's fp64 output is rescore4<METRIC> (dense_layout.h) on the row's quad -- rows (row & ~3) .. + 3 of its 32-row
// block -- read from the lane with lane & 3 == row & 3: no second accumulation loop, hence the bits of hipidx_search_dev,
// hipidx_search_scoped_dev and the IVF entries.  The fp32 output is its rounding.  An invalid entry is padding: no row is read
// and the outputs are the searches' padding values (-DBL_MAX / -FLT_MAX for IP, DBL_MAX / FLT_MAX for L2).  Duplicates are
// separate entries, no order is assumed.
//
// A workgroup (256 threads = 4 waves) takes one query and `chunk` consecutive entries of its list: the query goes to LDS once
// as d_pad zero-padded floats (at most 4 KiB), the entries' local rows (-1: padding) beside it, then wave w scores entries
// w, w + 4, ... one at a time; the row is wave-uniform (readfirstlane), so padding is a scalar branch.  chunk is the smallest
// of 4, 8, .. 64 at which the grid has at most kScoreGridTarget workgroups, else 64: one query with 256 entries runs on 64
// workgroups, 16 384 x 50 pairs on 16 384.  A valid entry reads one 128-byte line of each piece of its quad (d_pad x 16 bytes,
// 16 KiB at d = 1024: 16 loads of 16 bytes per lane in two batches of 8, as in fin_kernel); row offsets are 64-bit (rescore4
// takes the block as int64_t).  One 64-bit integer atomic per workgroup counts (valid entries << 32) + 1 for
// hipidx_score_info; no float atomics, one writer per output.  Resource usage (-Rpass-analysis=kernel-resource-usage,
// gfx950), both metrics: 102 VGPRs, no scratch, no spill, LDS 4 KiB + 512 bytes, occupancy 4 waves / SIMD.
// Bound: HBM / Infinity Cache latency per wave (two dependent batches per entry) -- the occupancy, not the fp64 pipe, sets
// the rate.  1M x 1024, 50 random ids per query (tools/bench_score_ids.py, profiles/score_ids_1m.json; HIP events around the
// call): 1 query 0.014 ms, 64 queries 0.026 ms, 16 384 queries 2.41 ms = 5.6 TB/s of the quad lines read.
// ------------------------------------------------------------------------------------------------------
constexpr int kScoreThreads = 256;
constexpr int kScoreMaxChunk = 64;          // entries per workgroup, at most: one wave reads the chunk's ids
constexpr int kScoreMinChunk = 4;           // one entry per wave
constexpr i64 kScoreGridTarget = 4096;      // workgroups beyond which the chunk grows

struct ScoreArgs {
    const float4* xb;
    const float* q;       // [nq, d]
    const i64* ids;       // [nq, depth]
    double* out64;        // [nq, depth]
    float* out32;         // [nq, depth] or null
    u64* counter;         // (valid entries << 32) + workgroups
    i64 ntotal, id_base;
    int d, P, depth, chunk, groups;   // groups = ceil(depth / chunk) workgroups per query
};

template <int METRIC>
__global__ __launch_bounds__(kScoreThreads) void score_ids_kernel(ScoreArgs a)
{
    constexpr int NW = kScoreThreads / 64;
    __shared__ float qv[kMaxDPad];
    __shared__ i64 rows[kScoreMaxChunk];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qi = blockIdx.x / a.groups;
    const int j0 = (blockIdx.x - qi * a.groups) * a.chunk;
    const int cn = min(a.chunk, a.depth - j0);            // 1..chunk entries
    const int dpad = a.P * 8;
    const float* src = a.q + (i64)qi * a.d;
    for (int c = tid; c < dpad; c += kScoreThreads) qv[c] = c < a.d ? src[c] : 0.f;
    if (tid < 64) {
        i64 row = -1;
        if (tid < cn) {
            const i64 c = a.ids[(i64)qi * a.depth + j0 + tid];
            // c >= id_base makes the difference exact in unsigned arithmetic whatever the sign of id_base
            if (c >= 0 && c >= a.id_base && (u64)c - (u64)a.id_base < (u64)a.ntotal) row = (i64)((u64)c - (u64)a.id_base);
        }
        rows[tid] = row;
        const int n_valid = __popcll(__ballot(row >= 0));
        if (tid == 0) atomicAdd(a.counter, ((u64)n_valid << 32) | 1ull);
    }
    __syncthreads();
    for (int j = wave; j < cn; j += NW) {
        const i64 rv = rows[j];
        const i64 row = (i64)(((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)((u64)rv >> 32)) << 32) |
                              (u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(u64)rv));
        const i64 o = (i64)qi * a.depth + j0 + j;
        if (row < 0) {                                    // padding (wave-uniform): nothing is read
            if (lane == 0) {
                a.out64[o] = METRIC == HIPRAG_METRIC_IP ? -DBL_MAX : DBL_MAX;
                if (a.out32) a.out32[o] = METRIC == HIPRAG_METRIC_IP ? -FLT_MAX : FLT_MAX;
            }
            continue;
        }
        const int r = (int)(row % kRowsPerBlock);
        const double sc = rescore4<METRIC>(a.xb, a.P, row / kRowsPerBlock, r & ~3, qv);
        if (lane == (r & 3)) {
            a.out64[o] = sc;
            if (a.out32) a.out32[o] = (float)sc;
        }
    }
}

}  // namespace

// hipidx_score_ids_dev under the index mutex (include/hiprag.h).  Every check runs before anything is enqueued.
int32_t score_ids_dev(DenseIndex& X, const float* q_dev, int nq, const int64_t* ids_dev, int depth, double* out64, float* out32,
                      hipStream_t st)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(depth >= 1, "depth must be at least 1 (got %d)", depth);
    HR_REQUIRE((i64)nq * depth < (1ll << 31), "nq x depth = %lld pairs is beyond one call (2^31)", (long long)nq * depth);
    HR_REQUIRE(q_dev, "q is null");
    HR_REQUIRE(ids_dev, "ids is null");
    HR_REQUIRE(out64, "out_scores64 is null");
    int32_t rc;
    if ((rc = X.score_stat.reserve(8))) return rc;       // made once per handle
    int chunk = kScoreMinChunk;
    while (chunk < kScoreMaxChunk && (i64)nq * ((depth + chunk - 1) / chunk) > kScoreGridTarget) chunk *= 2;
    ScoreArgs a;
    a.xb = X.xb.as<float4>(); a.q = q_dev; a.ids = reinterpret_cast<const i64*>(ids_dev); a.out64 = out64; a.out32 = out32;
    a.counter = X.score_stat.as<u64>();
    a.ntotal = X.ntotal; a.id_base = X.id_base;
    a.d = X.d; a.P = X.P; a.depth = depth; a.chunk = chunk; a.groups = (depth + chunk - 1) / chunk;
    const i64 grid = (i64)nq * a.groups;                  // <= nq x depth < 2^31
    HR_CHECK_HIP(hipMemsetAsync(X.score_stat.p, 0, 8, st));
    if ((rc = X.wait_adds_stream(st))) return rc;
    if (X.metric == HIPRAG_METRIC_IP) hipLaunchKernelGGL(score_ids_kernel<HIPRAG_METRIC_IP>, dim3((unsigned)grid), dim3(kScoreThreads), 0, st, a);
    else hipLaunchKernelGGL(score_ids_kernel<HIPRAG_METRIC_L2>, dim3((unsigned)grid), dim3(kScoreThreads), 0, st, a);
    HR_CHECK_HIP(hipGetLastError());
    X.score_pairs = (i64)nq * depth;
    return HIPRAG_OK;
}

}  // namespace hiprag

using namespace hiprag;

extern "C" {

// The exact scores of the rows `ids_dev` names, for every query (include/hiprag.h).
int32_t hipidx_score_ids_dev(uint64_t h, const float* q_dev, int32_t nq, const int64_t* ids_dev, int32_t depth,
                             double* out_scores64_dev, float* out_scores_dev, void* stream)
{
    GET_INDEX(h);
    return score_ids_dev(*ix, q_dev, nq, ids_dev, depth, out_scores64_dev, out_scores_dev, (hipStream_t)stream);
}

int32_t hipidx_score_ids(uint64_t h, const float* q_host, int32_t nq, const int64_t* ids_host, int32_t depth,
                         double* out_scores64, float* out_scores)
{
    GET_INDEX(h);
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(depth >= 1, "depth must be at least 1 (got %d)", depth);
    HR_REQUIRE((i64)nq * depth < (1ll << 31), "nq x depth = %lld pairs is beyond one call (2^31)", (long long)nq * depth);
    HR_REQUIRE(q_host, "q is null");
    HR_REQUIRE(ids_host, "ids is null");
    HR_REQUIRE(out_scores64, "out_scores64 is null");
    const size_t n = (size_t)nq * depth;
    int32_t rc;
    if ((rc = ix->qbuf.reserve((size_t)nq * ix->d * sizeof(float)))) return rc;
    if ((rc = ix->oid.reserve(n * sizeof(int64_t)))) return rc;
    if ((rc = ix->o64.reserve(n * sizeof(double)))) return rc;
    if ((rc = ix->o32.reserve(n * sizeof(float)))) return rc;
    HR_CHECK_HIP(hipMemcpy(ix->qbuf.p, q_host, (size_t)nq * ix->d * sizeof(float), hipMemcpyHostToDevice));
    HR_CHECK_HIP(hipMemcpy(ix->oid.p, ids_host, n * sizeof(int64_t), hipMemcpyHostToDevice));
    if ((rc = score_ids_dev(*ix, ix->qbuf.as<float>(), nq, ix->oid.as<int64_t>(), depth, ix->o64.as<double>(),
                            out_scores ? ix->o32.as<float>() : nullptr, nullptr)))
        return rc;
    HR_CHECK_HIP(hipMemcpy(out_scores64, ix->o64.p, n * sizeof(double), hipMemcpyDeviceToHost));
    if (out_scores) HR_CHECK_HIP(hipMemcpy(out_scores, ix->o32.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

// { valid entries, padding entries, workgroups launched, 0 } of the last hipidx_score_ids* call; synchronises
int32_t hipidx_score_info(uint64_t h, int64_t* out4)
{
    GET_INDEX(h);
    HR_REQUIRE(out4, "out4 is null");
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (ix->score_stat.p) {
        unsigned long long word = 0;
        HR_CHECK_HIP(hipDeviceSynchronize());
        HR_CHECK_HIP(hipMemcpy(&word, ix->score_stat.p, 8, hipMemcpyDeviceToHost));
        out4[0] = (int64_t)(word >> 32);
        out4[1] = ix->score_pairs - out4[0];
        out4[2] = (int64_t)(word & 0xFFFFFFFFull);
    }
    return HIPRAG_OK;
}

}  // extern "C"
