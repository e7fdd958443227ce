// maxsim.hip -- late-interaction scoring (hipmaxsim_*, include/hiprag.h): BGE-M3's colbert_score without a temperature over
// the vectors of a multi-vector store (multivec.hip).  The model of the reference (rag/config.py:9) has this third output;
// here it is a second-stage ranker beside the cross-encoder (rag/config.py:25-27) that costs no forward per pair.
//
// Kernels: maxsim_kernel<Docs>, one body for every format of the store, one workgroup of four waves per (query, candidate).
// A tile of up to 32 query vectors is staged in LDS (rows padded by 16 bytes, so the 16 lanes of a ds_read_b128 phase hit 64
// different banks); each wave takes 32 document vectors at a time against it on v_mfma_f32_32x32x16_bf16, documents as the A
// operand straight from global memory.  How a stored row becomes those operands is all a format decides: DocsBf16, DocsFp8 and
// DocsMxfp4, one dot_tile each (maxsim_docs.h, shared with the search kernel of maxsim_search.hip).  The two lanes that share a document row fetch whole 128-byte lines between them, and the query side
// reads the same permutation of k from LDS -- a dot product does not care.  The accumulator then has the query on the lane
// and the documents in its registers: max_j is 15 v_max in a lane and one exchange between the lane halves.  Rows behind the
// document's end repeat its last row, which cannot change a maximum, so nothing is masked and nothing outside the document
// is read.  Waves combine through LDS; one thread adds the maxima in fp64 in ascending query order.  maxsim_select_kernel is
// the selection of rerank.hip with this call's rule for a valid candidate.
#include <algorithm>
#include <cfloat>

#include "maxsim_docs.h"
#include "multivec.h"

namespace hiprag {
namespace {

using namespace mvk;   // DocsBf16, DocsFp8, DocsMxfp4, the fragment types and kRowPad (maxsim_docs.h)

constexpr int kThreads = 256, kWaves = 4, kTile = 32;
constexpr int kMaxDepth = 256, kMaxQStride = 512;

// Lq of query qi, Ld and first vector of candidate c: Ld = 0 marks a padding candidate (nothing of it may be read).
__device__ __forceinline__ void resolve_pair(const int32_t* __restrict__ q_counts, int q_stride, int qi, int64_t c, int64_t id_base,
                                             int64_t n_docs, const int64_t* __restrict__ doc_off, int* lq, int64_t* d0, int* ld)
{
    *lq = min(max(q_counts[qi], 0), q_stride);
    *ld = 0;
    *d0 = 0;
    if (*lq > 0 && c >= id_base && c - id_base < n_docs) {   // c >= id_base first: the difference cannot overflow
        const int64_t doc = c - id_base;
        *d0 = doc_off[doc];
        *ld = (int)(doc_off[doc + 1] - *d0);
    }
}

template <class Docs>
__global__ __launch_bounds__(kThreads) void maxsim_kernel(const uint16_t* __restrict__ q_vecs, const int32_t* __restrict__ q_counts,
                                                          int q_stride, int dim, const int64_t* __restrict__ cand, int depth,
                                                          int64_t id_base, int64_t n_docs, const int64_t* __restrict__ doc_off,
                                                          Docs docs, float* __restrict__ pair_scores,
                                                          unsigned long long* __restrict__ counters)
{
    extern __shared__ __align__(16) unsigned char q_lds[];   // [kTile][dim * 2 + kRowPad]
    __shared__ float wave_max[kWaves][kTile];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int64_t pair = blockIdx.x;
    const int qi = (int)(pair / depth);
    int lq, ld;
    int64_t d0;
    resolve_pair(q_counts, q_stride, qi, cand[pair], id_base, n_docs, doc_off, &lq, &d0, &ld);
    if (ld <= 0) {   // uniform over the workgroup
        if (tid == 0) {
            pair_scores[pair] = -FLT_MAX;
            atomicAdd(counters + 1, 1ull);
        }
        return;
    }
    const int pieces = dim >> 3;              // 16-byte pieces of a query vector
    const int pitch = dim * 2 + kRowPad;
    const int n_doc_tiles = (ld + kTile - 1) / kTile;
    const uint4* q_base = reinterpret_cast<const uint4*>(q_vecs) + (int64_t)qi * q_stride * pieces;
    const unsigned char* my_q = q_lds + r * pitch + h * 64;
    double sum = 0.0;   // thread 0 only
    for (int q0 = 0; q0 < lq; q0 += kTile) {
        const int nq_tile = min(kTile, lq - q0);
        __syncthreads();   // the tile before this one has been read, and so has wave_max
        for (int p = tid; p < kTile * pieces; p += kThreads) {
            const int row = p / pieces, piece = p - row * pieces;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row < nq_tile) v = q_base[(int64_t)(q0 + row) * pieces + piece];
            *reinterpret_cast<uint4*>(q_lds + row * pitch + piece * 16) = v;
        }
        __syncthreads();
        float m = -INFINITY;
        for (int dt = wave; dt < n_doc_tiles; dt += kWaves) {
            const int row = min(dt * kTile + r, ld - 1);
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
            docs.dot_tile(acc, d0 + row, h, my_q, dim);
#pragma unroll
            for (int i = 0; i < 16; ++i) m = fmaxf(m, acc[i]);   // 16 of the tile's 32 documents; the other lane half has the rest
        }
        m = fmaxf(m, __shfl_xor(m, 32));
        if (h == 0) wave_max[wave][r] = m;
        __syncthreads();
        if (tid == 0) {
            const int nw = min(kWaves, n_doc_tiles);
            for (int i = 0; i < nq_tile; ++i) {
                float mi = wave_max[0][i];
                for (int w = 1; w < nw; ++w) mi = fmaxf(mi, wave_max[w][i]);
                sum += (double)mi;
            }
        }
    }
    if (tid == 0) {
        pair_scores[pair] = (float)(sum / (double)lq);
        atomicAdd(counters + 0, 1ull);
        atomicAdd(counters + 2, (unsigned long long)ld * (unsigned long long)((lq + kTile - 1) / kTile));
    }
}

// rerank_select_kernel (rerank.hip) with this call's validity: one workgroup per query, rank by counting under (score
// descending, position ascending); ranks past the valid candidates get id -1, -FLT_MAX, position -1.
__global__ __launch_bounds__(kMaxDepth) void maxsim_select_kernel(const int32_t* __restrict__ q_counts, int q_stride,
                                                                  const int64_t* __restrict__ cand, int depth, int64_t id_base,
                                                                  int64_t n_docs, const int64_t* __restrict__ doc_off,
                                                                  const float* __restrict__ pair_scores, int k,
                                                                  float* __restrict__ out_scores, int64_t* __restrict__ out_ids,
                                                                  int32_t* __restrict__ out_pos)
{
    __shared__ float sl[kMaxDepth];
    __shared__ int sv[kMaxDepth];
    const int qi = blockIdx.x, t = threadIdx.x;
    const int64_t base = (int64_t)qi * depth;
    int64_t c = -1;
    float l = -FLT_MAX;
    bool valid = false;
    if (t < depth) {
        c = cand[base + t];
        int lq, ld;
        int64_t d0;
        resolve_pair(q_counts, q_stride, qi, c, id_base, n_docs, doc_off, &lq, &d0, &ld);
        valid = ld > 0;
        if (valid) l = pair_scores[base + t];
    }
    sl[t] = l;
    sv[t] = valid ? 1 : 0;
    if (t < k) {
        out_scores[(int64_t)qi * k + t] = -FLT_MAX;
        out_ids[(int64_t)qi * k + t] = -1;
        if (out_pos) out_pos[(int64_t)qi * k + t] = -1;
    }
    __syncthreads();   // also orders the pre-fill above before the ranked stores below
    if (!valid) return;
    int rank = 0;
    for (int j = 0; j < depth; ++j)
        rank += (sv[j] && (sl[j] > l || (sl[j] == l && j < t))) ? 1 : 0;
    if (rank < k) {
        out_scores[(int64_t)qi * k + rank] = l;
        out_ids[(int64_t)qi * k + rank] = c;
        if (out_pos) out_pos[(int64_t)qi * k + rank] = t;
    }
}

int32_t check_shape(int32_t nq, int32_t q_stride, int32_t depth, int64_t id_base, int32_t k)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(1 <= k && k <= depth && depth <= kMaxDepth, "1 <= k <= depth <= %d does not hold (k = %d, depth = %d)", kMaxDepth, k, depth);
    HR_REQUIRE(1 <= q_stride && q_stride <= kMaxQStride, "q_stride must be in 1..%d (got %d)", kMaxQStride, q_stride);
    HR_REQUIRE((int64_t)nq * depth < (1ll << 31), "nq x depth = %lld must be below 2^31", (long long)nq * depth);
    HR_REQUIRE(id_base >= 0, "id_base must not be negative (got %lld)", (long long)id_base);
    return HIPRAG_OK;
}

// the store's mutex is held
int32_t maxsim_impl(MultiVecStore& s, const void* q_vecs_dev, const int32_t* q_counts_dev, int32_t q_stride, int32_t nq,
                    const int64_t* cand_dev, int32_t depth, int64_t id_base, int32_t k, float* out_pair_scores_dev,
                    float* out_scores_dev, int64_t* out_ids_dev, int32_t* out_pos_dev, hipStream_t st)
{
    int32_t rc;
    if ((rc = check_shape(nq, q_stride, depth, id_base, k))) return rc;
    HR_REQUIRE(q_vecs_dev && q_counts_dev && cand_dev && out_scores_dev && out_ids_dev, "null argument");
    HR_REQUIRE(((uintptr_t)q_vecs_dev & 15) == 0, "q_vecs must be aligned to 16 bytes");
    // ---- every check has passed: from here the call enqueues -----------------------------------------------------------
    const int64_t pairs = (int64_t)nq * depth;
    float* scores = out_pair_scores_dev;
    if (!scores) {
        if ((rc = s.pair_scores.reserve((size_t)pairs * sizeof(float)))) return rc;
        scores = s.pair_scores.as<float>();
    }
    if ((rc = s.counters.reserve(3 * sizeof(unsigned long long)))) return rc;
    const size_t lds = (size_t)kTile * ((size_t)s.dim * 2 + kRowPad);
    const bool fp8 = s.format == kMvFp8, fp4 = s.format == kMvMxfp4;   // a store has one format for life, so one instantiation and one opt-in
    if (!s.lds_opted_in) {
        HR_CHECK_HIP(hipFuncSetAttribute(fp4   ? reinterpret_cast<const void*>(maxsim_kernel<DocsMxfp4>)
                                         : fp8 ? reinterpret_cast<const void*>(maxsim_kernel<DocsFp8>)
                                               : reinterpret_cast<const void*>(maxsim_kernel<DocsBf16>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, kTile * (1024 * 2 + kRowPad)));
        s.lds_opted_in = true;
    }
    HR_CHECK_HIP(hipMemsetAsync(s.counters.p, 0, 3 * sizeof(unsigned long long), st));
    const auto launch = [&](auto docs) {
        hipLaunchKernelGGL(maxsim_kernel<decltype(docs)>, dim3((unsigned)pairs), dim3(kThreads), lds, st, (const uint16_t*)q_vecs_dev,
                           q_counts_dev, (int)q_stride, (int)s.dim, cand_dev, (int)depth, id_base, (int64_t)s.csr.n_docs,
                           (const int64_t*)s.csr.offsets.as<int64_t>(), docs, scores, s.counters.as<unsigned long long>());
    };
    if (fp4) launch(DocsMxfp4{s.codes.as<unsigned char>(), s.scales.as<unsigned char>()});
    else if (fp8) launch(DocsFp8{s.codes.as<unsigned char>(), s.scales.as<float>()});
    else launch(DocsBf16{s.vecs.as<uint16_t>()});
    HR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(maxsim_select_kernel, dim3((unsigned)nq), dim3(kMaxDepth), 0, st, q_counts_dev, (int)q_stride, cand_dev, (int)depth,
                       id_base, (int64_t)s.csr.n_docs, (const int64_t*)s.csr.offsets.as<int64_t>(), (const float*)scores, (int)k, out_scores_dev,
                       out_ids_dev, out_pos_dev);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

}  // namespace

int32_t maxsim_candidates(MultiVecStore& s, const void* q_vecs_dev, const int32_t* q_counts_dev, int32_t q_stride, int32_t nq,
                          const int64_t* cand_dev, int32_t depth, int64_t id_base, int32_t k, float* out_scores_dev,
                          int64_t* out_ids_dev, hipStream_t st)
{
    return maxsim_impl(s, q_vecs_dev, q_counts_dev, q_stride, nq, cand_dev, depth, id_base, k, nullptr, out_scores_dev, out_ids_dev,
                       nullptr, st);
}

}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipmaxsim_dev(uint64_t mv_h, const void* q_vecs_dev, const int32_t* q_counts_dev, int32_t q_stride, int32_t nq,
                      const int64_t* cand_ids_dev, int32_t depth, int64_t id_base, int32_t k, float* out_pair_scores_dev,
                      float* out_scores_dev, int64_t* out_ids_dev, int32_t* out_pos_dev, void* stream)
{
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    return maxsim_impl(*s, q_vecs_dev, q_counts_dev, q_stride, nq, cand_ids_dev, depth, id_base, k, out_pair_scores_dev, out_scores_dev,
                       out_ids_dev, out_pos_dev, (hipStream_t)stream);
}

int32_t hipmaxsim_host(uint64_t mv_h, const void* q_vecs_host, const int32_t* q_counts_host, int32_t q_stride, int32_t nq,
                       const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t k, float* out_pair_scores,
                       float* out_scores, int64_t* out_ids, int32_t* out_pos)
{
    int32_t rc;
    if ((rc = check_shape(nq, q_stride, depth, id_base, k))) return rc;
    HR_REQUIRE(q_vecs_host && q_counts_host && cand_ids_host && out_scores && out_ids, "null argument");
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    const size_t pairs = (size_t)nq * depth, nk = (size_t)nq * k, qb = (size_t)nq * q_stride * s->dim * 2;
    DevBuf qv, qc, cand, ps, os, oi, op;
    if ((rc = qv.reserve(qb)) || (rc = qc.reserve((size_t)nq * 4)) || (rc = cand.reserve(pairs * 8)) || (rc = ps.reserve(pairs * 4)) ||
        (rc = os.reserve(nk * 4)) || (rc = oi.reserve(nk * 8)) || (rc = op.reserve(nk * 4)))
        return rc;
    HR_CHECK_HIP(hipMemcpy(qv.p, q_vecs_host, qb, hipMemcpyHostToDevice));
    HR_CHECK_HIP(hipMemcpy(qc.p, q_counts_host, (size_t)nq * 4, hipMemcpyHostToDevice));
    HR_CHECK_HIP(hipMemcpy(cand.p, cand_ids_host, pairs * 8, hipMemcpyHostToDevice));
    rc = maxsim_impl(*s, qv.p, qc.as<int32_t>(), q_stride, nq, cand.as<int64_t>(), depth, id_base, k, ps.as<float>(), os.as<float>(),
                     oi.as<int64_t>(), op.as<int32_t>(), nullptr);
    if (rc) { (void)hipDeviceSynchronize(); return rc; }   // whatever was enqueued is done before the frame's buffers go
    if (out_pair_scores) HR_CHECK_HIP(hipMemcpy(out_pair_scores, ps.p, pairs * 4, hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_scores, os.p, nk * 4, hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_ids, oi.p, nk * 8, hipMemcpyDeviceToHost));
    if (out_pos) HR_CHECK_HIP(hipMemcpy(out_pos, op.p, nk * 4, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hipmaxsim_info(uint64_t mv_h, int64_t* out4)
{
    HR_REQUIRE(out4, "null out");
    GET_MV(s, mv_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_CHECK_HIP(hipDeviceSynchronize());
    unsigned long long c[3] = {0, 0, 0};
    if (s->counters.p) HR_CHECK_HIP(hipMemcpy(c, s->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    out4[0] = (int64_t)c[0];
    out4[1] = (int64_t)c[1];
    out4[2] = (int64_t)c[2];
    out4[3] = 0;
    return HIPRAG_OK;
}

}  // extern "C"
