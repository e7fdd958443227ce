// m3_score.hip -- the last step of hipm3_score* (lib.cpp): BGE-M3's "dense + sparse + colbert" score of every candidate from
// the three components their own entries wrote, and the candidates of a query ranked by it.
#include <cfloat>

#include "common.h"

namespace hiprag {
namespace {

constexpr int kM3MaxDepth = 256;   // candidates per query = threads of the workgroup (hipmaxsim_dev's and hiprerank_dev's limit)

// One workgroup per query, thread t = candidate t (maxsim_select_kernel's shape).  A candidate is VALID iff it names a row of
// the dense index (hipidx_score_ids' rule).  For a valid candidate, in fp64 with contraction off:
//   s_d = the dense score (IP), 1.0 - 0.5 * dist (L2: the inner product of unit vectors);  s_s = (double)sparse score;
//   s_c = (double)MaxSim pair score, 0.0 where that pair is padding (-FLT_MAX: a document or a query without vectors);
//   combined = (((w_d * s_d) + (w_s * s_s)) + (w_c * s_c)) / W, the terms of legs that were not run (null pointer) left out.
// Rank by counting under (combined descending, position ascending); ranks past the valid candidates get id -1, -DBL_MAX,
// position -1.  out_parts: the three fp32 components as their entries wrote them (padding values included), 0.0f for a leg
// that was not run; out_pairs: combined in candidate order, -DBL_MAX for an invalid candidate.
__global__ __launch_bounds__(kM3MaxDepth) void m3_combine_kernel(M3Combine a)
{
#pragma clang fp contract(off)
    __shared__ double sl[kM3MaxDepth];
    __shared__ int sv[kM3MaxDepth];
    const int qi = blockIdx.x, t = threadIdx.x;
    const int64_t base = (int64_t)qi * a.depth;
    int64_t c = -1;
    double l = -DBL_MAX;
    bool valid = false;
    if (t < a.depth) {
        c = a.cand[base + t];
        valid = c >= 0 && c >= a.id_base && (uint64_t)c - (uint64_t)a.id_base < (uint64_t)a.ntotal;
        if (valid) {
            double acc = 0.0;
            bool have = false;
            if (a.dense64) {
                const double raw = a.dense64[base + t];
                const double sd = a.l2 ? 1.0 - 0.5 * raw : raw;
                acc = a.w_dense * sd;
                have = true;
            }
            if (a.sparse32) {
                const double p = a.w_sparse * (double)a.sparse32[base + t];
                acc = have ? acc + p : p;
                have = true;
            }
            if (a.maxsim32) {
                const float ms = a.maxsim32[base + t];
                const double p = a.w_colbert * (ms == -FLT_MAX ? 0.0 : (double)ms);
                acc = have ? acc + p : p;
            }
            l = acc / a.w_sum;
        }
        if (a.out_parts) {
            float* o = a.out_parts + (base + t) * 3;
            o[0] = a.dense32 ? a.dense32[base + t] : 0.f;
            o[1] = a.sparse32 ? a.sparse32[base + t] : 0.f;
            o[2] = a.maxsim32 ? a.maxsim32[base + t] : 0.f;
        }
        if (a.out_pairs) a.out_pairs[base + t] = l;
    }
    sl[t] = l;
    sv[t] = valid ? 1 : 0;
    if (t < a.k) {
        a.out_scores[(int64_t)qi * a.k + t] = -DBL_MAX;
        a.out_ids[(int64_t)qi * a.k + t] = -1;
        if (a.out_pos) a.out_pos[(int64_t)qi * a.k + t] = -1;
    }
    __syncthreads();   // also orders the pre-fill above before the ranked stores below
    if (!valid) return;
    int rank = 0;
    for (int j = 0; j < a.depth; ++j) rank += (sv[j] && (sl[j] > l || (sl[j] == l && j < t))) ? 1 : 0;
    if (rank < a.k) {
        a.out_scores[(int64_t)qi * a.k + rank] = l;
        a.out_ids[(int64_t)qi * a.k + rank] = c;
        if (a.out_pos) a.out_pos[(int64_t)qi * a.k + rank] = t;
    }
}

}  // namespace

// the caller (hipm3_score_dev) has checked 1 <= k <= depth <= 256 and the pointers
int32_t launch_m3_combine(const M3Combine& a, int nq, hipStream_t st)
{
    hipLaunchKernelGGL(m3_combine_kernel, dim3((unsigned)nq), dim3(kM3MaxDepth), 0, st, a);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

}  // namespace hiprag
