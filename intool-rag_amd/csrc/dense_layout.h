// dense_layout.h -- the blocked row layout of the flat index and the fp64 re-score that reads it.  Device code that more
// than one translation unit runs lives here as __device__ __forceinline__ text (the library is built without relocatable
// device code): fin_kernel and exhaustive_kernel (dense_index.hip), ivf_probe_kernel and ivf_batch_kernel (ivf_search.hip)
// and scoped_kernel (dense_scoped.hip) all score a row with the helpers below, which is why a row's score is the same bits
// whichever of them computed it.  The layout itself is described at the top of dense_index.hip.
#pragma once
#include "common.h"
#include "topk_device.h"

namespace hiprag {
namespace {

constexpr int kRowsPerBlock = 32;
constexpr int kPieceFloats = 256;
constexpr int kPieceVec4 = 64;
// Position (in float4 units) inside a 1 KiB piece of the four k-values [8p + 4h, 8p + 4h + 4) of row r of the block:
// quad-major, so that the 4 rows x 2 halves of a row QUAD are one contiguous 128-byte line of every piece -- the unit the
// fp64 re-score reads (128 whole lines per quad instead of 256 half lines 512 bytes apart).  The q64 scan reads whole
// pieces and only permutes which lane takes which 16 bytes.
__host__ __device__ __forceinline__ int piece_slot(int h, int r) { return ((r >> 2) << 3) | (h << 2) | (r & 3); }
constexpr int kMaxDPad = 1024;     // d_pad limit (the 128 KiB query tile of the scan)
constexpr int kMaxK = 1000;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------------
// fp64 re-scoring of one 4-row group straight from the blocked layout (wave-wide; result for row r0 + (lane&3)
// is returned in every lane with that low index).  The summation order depends only on the row's contents: lane
// (pq, hh) of a row's 16 lanes sums pieces p = pq, pq + 8, ... in order, four elements each, and the 16 partial sums are
// combined by the xor-4/8/16/32 butterfly.  The three steps are helpers because the IVF batch kernel (ivf_batch_kernel)
// keeps a quad group's pieces in registers and scores them against many queries: both callers run the same accumulate
// and reduce code, so a row's score is the same bits whichever path computed it.
// ------------------------------------------------------------------------------------------------------
// pieces pq + 8 * (8 * half + i), i = 0..7, of this lane's row.  P <= 128 (LDS limit of the scan), so a lane touches at
// most 16 pieces.  UNCONDITIONAL loads (pieces past P re-read the last one and are skipped by rescore_acc8):
// `p < P ? src[..] : 0` is compiled into branch + load + s_waitcnt vmcnt(0), i.e. sixteen serialized memory round trips
// per quad
template <int half>
__device__ __forceinline__ void rescore_load8(float4 (&x)[8], const float4* src, int pq, int P)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = min(pq + 8 * (8 * half + i), P - 1);
        x[i] = src[p * kPieceVec4];
    }
}
template <int METRIC, int half>
__device__ __forceinline__ void rescore_acc8(double& acc, const float4 (&x)[8], int pq, int hh, int P,
                                             const float* __restrict__ qv /* LDS, d_pad floats, zero padded */)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = pq + 8 * (8 * half + i);
        if (p < P) {
            const float* qq = qv + 8 * p + 4 * hh;
            if (METRIC == HIPRAG_METRIC_IP) {
                acc += (double)x[i].x * (double)qq[0];
                acc += (double)x[i].y * (double)qq[1];
                acc += (double)x[i].z * (double)qq[2];
                acc += (double)x[i].w * (double)qq[3];
            } else {
                double t;
                t = (double)x[i].x - (double)qq[0]; acc += t * t;
                t = (double)x[i].y - (double)qq[1]; acc += t * t;
                t = (double)x[i].z - (double)qq[2]; acc += t * t;
                t = (double)x[i].w - (double)qq[3]; acc += t * t;
            }
        }
    }
}
__device__ __forceinline__ double rescore_reduce16(double acc)
{
#pragma unroll
    for (int off = 4; off <= 32; off <<= 1) acc += __shfl_xor(acc, off);
    return acc;
}

template <int METRIC>
__device__ __forceinline__ double rescore4(const float4* __restrict__ xb, int P, int64_t blk, int r0,
                                           const float* __restrict__ qv /* LDS, d_pad floats, zero padded */)
{
    const int lane = threadIdx.x & 63;
    const int rr = lane & 3, hh = (lane >> 2) & 1, pq = lane >> 3;
    const float4* src = xb + blk * P * kPieceVec4 + piece_slot(hh, r0 + rr);
    // Loads go out in batches of 8 before their first use: a dependent-latency loop here costs an HBM round trip per
    // piece and used to dominate the finish kernel; all 16 at once spills at the 128-VGPR budget of the 16-wave finish
    // workgroup.  (P >= 1: d >= 1.)
    double acc = 0.0;
    float4 x[8];
    rescore_load8<0>(x, src, pq, P);
    rescore_acc8<METRIC, 0>(acc, x, pq, hh, P, qv);
    rescore_load8<1>(x, src, pq, P);
    rescore_acc8<METRIC, 1>(acc, x, pq, hh, P, qv);
    return rescore_reduce16(acc);
}
}  // namespace
}  // namespace hiprag
