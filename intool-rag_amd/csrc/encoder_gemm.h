// encoder_gemm.h -- the encoder's three GEMM families, C = A[M,K] * W[N,K]^T in bf16 with fp32 accumulation on
// v_mfma_f32_16x16x32_bf16, and the one launcher each is started from:
//   gemm_bf16_kernel    128 x 128 x 64 LDS-tiled, fused epilogues: QKV (bias, 1/8 scale on q, head-major q/k and TRANSPOSED
//                       v), GELU (bias + erf-GELU), RESID (bias + residual -> fp32 pre-LayerNorm buffer), PART (raw partials)
//   gemm256_kernel      256 x 256 persistent tiles for big batches (gemm256.h)
//   gemm_skinny_kernel  the same products for a few hundred token rows (one query, a few short texts) as weight-streaming
//                       workgroups of 16/32 columns; split-K partials are summed by the LayerNorm
// Which family a batch takes is decided in encoder_plan.h.  Included by encoder.hip alone, inside hiprag's anonymous
// namespace; Encoder's forward and the test hooks (hipenc_linear_ex) both launch through launch_tiled / launch256_grid /
// launch_skinny, so a hook runs the grid the model runs.
// LDS tiles are stored k-chunk-major ([k/8][row][8 bf16]) with row ^= (chunk & 7): fragment reads (ds_read_b128) and
// the staging writes are both bank-conflict free (checked by brute force over the ds_read_b128 lane groups).
#pragma once

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __bf16 bf16;

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kGemmThreads = 256;
static_assert(BM == kTileM && BN == kTileN && BK == kTileK, "encoder_plan.h plans for these tiles");

__device__ __forceinline__ int swz_unit(int kc, int row, int rows) { return kc * rows + (row ^ (kc & 7)); }

// The values are template arguments of the kernels, i.e. part of their symbol names; hipenc_linear_ex's `epilogue` has a
// numbering of its own (encoder.hip: abi_epilogue).
enum { EPI_QKV = 0, EPI_GELU = 1, EPI_RESID = 2, EPI_PART = 3, EPI_RESID16 = 4 };   // RESID16: bf16 pre-LayerNorm rows (gemm256.h)

struct GemmArgs {
    const bf16* A;      // [M, K] row-major
    const bf16* W;      // [N, K] row-major (torch Linear weight)
    const float* bias;  // [N]
    int M, N, K;
    // EPI_QKV
    bf16* q;            // [nseq, heads, S, 64]
    bf16* k;            // [nseq, heads, S, 64]
    bf16* vt;           // [nseq, heads, 64, S]
    int S, heads, H;
    // EPI_GELU
    bf16* out_bf16;     // [M, N]
    // EPI_RESID
    const bf16* resid;  // [M, N]
    float* out_f32;     // [M, N]
    // EPI_PART: raw fp32 partial products [ksplit][M][N] (K split over workgroups; the LayerNorm that follows adds them)
    int ksplit;
};

// Exact-erf GELU, x * Phi(x), with ONE transcendental per element.  Phi(-z) = erfc(z / sqrt 2) / 2 for z = |x| is written
// as exp2(p(z)), p = degree-7 polynomial fit of log2 Phi(-z) on [0, 6] (Chebyshev least squares in fp64, monomial
// coefficients below): relative error of Phi(-z) <= 9.1e-6, absolute error of the GELU value <= 5.1e-7 over all x
// (checked against fp64 erf on 2M points; bf16, which the value is rounded to next, resolves 3.9e-3 relative).  Then
// GELU(x) = x * (x > 0 ? 1 - Phi(-z) : Phi(-z)); beyond |x| = 6 the tail is clamped at Phi(-6) = 1e-9.
// The Abramowitz-Stegun form used before took two transcendentals (v_rcp, v_exp: 8 issue cycles each) and ~15 other
// instructions per element; the H -> F epilogue runs 128 of these per lane and tile with nothing to hide behind.
__device__ __forceinline__ float gelu_exact(float x)
{
    const float z = fminf(fabsf(x), 6.f);
    float p = -1.9448814327915898e-06f;
    p = __builtin_fmaf(p, z, 6.385969027178362e-05f);
    p = __builtin_fmaf(p, z, -0.0009488638024777174f);
    p = __builtin_fmaf(p, z, 0.008582341484725475f);
    p = __builtin_fmaf(p, z, -0.05411824584007263f);
    p = __builtin_fmaf(p, z, -0.4582975208759308f);
    p = __builtin_fmaf(p, z, -1.1513246297836304f);
    p = __builtin_fmaf(p, z, -0.9999869465827942f);
    const float t = __builtin_amdgcn_exp2f(p);
    return x * (x > 0.f ? 1.f - t : t);
}

// LDS tile image: 128 rows x 64 bf16 = 128-B rows of eight 16-B chunks, chunk kc of row r stored at slot kc ^ (r & 7).
// One global_load_lds_dwordx4 wave-instruction fills eight whole rows (lane = row*8 + slot fetches chunk slot ^ (row&7)
// of its row: LDS side lane-linear as the DMA requires, global side 128 B contiguous per row), and the MFMA fragment
// reads (16 rows x one chunk per ds_read_b128 lane group) hit 16 distinct 16-B bank slots: conflict-free both ways.
__device__ __forceinline__ int tile_unit(int row, int kc) { return row * 8 + (kc ^ (row & 7)); }

typedef __attribute__((address_space(3))) void* lds_ptr_t;

template <int EPI>
__global__ __launch_bounds__(kGemmThreads) void gemm_bf16_kernel(GemmArgs g)
{
    __shared__ bf16x8 lds[2][2][BM * BK / 8];  // [buffer][A|B][unit]; 64 KiB, reused as the fp32 C tile in the epilogue
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;    // 2 x 2 waves, 64 x 64 each
    const int r16 = lane & 15, kq = lane >> 4;

    // XCD-aware block mapping: consecutive block ids go round-robin over the 8 XCDs, so give each XCD a contiguous range
    // of tiles; inside it the N index runs fastest, i.e. the blocks sharing an A row-panel share one L2.
    const int nbn = g.N / BN;
    const int ksplit = EPI == EPI_PART ? g.ksplit : 1;
    const int nblk = gridDim.x / ksplit;
    const int split = blockIdx.x / nblk, bid = blockIdx.x - split * nblk;
    const int per = nblk >> 3, rem = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int pid = (xcd < rem ? xcd * (per + 1) : rem * (per + 1) + (xcd - rem) * per) + idx;
    // tile order inside an XCD's range: groups of 8 column tiles, row tiles fastest inside a group -- the group's weight
    // tiles (1024 rows of W = 2 MB at K = 1024) stay L2-resident while the activations stream past them (3 % over
    // row-major tile order on the 256 x 512 batch)
    constexpr int GN = 8;
    const int nbm = nblk / nbn;
    const int grp = pid / (GN * nbm), rest = pid - grp * GN * nbm;
    const int gw = min(GN, nbn - grp * GN);          // width of this (possibly last, narrower) group
    const int m0 = (rest / gw) * BM, n0 = (grp * GN + rest % gw) * BN;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging by LDS-DMA: 16 wave-instructions of 1 KiB per operand tile, 4 per wave
    const int srow = lane >> 3, sslot = lane & 7;
    auto stage = [&](int buf, int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int inst = wave * 4 + i;
            const int row = inst * 8 + srow;
            const int kc = sslot ^ (row & 7);
            const bf16* ga = g.A + (size_t)(m0 + row) * g.K + k0 + kc * 8;
            const bf16* gb = g.W + (size_t)(n0 + row) * g.K + k0 + kc * 8;
            __builtin_amdgcn_global_load_lds((const void*)ga, (lds_ptr_t)&lds[buf][0][inst * 64], 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)gb, (lds_ptr_t)&lds[buf][1][inst * 64], 16, 0, 0);
        }
    };

    const int nk = g.K / ksplit / BK;
    const int kbeg = split * (g.K / ksplit);
    stage(0, kbeg);
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of tile kt has landed
        __syncthreads();                                   // ... everyone's has, and buffer buf^1 is no longer being read
        if (kt + 1 < nk) stage(buf ^ 1, kbeg + (kt + 1) * BK);    // DMA of the next tile flies under this tile's MFMAs
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[4], bfr[4];
            const int kc = ks * 4 + kq;
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = lds[buf][0][tile_unit(wr * 64 + i * 16 + r16, kc)];
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[j] = lds[buf][1][tile_unit(wc * 64 + j * 16 + r16, kc)];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();  // all fragment reads done: the staging buffers become the C tile

    // ---- epilogue: C tile through LDS so that every global store is a 16-byte vector ---------------------------------
    float* ct = reinterpret_cast<float*>(&lds[0][0][0]);  // [128][128] fp32 = 64 KiB
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                ct[(wr * 64 + i * 16 + 4 * kq + r) * BN + wc * 64 + j * 16 + r16] = acc[i][j][r];
    __syncthreads();

    if (EPI == EPI_QKV && n0 >= 2 * g.H) {
        // V third: stored transposed [seq, head, d, S]: thread = one column (d) x 8 consecutive tokens -> one 16-B store
        const int col = tid & 127, half = tid >> 7;
        const int n = n0 + col;
        const float bias = g.bias[n];
        const int hn = n - 2 * g.H;
        const int head = hn >> 6, dd = hn & 63;
        for (int rc = half; rc < 16; rc += 2) {
            const int m = m0 + rc * 8;
            if (m >= g.M) break;
            const int seq = m / g.S, s0 = m - seq * g.S;
            bf16x8 v;
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = (bf16)(ct[(rc * 8 + t) * BN + col] + bias);
            *reinterpret_cast<bf16x8*>(g.vt + (((size_t)seq * g.heads + head) * 64 + dd) * g.S + s0) = v;
        }
        return;
    }
    // row-major outputs: thread = 8 consecutive columns of one row; 16 column groups x 128 rows = 2048 vectors
    for (int v = tid; v < BM * (BN / 8); v += kGemmThreads) {
        const int row = v >> 4, cg = v & 15;
        const int m = m0 + row, n = n0 + cg * 8;
        if (m >= g.M) continue;
        const float4 c0 = *reinterpret_cast<const float4*>(ct + row * BN + cg * 8);
        const float4 c1 = *reinterpret_cast<const float4*>(ct + row * BN + cg * 8 + 4);
        if (EPI == EPI_PART) {
            float* dst = g.out_f32 + ((size_t)split * g.M + m) * g.N + n;
            *reinterpret_cast<float4*>(dst) = c0;
            *reinterpret_cast<float4*>(dst + 4) = c1;
            continue;
        }
        const float4 b0 = *reinterpret_cast<const float4*>(g.bias + n);
        const float4 b1 = *reinterpret_cast<const float4*>(g.bias + n + 4);
        float x[8] = {c0.x + b0.x, c0.y + b0.y, c0.z + b0.z, c0.w + b0.w, c1.x + b1.x, c1.y + b1.y, c1.z + b1.z, c1.w + b1.w};
        if (EPI == EPI_QKV) {
            const int which = n / g.H, hn = n - which * g.H;   // which in {0 (q), 1 (k)}: the V third returned above
            const int head = hn >> 6, dd = hn & 63;
            const int seq = m / g.S, s = m - seq * g.S;
            const float scale = which == 0 ? 0.125f : 1.f;     // 1/sqrt(64) folded into q, exact
            bf16x8 o;
#pragma unroll
            for (int t = 0; t < 8; ++t) o[t] = (bf16)(x[t] * scale);
            bf16* dst = (which == 0 ? g.q : g.k) + ((((size_t)seq * g.heads + head) * g.S + s) * 64 + dd);
            *reinterpret_cast<bf16x8*>(dst) = o;
        } else if (EPI == EPI_GELU) {
            bf16x8 o;
#pragma unroll
            for (int t = 0; t < 8; ++t) o[t] = (bf16)gelu_exact(x[t]);
            *reinterpret_cast<bf16x8*>(g.out_bf16 + (size_t)m * g.N + n) = o;
        } else {
            const bf16x8 rs = *reinterpret_cast<const bf16x8*>(g.resid + (size_t)m * g.N + n);
            float4 o0, o1;
            o0.x = x[0] + (float)rs[0]; o0.y = x[1] + (float)rs[1]; o0.z = x[2] + (float)rs[2]; o0.w = x[3] + (float)rs[3];
            o1.x = x[4] + (float)rs[4]; o1.y = x[5] + (float)rs[5]; o1.z = x[6] + (float)rs[6]; o1.w = x[7] + (float)rs[7];
            float* dst = g.out_f32 + (size_t)m * g.N + n;
            *reinterpret_cast<float4*>(dst) = o0;
            *reinterpret_cast<float4*>(dst + 4) = o1;
        }
    }
}

#include "gemm256.h"
static_assert(G2_T == kBigTile && G2_BK == kBigK, "encoder_plan.h plans for these tiles");

// ---------------------------------------------------------------------------------------------------------
// Small-batch GEMM (the single-query latency path: embed_single / a handful of short texts, rows <= ~1024).
// With 64..1024 activation rows the 128x128 tiles above leave 8..32 workgroups walking K serially (40 us for the F->H
// GEMM of one query); here the work is what it really is -- streaming the weight matrix once: a workgroup owns 16 output
// columns over a K range of <= 1024 (its four waves a quarter each, W fragments loaded straight from HBM in MFMA layout,
// 16 B per lane, and kept in registers), multiplies them with up to four 64-row blocks of A (fragments from L2), sums the
// four waves' partial tiles through LDS in a fixed order and runs the epilogue.  K > 1024 splits over workgroups
// (ksplit = K / Kc) which write raw fp32 partials [ksplit][M][N]; the LayerNorm that follows adds them up in split order,
// so there are no atomics and results do not depend on scheduling.
// ---------------------------------------------------------------------------------------------------------
constexpr int SK_STEPS = 8;   // 32-deep MFMA steps per wave (K range per workgroup <= 4 * 8 * 32 = 1024)
static_assert(4 * SK_STEPS * 32 == kSkinnyMaxK && 4 * 32 == kSkinnyKGrain, "encoder_plan.h plans for this K range");

// NT: 16-column tiles per wave (the workgroup owns 16 * NT output columns; NT = 2 halves the L2 reads of A, which every
// column tile repeats, and is used from 128 rows up).  FULL: the K range per workgroup is exactly 1024 (the real model:
// H = 1024, F = 4096) -- every load is issued before the first MFMA; otherwise a plain loop over `steps`.
template <int EPI, int NT, bool FULL>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(GemmArgs g, int kc, int steps, int mb_per_wg)
{
    constexpr int WN = 16 * NT;
    __shared__ float red[4][64][WN];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    const int ntile = g.N / WN;
    const int split = blockIdx.x / ntile, n0 = (blockIdx.x - split * ntile) * WN;
    const int kw0 = split * kc + wave * (kc >> 2);
    const size_t k16 = (size_t)16 * g.K;

    const bf16* wp = g.W + (size_t)(n0 + r16) * g.K + kw0 + kq * 8;
    bf16x8 bfr[NT][SK_STEPS];
    if (FULL) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int s = 0; s < SK_STEPS; ++s) bfr[j][s] = *reinterpret_cast<const bf16x8*>(wp + j * k16 + s * 32);
    }

    const int mb0 = blockIdx.y * mb_per_wg, mb1 = min(mb0 + mb_per_wg, g.M >> 6);
    for (int mb = mb0; mb < mb1; ++mb) {
        f32x4 acc[4][NT];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const bf16* ap = g.A + (size_t)(mb * 64 + r16) * g.K + kw0 + kq * 8;
        if (FULL) {
            bf16x8 af[4][SK_STEPS];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int s = 0; s < SK_STEPS; ++s) af[i][s] = *reinterpret_cast<const bf16x8*>(ap + i * k16 + s * 32);
            __builtin_amdgcn_sched_barrier(0);  // all 32 (+ 8 NT) loads in flight before the first MFMA waits: one round trip
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int s = 0; s < SK_STEPS; ++s)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][s], bfr[j][s], acc[i][j], 0, 0, 0);
        } else {
#pragma unroll 1
            for (int s = 0; s < steps; ++s) {
                bf16x8 b[NT], a[4];
#pragma unroll
                for (int j = 0; j < NT; ++j) b[j] = *reinterpret_cast<const bf16x8*>(wp + j * k16 + s * 32);
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8*>(ap + i * k16 + s * 32);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[wave][i * 16 + 4 * kq + r][j * 16 + r16] = acc[i][j][r];
        __syncthreads();

        typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
        if (EPI == EPI_QKV && n0 >= 2 * g.H) {
            // V third, stored transposed [seq, head, d, S]: one column x 4 consecutive tokens -> one 8-B store
#pragma unroll
            for (int e = 0; e < NT; ++e) {
                const int ch = tid + 256 * e;
                const int col = ch % WN, rg = (ch / WN) * 4;
                const int n = n0 + col, hn = n - 2 * g.H;
                const int head = hn >> 6, dd = hn & 63;
                const float bias = g.bias[n];
                const int m = mb * 64 + rg;
                const int seq = m / g.S, s0 = m - seq * g.S;
                bf16x4 v;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    v[u] = (bf16)((((red[0][rg + u][col] + red[1][rg + u][col]) + red[2][rg + u][col]) + red[3][rg + u][col]) + bias);
                *reinterpret_cast<bf16x4*>(g.vt + (((size_t)seq * g.heads + head) * 64 + dd) * g.S + s0) = v;
            }
        } else {
            // row-major outputs: 4 consecutive columns of one row per item
#pragma unroll
            for (int e = 0; e < NT; ++e) {
                const int ch = tid + 256 * e;
                const int row = ch / (4 * NT), c4 = (ch % (4 * NT)) * 4;
                const int m = mb * 64 + row, n = n0 + c4;
                const float4 p0 = *reinterpret_cast<const float4*>(&red[0][row][c4]);
                const float4 p1 = *reinterpret_cast<const float4*>(&red[1][row][c4]);
                const float4 p2 = *reinterpret_cast<const float4*>(&red[2][row][c4]);
                const float4 p3 = *reinterpret_cast<const float4*>(&red[3][row][c4]);
                float x[4] = {((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y, ((p0.z + p1.z) + p2.z) + p3.z,
                              ((p0.w + p1.w) + p2.w) + p3.w};
                if (EPI == EPI_PART) {
                    *reinterpret_cast<float4*>(g.out_f32 + ((size_t)split * g.M + m) * g.N + n) = make_float4(x[0], x[1], x[2], x[3]);
                } else {
                    const float4 b = *reinterpret_cast<const float4*>(g.bias + n);
                    x[0] += b.x; x[1] += b.y; x[2] += b.z; x[3] += b.w;
                    bf16x4 o;
                    if (EPI == EPI_QKV) {
                        const int which = n / g.H, hn = n - which * g.H;   // 0 (q) or 1 (k)
                        const int head = hn >> 6, dd = hn & 63;
                        const int seq = m / g.S, s = m - seq * g.S;
                        const float scale = which == 0 ? 0.125f : 1.f;
#pragma unroll
                        for (int u = 0; u < 4; ++u) o[u] = (bf16)(x[u] * scale);
                        bf16* dst = (which == 0 ? g.q : g.k) + ((((size_t)seq * g.heads + head) * g.S + s) * 64 + dd);
                        *reinterpret_cast<bf16x4*>(dst) = o;
                    } else {  // EPI_GELU
#pragma unroll
                        for (int u = 0; u < 4; ++u) o[u] = (bf16)gelu_exact(x[u]);
                        *reinterpret_cast<bf16x4*>(g.out_bf16 + (size_t)m * g.N + n) = o;
                    }
                }
            }
        }
        __syncthreads();  // the partial tiles are free for the next row block
    }
}

// ---- the launchers, and which epilogues each family has (a kernel is instantiated for these and no others) ----------------
constexpr bool tiled_has(int epi) { return epi == EPI_QKV || epi == EPI_GELU || epi == EPI_RESID || epi == EPI_PART; }
constexpr bool tile256_has(int epi) { return epi == EPI_QKV || epi == EPI_GELU || epi == EPI_RESID || epi == EPI_RESID16; }
constexpr bool skinny_has(int epi) { return epi == EPI_QKV || epi == EPI_GELU || epi == EPI_PART; }

// 128 x 128 tiles over Mpad padded rows (a.M is the number of rows the epilogue may write); EPI_PART multiplies the grid
// by a.ksplit and writes fp32 partials [ksplit][a.M][N].
template <int EPI>
static void launch_tiled(const GemmArgs& a, int Mpad, hipStream_t st)
{
    static_assert(tiled_has(EPI), "the 128-tile kernel has no such epilogue");
    const int ks = EPI == EPI_PART ? a.ksplit : 1;
    hipLaunchKernelGGL(gemm_bf16_kernel<EPI>, dim3((a.N / BN) * (Mpad / BM) * ks), dim3(kGemmThreads), 0, st, a);
}

// 256 x 256 persistent tiles: one workgroup per CU at most; max_wg > 0 caps the grid further (test hook: several tiles per
// workgroup at small shapes).  Any grid in [1, tiles] is valid: the kernel's XCD order needs grid % 8 == 0 and falls back
// to the plain order vw = blockIdx.x otherwise, both of which visit every tile exactly once.
template <int EPI>
static void launch256_grid(const GemmArgs& a, int Mpad, int n_cu, int max_wg, hipStream_t st)
{
    static_assert(tile256_has(EPI), "the 256-tile kernel has no such epilogue");
    const int nbm = Mpad / G2_T, nbn = a.N / G2_T;
    int grid = std::min(nbm * nbn, n_cu);
    if (max_wg > 0) grid = std::min(grid, max_wg);
    hipLaunchKernelGGL(gemm256_kernel<EPI>, dim3(grid), dim3(G2_THREADS), 0, st, a, nbm, nbn);
}

template <int EPI>
static void launch_skinny(GemmArgs a, hipStream_t st)
{
    static_assert(skinny_has(EPI), "the small-batch kernel has no such epilogue");
    const int sp = skinny_split(a.K), kc = a.K / sp, steps = kc / 128;
    const bool wide = a.M >= 128 && a.N % 32 == 0;     // two column tiles per wave: half the L2 reads of A
    // row blocks run one after the other inside a workgroup (a round trip to L2 each): spread them over workgroups
    // until the launch has ~1024 of them, W comes out of L2 for all but the first
    const int gx = (a.N / (wide ? 32 : 16)) * sp, mblocks = a.M >> 6;
    const int mb = std::max(1, (gx * mblocks + 1023) / 1024);
    const dim3 grid(gx, (mblocks + mb - 1) / mb);
    if (steps == SK_STEPS) {
        if (wide) hipLaunchKernelGGL((gemm_skinny_kernel<EPI, 2, true>), grid, dim3(256), 0, st, a, kc, steps, mb);
        else hipLaunchKernelGGL((gemm_skinny_kernel<EPI, 1, true>), grid, dim3(256), 0, st, a, kc, steps, mb);
    } else {
        if (wide) hipLaunchKernelGGL((gemm_skinny_kernel<EPI, 2, false>), grid, dim3(256), 0, st, a, kc, steps, mb);
        else hipLaunchKernelGGL((gemm_skinny_kernel<EPI, 1, false>), grid, dim3(256), 0, st, a, kc, steps, mb);
    }
}
