// encoder_layers.h -- what a layer of the encoder runs besides its GEMMs (encoder_gemm.h), and the launchers:
//   K5  embed_ln_kernel      gather + LayerNorm -> bf16; embed_ln_packed_kernel: the same row body over a packed batch
//       layernorm_kernel     fp32 pre-LN rows (or split-K partials + bias + residual) -> bf16
//       layernorm16_kernel   bf16 pre-LN rows (big-batch path) -> bf16
//   K7  attention2_kernel    flash-style, computed transposed: 128 queries x 32-key tiles, online softmax in fp32, P stays in registers;
//                            ONE body over two layouts of the batch (AttPadded, AttPacked: encoder_packed.h)
// Included by encoder.hip alone, inside hiprag's anonymous namespace, after encoder_gemm.h (bf16x8, lds_ptr_t).  Encoder's
// forward and the test hooks (hipenc_attention, hipenc_attention_packed, hipenc_layernorm) both come through launch_attention /
// launch_attention_packed / launch_layernorm / launch_layernorm16, so a hook runs the grid and arguments the model runs.
#pragma once

// ---------------------------------------------------------------------------------------------------------
// LayerNorm over rows of an fp32 [M,H] buffer -> bf16; one wave per row.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// PARTS: the row is the sum of `nsplit` fp32 partial products (gemm_skinny_kernel<EPI_PART>, split order) + bias + the
// bf16 residual row -- the same (c + bias) + residual order as the EPI_RESID epilogue of the tiled GEMM.
template <bool PARTS>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, bf16* __restrict__ y, int M, int H,
                                                       float eps, int nsplit, const float* __restrict__ bias,
                                                       const bf16* __restrict__ resid)
{
    // one wave per row; the row is read ONCE (16 B per lane per load, kept in registers: H <= 2048 -> <= 8 float4)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)row * H);
    const int nv = H >> 8;  // float4 per lane (H is a multiple of 128; a 128-wide remainder is handled by half the lanes)
    float4 v[8], gm[8], bt[8];
    float s = 0.f;
    const int nvec = H >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    const float4* b4 = reinterpret_cast<const float4*>(beta);
    // every load of the row's working set is issued up front and UNCONDITIONALLY (clamped column): a load under a lane
    // mask is compiled into branch + load + wait, one memory round trip each
    if (PARTS) {   // latency path only: the batch path is bandwidth-bound and better off with fewer live registers
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int cc = min(i * 64 + lane, nvec - 1);
            gm[i] = g4[cc];
            bt[i] = b4[cc];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = i * 64 + lane;
        if (PARTS) {
            v[i] = xr[min(c, nvec - 1)];
            if (c >= nvec) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            v[i] = c < nvec ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (PARTS) {
            typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4r;
            const int cc = min(c, nvec - 1);
            float4 p[3];
#pragma unroll
            for (int sp = 1; sp < 4; ++sp) p[sp - 1] = xr[(size_t)min(sp, nsplit - 1) * M * (H >> 2) + cc];
            const float4 b = reinterpret_cast<const float4*>(bias)[cc];
            const bf16x4r rs = reinterpret_cast<const bf16x4r*>(resid + (size_t)row * H)[cc];
            if (c < nvec) {
#pragma unroll
                for (int sp = 1; sp < 4; ++sp)
                    if (sp < nsplit) { v[i].x += p[sp - 1].x; v[i].y += p[sp - 1].y; v[i].z += p[sp - 1].z; v[i].w += p[sp - 1].w; }
                v[i].x = (v[i].x + b.x) + (float)rs[0]; v[i].y = (v[i].y + b.y) + (float)rs[1];
                v[i].z = (v[i].z + b.z) + (float)rs[2]; v[i].w = (v[i].w + b.w) + (float)rs[3];
            }
        }
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    (void)nv;
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = i * 64 + lane;
        if (c < nvec) {
            const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    bf16x4* yr = reinterpret_cast<bf16x4*>(y + (size_t)row * H);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = i * 64 + lane;
        if (c < nvec) {
            const float4 g = PARTS ? gm[i] : g4[c], b = PARTS ? bt[i] : b4[c];
            bf16x4 o;
            o[0] = (bf16)((v[i].x - mean) * rstd * g.x + b.x);
            o[1] = (bf16)((v[i].y - mean) * rstd * g.y + b.y);
            o[2] = (bf16)((v[i].z - mean) * rstd * g.z + b.z);
            o[3] = (bf16)((v[i].w - mean) * rstd * g.w + b.w);
            yr[c] = o;
        }
    }
}

// LayerNorm over bf16 pre-LN rows (the big-batch path: gemm256's RESID16 epilogue) -> bf16.  One wave per FOUR consecutive
// rows: all of their loads (16 B per lane each, H <= 1024 here: 2 per row) are in flight before the first reduction, gamma
// and beta are loaded once per wave; statistics in fp32.  HBM-bound: 2 + 2 bytes per element.
constexpr int kLn16Rows = 4;
__global__ __launch_bounds__(256) void layernorm16_kernel(const bf16* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, bf16* __restrict__ y, int M, int H,
                                                         float eps)
{
    const int lane = threadIdx.x & 63;
    const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * kLn16Rows;
    if (row0 >= M) return;
    const int nvec = H >> 3;                                   // 16-B vectors per row, <= 128
    const int c0 = min(lane, nvec - 1), c1 = min(64 + lane, nvec - 1);
    const bool a0 = lane < nvec, a1 = 64 + lane < nvec;
    bf16x8 v[kLn16Rows][2];
#pragma unroll
    for (int r = 0; r < kLn16Rows; ++r) {
        const bf16x8* xr = reinterpret_cast<const bf16x8*>(x + (size_t)min(row0 + r, M - 1) * H);
        v[r][0] = xr[c0];
        v[r][1] = xr[c1];
    }
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    const float4* b4 = reinterpret_cast<const float4*>(beta);
    float gg[2][8], bb[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = i == 0 ? c0 : c1;
        const float4 g0 = g4[2 * c], g1 = g4[2 * c + 1], b0 = b4[2 * c], b1 = b4[2 * c + 1];
        gg[i][0] = g0.x; gg[i][1] = g0.y; gg[i][2] = g0.z; gg[i][3] = g0.w; gg[i][4] = g1.x; gg[i][5] = g1.y; gg[i][6] = g1.z; gg[i][7] = g1.w;
        bb[i][0] = b0.x; bb[i][1] = b0.y; bb[i][2] = b0.z; bb[i][3] = b0.w; bb[i][4] = b1.x; bb[i][5] = b1.y; bb[i][6] = b1.z; bb[i][7] = b1.w;
    }
#pragma unroll
    for (int r = 0; r < kLn16Rows; ++r) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += (a0 ? (float)v[r][0][e] : 0.f) + (a1 ? (float)v[r][1][e] : 0.f);
        const float mean = wave_sum(s) / (float)H;
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d0 = (float)v[r][0][e] - mean, d1 = (float)v[r][1][e] - mean;
            q += (a0 ? d0 * d0 : 0.f) + (a1 ? d1 * d1 : 0.f);
        }
        const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
        if (row0 + r < M) {
            bf16x8* yr = reinterpret_cast<bf16x8*>(y + (size_t)(row0 + r) * H);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (bf16)(((float)v[r][i][e] - mean) * rstd * gg[i][e] + bb[i][e]);
                if (i == 0 ? a0 : a1) yr[i == 0 ? c0 : c1] = o;
            }
        }
    }
}

// K5: embeddings.  tokens [nseq, S] (pad beyond len), position id = s + pad_id + 1 for real tokens, pad_id for pads
// (transformers' create_position_ids_from_input_ids with no interior pads).  One wave per token.
// The row body of both layouts: `real` rows hold token `tok` at position s of their sequence; the others are zeros.
__device__ __forceinline__ void embed_ln_row(bf16* __restrict__ yr, bool real, int tok, int s, int lane,
                                             const bf16* __restrict__ word, const bf16* __restrict__ pos,
                                             const bf16* __restrict__ type0, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, int H, int pad_id, float eps)
{
    if (!real) {  // padding rows are zeros: they never reach a real token (keys are masked)
        for (int c = lane; c < H; c += 64) yr[c] = (bf16)0.f;
        return;
    }
    const bf16* w = word + (size_t)tok * H;
    const bf16* p = pos + (size_t)(s + pad_id + 1) * H;
    float vals[32];  // H <= 2048
    float sum = 0.f;
    int n = 0;
    for (int c = lane; c < H; c += 64, ++n) {
        const float t = (float)w[c] + (float)p[c] + (float)type0[c];
        vals[n] = t;
        sum += t;
    }
    const float mean = wave_sum(sum) / (float)H;
    float var = 0.f;
    for (int i = 0; i < n; ++i) { const float t = vals[i] - mean; var += t * t; }
    const float rstd = rsqrtf(wave_sum(var) / (float)H + eps);
    n = 0;
    for (int c = lane; c < H; c += 64, ++n) yr[c] = (bf16)((vals[n] - mean) * rstd * gamma[c] + beta[c]);
}

__global__ __launch_bounds__(256) void embed_ln_kernel(const int* __restrict__ tokens, const int* __restrict__ lens, int S,
                                                      int nseq, const bf16* __restrict__ word, const bf16* __restrict__ pos,
                                                      const bf16* __restrict__ type0, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, bf16* __restrict__ y, int H, int pad_id,
                                                      float eps, int M)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int seq = row / S, s = row - seq * S;
    const bool real = seq < nseq && s < lens[seq];
    embed_ln_row(y + (size_t)row * H, real, real ? tokens[(size_t)seq * S + s] : 0, s, lane, word, pos, type0, gamma, beta, H,
                 pad_id, eps);
}

// K5 for a packed batch (encoder_packed.h): tokens [Tp], row -> (sequence, position) through the granule owners.  Rows at
// and behind Tp (GEMM padding up to M) are zeros like every other padding row.
__global__ __launch_bounds__(256) void embed_ln_packed_kernel(const int* __restrict__ tokens, const int* __restrict__ lens,
                                                             const int* __restrict__ row_off, const int* __restrict__ gran_seq,
                                                             int Tp, const bf16* __restrict__ word, const bf16* __restrict__ pos,
                                                             const bf16* __restrict__ type0, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, bf16* __restrict__ y, int H,
                                                             int pad_id, float eps, int M)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    int s = 0;
    bool real = false;
    if (row < Tp) {
        const int seq = gran_seq[row >> 6];
        s = row - row_off[seq];
        real = s < lens[seq];
    }
    embed_ln_row(y + (size_t)row * H, real, real ? tokens[row] : 0, s, lane, word, pos, type0, gamma, beta, H, pad_id, eps);
}

// ---------------------------------------------------------------------------------------------------------
// K7: attention -- transposed flash attention on v_mfma_f32_32x32x16_bf16 with LDS-DMA staging.
// q,k: [nseq, heads, S, 64] (q pre-scaled by 1/8), vt: [nseq, heads, 64, S]; ctx out: [M, H] row-major.  Everything is computed
// TRANSPOSED (S^T = K Q^T, O^T = V^T P^T) so that the probabilities never leave registers.
// What round 1's kernel (16x16x32 MFMAs, register staging; removed in round 3) spent its time on was not the matrix pipe
// (0.17 busy, r01) but ~550 vector instructions per 64-key tile and wave: the key mask, the rescale of the output accumulators and their trips to and from the accumulator file on
// EVERY tile, three operations per exponential, four cross-lane shuffles per tile, K / V tiles hauled global -> registers
// -> LDS between two barriers.  Here:
//   * a wave owns ONE tile of 32 queries; S^T = K Q^T puts a query on lanes q and q + 32, each holding 16 of a 32-key
//     tile's scores: the row maximum needs one v_permlane32_swap per 64 keys, the row sum none at all until the end
//     (every lane keeps its own partial sum; the rescale factor is the same for both halves);
//   * the accumulators are rescaled only in tiles where some row maximum of the wave actually rose (wave-uniform branch;
//     exact -- not a thresholded skip), the key mask only runs in the one tile that crosses the sequence length;
//   * p = exp2(s * log2e - m * log2e): one fma + one v_exp per score;
//   * K and V^T tiles (8 KiB each) arrive by LDS-DMA into a double buffer, swizzled on the source side
//     (chunk ^ ((row >> 1) & 7): conflict-free for the b128 K-fragment reads AND the 8-byte V^T-fragment reads): one
//     barrier per tile, the next tile's DMA in flight under this tile's MFMAs;
//   * P^T never leaves registers: element j of lane half h of k-step s is key 16 s + 8 (j >> 2) + 4 h + (j & 3) -- the order
//     the S^T accumulators already have -- and the V^T fragments are read in that order (two 8-byte runs);
//   * the output tile goes through the (by then free) LDS buffers into 16-byte row-major stores.
// grid (ceil(S/128), heads, nseq), 4 waves x 32 queries.
// ---------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(16))) float f32x16;

// The kernel is ONE body over two layouts of the batch; a layout says where a workgroup's sequence lies:
//   AttPadded  q, k [nseq][heads][S][64], vt [nseq][heads][64][S], ctx rows seq * S + query; grid (ceil(S/128), heads, nseq)
//   AttPacked  (encoder_packed.h) q, k [heads][Tp][64], vt [heads][64][Tp], the sequence's rows start at row_off[seq];
//              grid (work items, heads): item = (seq, 128-query tile counted FROM THE SEQUENCE'S FIRST ROW).  A tile of a
//              sequence with 64 or 192 rows overhangs into the next sequence's rows, or past Tp: its queries are read
//              clamped to Tp - 1 and never stored (the guard is the sequence's own row count, not the batch's).
struct AttPadded {
    int S;
};
struct AttPacked {
    int Tp;
    const int* row_off;
    const int* items;   // [n][2]: seq, query tile
};
struct AttSeq {
    int seq, q0;
    size_t qk0;     // first element of the sequence's rows in this head's q and k
    size_t v0;      // first element of the sequence's columns in row 0 of this head's V^T
    int vstride;    // elements between V^T rows
    int qlast;      // last readable query row, counted from the sequence's first
    int rows;       // rows of the sequence that may be stored
    size_t ctx0;    // the sequence's first row of ctx
};
__device__ __forceinline__ AttSeq att_seq(const AttPadded& a, const int*, int head, int heads)
{
    const int seq = blockIdx.z, S = a.S;
    const size_t hb = (size_t)seq * heads + head;
    return {seq, (int)blockIdx.x * 128, hb * S * 64, hb * 64 * S, S, S - 1, S, (size_t)seq * S};
}
__device__ __forceinline__ AttSeq att_seq(const AttPacked& a, const int* lens, int head, int)
{
    const int seq = a.items[2 * blockIdx.x], r0 = a.row_off[seq];
    return {seq, a.items[2 * blockIdx.x + 1] * 128, ((size_t)head * a.Tp + r0) * 64, (size_t)head * 64 * a.Tp + r0, a.Tp,
            a.Tp - 1 - r0, (lens[seq] + 63) & ~63, (size_t)r0};
}

template <class Layout>
__global__ __launch_bounds__(256, 2) void attention2_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                                                        const bf16* __restrict__ vt, const int* __restrict__ lens,
                                                        bf16* __restrict__ ctx, Layout lay, int heads, int H)
{
    __shared__ __attribute__((aligned(16))) char lds[2 * 16384];   // [buffer][K tile 8 KiB | V^T tile 8 KiB]
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, hh = lane >> 5;
    const int head = blockIdx.y;
    const AttSeq at = att_seq(lay, lens, head, heads);
    const int seq = at.seq, q0 = at.q0, S = at.vstride;
    const int len = lens[seq];
    if (q0 >= len) return;   // whole query tile is padding (ctx rows stay zero: memset by the caller)
    const bf16* qh = q + at.qk0;
    const bf16* kh = k + at.qk0;
    const bf16* vh = vt + at.v0;
    const int nt = (len + 63) >> 6;

    // staging: 16 wave-instructions per tile (8 rows of 128 B each), 4 per wave: waves 0,1 the K tile, waves 2,3 V^T
    const int srow = lane >> 3, sslot = lane & 7;
    auto issue = [&](int t, int buf) {
        const int kt0 = t * 64;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int inst = (wave & 1) * 4 + u;             // 0..7 inside the operand tile
            const int row = inst * 8 + srow;                 // key (K) or d (V^T)
            const int chunk = sslot ^ ((row >> 1) & 7);
            const bf16* src = wave < 2 ? kh + (size_t)(kt0 + row) * 64 + chunk * 8 : vh + (size_t)row * S + kt0 + chunk * 8;
            char* dst = lds + buf * 16384 + (wave < 2 ? 0 : 8192) + inst * 1024;
            __builtin_amdgcn_global_load_lds((const void*)src, (lds_ptr_t)dst, 16, 0, 0);
        }
    };
    issue(0, 0);

    // Q fragments (B operand of S^T = K Q^T): lane (query r32, half hh) holds Q[query][16 ks + 8 hh .. + 7], ks = 0..3
    bf16x8 qf[4];
    {
        const int qi = min(q0 + wave * 32 + r32, at.qlast);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qh + (size_t)qi * 64 + ks * 16 + hh * 8);
    }
    f32x16 o[2];   // O^T tiles: d = 32 dt + (r & 3) + 8 (r >> 2) + 4 hh, query r32
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float mrow = -INFINITY, lpart = 0.f;       // running max of the query's row; THIS lane's share of the row sum
    const float LOG2E = 1.4426950408889634f;
    const int swz = (r32 >> 1) & 7;            // swizzle of this lane's LDS row (row = r32 in every fragment read)
    // 16 registers of zeros that stay zeros: the first MFMA of every score tile takes them as its C operand (D != C), which
    // saves the 32 v_mov per tile that zeroing two accumulator tiles costs; opaque, or hipcc re-materialises them
    f32x16 zero16;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
    asm volatile("" : "+v"(zero16));

    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1, kt0 = t * 64;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of tile t has landed
        __builtin_amdgcn_s_barrier();                       // ... everyone's has; buffer buf ^ 1 is no longer being read
        if (t + 1 < nt) issue(t + 1, buf ^ 1);
        const char* kb = lds + buf * 16384;
        const char* vb = kb + 8192;
        // S^T tiles: sc[kt][r] = score(key kt0 + 32 kt + (r & 3) + 8 (r >> 2) + 4 hh, query r32)
        f32x16 sc[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kb + (kt * 32 + r32) * 128 + (((2 * ks + hh) ^ swz) << 4));
                sc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], ks == 0 ? zero16 : sc[kt], 0, 0, 0);
            }
        }
        if (kt0 + 64 > len) {   // the one tile that crosses the sequence length: padded keys never win
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kt0 + 32 * kt + (r & 3) + 8 * (r >> 2) + 4 * hh >= len) sc[kt][r] = -INFINITY;
        }
        float tmax = sc[0][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, sc[0][r]);
#pragma unroll
        for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, sc[1][r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));           // the other half of the query's scores
        if (__any(tmax > mrow)) {                            // some row maximum of this wave rose: rescale (exact)
            const float mn = fmaxf(mrow, tmax);              // finite: key 0 of the first tile is always valid
            const float alpha = __builtin_amdgcn_exp2f((mrow - mn) * LOG2E);
            mrow = mn;
            lpart *= alpha;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
        }
        const float mL = mrow * LOG2E;
        // P^T fragments: k-step s of key tile kt takes accumulator registers 8 s .. 8 s + 7
        bf16x8 pf[2][2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[kt][8 * s + j], LOG2E, -mL));
                    lpart += p;
                    pf[kt][s][j] = (bf16)p;
                }
        // O^T += V^T P^T: A fragment of d tile dt, key tile kt, k-step s = V^T[d = 32 dt + r32][keys 32 kt + 16 s + 4 hh + 0..3
        // and 32 kt + 16 s + 8 + 4 hh + 0..3]: two 8-byte runs, 16-B chunk (4 kt + 2 s) resp. (4 kt + 2 s + 1), half hh
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const char* vr = vb + (dt * 32 + r32) * 128 + hh * 8;
                    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vr + (((4 * kt + 2 * s) ^ swz) << 4));
                    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vr + (((4 * kt + 2 * s + 1) ^ swz) << 4));
                    const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[kt][s], o[dt], 0, 0, 0);
                }
    }
    // row sum: the two halves of a query hold disjoint keys
    const float inv = 1.f / (lpart + __shfl_xor(lpart, 32));
    __builtin_amdgcn_s_barrier();    // every wave is done with the K / V^T buffers: they become the output staging area
    char* ob = lds + wave * 4096;    // 32 queries x 128 B, 16-B chunk c of row q at c ^ (q & 7)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            bf16x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (bf16)(o[dt][4 * g4 + r] * inv);
            const int d = 32 * dt + 8 * g4 + 4 * hh;       // 4 consecutive d
            *reinterpret_cast<bf16x4*>(ob + r32 * 128 + (((d >> 3) ^ (r32 & 7)) << 4) + (d & 4) * 2) = v;
        }
    // read back: 8 lanes per query row (16 B each), 8 rows per pass, 4 passes
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int row = p * 8 + (lane >> 3), c = lane & 7;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(ob + row * 128 + ((c ^ (row & 7)) << 4));
        const int qi = q0 + wave * 32 + row;
        if (qi < at.rows) *reinterpret_cast<bf16x8*>(ctx + (at.ctx0 + qi) * H + head * 64 + c * 8) = v;
    }
}

// ---- the launchers --------------------------------------------------------------------------------------------------------
// The two places attention2_kernel is launched from, one per layout.  ctx must be zero-filled by the caller (skipped tiles).
static void launch_attention(const bf16* q, const bf16* k, const bf16* vt, const int* lens, bf16* ctx, int nseq, int S, int heads,
                             hipStream_t st)
{
    hipLaunchKernelGGL(attention2_kernel<AttPadded>, dim3((S + 127) / 128, heads, nseq), dim3(256), 0, st, q, k, vt, lens, ctx,
                       AttPadded{S}, heads, heads * 64);
}

// Packed: row_off [nseq + 1], lens [nseq] and the work list items [n_items][2] (packed_layout's) on the device.
static void launch_attention_packed(const bf16* q, const bf16* k, const bf16* vt, const int* row_off, const int* lens,
                                    const int* items, int n_items, int Tp, int heads, bf16* ctx, hipStream_t st)
{
    if (n_items == 0) return;
    hipLaunchKernelGGL(attention2_kernel<AttPacked>, dim3(n_items, heads, 1), dim3(256), 0, st, q, k, vt, lens, ctx,
                       AttPacked{Tp, row_off, items}, heads, heads * 64);
}

// fp32 rows -> bf16 (PARTS = false), or `nsplit` fp32 partials + bias + bf16 residual -> bf16 (PARTS = true)
template <bool PARTS>
static void launch_layernorm(const float* x, const float* gamma, const float* beta, bf16* y, int M, int H, float eps, int nsplit,
                             const float* bias, const bf16* resid, hipStream_t st)
{
    hipLaunchKernelGGL(layernorm_kernel<PARTS>, dim3((M + 3) / 4), dim3(256), 0, st, x, gamma, beta, y, M, H, eps, nsplit, bias,
                       resid);
}

static void launch_layernorm16(const bf16* x, const float* gamma, const float* beta, bf16* y, int M, int H, float eps, hipStream_t st)
{
    hipLaunchKernelGGL(layernorm16_kernel, dim3((M + 4 * kLn16Rows - 1) / (4 * kLn16Rows)), dim3(256), 0, st, x, gamma, beta, y, M,
                       H, eps);
}
