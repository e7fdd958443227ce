// encoder_heads.h -- what the encoder makes of the last hidden state: the pooled embedding (pool_kernel), the classification
// logit (rerank_head_kernel), BGE-M3's lexical weights (lexical_kernel) and its multi-vectors (colbert_norm_kernel behind a
// raw-partials GEMM of encoder_gemm.h).  Included by encoder.hip alone, inside hiprag's anonymous namespace, after
// encoder_gemm.h and encoder_layers.h (wave_sum).
#pragma once

// K10a: CLS row (token 0 of each sequence) -> L2 normalise -> fp32 [nseq, H]; zero for empty sequences.
// row_off != null: a packed batch (encoder_packed.h), the CLS row of sequence i is row row_off[i] and S is not read.  An empty
// sequence has no row there: its zeros are written without reading x.
__global__ __launch_bounds__(64) void pool_kernel(const bf16* __restrict__ x, const int* __restrict__ lens, int S, int H,
                                                 float* __restrict__ out, int normalize, const int* __restrict__ row_off)
{
    const int seq = blockIdx.x, lane = threadIdx.x;
    if (row_off && lens[seq] <= 0) {
        for (int c = lane; c < H; c += 64) out[(size_t)seq * H + c] = 0.f;
        return;
    }
    const bf16* xr = x + (row_off ? (size_t)row_off[seq] : (size_t)seq * S) * H;
    float ss = 0.f;
    for (int c = lane; c < H; c += 64) { const float v = (float)xr[c]; ss += v * v; }
    ss = wave_sum(ss);
    const float inv = (lens[seq] > 0) ? (normalize ? 1.f / fmaxf(sqrtf(ss), 1e-12f) : 1.f) : 0.f;
    for (int c = lane; c < H; c += 64) out[(size_t)seq * H + c] = (float)xr[c] * inv;
}

// K10b: XLM-R classification head on the CLS row: logit = w_out . tanh(W_dense cls + b_dense) + b_out.
__global__ __launch_bounds__(256) void rerank_head_kernel(const bf16* __restrict__ x, int S, int H,
                                                         const bf16* __restrict__ wd, const float* __restrict__ bd,
                                                         const bf16* __restrict__ wo, const float* __restrict__ bo,
                                                         float* __restrict__ logits, const int* __restrict__ row_off)
{
    __shared__ float cls[2048];
    __shared__ float part[4];
    const int seq = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bf16* xr = x + (row_off ? (size_t)row_off[seq] : (size_t)seq * S) * H;   // packed: no sequence is empty (checked)
    for (int c = tid; c < H; c += 256) cls[c] = (float)xr[c];
    __syncthreads();
    float acc = 0.f;
    for (int n = wave; n < H; n += 4) {  // one wave per output feature
        const bf16* w = wd + (size_t)n * H;
        float s = 0.f;
        for (int c = lane; c < H; c += 64) s += (float)w[c] * cls[c];
        s = wave_sum(s);
        if (lane == 0) acc += (float)wo[n] * tanhf(s + bd[n]);
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (tid == 0) logits[seq] = part[0] + part[1] + part[2] + part[3] + bo[0];
}

// K10c: BGE-M3's lexical head (hipenc_forward_lexical): w_t = relu(sparse_linear(hidden_t)) per token, then per sequence
// the distinct token ids with their largest weight, ascending by id.  One 256-thread workgroup per sequence; ids and
// weights stay in LDS.
//   weights   wave v takes positions v, v + 4, ..: lane l sums the products x[c] * w[c] over c = l, l + 64, .. in ascending
//             c (fp32; a product of two bf16 values is exact in fp32, so a fused multiply-add gives the same bits), the 64
//             partial sums go through wave_sum's butterfly (offsets 32, 16, .., 1: every lane ends with the same bits),
//             then + bias, then max(0, .).  hiprag.lexical.lexical_reference restates exactly this.
//   dedupe    position t REPRESENTS its id if no earlier position holds the same id; its weight is the maximum over the
//             positions of that id.  It is kept if the id is not an unused one and the maximum is > 0.  A kept position's
//             place in the row is the number of kept positions with a smaller id.  Two passes of L x L comparisons over
//             LDS (L <= 2048): no sort, no atomics on floats, the same bits from run to run.
constexpr int kLexMaxLen = 2048;
constexpr int kLexMaxUnused = 16;
struct LexUnused {
    int n;
    int ids[kLexMaxUnused];
};

__global__ __launch_bounds__(256) void lexical_kernel(const bf16* __restrict__ x, const int* __restrict__ tok, const int* __restrict__ lens,
                                                      int S, int H, int max_len, const bf16* __restrict__ lw, const float* __restrict__ lb,
                                                      LexUnused unused, int* __restrict__ out_terms, float* __restrict__ out_weights,
                                                      int* __restrict__ out_counts)
{
    __shared__ int ids[kLexMaxLen];
    __shared__ float wt[kLexMaxLen];     // weight of every position
    __shared__ float kept[kLexMaxLen];   // > 0: the position represents a kept id, the value is the id's weight
    __shared__ int count;
    const int seq = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = min(lens[seq], max_len);
    if (tid == 0) count = 0;
    const float bias = lb[0];
    for (int t = wave; t < len; t += 4) {
        const bf16* xr = x + ((size_t)seq * S + t) * H;
        float s = 0.f;
        for (int c = lane; c < H; c += 64) s += (float)xr[c] * (float)lw[c];
        s = wave_sum(s);
        if (lane == 0) {
            wt[t] = fmaxf(0.f, s + bias);
            ids[t] = tok[(size_t)seq * S + t];
        }
    }
    __syncthreads();
    int mine = 0;
    for (int t = tid; t < len; t += 256) {
        const int id = ids[t];
        float m = wt[t];
        bool first = true;
        for (int u = 0; u < len; ++u) {
            if (ids[u] == id) {
                m = fmaxf(m, wt[u]);
                first = first && u >= t;
            }
        }
        bool used = true;
        for (int j = 0; j < unused.n; ++j) used = used && unused.ids[j] != id;
        const bool keep = first && used && m > 0.f;
        kept[t] = keep ? m : 0.f;
        mine += keep;
    }
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    const int n = count;
    for (int t = tid; t < len; t += 256) {
        const float m = kept[t];
        if (!(m > 0.f)) continue;
        const int id = ids[t];
        int rank = 0;
        for (int u = 0; u < len; ++u) rank += (kept[u] > 0.f && ids[u] < id) ? 1 : 0;
        out_terms[(size_t)seq * max_len + rank] = id;
        out_weights[(size_t)seq * max_len + rank] = m;
    }
    for (int i = n + tid; i < max_len; i += 256) {
        out_terms[(size_t)seq * max_len + i] = -1;
        out_weights[(size_t)seq * max_len + i] = 0.f;
    }
    if (tid == 0) out_counts[seq] = n;
}

// where hipenc_forward_lexical's sparse outputs go (all device memory)
struct LexOut {
    int* terms;
    float* weights;
    int* counts;
    int max_len;
};

// K10d: BGE-M3's multi-vector (ColBERT) head (hipenc_forward_colbert): y_t = normalise(colbert_linear(hidden_t)) for every
// position but CLS.  The product is the raw-partials form of the GEMMs above (no epilogue is added to the hot kernels); this
// kernel is what follows it, one wave per token row:
//   v[n]  = (partial 0 + partial 1 + .. in split order) + b[n]
//   ss    = sum of v[n]^2: lane l adds columns l, l + 64, .. in ascending order (the square and the add are rounded
//           separately: no contraction), then wave_sum's butterfly -- pool_kernel's order
//   y[n]  = bf16(v[n] * (1.f / fmaxf(sqrtf(ss), 1e-12f)))
// Row s >= 1 of sequence i goes to row s - 1 of the sequence's output block if s - 1 < count = max(0, len - 1); the rows at
// and behind count are written as zeros; the wave of row 0 (CLS) writes the count.  hiprag.colbert.colbert_reference
// restates exactly this.
__global__ __launch_bounds__(256) void colbert_norm_kernel(const float* __restrict__ parts, int nsplit, int T,
                                                           const float* __restrict__ bias, const int* __restrict__ lens, int S, int H,
                                                           bf16* __restrict__ out_vecs, int row_stride, int* __restrict__ out_counts)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const int seq = row / S, s = row - seq * S;
    const int count = min(max(lens[seq] - 1, 0), row_stride);
    if (s == 0) {
        if (lane == 0) out_counts[seq] = count;
        return;
    }
    const int p = s - 1;
    if (p >= row_stride) return;
    bf16* dst = out_vecs + ((size_t)seq * row_stride + p) * H;
    if (p >= count) {
        for (int c = lane; c < H; c += 64) dst[c] = (bf16)0.f;
        return;
    }
    float v[32];   // H <= 2048
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const int c = i * 64 + lane;
        if (c < H) {
            float a = parts[(size_t)row * H + c];
            for (int sp = 1; sp < nsplit; ++sp) a = a + parts[((size_t)sp * T + row) * H + c];
            a = a + bias[c];
            v[i] = a;
            const float sq = a * a;
            ss = ss + sq;
        }
    }
    ss = wave_sum(ss);
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const int c = i * 64 + lane;
        if (c < H) dst[c] = (bf16)(v[i] * inv);
    }
}

// where hipenc_forward_colbert's vectors go (device memory)
struct ColOut {
    bf16* vecs;
    int* counts;
    int row_stride;
};

// The ColBERT head over T token rows X (Mpad rows readable): raw partials into `pre` ([splits][T][H] floats), then the kernel
// above.  small: the small-batch GEMM (T a multiple of 64; it makes skinny_split(H) partials); otherwise 128 x 128 tiles with
// K split `ksplit` ways.  Encoder's forward and the hipenc_colbert_rows hook both come through here.
static void launch_colbert_head(const bf16* X, int T, int Mpad, int H, bool small, int ksplit, const bf16* w, const float* b,
                                float* pre, const int* lens_dev, int S, const ColOut& out, hipStream_t st)
{
    GemmArgs g{};
    g.A = X; g.W = w; g.bias = b; g.M = T; g.N = H; g.K = H; g.out_f32 = pre;
    int nsplit;
    if (small) {
        launch_skinny<EPI_PART>(g, st);
        nsplit = skinny_split(H);
    } else {
        g.ksplit = ksplit;
        launch_tiled<EPI_PART>(g, Mpad, st);
        nsplit = ksplit;
    }
    hipLaunchKernelGGL(colbert_norm_kernel, dim3((T + 3) / 4), dim3(256), 0, st, (const float*)pre, nsplit, T, b, lens_dev, S, H,
                       out.vecs, out.row_stride, out.counts);
}
