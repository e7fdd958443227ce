// encoder.hip -- XLM-RoBERTa-large-shaped batch encoder (BGE-M3 / bge-reranker-v2-m3 architecture) on MFMA: the host side.
//
// Replaces the transformer forward the reference reaches through
//   rag/providers/hf/embeddings.py:54,77  (LangChain HuggingFaceEmbeddings -> sentence-transformers encode:
//   CLS pooling + L2 normalisation, normalize_embeddings=True at :34)
// and supplies the cross-encoder scoring the reference only configures (rag/config.py:25-27).
//
// Architecture (post-LN BERT family): embeddings (word + learned position + type) -> LayerNorm -> L x [ QKV projection,
// 16-head scaled-dot-product attention with key padding mask, output projection + residual + LayerNorm,
// FFN (H->F, exact-erf GELU, F->H) + residual + LayerNorm ] -> CLS row -> L2 normalise (embedding) or
// dense+tanh+out_proj (reranker logit).  Weights stay in torch-owned HBM tensors; this file only receives pointers.
//
// The pieces, all compiled into this ONE translation unit (the kernel headers are included by no other file):
//   encoder_plan.h    the policy: which GEMM family a batch takes, the K splits, the workspace size (host-only)
//   encoder_packed.h  the layout of a packed batch: row offsets, granule owners, the attention work list (host-only)
//   encoder_gemm.h    K6/K8/K9 the three GEMM families (128-tile, 256-tile through gemm256.h, small-batch) and their launchers
//   encoder_layers.h  K5 embedding, the LayerNorms, K7 attention and their launchers
//   encoder_heads.h   K10 pool, classification, lexical and ColBERT heads
//   here              Encoder (the forward), EncoderLease (encoder_internal.h, for rerank.hip), the C ABI and the test hooks
// Bound: MFMA (bf16 dense peak ~2.5 PFLOP/s); flops/token ~ L*(8H^2 + 4HF) + attention.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "common.h"
#include "encoder_internal.h"
#include "encoder_packed.h"
#include "encoder_plan.h"

namespace hiprag {
namespace {

#include "encoder_gemm.h"
#include "encoder_layers.h"
#include "encoder_heads.h"

// What a forward leaves in its output
enum class EncOut : int {
    embedding = 0,   // L2-normalised CLS rows, f32 [nseq, H] (hipenc_forward)
    logits = 1,      // classification-head logits, f32 [nseq] (hipenc_score_pairs, EncoderLease::score_dev)
    cls = 2,         // the CLS rows as they are, f32 [nseq, H]
    hidden = 3,      // test hook (hipenc_forward_hidden): the final x rows as the kernels left them, bf16 [nseq, S, H]
    lexical = 4,     // the embedding unless out is null, and the lexical rows into HeadDest::lex (hipenc_forward_lexical)
    colbert = 5,     // the embedding unless out is null, and the per-token vectors into HeadDest::col (hipenc_forward_colbert)
    m3 = 6,          // the embedding unless out is null, and BOTH per-token heads over the same rows (hipenc_forward_m3)
};

// where the per-token heads write: `lex` is read in EncOut::lexical and EncOut::m3, `col` in EncOut::colbert and EncOut::m3
struct HeadDest {
    LexOut lex{};
    ColOut col{};
};

// ---------------------------------------------------------------------------------------------------------
struct Encoder {
    std::mutex mu;
    int device = 0;
    hipenc_config cfg{};
    hipenc_weights w{};
    std::vector<hipenc_layer_weights> layers;
    DevBuf tokens, lens, x, q, k, vt, ctx, pre, ffn, pooled;
    DevBuf ptab;                     // a packed batch's tables: lens | row_off | gran_seq | items
    int64_t packed_last[4] = {0, 0, 0, -1};   // hipenc_packed_info: Tp, real tokens, sequences, path of the last packed forward
    const void* lex_w = nullptr;     // lexical head (hipenc_set_lexical_head): bf16 [H], caller's device memory
    const float* lex_b = nullptr;    // f32 [1]
    LexUnused lex_unused{};          // token ids that never get a lexical weight (copied)
    const void* col_w = nullptr;     // ColBERT head (hipenc_set_colbert_head): bf16 [H][H], caller's device memory
    const float* col_b = nullptr;    // f32 [H]
    double flops_last = 0.0;
    int small_rows = kSmallRowsDefault;   // HIPENC_SMALL_ROWS
    int n_cu = 256;
    int use256 = 1;          // HIPENC_GEMM256=0 keeps every batch on the 128 x 128 kernel (A/B runs)

    EncShape shape() const { return {cfg.hidden, cfg.ffn, n_cu, small_rows, use256}; }
    EncPlan plan(int nseq, int S) const { return plan_forward(shape(), nseq, S); }

    // The staging part: validates the host batch, pads it to S into `tokens` / `lens` and runs the forward over them.
    int32_t forward(const int32_t* tok_host, const int32_t* lens_host, int nseq, int max_len, void* out_dev, EncOut mode,
                    hipStream_t st, const HeadDest& heads = {})
    {
        const int S = round_up(max_len, kSkinnyRows);
        const EncPlan pl = plan(nseq, S);
        int32_t rc;
        if ((rc = tokens.reserve((size_t)nseq * S * 4))) return rc;
        if ((rc = lens.reserve((size_t)nseq * 4))) return rc;
        if ((rc = reserve_work(pl))) return rc;
        // host staging: pad token rows to S with pad_id
        std::vector<int32_t> tp((size_t)nseq * S, cfg.pad_id);
        for (int s = 0; s < nseq; ++s) {
            if (lens_host[s] < 0 || lens_host[s] > max_len) { set_error("seq_lens[%d]=%d outside [0,%d]", s, lens_host[s], max_len); return HIPRAG_E_INVALID; }
            for (int t = 0; t < lens_host[s]; ++t) {
                const int32_t id = tok_host[(size_t)s * max_len + t];
                if (id < 0 || id >= cfg.vocab) { set_error("token id %d outside the vocabulary", id); return HIPRAG_E_INVALID; }
                tp[(size_t)s * S + t] = id;
            }
        }
        HR_CHECK_HIP(hipMemcpyAsync(tokens.p, tp.data(), tp.size() * 4, hipMemcpyHostToDevice, st));
        HR_CHECK_HIP(hipMemcpyAsync(lens.p, lens_host, (size_t)nseq * 4, hipMemcpyHostToDevice, st));
        HR_CHECK_HIP(hipStreamSynchronize(st));  // tp is a local vector
        return run_forward(pl, tokens.as<int>(), lens.as<int>(), nseq, S, out_dev, mode, st, heads);
    }

    // The part that starts at embed_ln_kernel: nseq rows of S tokens (S a multiple of 64, pad_id behind each length) and their
    // lengths, ALREADY ON THE DEVICE and ordered on `st`.  Nothing is staged and the host waits for nothing.  The ids index the
    // embedding table unchecked: whoever wrote them has range-checked them (forward above; csrc/rerank.hip, whose ids passed
    // hiptok_append's check or its own).  That is why no C-ABI entry takes device tokens.
    int32_t forward_dev(const int* tok_dev, const int* lens_dev, int nseq, int S, void* out_dev, EncOut mode, hipStream_t st,
                        const HeadDest& heads = {})
    {
        return run_forward(plan(nseq, S), tok_dev, lens_dev, nseq, S, out_dev, mode, st, heads);
    }

    int32_t reserve_work(const EncPlan& p)
    {
        const size_t act = (size_t)p.M * cfg.hidden * 2;
        int32_t rc;
        if ((rc = x.reserve(act))) return rc;
        if ((rc = q.reserve(act))) return rc;
        if ((rc = k.reserve(act))) return rc;
        if ((rc = vt.reserve(act))) return rc;
        if ((rc = ctx.reserve(act))) return rc;
        if ((rc = pre.reserve(p.pre_bytes))) return rc;
        return ffn.reserve((size_t)p.M * cfg.ffn * 2);
    }

    // One GEMM of the stack on the plan's family.  a.M is the rows the epilogue may write; the small-batch kernel has no
    // padding rows (every row block is a real one).  For the epilogues all three families have: QKV and GELU.
    template <int EPI>
    void gemm(const EncPlan& p, GemmArgs a, hipStream_t st) const
    {
        switch (p.path) {
        case EncPath::small: a.M = p.T; launch_skinny<EPI>(a, st); break;
        case EncPath::big: launch256_grid<EPI>(a, p.M, n_cu, 0, st); break;
        case EncPath::tiled: launch_tiled<EPI>(a, p.M, st); break;
        }
    }

    // x = LayerNorm(A W^T + bias + x): an N = H product over K and the LayerNorm that follows it, in the form the plan's
    // family has -- small: fp32 partials (as many as launch_skinny makes of this K), summed with bias and residual by the
    // LayerNorm; big: bf16 pre-LayerNorm rows (half the store and LayerNorm-read bytes); tiled: partials if K is split
    // `split` > 1 ways, else the residual epilogue and a plain LayerNorm.
    void project_ln(const EncPlan& p, const bf16* A, const void* W, const void* bias, int K, int split, const void* ln_g,
                    const void* ln_b, hipStream_t st)
    {
        const int H = cfg.hidden;
        const bf16* X = x.as<bf16>();
        const float *b = (const float*)bias, *gamma = (const float*)ln_g, *beta = (const float*)ln_b;
        GemmArgs o{};
        o.A = A; o.W = (const bf16*)W; o.bias = b; o.M = p.M; o.N = H; o.K = K;
        o.resid = X; o.out_f32 = pre.as<float>();
        if (p.path == EncPath::small) {
            o.M = p.T;
            launch_skinny<EPI_PART>(o, st);
            launch_layernorm<true>(pre.as<float>(), gamma, beta, x.as<bf16>(), p.T, H, cfg.ln_eps, skinny_split(K), b, X, st);
        } else if (p.path == EncPath::big) {
            o.out_bf16 = pre.as<bf16>();
            launch256_grid<EPI_RESID16>(o, p.M, n_cu, 0, st);
            launch_layernorm16(pre.as<bf16>(), gamma, beta, x.as<bf16>(), p.M, H, cfg.ln_eps, st);
        } else if (split > 1) {
            o.ksplit = split;
            launch_tiled<EPI_PART>(o, p.M, st);
            launch_layernorm<true>(pre.as<float>(), gamma, beta, x.as<bf16>(), p.M, H, cfg.ln_eps, split, b, X, st);
        } else {
            launch_tiled<EPI_RESID>(o, p.M, st);
            launch_layernorm<false>(pre.as<float>(), gamma, beta, x.as<bf16>(), p.M, H, cfg.ln_eps, 1, nullptr, nullptr, st);
        }
    }

    void launch_pool(const int* lens_dev, int nseq, int S, float* out, bool normalize, hipStream_t st, const int* row_off = nullptr)
    {
        hipLaunchKernelGGL(pool_kernel, dim3(nseq), dim3(64), 0, st, x.as<bf16>(), lens_dev, S, cfg.hidden, out, normalize ? 1 : 0,
                           row_off);
    }

    // The layers of both layouts, from the embedded rows in x to the last hidden state in x.  S: what the QKV epilogue takes
    // for the sequence length (packed: Tp, ONE sequence of Tp rows); attention(): the layout's launch, q / k / vt -> ctx.
    template <class Attention>
    void run_layers(const EncPlan& pl, int S, hipStream_t st, Attention attention)
    {
        const int H = cfg.hidden, F = cfg.ffn, T = pl.T, M = pl.M;
        const bf16* X = x.as<bf16>();
        for (int l = 0; l < cfg.layers; ++l) {
            const hipenc_layer_weights& L = layers[l];
            GemmArgs g{};
            g.A = X; g.W = (const bf16*)L.wqkv; g.bias = (const float*)L.bqkv; g.N = 3 * H; g.K = H;
            g.q = q.as<bf16>(); g.k = k.as<bf16>(); g.vt = vt.as<bf16>(); g.S = S; g.heads = cfg.heads; g.H = H;
            g.M = T;   // rows >= T exist only as GEMM padding; the QKV scatter must not write them
            gemm<EPI_QKV>(pl, g, st);
            attention();
            project_ln(pl, ctx.as<bf16>(), L.wo, L.bo, H, pl.osplit, L.ln1_g, L.ln1_b, st);
            GemmArgs f1{};
            f1.A = X; f1.W = (const bf16*)L.w1; f1.bias = (const float*)L.b1; f1.M = M; f1.N = F; f1.K = H;
            f1.out_bf16 = ffn.as<bf16>();
            gemm<EPI_GELU>(pl, f1, st);
            project_ln(pl, ffn.as<bf16>(), L.w2, L.b2, F, pl.dsplit, L.ln2_g, L.ln2_b, st);
        }
    }

    int32_t run_forward(const EncPlan& pl, const int* tok_dev, const int* lens_dev, int nseq, int S, void* out_dev, EncOut mode,
                        hipStream_t st, const HeadDest& heads)
    {
        const int H = cfg.hidden, F = cfg.ffn, T = pl.T, M = pl.M;
        if (mode == EncOut::logits && (!w.cls_dense_w || !w.cls_out_w)) { set_error("encoder was created without a classification head"); return HIPRAG_E_INVALID; }
        int32_t rc;
        if ((rc = reserve_work(pl))) return rc;
        HR_CHECK_HIP(hipMemsetAsync(ctx.p, 0, (size_t)M * H * 2, st));  // rows of skipped (all-padding) query tiles

        const bf16* X = x.as<bf16>();
        hipLaunchKernelGGL(embed_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, st, tok_dev, lens_dev, S, nseq,
                           (const bf16*)w.word_emb, (const bf16*)w.pos_emb, (const bf16*)w.type_emb, (const float*)w.emb_ln_g,
                           (const float*)w.emb_ln_b, x.as<bf16>(), H, cfg.pad_id, cfg.ln_eps, M);
        run_layers(pl, S, st, [&] {
            launch_attention(q.as<bf16>(), k.as<bf16>(), vt.as<bf16>(), lens_dev, ctx.as<bf16>(), nseq, S, cfg.heads, st);
        });
        switch (mode) {
        case EncOut::hidden:
            HR_CHECK_HIP(hipMemcpyAsync(out_dev, x.p, (size_t)T * H * 2, hipMemcpyDeviceToDevice, st));
            break;
        case EncOut::embedding:
        case EncOut::cls:
            launch_pool(lens_dev, nseq, S, (float*)out_dev, mode == EncOut::embedding, st);
            break;
        case EncOut::lexical:
            if (out_dev) launch_pool(lens_dev, nseq, S, (float*)out_dev, true, st);
            hipLaunchKernelGGL(lexical_kernel, dim3(nseq), dim3(256), 0, st, X, tok_dev, lens_dev, S, H, heads.lex.max_len,
                               (const bf16*)lex_w, lex_b, lex_unused, heads.lex.terms, heads.lex.weights, heads.lex.counts);
            break;
        case EncOut::colbert:
            if (out_dev) launch_pool(lens_dev, nseq, S, (float*)out_dev, true, st);
            // the head's partials fit the buffer the stack's N = H products use (EncPlan::head_split)
            launch_colbert_head(X, T, M, H, pl.path == EncPath::small, pl.head_split, (const bf16*)col_w, col_b, pre.as<float>(),
                                lens_dev, S, heads.col, st);
            break;
        case EncOut::m3:
            // The three heads one after the other on `st`, each the launch of its own mode.  All of them READ x (and tokens /
            // lens) and none writes it: the pool writes out_dev, lexical_kernel its three outputs (ids and weights stay in
            // LDS), the ColBERT product its raw partials into `pre` -- which no other head touches -- and colbert_norm_kernel
            // the vectors and counts.  So every output is what the single-head forward writes.
            if (out_dev) launch_pool(lens_dev, nseq, S, (float*)out_dev, true, st);
            hipLaunchKernelGGL(lexical_kernel, dim3(nseq), dim3(256), 0, st, X, tok_dev, lens_dev, S, H, heads.lex.max_len,
                               (const bf16*)lex_w, lex_b, lex_unused, heads.lex.terms, heads.lex.weights, heads.lex.counts);
            launch_colbert_head(X, T, M, H, pl.path == EncPath::small, pl.head_split, (const bf16*)col_w, col_b, pre.as<float>(),
                                lens_dev, S, heads.col, st);
            break;
        case EncOut::logits:
            hipLaunchKernelGGL(rerank_head_kernel, dim3(nseq), dim3(256), 0, st, X, S, H, (const bf16*)w.cls_dense_w,
                               (const float*)w.cls_dense_b, (const bf16*)w.cls_out_w, (const float*)w.cls_out_b, (float*)out_dev, (const int*)nullptr);
            break;
        }
        HR_CHECK_HIP(hipGetLastError());
        double tok = (double)T;
        flops_last = tok * cfg.layers * (8.0 * H * H + 4.0 * H * F) + (double)nseq * cfg.layers * 4.0 * S * (double)S * H;
        return HIPRAG_OK;
    }

    // ---- packed batches (encoder_packed.h): no row of the GEMMs belongs to a sequence's padding up to the batch's longest ----
    // The plan is that of ONE sequence of Tp rows: the GEMM family depends on the row count alone.
    EncPlan plan_packed(int Tp) const { return plan_forward(shape(), 1, Tp); }

    // The staging part: validates the host batch (tokens one sequence after another, offsets [nseq + 1]), lays it out, copies
    // the padded token rows and the tables (two copies, one synchronise, as forward) and runs the packed forward.
    // EncOut::hidden writes the REAL rows only, in order: bf16 [offsets[nseq]][H].
    int32_t forward_packed(const int32_t* tok_host, const int32_t* off_host, int nseq, void* out_dev, EncOut mode, hipStream_t st)
    {
        const int H = cfg.hidden;
        HR_REQUIRE(off_host[0] == 0, "offsets must start at 0 (got %d)", off_host[0]);
        std::vector<int32_t> lens_h((size_t)nseq);
        for (int s = 0; s < nseq; ++s) {
            const int64_t d = (int64_t)off_host[s + 1] - off_host[s];
            HR_REQUIRE(d >= 0, "offsets descend at sequence %d", s);
            HR_REQUIRE(d >= 1 || mode != EncOut::logits, "sequence %d is empty: a pair has at least one token", s);
            HR_REQUIRE(d + cfg.pad_id + 1 < cfg.max_pos, "sequence %d of %lld tokens exceeds the position table", s, (long long)d);
            lens_h[s] = (int32_t)d;
        }
        for (int t = 0; t < off_host[nseq]; ++t)
            HR_REQUIRE(tok_host[t] >= 0 && tok_host[t] < cfg.vocab, "token id %d outside the vocabulary", tok_host[t]);
        PackedLayout lay;
        HR_REQUIRE(packed_layout(lens_h.data(), nseq, lay), "the packed batch has 2^30 rows or more");
        if (lay.Tp == 0) {   // every sequence is empty: zeros, and no GEMM
            if (mode == EncOut::embedding || mode == EncOut::cls) HR_CHECK_HIP(hipMemsetAsync(out_dev, 0, (size_t)nseq * H * 4, st));
            flops_last = 0.0;
            packed_last[0] = 0; packed_last[1] = 0; packed_last[2] = nseq; packed_last[3] = -1;
            return HIPRAG_OK;
        }
        const EncPlan pl = plan_packed(lay.Tp);
        const size_t n_gran = lay.gran_seq.size(), n_tab = (size_t)nseq + ((size_t)nseq + 1) + n_gran + lay.items.size();
        int32_t rc;
        if ((rc = tokens.reserve((size_t)lay.Tp * 4))) return rc;
        if ((rc = ptab.reserve(n_tab * 4))) return rc;
        if ((rc = reserve_work(pl))) return rc;
        std::vector<int32_t> tp((size_t)lay.Tp, cfg.pad_id), tab;
        for (int s = 0; s < nseq; ++s) std::copy(tok_host + off_host[s], tok_host + off_host[s + 1], tp.begin() + lay.row_off[s]);
        tab.reserve(n_tab);
        tab.insert(tab.end(), lens_h.begin(), lens_h.end());
        tab.insert(tab.end(), lay.row_off.begin(), lay.row_off.end());
        tab.insert(tab.end(), lay.gran_seq.begin(), lay.gran_seq.end());
        tab.insert(tab.end(), lay.items.begin(), lay.items.end());
        HR_CHECK_HIP(hipMemcpyAsync(tokens.p, tp.data(), tp.size() * 4, hipMemcpyHostToDevice, st));
        HR_CHECK_HIP(hipMemcpyAsync(ptab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
        HR_CHECK_HIP(hipStreamSynchronize(st));  // tp and tab are local vectors
        PackedBatch b{};
        b.tok = tokens.as<int32_t>();
        b.lens = ptab.as<int32_t>();
        b.row_off = b.lens + nseq;
        b.gran_seq = b.row_off + nseq + 1;
        b.items = b.gran_seq + n_gran;
        b.nseq = nseq; b.Tp = lay.Tp; b.n_items = lay.n_items(); b.real = lay.real; b.sum_r2 = lay.sum_r2;
        if ((rc = run_forward_packed(pl, b, out_dev, mode, st))) return rc;
        if (mode == EncOut::hidden)
            for (int s = 0; s < nseq; ++s)
                if (lens_h[s])
                    HR_CHECK_HIP(hipMemcpyAsync((char*)out_dev + (size_t)off_host[s] * H * 2, x.as<char>() + (size_t)lay.row_off[s] * H * 2,
                                                (size_t)lens_h[s] * H * 2, hipMemcpyDeviceToDevice, st));
        return HIPRAG_OK;
    }

    // The part that starts at embed_ln_packed_kernel: a packed batch ALREADY ON THE DEVICE and ordered on `st`, Tp > 0.  As in
    // forward_dev the ids index the embedding table unchecked.  EncOut::hidden leaves the rows in x for the caller to copy.
    int32_t run_forward_packed(const EncPlan& pl, const PackedBatch& b, void* out_dev, EncOut mode, hipStream_t st)
    {
        const int H = cfg.hidden, F = cfg.ffn, M = pl.M;
        if (mode == EncOut::logits && (!w.cls_dense_w || !w.cls_out_w)) { set_error("encoder was created without a classification head"); return HIPRAG_E_INVALID; }
        if (mode == EncOut::lexical || mode == EncOut::colbert || mode == EncOut::m3) { set_error("the lexical and ColBERT heads take padded batches only"); return HIPRAG_E_UNSUPPORTED; }
        int32_t rc;
        if ((rc = reserve_work(pl))) return rc;
        HR_CHECK_HIP(hipMemsetAsync(ctx.p, 0, (size_t)M * H * 2, st));  // padding rows inside a sequence's last 128-query tile
        hipLaunchKernelGGL(embed_ln_packed_kernel, dim3((M + 3) / 4), dim3(256), 0, st, b.tok, b.lens, b.row_off, b.gran_seq, b.Tp,
                           (const bf16*)w.word_emb, (const bf16*)w.pos_emb, (const bf16*)w.type_emb, (const float*)w.emb_ln_g,
                           (const float*)w.emb_ln_b, x.as<bf16>(), H, cfg.pad_id, cfg.ln_eps, M);
        run_layers(pl, b.Tp, st, [&] {
            launch_attention_packed(q.as<bf16>(), k.as<bf16>(), vt.as<bf16>(), b.row_off, b.lens, b.items, b.n_items, b.Tp, cfg.heads,
                                    ctx.as<bf16>(), st);
        });
        if (mode == EncOut::embedding || mode == EncOut::cls)
            launch_pool(b.lens, b.nseq, 0, (float*)out_dev, mode == EncOut::embedding, st, b.row_off);
        else if (mode == EncOut::logits)
            hipLaunchKernelGGL(rerank_head_kernel, dim3(b.nseq), dim3(256), 0, st, x.as<bf16>(), 0, H, (const bf16*)w.cls_dense_w,
                               (const float*)w.cls_dense_b, (const bf16*)w.cls_out_w, (const float*)w.cls_out_b, (float*)out_dev, b.row_off);
        HR_CHECK_HIP(hipGetLastError());
        // the GEMM term counts the real rows, the attention term every sequence's own granule-rounded square
        flops_last = (double)b.real * cfg.layers * (8.0 * H * H + 4.0 * H * F) + (double)cfg.layers * 4.0 * b.sum_r2 * H;
        packed_last[0] = b.Tp; packed_last[1] = b.real; packed_last[2] = b.nseq; packed_last[3] = (int64_t)pl.path;
        return HIPRAG_OK;
    }
};

Registry<Encoder>& reg()
{
    static Registry<Encoder> r;
    return r;
}

}  // namespace

size_t clear_encoder_registry() { return reg().clear(); }

// ---- encoder_internal.h: the device-token forward for csrc/rerank.hip ---------------------------------------------------
int32_t EncoderLease::acquire(uint64_t h)
{
    auto e = reg().get(h);
    if (!e) { set_error("unknown encoder handle"); return HIPRAG_E_HANDLE; }
    lock_ = std::unique_lock<std::mutex>(e->mu);
    view_.device = e->device;
    view_.vocab = e->cfg.vocab;
    view_.pad_id = e->cfg.pad_id;
    view_.max_pos = e->cfg.max_pos;
    view_.has_head = e->w.cls_dense_w && e->w.cls_out_w;
    enc_ = e;
    HR_CHECK_HIP(hipSetDevice(e->device));
    return HIPRAG_OK;
}

int32_t EncoderLease::reserve_tokens(size_t pairs, int S, int32_t** tok_dev, int32_t** lens_dev)
{
    Encoder* e = static_cast<Encoder*>(enc_.get());
    int32_t rc;
    if ((rc = e->tokens.reserve(pairs * (size_t)S * 4))) return rc;
    if ((rc = e->lens.reserve(pairs * 4))) return rc;
    *tok_dev = e->tokens.as<int32_t>();
    *lens_dev = e->lens.as<int32_t>();
    return HIPRAG_OK;
}

int32_t EncoderLease::score_dev(const int32_t* tok_dev, const int32_t* lens_dev, int nseq, int S, float* out_logits_dev, hipStream_t st)
{
    return static_cast<Encoder*>(enc_.get())->forward_dev(tok_dev, lens_dev, nseq, S, out_logits_dev, EncOut::logits, st);
}

int32_t EncoderLease::reserve_packed(size_t rows, size_t table_words, int32_t** tok_dev, int32_t** tab_dev)
{
    Encoder* e = static_cast<Encoder*>(enc_.get());
    int32_t rc;
    if ((rc = e->tokens.reserve(rows * 4))) return rc;
    if ((rc = e->ptab.reserve(table_words * 4))) return rc;
    *tok_dev = e->tokens.as<int32_t>();
    *tab_dev = e->ptab.as<int32_t>();
    return HIPRAG_OK;
}

int32_t EncoderLease::reserve_packed_work(int Tp)
{
    Encoder* e = static_cast<Encoder*>(enc_.get());
    return e->reserve_work(e->plan_packed(Tp));
}

int32_t EncoderLease::score_packed_dev(const PackedBatch& b, float* out_logits_dev, hipStream_t st)
{
    Encoder* e = static_cast<Encoder*>(enc_.get());
    return e->run_forward_packed(e->plan_packed(b.Tp), b, out_logits_dev, EncOut::logits, st);
}
}  // namespace hiprag

using namespace hiprag;

// What every forward entry does around Encoder::forward: handle, the encoder's mutex, its device, the batch-shape check,
// then the entry's own checks (`entry_checks(encoder)`: a status; they come BEFORE the empty batch returns), the empty
// batch, the null check (`outputs`: the entry's required outputs are all there) and the position table.
template <class EntryChecks>
static int32_t enc_run(uint64_t h, const int32_t* token_ids, const int32_t* seq_lens, int32_t nseq, int32_t max_len, bool outputs,
                       void* out_dev, EncOut mode, const HeadDest& heads, void* stream, EntryChecks entry_checks)
{
    auto e = reg().get(h);
    if (!e) { set_error("unknown encoder handle"); return HIPRAG_E_HANDLE; }
    std::lock_guard<std::mutex> guard(e->mu);
    HR_CHECK_HIP(hipSetDevice(e->device));
    HR_REQUIRE(nseq >= 0 && max_len > 0, "bad batch shape");
    if (const int32_t rc = entry_checks(*e)) return rc;
    if (nseq == 0) return HIPRAG_OK;
    HR_REQUIRE(token_ids && seq_lens && outputs, "null argument");
    HR_REQUIRE(max_len + e->cfg.pad_id + 1 < e->cfg.max_pos, "max_len %d exceeds the position table", max_len);
    return e->forward(token_ids, seq_lens, nseq, max_len, out_dev, mode, (hipStream_t)stream, heads);
}

static int32_t enc_run(uint64_t h, const int32_t* token_ids, const int32_t* seq_lens, int32_t nseq, int32_t max_len, void* out_dev,
                       EncOut mode, void* stream)
{
    return enc_run(h, token_ids, seq_lens, nseq, max_len, out_dev != nullptr, out_dev, mode, HeadDest{}, stream,
                   [](const Encoder&) -> int32_t { return HIPRAG_OK; });
}

// hipenc_linear_ex's `epilogue` (include/hiprag.h) is numbered on its own; the kernels' EPI_* are template arguments.
enum AbiEpilogue : int32_t { ABI_EPI_QKV = 0, ABI_EPI_GELU = 1, ABI_EPI_RESID = 2, ABI_EPI_RESID16 = 3, ABI_EPI_PART = 4 };
static int abi_epilogue(int32_t epilogue)
{
    switch (epilogue) {
    case ABI_EPI_QKV: return EPI_QKV;
    case ABI_EPI_GELU: return EPI_GELU;
    case ABI_EPI_RESID: return EPI_RESID;
    case ABI_EPI_RESID16: return EPI_RESID16;
    default: return EPI_PART;
    }
}

// f(std::integral_constant<int, EPI>) for the runtime epilogue `epi`
template <class F>
static void with_epilogue(int epi, F&& f)
{
    switch (epi) {
    case EPI_QKV: f(std::integral_constant<int, EPI_QKV>{}); break;
    case EPI_GELU: f(std::integral_constant<int, EPI_GELU>{}); break;
    case EPI_RESID: f(std::integral_constant<int, EPI_RESID>{}); break;
    case EPI_PART: f(std::integral_constant<int, EPI_PART>{}); break;
    case EPI_RESID16: f(std::integral_constant<int, EPI_RESID16>{}); break;
    }
}

extern "C" {

int32_t hipenc_create(const hipenc_config* cfg, const hipenc_weights* weights, int32_t device, uint64_t* out_handle)
{
    HR_REQUIRE(cfg && weights && out_handle, "null argument");
    HR_REQUIRE(cfg->hidden > 0 && cfg->hidden % 128 == 0 && cfg->hidden <= 2048, "hidden must be a multiple of 128, <= 2048");
    HR_REQUIRE(cfg->heads * 64 == cfg->hidden, "head_dim must be 64 (heads * 64 == hidden)");
    HR_REQUIRE(cfg->ffn > 0 && cfg->ffn % 128 == 0, "ffn must be a multiple of 128");
    HR_REQUIRE(cfg->layers > 0 && cfg->vocab > 0 && cfg->max_pos > cfg->pad_id + 1, "bad encoder config");
    HR_REQUIRE(weights->layers && weights->word_emb && weights->pos_emb && weights->type_emb && weights->emb_ln_g &&
                   weights->emb_ln_b, "null weight pointer");
    auto e = std::make_shared<Encoder>();
    e->device = device;
    e->cfg = *cfg;
    e->w = *weights;
    e->layers.assign(weights->layers, weights->layers + cfg->layers);
    if (const char* sr = std::getenv("HIPENC_SMALL_ROWS")) e->small_rows = std::atoi(sr);
    if (const char* g2 = std::getenv("HIPENC_GEMM256")) e->use256 = std::atoi(g2);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) e->n_cu = cus;
    }
    for (const auto& L : e->layers)
        HR_REQUIRE(L.wqkv && L.bqkv && L.wo && L.bo && L.ln1_g && L.ln1_b && L.w1 && L.b1 && L.w2 && L.b2 && L.ln2_g && L.ln2_b,
                   "null layer weight pointer");
    e->w.layers = nullptr;
    HR_CHECK_HIP(hipSetDevice(device));
    *out_handle = reg().put(e);
    return HIPRAG_OK;
}

int32_t hipenc_destroy(uint64_t h)
{
    auto e = reg().get(h);
    if (!e) { set_error("unknown encoder handle"); return HIPRAG_E_HANDLE; }
    {
        std::lock_guard<std::mutex> guard(e->mu);
        (void)hipSetDevice(e->device);
        (void)hipDeviceSynchronize();
    }
    reg().erase(h);
    return HIPRAG_OK;
}

int32_t hipenc_shape(uint64_t h, hipenc_shape_t* out)
{
    auto e = reg().get(h);
    if (!e) { set_error("unknown encoder handle"); return HIPRAG_E_HANDLE; }
    HR_REQUIRE(out, "null out");
    *out = e->shape();   // fixed at creation: no lock
    return HIPRAG_OK;
}

int32_t hipenc_forward_plan(const hipenc_shape_t* shape, int32_t nseq, int32_t S, hipenc_plan_t* out)
{
    HR_REQUIRE(shape && out, "null argument");
    HR_REQUIRE(shape->hidden > 0 && shape->hidden % 128 == 0 && shape->hidden <= 2048 && shape->ffn > 0 && shape->ffn % 128 == 0,
               "hipenc_forward_plan: hidden a multiple of 128, <= 2048; ffn a multiple of 128");
    HR_REQUIRE(shape->n_cu > 0 && nseq > 0 && S > 0 && S % kSkinnyRows == 0 && (int64_t)nseq * S < (1 << 30),
               "hipenc_forward_plan: n_cu, nseq positive, S a positive multiple of 64");
    const EncPlan p = plan_forward(*shape, nseq, S);
    *out = {p.T, p.M, (int32_t)p.path, p.osplit, p.dsplit, p.fsplit, p.head_split, (int64_t)p.pre_bytes};
    return HIPRAG_OK;
}

int32_t hipenc_forward(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq, int32_t max_len,
                       float* out_dev, void* stream)
{
    return enc_run(h, token_ids_host, seq_lens_host, nseq, max_len, out_dev, EncOut::embedding, stream);
}

int32_t hipenc_set_lexical_head(uint64_t h, const void* w_dev, const float* b_dev, const int32_t* unused_ids_host, int32_t n_unused)
{
    auto e = reg().get(h);
    if (!e) { set_error("unknown encoder handle"); return HIPRAG_E_HANDLE; }
    std::lock_guard<std::mutex> guard(e->mu);
    HR_REQUIRE(w_dev && b_dev, "null lexical head weight or bias");
    HR_REQUIRE(n_unused >= 0 && n_unused <= kLexMaxUnused, "n_unused must be in 0..%d (got %d)", kLexMaxUnused, n_unused);
    HR_REQUIRE(unused_ids_host || n_unused == 0, "unused_ids is null");
    e->lex_w = w_dev;
    e->lex_b = b_dev;
    e->lex_unused = LexUnused{};
    e->lex_unused.n = n_unused;
    for (int i = 0; i < n_unused; ++i) e->lex_unused.ids[i] = unused_ids_host[i];
    return HIPRAG_OK;
}

int32_t hipenc_forward_lexical(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq, int32_t max_len,
                               float* out_dense_dev, int32_t* out_terms_dev, float* out_weights_dev, int32_t* out_counts_dev, void* stream)
{
    HeadDest heads;
    heads.lex = {out_terms_dev, out_weights_dev, out_counts_dev, max_len};
    return enc_run(h, token_ids_host, seq_lens_host, nseq, max_len, out_terms_dev && out_weights_dev && out_counts_dev, out_dense_dev,
                   EncOut::lexical, heads, stream, [&](const Encoder& e) -> int32_t {
                       HR_REQUIRE(e.lex_w && e.lex_b, "no lexical head: call hipenc_set_lexical_head first");
                       if (max_len > kLexMaxLen) { set_error("max_len %d is beyond the lexical head's %d positions per sequence", max_len, kLexMaxLen); return HIPRAG_E_UNSUPPORTED; }
                       return HIPRAG_OK;
                   });
}

int32_t hipenc_set_colbert_head(uint64_t h, const void* w_dev, const float* b_dev)
{
    auto e = reg().get(h);
    if (!e) { set_error("unknown encoder handle"); return HIPRAG_E_HANDLE; }
    std::lock_guard<std::mutex> guard(e->mu);
    HR_REQUIRE(w_dev && b_dev, "null ColBERT head weight or bias");
    e->col_w = w_dev;
    e->col_b = b_dev;
    return HIPRAG_OK;
}

int32_t hipenc_forward_colbert(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq, int32_t max_len,
                               float* out_dense_dev, void* out_vecs_dev, int32_t* out_counts_dev, void* stream)
{
    HeadDest heads;
    heads.col = {(bf16*)out_vecs_dev, out_counts_dev, max_len - 1};
    return enc_run(h, token_ids_host, seq_lens_host, nseq, max_len, out_vecs_dev && out_counts_dev, out_dense_dev, EncOut::colbert,
                   heads, stream, [&](const Encoder& e) -> int32_t {
                       HR_REQUIRE(e.col_w && e.col_b, "no ColBERT head: call hipenc_set_colbert_head first");
                       HR_REQUIRE(max_len >= 2, "max_len must be at least 2 (got %d): the CLS position carries no vector", max_len);
                       return HIPRAG_OK;
                   });
}

// dense, lexical and ColBERT outputs from ONE forward (include/hiprag.h): the union of the two head entries' checks
int32_t hipenc_forward_m3(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq, int32_t max_len,
                          float* out_dense_dev, int32_t* out_terms_dev, float* out_weights_dev, int32_t* out_lex_counts_dev,
                          void* out_vecs_dev, int32_t* out_col_counts_dev, void* stream)
{
    HeadDest heads;
    heads.lex = {out_terms_dev, out_weights_dev, out_lex_counts_dev, max_len};
    heads.col = {(bf16*)out_vecs_dev, out_col_counts_dev, max_len - 1};
    return enc_run(h, token_ids_host, seq_lens_host, nseq, max_len,
                   out_terms_dev && out_weights_dev && out_lex_counts_dev && out_vecs_dev && out_col_counts_dev, out_dense_dev, EncOut::m3,
                   heads, stream, [&](const Encoder& e) -> int32_t {
                       HR_REQUIRE(e.lex_w && e.lex_b, "no lexical head: call hipenc_set_lexical_head first");
                       HR_REQUIRE(e.col_w && e.col_b, "no ColBERT head: call hipenc_set_colbert_head first");
                       HR_REQUIRE(max_len >= 2, "max_len must be at least 2 (got %d): the CLS position carries no vector", max_len);
                       if (max_len > kLexMaxLen) { set_error("max_len %d is beyond the lexical head's %d positions per sequence", max_len, kLexMaxLen); return HIPRAG_E_UNSUPPORTED; }
                       return HIPRAG_OK;
                   });
}

int32_t hipenc_colbert_rows(const void* x_dev, const int32_t* lens_dev, int32_t nseq, int32_t S, const void* w_dev, const float* b_dev,
                            int32_t H, void* out_vecs_dev, int32_t* out_counts_dev, int32_t row_stride, void* stream)
{
    HR_REQUIRE(x_dev && lens_dev && w_dev && b_dev && out_vecs_dev && out_counts_dev, "null argument");
    HR_REQUIRE(nseq > 0 && S > 0 && S % 64 == 0, "nseq positive and S a positive multiple of 64");
    HR_REQUIRE(H > 0 && H % 128 == 0 && H <= 2048, "H must be a multiple of 128, <= 2048");
    HR_REQUIRE(row_stride >= 1 && row_stride <= S - 1, "row_stride must be in 1..S - 1 (got %d)", row_stride);
    HR_REQUIRE((int64_t)nseq * S < (1 << 24), "too many rows for the hook");
    hipStream_t st = (hipStream_t)stream;
    // The hook has no handle, and of the forward's three forms of the head's product it has the two that differ: the plan of
    // a model of this width whose FFN is as wide (so that F adds no condition), with the DEFAULT small-batch row count
    // (kSmallRowsDefault, whatever HIPENC_SMALL_ROWS says) and the 256-tile kernel off (on the big path the head runs the
    // 128-tile kernel unsplit, as it does here at that many rows).
    const EncPlan pl = plan_forward(EncShape{H, H, 1, kSmallRowsDefault, 0}, nseq, S);
    const int T = pl.T, Mpad = pl.M;
    DevBuf xp, pre;   // the rows padded to whole tiles, and the partials
    int32_t rc;
    if ((rc = xp.reserve((size_t)Mpad * H * 2))) return rc;
    if ((rc = pre.reserve((size_t)T * H * 4 * pl.head_split))) return rc;
    HR_CHECK_HIP(hipMemsetAsync(xp.p, 0, (size_t)Mpad * H * 2, st));
    HR_CHECK_HIP(hipMemcpyAsync(xp.p, x_dev, (size_t)T * H * 2, hipMemcpyDeviceToDevice, st));
    const ColOut col{(bf16*)out_vecs_dev, out_counts_dev, row_stride};
    launch_colbert_head(xp.as<bf16>(), T, Mpad, H, pl.path == EncPath::small, pl.head_split, (const bf16*)w_dev, b_dev, pre.as<float>(),
                        lens_dev, S, col, st);
    const hipError_t le = hipGetLastError();
    HR_CHECK_HIP(hipStreamSynchronize(st));   // the frame's buffers go
    HR_CHECK_HIP(le);
    return HIPRAG_OK;
}

int32_t hipenc_score_pairs(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq,
                           int32_t max_len, float* out_logits_dev, void* stream)
{
    return enc_run(h, token_ids_host, seq_lens_host, nseq, max_len, out_logits_dev, EncOut::logits, stream);
}

int32_t hipenc_forward_hidden(uint64_t h, const int32_t* token_ids_host, const int32_t* seq_lens_host, int32_t nseq,
                              int32_t max_len, void* out_hidden_dev, void* stream)
{
    return enc_run(h, token_ids_host, seq_lens_host, nseq, max_len, out_hidden_dev, EncOut::hidden, stream);
}

int32_t hipenc_attention(const void* q_dev, const void* k_dev, const void* vt_dev, const int32_t* lens_dev, void* ctx_dev,
                         int32_t nseq, int32_t S, int32_t heads, void* stream)
{
    HR_REQUIRE(q_dev && k_dev && vt_dev && lens_dev && ctx_dev, "null argument");
    HR_REQUIRE(nseq > 0 && heads > 0 && S > 0 && S % 64 == 0, "nseq, heads positive and S a positive multiple of 64");
    hipStream_t st = (hipStream_t)stream;
    HR_CHECK_HIP(hipMemsetAsync(ctx_dev, 0, (size_t)nseq * S * heads * 64 * 2, st));   // as forward does: skipped tiles stay zero
    launch_attention((const bf16*)q_dev, (const bf16*)k_dev, (const bf16*)vt_dev, (const int*)lens_dev, (bf16*)ctx_dev, nseq, S,
                     heads, st);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

// ---- packed batches --------------------------------------------------------------------------------------------------------
// What every packed entry does around Encoder::forward_packed: handle, mutex, device, nseq, the head (score), the empty
// batch, the null check; the batch's own checks are forward_packed's and come before anything is enqueued.
static int32_t enc_run_packed(uint64_t h, const int32_t* tokens, const int32_t* offsets, int32_t nseq, void* out_dev, EncOut mode,
                              void* stream)
{
    auto e = reg().get(h);
    if (!e) { set_error("unknown encoder handle"); return HIPRAG_E_HANDLE; }
    std::lock_guard<std::mutex> guard(e->mu);
    HR_CHECK_HIP(hipSetDevice(e->device));
    HR_REQUIRE(nseq >= 0, "bad batch shape");
    HR_REQUIRE(mode != EncOut::logits || (e->w.cls_dense_w && e->w.cls_out_w), "encoder was created without a classification head");
    if (nseq == 0) return HIPRAG_OK;
    HR_REQUIRE(offsets && out_dev, "null argument");
    HR_REQUIRE(tokens || offsets[nseq] == 0, "null argument");
    return e->forward_packed(tokens, offsets, nseq, out_dev, mode, (hipStream_t)stream);
}

int32_t hipenc_forward_packed(uint64_t h, const int32_t* tokens_host, const int32_t* offsets_host, int32_t nseq, float* out_dev,
                              void* stream)
{
    return enc_run_packed(h, tokens_host, offsets_host, nseq, out_dev, EncOut::embedding, stream);
}

int32_t hipenc_score_pairs_packed(uint64_t h, const int32_t* tokens_host, const int32_t* offsets_host, int32_t nseq,
                                  float* out_logits_dev, void* stream)
{
    return enc_run_packed(h, tokens_host, offsets_host, nseq, out_logits_dev, EncOut::logits, stream);
}

int32_t hipenc_forward_hidden_packed(uint64_t h, const int32_t* tokens_host, const int32_t* offsets_host, int32_t nseq,
                                     void* out_hidden_dev, void* stream)
{
    return enc_run_packed(h, tokens_host, offsets_host, nseq, out_hidden_dev, EncOut::hidden, stream);
}

int32_t hipenc_packed_layout(const int32_t* lens_host, int32_t nseq, int32_t* out_row_off, int32_t* out_gran_seq,
                             int32_t* out_items, int32_t* out_counts)
{
    HR_REQUIRE(nseq >= 0 && out_counts && (lens_host || nseq == 0), "hipenc_packed_layout: nseq >= 0, lens and out_counts not null");
    PackedLayout lay;
    HR_REQUIRE(packed_layout(lens_host, nseq, lay), "hipenc_packed_layout: a negative length, or 2^30 packed rows or more");
    out_counts[0] = lay.Tp;
    out_counts[1] = lay.n_items();
    if (out_row_off) std::copy(lay.row_off.begin(), lay.row_off.end(), out_row_off);
    if (out_gran_seq) std::copy(lay.gran_seq.begin(), lay.gran_seq.end(), out_gran_seq);
    if (out_items) std::copy(lay.items.begin(), lay.items.end(), out_items);
    return HIPRAG_OK;
}

int32_t hipenc_packed_info(uint64_t h, int64_t* out4)
{
    auto e = reg().get(h);
    if (!e) { set_error("unknown encoder handle"); return HIPRAG_E_HANDLE; }
    HR_REQUIRE(out4, "null out");
    std::lock_guard<std::mutex> guard(e->mu);
    std::copy(e->packed_last, e->packed_last + 4, out4);
    return HIPRAG_OK;
}

int32_t hipenc_attention_packed(const void* q_dev, const void* k_dev, const void* vt_dev, const int32_t* row_off_dev,
                                const int32_t* lens_dev, const int32_t* items_dev, int32_t n_items, int32_t nseq, int32_t Tp,
                                int32_t heads, void* ctx_dev, void* stream)
{
    HR_REQUIRE(q_dev && k_dev && vt_dev && row_off_dev && lens_dev && ctx_dev, "null argument");
    HR_REQUIRE(items_dev || n_items == 0, "null argument");
    HR_REQUIRE(nseq > 0 && heads > 0 && n_items >= 0 && Tp > 0 && Tp % kPackGranule == 0 && Tp < kPackMaxRows,
               "nseq, heads positive, n_items >= 0 and Tp a positive multiple of 64 below 2^30");
    hipStream_t st = (hipStream_t)stream;
    HR_CHECK_HIP(hipMemsetAsync(ctx_dev, 0, (size_t)Tp * heads * 64 * 2, st));   // as the forward does
    launch_attention_packed((const bf16*)q_dev, (const bf16*)k_dev, (const bf16*)vt_dev, (const int*)row_off_dev, (const int*)lens_dev,
                            (const int*)items_dev, n_items, Tp, heads, (bf16*)ctx_dev, st);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

int32_t hipenc_linear_ex(const void* a_dev, const void* w_dev, const float* bias_dev, int32_t M, int32_t N, int32_t K,
                         int32_t epilogue, const void* resid_dev, void* out_dev, void* out_k_dev, void* out_vt_dev, int32_t S,
                         int32_t heads, int32_t impl, int32_t m_valid, int32_t ksplit, int32_t max_workgroups,
                         int32_t* out_splits, void* stream)
{
    HR_REQUIRE(a_dev && w_dev && out_dev, "null argument");
    HR_REQUIRE(epilogue >= ABI_EPI_QKV && epilogue <= ABI_EPI_PART,
               "epilogue: 0 = qkv, 1 = gelu, 2 = bias + residual -> f32, 3 = bias + residual -> bf16, 4 = raw fp32 partials");
    const int epi = abi_epilogue(epilogue);   // from here on the kernels' numbering alone
    HR_REQUIRE(bias_dev || epi == EPI_PART, "null bias");
    HR_REQUIRE(impl >= 0 && impl <= 3, "impl: 0 = auto, 1 = 128 x 128 tiles, 2 = 256 x 256 persistent tiles, 3 = small-batch kernel");
    HR_REQUIRE(M > 0 && N > 0 && K > 0, "M, N, K positive");
    HR_REQUIRE(m_valid > 0 && m_valid <= M && m_valid % 64 == 0, "m_valid: a positive multiple of 64, at most M");
    HR_REQUIRE(max_workgroups >= 0, "max_workgroups >= 0 (0 = no cap)");
    HR_REQUIRE(max_workgroups == 0 || impl == 2, "max_workgroups caps the persistent 256-tile kernel only (impl 2)");
    hipStream_t st = (hipStream_t)stream;
    GemmArgs g{};
    g.A = (const bf16*)a_dev; g.W = (const bf16*)w_dev; g.bias = bias_dev; g.M = m_valid; g.N = N; g.K = K;
    if (epi == EPI_QKV) {
        HR_REQUIRE(out_k_dev && out_vt_dev && S > 0 && heads > 0 && N == 3 * heads * 64 && M % S == 0 && S % 64 == 0,
                   "qkv epilogue: N = 3 * heads * 64, M a multiple of S, S a multiple of 64");
        g.q = (bf16*)out_dev; g.k = (bf16*)out_k_dev; g.vt = (bf16*)out_vt_dev; g.S = S; g.heads = heads; g.H = heads * 64;
    } else if (epi == EPI_GELU) {
        g.out_bf16 = (bf16*)out_dev;
    } else if (epi == EPI_PART) {
        g.out_f32 = (float*)out_dev;
    } else {
        HR_REQUIRE(resid_dev, "null residual");
        g.resid = (const bf16*)resid_dev; g.out_f32 = (float*)out_dev; g.out_bf16 = (bf16*)out_dev;
    }
    if (impl == 3) {
        // the small-batch kernel as forward launches it: every row is a real row there (g.M = T), so there is no padding
        HR_REQUIRE(skinny_has(epi), "the small-batch kernel has the qkv, gelu and partials epilogues");
        HR_REQUIRE(M % 64 == 0 && m_valid == M, "the small-batch kernel takes whole 64-row blocks and no padding rows (m_valid = M)");
        HR_REQUIRE(N % 16 == 0 && skinny_ok(K), "the small-batch kernel needs N a multiple of 16 and K / ceil(K / 1024) a multiple of 128");
        const int sp = skinny_split(K);
        HR_REQUIRE(epi == EPI_PART || sp == 1, "K > 1024 splits over workgroups: partials epilogue only");
        HR_REQUIRE(ksplit == 0 || ksplit == sp, "the small-batch kernel picks its own split, ceil(K / 1024): pass ksplit 0");
        with_epilogue(epi, [&](auto E) { if constexpr (skinny_has(E.value)) launch_skinny<E.value>(g, st); });
        if (out_splits) *out_splits = sp;
        HR_CHECK_HIP(hipGetLastError());
        return HIPRAG_OK;
    }
    HR_REQUIRE(M % BM == 0 && N % BN == 0 && K % BK == 0, "M, N multiples of 128 and K of 64");
    HR_REQUIRE(epi != EPI_RESID16 || impl != 1, "the bf16 residual epilogue exists in the 256-tile kernel only");
    if (epi == EPI_PART) {
        HR_REQUIRE(impl == 1, "raw partials come from the 128-tile kernel (impl 1) or the small-batch kernel (impl 3)");
        HR_REQUIRE(ksplit >= 1 && ksplit <= 4 && K % (ksplit * BK) == 0, "ksplit in 1..4 with K a multiple of ksplit * 64");
        g.ksplit = ksplit;
        launch_tiled<EPI_PART>(g, M, st);
        if (out_splits) *out_splits = ksplit;
        HR_CHECK_HIP(hipGetLastError());
        return HIPRAG_OK;
    }
    HR_REQUIRE(ksplit == 0 || ksplit == 1, "ksplit belongs to the partials epilogue");
    int dev = 0, cus = 256;
    HR_CHECK_HIP(hipGetDevice(&dev));
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    // the QKV scatter of the 256-tile kernel wants whole tiles inside each of q, k and v
    const bool can256 = tile256_shape_ok(M, N, K) && (epi != EPI_QKV || g.H % G2_T == 0);
    HR_REQUIRE(impl != 2 || can256, "the 256-tile kernel needs M, N multiples of 256 and K of 128");
    HR_REQUIRE(epi != EPI_RESID16 || can256, "the bf16 residual epilogue needs M, N multiples of 256 and K of 128");
    if (impl == 2 || epi == EPI_RESID16 || (impl == 0 && can256 && tile256_fills_auto(M, N, cus))) {
        // the residual epilogues of the 256-tile kernel never mask rows (forward gives them whole tiles)
        HR_REQUIRE(epi == EPI_QKV || epi == EPI_GELU || m_valid == M,
                   "the residual epilogues of the 256-tile kernel write every row: m_valid = M");
        with_epilogue(epi, [&](auto E) { if constexpr (tile256_has(E.value)) launch256_grid<E.value>(g, M, cus, max_workgroups, st); });
    } else {
        with_epilogue(epi, [&](auto E) { if constexpr (tiled_has(E.value)) launch_tiled<E.value>(g, M, st); });
    }
    if (out_splits) *out_splits = 1;
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

int32_t hipenc_linear(const void* a_dev, const void* w_dev, const float* bias_dev, int32_t M, int32_t N, int32_t K,
                      int32_t epilogue, const void* resid_dev, void* out_dev, void* out_k_dev, void* out_vt_dev, int32_t S,
                      int32_t heads, int32_t impl, void* stream)
{
    HR_REQUIRE(bias_dev, "null argument");
    HR_REQUIRE(epilogue >= ABI_EPI_QKV && epilogue <= ABI_EPI_RESID16,
               "epilogue: 0 = qkv, 1 = gelu, 2 = bias + residual -> f32, 3 = bias + residual -> bf16");
    HR_REQUIRE(impl >= 0 && impl <= 2, "impl: 0 = auto, 1 = 128 x 128 tiles, 2 = 256 x 256 persistent tiles");
    HR_REQUIRE(M > 0 && M % BM == 0, "M, N multiples of 128 and K of 64");
    return hipenc_linear_ex(a_dev, w_dev, bias_dev, M, N, K, epilogue, resid_dev, out_dev, out_k_dev, out_vt_dev, S, heads, impl,
                            M, 0, 0, nullptr, stream);
}

int32_t hipenc_layernorm(const void* x_dev, const float* gamma_dev, const float* beta_dev, void* y_dev, int32_t M, int32_t H,
                         float eps, int32_t form, int32_t nsplit, const float* bias_dev, const void* resid_dev, void* stream)
{
    HR_REQUIRE(x_dev && gamma_dev && beta_dev && y_dev, "null argument");
    HR_REQUIRE(form >= 0 && form <= 2, "form: 0 = fp32 rows, 1 = fp32 partials + bias + bf16 residual, 2 = bf16 rows");
    HR_REQUIRE(M > 0 && H > 0 && H % 128 == 0 && H <= (form == 2 ? 1024 : 2048),
               "M positive; H a multiple of 128, at most 2048 (bf16 rows: 1024)");
    hipStream_t st = (hipStream_t)stream;
    if (form == 0) {
        launch_layernorm<false>((const float*)x_dev, gamma_dev, beta_dev, (bf16*)y_dev, M, H, eps, 1, nullptr, nullptr, st);
    } else if (form == 1) {
        HR_REQUIRE(nsplit >= 1 && nsplit <= 4 && bias_dev && resid_dev, "form 1: nsplit in 1..4, bias and residual");
        launch_layernorm<true>((const float*)x_dev, gamma_dev, beta_dev, (bf16*)y_dev, M, H, eps, nsplit, bias_dev,
                               (const bf16*)resid_dev, st);
    } else {
        launch_layernorm16((const bf16*)x_dev, gamma_dev, beta_dev, (bf16*)y_dev, M, H, eps, st);
    }
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

int32_t hipenc_last_flops(uint64_t h, double* out_flops)
{
    auto e = reg().get(h);
    if (!e) { set_error("unknown encoder handle"); return HIPRAG_E_HANDLE; }
    HR_REQUIRE(out_flops, "null out");
    std::lock_guard<std::mutex> guard(e->mu);   // forward writes it under the mutex
    *out_flops = e->flops_last;
    return HIPRAG_OK;
}

}  // extern "C"
