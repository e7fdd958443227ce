// rerank.hip -- the device rerank call (hiprerank_*, include/hiprag.h): cross-encoder logits of (query, candidate passage)
// pairs and the best k of every query, from candidate ids that are still on the device.
//
// Stands for the reranker the reference only configures (rag/config.py:25-27).  The passages are not tokenised again: their
// token bodies lie in a passage token store (token_store.hip).  One kernel assembles every `<s> q </s></s> p </s>` pair of
// the call straight into the encoder's token buffer, the encoder's forward runs from there in sub-batches (no host staging,
// no synchronisation: Encoder::forward_dev), and one kernel orders every query's candidates by (logit descending, position
// ascending).
//
// Kernels: rerank_assemble_kernel (one workgroup per pair, one thread per token of the row: coalesced 4-byte stores, the
// passage read is one contiguous run of the CSR) and rerank_select_kernel (one workgroup per query, rank by counting in LDS:
// depth <= 256, so 64 K comparisons at most).  Both are latency-bound beside a 24-layer forward.
//
// The PACKED call (hiprerank_packed_*) gives every pair its own length rounded up to 64 rows instead of the store-wide S:
// rerank_pair_len_kernel, ONE copy of the lengths to pinned memory and ONE synchronise of the stream, the host's layout and cut
// into sub-batches (encoder_packed.h), one upload of the tables, rerank_assemble_packed_kernel, the encoder's packed forward
// per sub-batch, the same selection kernel.  It trades the padded call's "no host synchronisation" for rows.
#include <algorithm>
#include <cfloat>
#include <cstring>

#include <vector>

#include "encoder_internal.h"
#include "encoder_packed.h"
#include "token_store.h"

namespace hiprag {
namespace {

constexpr int kAsmThreads = 256;
constexpr int kMaxDepth = 256;

// pair(q, p, L) = [bos] + q[:room] + [eos, eos] + p[:max(0, room - len(q[:room]))] + [eos], room = max(0, L - 4); `pad` behind
// it up to S.  A candidate that names no stored document (negative, or outside [id_base, id_base + n_docs)) is a padding slot:
// the pair of an empty query and an empty passage, so that no row of the encoder batch is empty.  Its document row is never read.
// What the rule makes of one (query, candidate) slot: ql query and pl passage tokens from q0 / p0 on; the pair has ql + pl + 4.
struct PairShape {
    bool valid;
    int ql, pl, q0;
    int64_t p0;
};
__device__ __forceinline__ PairShape pair_shape(int64_t pair, const int64_t* __restrict__ cand, int depth, int64_t id_base, int64_t n_docs,
                                                const int64_t* __restrict__ doc_off, const int32_t* __restrict__ q_off, int room)
{
    const int qi = (int)(pair / depth);
    const int64_t c = cand[pair];
    PairShape p;
    p.valid = c >= id_base && c - id_base < n_docs;   // c >= id_base first: the difference cannot overflow for c >= 0
    p.ql = 0; p.pl = 0; p.p0 = 0;
    p.q0 = q_off[qi];
    if (p.valid) {
        const int64_t doc = c - id_base;
        p.p0 = doc_off[doc];
        p.ql = min(q_off[qi + 1] - p.q0, room);
        p.pl = (int)min(doc_off[doc + 1] - p.p0, (int64_t)max(0, room - p.ql));
    }
    return p;
}
// token t < ql + pl + 4 of the pair
__device__ __forceinline__ int pair_token(const PairShape& p, int t, const int32_t* __restrict__ q_tok, const int32_t* __restrict__ doc_tok,
                                          int bos, int eos)
{
    if (t == 0) return bos;
    if (t <= p.ql) return q_tok[p.q0 + t - 1];
    if (t <= p.ql + 2) return eos;
    if (t < p.ql + 3 + p.pl) return doc_tok[p.p0 + (t - p.ql - 3)];
    return eos;
}

__global__ __launch_bounds__(kAsmThreads) void rerank_assemble_kernel(const int64_t* __restrict__ cand, int depth, int64_t id_base,
                                                                      int64_t n_docs, const int64_t* __restrict__ doc_off,
                                                                      const int32_t* __restrict__ doc_tok,
                                                                      const int32_t* __restrict__ q_off, const int32_t* __restrict__ q_tok,
                                                                      int room, int S, int bos, int eos, int pad,
                                                                      int32_t* __restrict__ out_tok, int32_t* __restrict__ out_len,
                                                                      int32_t* __restrict__ counters)
{
    const int64_t pair = blockIdx.x;
    const PairShape p = pair_shape(pair, cand, depth, id_base, n_docs, doc_off, q_off, room);
    const int len = min(p.ql + p.pl + 4, S);   // <= S by the host's choice of S; the min keeps every store inside the row regardless
    int32_t* row = out_tok + pair * S;
    for (int t = threadIdx.x; t < S; t += kAsmThreads) row[t] = t < len ? pair_token(p, t, q_tok, doc_tok, bos, eos) : pad;
    if (threadIdx.x == 0) {
        out_len[pair] = len;
        atomicAdd(counters + (p.valid ? 0 : 1), 1);
    }
}

// ---- the packed call (hiprerank_packed_*): rows follow every pair's own length, not the store's longest document -------------
// Step 1: the length of every pair, by the rule's arithmetic (a padding slot is the 4-token pair); counts valid / padding.
__global__ __launch_bounds__(kAsmThreads) void rerank_pair_len_kernel(const int64_t* __restrict__ cand, int64_t pairs, int depth,
                                                                      int64_t id_base, int64_t n_docs, const int64_t* __restrict__ doc_off,
                                                                      const int32_t* __restrict__ q_off, int room,
                                                                      int32_t* __restrict__ out_len, int32_t* __restrict__ counters)
{
    const int64_t pair = (int64_t)blockIdx.x * kAsmThreads + threadIdx.x;
    if (pair >= pairs) return;
    const PairShape p = pair_shape(pair, cand, depth, id_base, n_docs, doc_off, q_off, room);
    out_len[pair] = p.ql + p.pl + 4;
    atomicAdd(counters + (p.valid ? 0 : 1), 1);
}

// Step 6: pair `pair` goes to rows row0[pair] .. of the packed token buffer: its tokens, then `pad` to the end of its last
// 64-row granule.  row0 is the host's layout of the SAME lengths (the kernel above): whole granules, so nothing else is written.
__global__ __launch_bounds__(kAsmThreads) void rerank_assemble_packed_kernel(const int64_t* __restrict__ cand, int depth, int64_t id_base,
                                                                             int64_t n_docs, const int64_t* __restrict__ doc_off,
                                                                             const int32_t* __restrict__ doc_tok,
                                                                             const int32_t* __restrict__ q_off, const int32_t* __restrict__ q_tok,
                                                                             int room, int bos, int eos, int pad,
                                                                             const int32_t* __restrict__ plen,
                                                                             const int32_t* __restrict__ row0, int32_t* __restrict__ out_tok)
{
    const int64_t pair = blockIdx.x;
    const PairShape p = pair_shape(pair, cand, depth, id_base, n_docs, doc_off, q_off, room);
    // plen is step 1's length, the one the layout was made of: the stores stay inside the pair's granules whatever cand holds now
    const int R = (plen[pair] + 63) & ~63, len = min(p.ql + p.pl + 4, plen[pair]);
    int32_t* row = out_tok + row0[pair];
    for (int t = threadIdx.x; t < R; t += kAsmThreads) row[t] = t < len ? pair_token(p, t, q_tok, doc_tok, bos, eos) : pad;
}

// One workgroup per query.  Valid candidates are ranked by counting those that come before them under (logit descending,
// position ascending); the first k go out.  Padding slots get -FLT_MAX in `logits`, and ranks past the valid candidates get
// id -1, -FLT_MAX, position -1.  A NaN logit compares false with everything: two candidates may then claim one rank (their
// place is unspecified), and the pre-filled padding stays where no one wrote.
__global__ __launch_bounds__(kMaxDepth) void rerank_select_kernel(const int64_t* __restrict__ cand, int depth, int64_t id_base,
                                                                  int64_t n_docs, float* __restrict__ logits, int k,
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
        valid = c >= id_base && c - id_base < n_docs;
        if (valid) l = logits[base + t];
        else logits[base + t] = -FLT_MAX;
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

int round64(int64_t v) { return (int)((v + 63) / 64 * 64); }

// Shape and query checks that need no handle.  `vocab`: what a query id must lie under.
int32_t check_queries(const int32_t* q_tokens, const int32_t* q_offsets, int32_t nq, int32_t vocab, int* longest)
{
    HR_REQUIRE(q_offsets, "q_offsets is null");
    HR_REQUIRE(q_offsets[0] == 0, "q_offsets must start at 0 (got %d)", q_offsets[0]);
    int lq = 0;
    for (int b = 0; b < nq; ++b) {
        HR_REQUIRE(q_offsets[b] <= q_offsets[b + 1], "q_offsets descend at query %d", b);
        lq = std::max(lq, q_offsets[b + 1] - q_offsets[b]);
    }
    HR_REQUIRE(q_tokens || q_offsets[nq] == 0, "q_tokens is null");
    for (int t = 0; t < q_offsets[nq]; ++t)
        HR_REQUIRE(q_tokens[t] >= 0 && q_tokens[t] < vocab, "query token %d = %d lies outside [0, vocab = %d)", t, q_tokens[t], vocab);
    *longest = lq;
    return HIPRAG_OK;
}

// S = min(max_len, 4 + longest query + longest document), rounded up to 64.  cand_host != NULL: the longest document among
// the call's valid candidates (the host entry and the test hook know the ids); otherwise the longest of the store.
int bound_S(const TokenStore& s, int max_len, int lq, const int64_t* cand_host, int64_t n_cand, int64_t id_base)
{
    int64_t ld = s.csr.longest;
    if (cand_host) {
        ld = 0;
        for (int64_t i = 0; i < n_cand; ++i) {
            const int64_t c = cand_host[i];
            if (c >= id_base && c - id_base < s.csr.n_docs) ld = std::max<int64_t>(ld, s.csr.len_host[(size_t)(c - id_base)]);
        }
    }
    return round64(std::min<int64_t>(max_len, 4 + (int64_t)lq + ld));
}

// The query arrays go to the device through the store's ring of pinned buffers: copied before this returns, waiting for
// nothing but the copy out of this buffer kStages calls ago.  -> q_off_dev (nq + 1 ints) and q_tok_dev behind it.
int32_t stage_queries(TokenStore& s, const int32_t* q_tokens, const int32_t* q_offsets, int32_t nq, hipStream_t st,
                      const int32_t** q_off_dev, const int32_t** q_tok_dev)
{
    const size_t n_off = (size_t)nq + 1, n_tok = (size_t)q_offsets[nq], words = n_off + n_tok;
    TokenStore::Stage& sg = s.stages[s.stage_next++ % TokenStore::kStages];
    int32_t rc;
    if (!sg.ev) HR_CHECK_HIP(hipEventCreateWithFlags(&sg.ev, hipEventDisableTiming));
    if (sg.used) HR_CHECK_HIP(hipEventSynchronize(sg.ev));
    if ((rc = sg.pin.reserve(words * 4))) return rc;
    if ((rc = s.q_dev.reserve(words * 4))) return rc;
    memcpy(sg.pin.p, q_offsets, n_off * 4);
    if (n_tok) memcpy(sg.pin.as<int32_t>() + n_off, q_tokens, n_tok * 4);
    HR_CHECK_HIP(hipMemcpyAsync(s.q_dev.p, sg.pin.p, words * 4, hipMemcpyHostToDevice, st));
    HR_CHECK_HIP(hipEventRecord(sg.ev, st));
    sg.used = true;
    *q_off_dev = s.q_dev.as<int32_t>();
    *q_tok_dev = s.q_dev.as<int32_t>() + n_off;
    return HIPRAG_OK;
}

// {valid pairs, padding slots} of the last padded call at [0], [1], of the last packed call at [2], [3]; zero until counted
int32_t reserve_counters(TokenStore& s)
{
    if (s.counters.p) return HIPRAG_OK;
    int32_t rc;
    if ((rc = s.counters.reserve(4 * sizeof(int32_t)))) return rc;
    HR_CHECK_HIP(hipMemset(s.counters.p, 0, 4 * sizeof(int32_t)));
    return HIPRAG_OK;
}

int32_t launch_assemble(TokenStore& s, const int64_t* cand_dev, int64_t pairs, int depth, int64_t id_base, const int32_t* q_off_dev,
                        const int32_t* q_tok_dev, int max_len, int S, int32_t* tok_dev, int32_t* lens_dev, hipStream_t st)
{
    int32_t rc;
    if ((rc = reserve_counters(s))) return rc;
    HR_CHECK_HIP(hipMemsetAsync(s.counters.p, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(rerank_assemble_kernel, dim3((unsigned)pairs), dim3(kAsmThreads), 0, st, cand_dev, depth, id_base, (int64_t)s.csr.n_docs,
                       (const int64_t*)s.csr.offsets.as<int64_t>(), (const int32_t*)s.tokens.as<int32_t>(), q_off_dev, q_tok_dev,
                       std::max(0, max_len - 4), S, (int)s.bos, (int)s.eos, (int)s.pad, tok_dev, lens_dev, s.counters.as<int32_t>());
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

// The checks of the padded and the packed call alike: those that need no handle ...
int32_t check_call(int32_t nq, int32_t k, int32_t depth, const void* cand_dev, const void* out_scores_dev, const void* out_ids_dev,
                   int32_t max_len, int64_t id_base, int64_t max_batch_tokens)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(1 <= k && k <= depth && depth <= kMaxDepth, "1 <= k <= depth <= %d does not hold (k = %d, depth = %d)", kMaxDepth, k, depth);
    HR_REQUIRE(cand_dev && out_scores_dev && out_ids_dev, "null argument");
    HR_REQUIRE(max_len >= 5, "max_len must be at least 5 (got %d): four special tokens and one of text", max_len);
    HR_REQUIRE(id_base >= 0, "id_base must not be negative (got %lld)", (long long)id_base);
    HR_REQUIRE(max_batch_tokens >= 0, "max_batch_tokens must not be negative");
    return HIPRAG_OK;
}
// ... and those of the encoder against the store
int32_t check_handles(const EncoderView& ev, const TokenStore& s, int32_t max_len)
{
    HR_REQUIRE(ev.has_head, "encoder was created without a classification head");
    HR_REQUIRE(ev.device == s.device, "the encoder lives on device %d, the token store on device %d", ev.device, s.device);
    HR_REQUIRE(s.vocab <= ev.vocab, "the store's vocabulary (%d) exceeds the encoder's (%d)", s.vocab, ev.vocab);
    HR_REQUIRE(s.pad == ev.pad_id, "the store pads with %d, the encoder with %d", s.pad, ev.pad_id);
    HR_REQUIRE(max_len + ev.pad_id + 1 < ev.max_pos, "max_len %d exceeds the position table", max_len);
    return HIPRAG_OK;
}

// hiprerank_dev and, with cand_host set (the ids the caller also holds on the host), the body of hiprerank_host.
int32_t rerank_impl(uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens, const int32_t* q_offsets, int32_t nq, const int64_t* cand_dev,
                    const int64_t* cand_host, int32_t depth, int64_t id_base, int32_t max_len, int32_t k, int64_t max_batch_tokens,
                    float* out_logits_dev, float* out_scores_dev, int64_t* out_ids_dev, int32_t* out_pos_dev, hipStream_t st)
{
    int32_t rc;
    if ((rc = check_call(nq, k, depth, cand_dev, out_scores_dev, out_ids_dev, max_len, id_base, max_batch_tokens))) return rc;
    EncoderLease enc;   // lock order: encoder, then store
    if ((rc = enc.acquire(enc_h))) return rc;
    const EncoderView& ev = enc.view();
    GET_TOK(s, tok_h);
    std::lock_guard<std::mutex> guard(s->mu);
    if ((rc = check_handles(ev, *s, max_len))) return rc;
    int lq = 0;
    if ((rc = check_queries(q_tokens, q_offsets, nq, ev.vocab, &lq))) return rc;
    // ---- every check has passed: from here the call enqueues -----------------------------------------------------------
    const int64_t pairs = (int64_t)nq * depth;
    const int S = bound_S(*s, max_len, lq, cand_host, pairs, id_base);
    const int64_t B = max_batch_tokens ? max_batch_tokens : 131072;
    const int64_t per = std::max<int64_t>(1, B / S);
    int32_t *tok_dev = nullptr, *lens_dev = nullptr;
    const int32_t *q_off_dev = nullptr, *q_tok_dev = nullptr;
    if ((rc = enc.reserve_tokens((size_t)pairs, S, &tok_dev, &lens_dev))) return rc;
    float* logits = out_logits_dev;
    if (!logits) {
        if ((rc = s->logits.reserve((size_t)pairs * sizeof(float)))) return rc;
        logits = s->logits.as<float>();
    }
    if ((rc = stage_queries(*s, q_tokens, q_offsets, nq, st, &q_off_dev, &q_tok_dev))) return rc;
    if ((rc = launch_assemble(*s, cand_dev, pairs, depth, id_base, q_off_dev, q_tok_dev, max_len, S, tok_dev, lens_dev, st))) return rc;
    int64_t batches = 0;
    for (int64_t o = 0; o < pairs; o += per, ++batches) {
        const int n = (int)std::min(per, pairs - o);
        if ((rc = enc.score_dev(tok_dev + o * S, lens_dev + o, n, S, logits + o, st))) return rc;
    }
    hipLaunchKernelGGL(rerank_select_kernel, dim3((unsigned)nq), dim3(kMaxDepth), 0, st, cand_dev, (int)depth, id_base, (int64_t)s->csr.n_docs,
                       logits, (int)k, out_scores_dev, out_ids_dev, out_pos_dev);
    HR_CHECK_HIP(hipGetLastError());
    s->last_S = S;
    s->last_batches = batches;
    return HIPRAG_OK;
}

// ---- the packed call ---------------------------------------------------------------------------------------------------
// Steps 1 and 2: every pair's length on the device, then on the host -- ONE copy to pinned memory and ONE synchronise of `st`.
int32_t pair_lengths(TokenStore& s, const int64_t* cand_dev, int64_t pairs, int depth, int64_t id_base, const int32_t* q_off_dev,
                     int max_len, hipStream_t st, const int32_t** lens_host)
{
    int32_t rc;
    if ((rc = reserve_counters(s))) return rc;
    if ((rc = s.pk_lens.reserve((size_t)pairs * 4))) return rc;
    if ((rc = s.pk_pin_lens.reserve((size_t)pairs * 4))) return rc;
    HR_CHECK_HIP(hipMemsetAsync(s.counters.as<int32_t>() + 2, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(rerank_pair_len_kernel, dim3((unsigned)((pairs + kAsmThreads - 1) / kAsmThreads)), dim3(kAsmThreads), 0, st, cand_dev,
                       pairs, depth, id_base, (int64_t)s.csr.n_docs, (const int64_t*)s.csr.offsets.as<int64_t>(), q_off_dev, std::max(0, max_len - 4),
                       s.pk_lens.as<int32_t>(), s.counters.as<int32_t>() + 2);
    HR_CHECK_HIP(hipGetLastError());
    HR_CHECK_HIP(hipMemcpyAsync(s.pk_pin_lens.p, s.pk_lens.p, (size_t)pairs * 4, hipMemcpyDeviceToHost, st));
    HR_CHECK_HIP(hipStreamSynchronize(st));
    *lens_host = s.pk_pin_lens.as<int32_t>();
    return HIPRAG_OK;
}

// Steps 3 and 4: the pairs, in order, cut greedily into sub-batches whose packed rows stay within B (a sub-batch holds at
// least one pair), each with its own layout.  The sub-batches lie one behind the other in the token buffer.
struct PackedCut {
    int64_t first;        // first pair
    int64_t base;         // first row of the token buffer
    PackedLayout lay;
};
int32_t cut_pairs(const int32_t* lens, int64_t pairs, int64_t B, std::vector<PackedCut>& cuts, int64_t* total_rows)
{
    cuts.clear();
    int64_t rows_all = 0;
    for (int64_t o = 0; o < pairs;) {
        int64_t n = 0, rows = 0;
        while (o + n < pairs) {
            const int64_t R = round64(lens[o + n]);
            if (n > 0 && rows + R > B) break;
            rows += R;
            ++n;
        }
        cuts.emplace_back();
        PackedCut& c = cuts.back();
        c.first = o;
        c.base = rows_all;
        HR_REQUIRE(packed_layout(lens + o, (int)n, c.lay), "a sub-batch of the packed rerank has 2^30 rows or more");
        rows_all += rows;
        o += n;
    }
    *total_rows = rows_all;
    return HIPRAG_OK;
}

// Step 5: one upload of every table.  Device layout (ints): row0 [pairs] -- the first row of every pair in the token buffer --
// then per sub-batch lens | row_off | gran_seq | items.  -> the PackedBatch of every sub-batch (tok not yet set).
int32_t upload_tables(TokenStore& s, const std::vector<PackedCut>& cuts, const int32_t* lens, int64_t pairs, int32_t* tab_dev, size_t words,
                      hipStream_t st, std::vector<PackedBatch>& batches)
{
    int32_t rc;
    if (!s.pk_ev) HR_CHECK_HIP(hipEventCreateWithFlags(&s.pk_ev, hipEventDisableTiming));
    if (s.pk_used) HR_CHECK_HIP(hipEventSynchronize(s.pk_ev));   // the last call's copy out of the pinned buffer
    if ((rc = s.pk_pin_tab.reserve(words * 4))) return rc;
    int32_t* t = s.pk_pin_tab.as<int32_t>();
    size_t at = (size_t)pairs;
    batches.clear();
    for (const PackedCut& c : cuts) {
        const int n = (int)c.lay.row_off.size() - 1;
        for (int i = 0; i < n; ++i) t[c.first + i] = (int32_t)(c.base + c.lay.row_off[i]);
        PackedBatch b{};
        b.lens = tab_dev + at;
        std::copy(lens + c.first, lens + c.first + n, t + at); at += (size_t)n;
        b.row_off = tab_dev + at;
        std::copy(c.lay.row_off.begin(), c.lay.row_off.end(), t + at); at += c.lay.row_off.size();
        b.gran_seq = tab_dev + at;
        std::copy(c.lay.gran_seq.begin(), c.lay.gran_seq.end(), t + at); at += c.lay.gran_seq.size();
        b.items = tab_dev + at;
        std::copy(c.lay.items.begin(), c.lay.items.end(), t + at); at += c.lay.items.size();
        b.nseq = n; b.Tp = c.lay.Tp; b.n_items = c.lay.n_items(); b.real = c.lay.real; b.sum_r2 = c.lay.sum_r2;
        batches.push_back(b);
    }
    HR_CHECK_HIP(hipMemcpyAsync(tab_dev, t, words * 4, hipMemcpyHostToDevice, st));
    HR_CHECK_HIP(hipEventRecord(s.pk_ev, st));
    s.pk_used = true;
    return HIPRAG_OK;
}

size_t table_words(const std::vector<PackedCut>& cuts, int64_t pairs)
{
    size_t w = (size_t)pairs;
    for (const PackedCut& c : cuts) w += (c.lay.row_off.size() - 1) + c.lay.row_off.size() + c.lay.gran_seq.size() + c.lay.items.size();
    return w;
}

int32_t launch_assemble_packed(TokenStore& s, const int64_t* cand_dev, int64_t pairs, int depth, int64_t id_base, const int32_t* q_off_dev,
                               const int32_t* q_tok_dev, int max_len, const int32_t* row0_dev, int32_t* tok_dev, hipStream_t st)
{
    hipLaunchKernelGGL(rerank_assemble_packed_kernel, dim3((unsigned)pairs), dim3(kAsmThreads), 0, st, cand_dev, depth, id_base,
                       (int64_t)s.csr.n_docs, (const int64_t*)s.csr.offsets.as<int64_t>(), (const int32_t*)s.tokens.as<int32_t>(), q_off_dev, q_tok_dev,
                       std::max(0, max_len - 4), (int)s.bos, (int)s.eos, (int)s.pad, (const int32_t*)s.pk_lens.as<int32_t>(), row0_dev, tok_dev);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

// hiprerank_packed_dev, and the body of hiprerank_packed_host
int32_t rerank_packed_impl(uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens, const int32_t* q_offsets, int32_t nq,
                           const int64_t* cand_dev, int32_t depth, int64_t id_base, int32_t max_len, int32_t k, int64_t max_batch_tokens,
                           float* out_logits_dev, float* out_scores_dev, int64_t* out_ids_dev, int32_t* out_pos_dev, hipStream_t st)
{
    int32_t rc;
    if ((rc = check_call(nq, k, depth, cand_dev, out_scores_dev, out_ids_dev, max_len, id_base, max_batch_tokens))) return rc;
    EncoderLease enc;   // lock order: encoder, then store
    if ((rc = enc.acquire(enc_h))) return rc;
    const EncoderView& ev = enc.view();
    GET_TOK(s, tok_h);
    std::lock_guard<std::mutex> guard(s->mu);
    if ((rc = check_handles(ev, *s, max_len))) return rc;
    int lq = 0;
    if ((rc = check_queries(q_tokens, q_offsets, nq, ev.vocab, &lq))) return rc;
    const int64_t pairs = (int64_t)nq * depth;
    HR_REQUIRE(pairs * round64(max_len) < ((int64_t)1 << 31), "nq * depth pairs of up to %d tokens pass 2^31 token rows", max_len);
    // ---- every check has passed: from here the call enqueues -----------------------------------------------------------
    const int64_t B = max_batch_tokens ? max_batch_tokens : 131072;
    const int32_t *q_off_dev = nullptr, *q_tok_dev = nullptr, *lens_host = nullptr;
    float* logits = out_logits_dev;
    if (!logits) {
        if ((rc = s->logits.reserve((size_t)pairs * sizeof(float)))) return rc;
        logits = s->logits.as<float>();
    }
    if ((rc = stage_queries(*s, q_tokens, q_offsets, nq, st, &q_off_dev, &q_tok_dev))) return rc;
    if ((rc = pair_lengths(*s, cand_dev, pairs, depth, id_base, q_off_dev, max_len, st, &lens_host))) return rc;
    std::vector<PackedCut> cuts;
    std::vector<PackedBatch> batches;
    int64_t rows = 0;
    if ((rc = cut_pairs(lens_host, pairs, B, cuts, &rows))) return rc;
    const size_t words = table_words(cuts, pairs);
    int32_t *tok_dev = nullptr, *tab_dev = nullptr;
    if ((rc = enc.reserve_packed((size_t)rows, words, &tok_dev, &tab_dev))) return rc;
    for (const PackedCut& c : cuts)   // the workspace of the largest sub-batch before the first one runs: no buffer grows under a forward
        if ((rc = enc.reserve_packed_work(c.lay.Tp))) return rc;
    if ((rc = upload_tables(*s, cuts, lens_host, pairs, tab_dev, words, st, batches))) return rc;
    if ((rc = launch_assemble_packed(*s, cand_dev, pairs, depth, id_base, q_off_dev, q_tok_dev, max_len, tab_dev, tok_dev, st))) return rc;
    for (size_t b = 0; b < batches.size(); ++b) {
        batches[b].tok = tok_dev + cuts[b].base;
        if ((rc = enc.score_packed_dev(batches[b], logits + cuts[b].first, st))) return rc;
    }
    hipLaunchKernelGGL(rerank_select_kernel, dim3((unsigned)nq), dim3(kMaxDepth), 0, st, cand_dev, (int)depth, id_base, (int64_t)s->csr.n_docs,
                       logits, (int)k, out_scores_dev, out_ids_dev, out_pos_dev);
    HR_CHECK_HIP(hipGetLastError());
    s->pk_rows = rows;
    s->pk_batches = (int64_t)batches.size();
    return HIPRAG_OK;
}

}  // namespace
}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hiprerank_dev(uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                      const int64_t* cand_ids_dev, int32_t depth, int64_t id_base, int32_t max_len, int32_t k, int64_t max_batch_tokens,
                      float* out_logits_dev, float* out_scores_dev, int64_t* out_ids_dev, int32_t* out_pos_dev, void* stream)
{
    return rerank_impl(enc_h, tok_h, q_tokens_host, q_offsets_host, nq, cand_ids_dev, nullptr, depth, id_base, max_len, k, max_batch_tokens,
                       out_logits_dev, out_scores_dev, out_ids_dev, out_pos_dev, (hipStream_t)stream);
}

// hiprerank_host and hiprerank_packed_host: candidates and outputs in host memory around the device call
static int32_t rerank_host_call(bool packed, uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host,
                                int32_t nq, const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t max_len, int32_t k,
                                int64_t max_batch_tokens, float* out_logits, float* out_scores, int64_t* out_ids, int32_t* out_pos)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(1 <= k && k <= depth && depth <= kMaxDepth, "1 <= k <= depth <= %d does not hold (k = %d, depth = %d)", kMaxDepth, k, depth);
    HR_REQUIRE(cand_ids_host && out_scores && out_ids, "null argument");
    {
        GET_TOK(s, tok_h);
        HR_CHECK_HIP(hipSetDevice(s->device));
    }
    const size_t pairs = (size_t)nq * depth, nk = (size_t)nq * k;
    DevBuf cand, lg, os, oi, op;
    int32_t rc;
    if ((rc = cand.reserve(pairs * 8)) || (rc = lg.reserve(pairs * 4)) || (rc = os.reserve(nk * 4)) || (rc = oi.reserve(nk * 8)) ||
        (rc = op.reserve(nk * 4)))
        return rc;
    HR_CHECK_HIP(hipMemcpy(cand.p, cand_ids_host, pairs * 8, hipMemcpyHostToDevice));
    rc = packed ? rerank_packed_impl(enc_h, tok_h, q_tokens_host, q_offsets_host, nq, cand.as<int64_t>(), depth, id_base, max_len, k,
                                     max_batch_tokens, lg.as<float>(), os.as<float>(), oi.as<int64_t>(), op.as<int32_t>(), nullptr)
                : rerank_impl(enc_h, tok_h, q_tokens_host, q_offsets_host, nq, cand.as<int64_t>(), cand_ids_host, depth, id_base, max_len, k,
                              max_batch_tokens, lg.as<float>(), os.as<float>(), oi.as<int64_t>(), op.as<int32_t>(), nullptr);
    if (rc) { (void)hipDeviceSynchronize(); return rc; }   // whatever was enqueued is done before the frame's buffers go
    if (out_logits) HR_CHECK_HIP(hipMemcpy(out_logits, lg.p, pairs * 4, hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_scores, os.p, nk * 4, hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_ids, oi.p, nk * 8, hipMemcpyDeviceToHost));
    if (out_pos) HR_CHECK_HIP(hipMemcpy(out_pos, op.p, nk * 4, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hiprerank_host(uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                  const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t max_len, int32_t k, int64_t max_batch_tokens,
                  float* out_logits, float* out_scores, int64_t* out_ids, int32_t* out_pos)
{
    return rerank_host_call(false, enc_h, tok_h, q_tokens_host, q_offsets_host, nq, cand_ids_host, depth, id_base, max_len, k,
                            max_batch_tokens, out_logits, out_scores, out_ids, out_pos);
}

int32_t hiprerank_packed_dev(uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                             const int64_t* cand_ids_dev, int32_t depth, int64_t id_base, int32_t max_len, int32_t k,
                             int64_t max_batch_tokens, float* out_logits_dev, float* out_scores_dev, int64_t* out_ids_dev,
                             int32_t* out_pos_dev, void* stream)
{
    return rerank_packed_impl(enc_h, tok_h, q_tokens_host, q_offsets_host, nq, cand_ids_dev, depth, id_base, max_len, k, max_batch_tokens,
                              out_logits_dev, out_scores_dev, out_ids_dev, out_pos_dev, (hipStream_t)stream);
}

int32_t hiprerank_packed_host(uint64_t enc_h, uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                              const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t max_len, int32_t k,
                              int64_t max_batch_tokens, float* out_logits, float* out_scores, int64_t* out_ids, int32_t* out_pos)
{
    return rerank_host_call(true, enc_h, tok_h, q_tokens_host, q_offsets_host, nq, cand_ids_host, depth, id_base, max_len, k,
                            max_batch_tokens, out_logits, out_scores, out_ids, out_pos);
}

int32_t hiprerank_packed_info(uint64_t tok_h, int64_t* out4)
{
    HR_REQUIRE(out4, "null out");
    GET_TOK(s, tok_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_CHECK_HIP(hipDeviceSynchronize());
    int32_t c[4] = {0, 0, 0, 0};
    if (s->counters.p) HR_CHECK_HIP(hipMemcpy(c, s->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    out4[0] = c[2];
    out4[1] = c[3];
    out4[2] = s->pk_rows;
    out4[3] = s->pk_batches;
    return HIPRAG_OK;
}

int32_t hiprerank_assemble_packed(uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                                  const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t max_len,
                                  int32_t* out_tokens_host, int32_t* out_row_off_host, int32_t* out_lens_host, int32_t* out_Tp)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(1 <= depth && depth <= kMaxDepth, "depth must be in 1..%d (got %d)", kMaxDepth, depth);
    HR_REQUIRE(cand_ids_host && out_tokens_host && out_row_off_host && out_lens_host && out_Tp, "null argument");
    HR_REQUIRE(max_len >= 5, "max_len must be at least 5 (got %d): four special tokens and one of text", max_len);
    HR_REQUIRE(id_base >= 0, "id_base must not be negative (got %lld)", (long long)id_base);
    GET_TOK(s, tok_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    int lq = 0;
    int32_t rc;
    if ((rc = check_queries(q_tokens_host, q_offsets_host, nq, s->vocab, &lq))) return rc;
    const int64_t pairs = (int64_t)nq * depth;
    HR_REQUIRE(pairs * round64(max_len) < ((int64_t)1 << 30), "too many rows for the hook");
    DevBuf cand, tok, tab;
    if ((rc = cand.reserve((size_t)pairs * 8))) return rc;
    HR_CHECK_HIP(hipMemcpy(cand.p, cand_ids_host, (size_t)pairs * 8, hipMemcpyHostToDevice));
    const int32_t *q_off_dev = nullptr, *q_tok_dev = nullptr, *lens_host = nullptr;
    std::vector<PackedCut> cuts;
    std::vector<PackedBatch> batches;
    int64_t rows = 0;
    rc = stage_queries(*s, q_tokens_host, q_offsets_host, nq, nullptr, &q_off_dev, &q_tok_dev);
    if (!rc) rc = pair_lengths(*s, cand.as<int64_t>(), pairs, depth, id_base, q_off_dev, max_len, nullptr, &lens_host);
    if (!rc) rc = cut_pairs(lens_host, pairs, (int64_t)1 << 30, cuts, &rows);   // ONE layout over all the pairs
    const size_t words = rc ? 0 : table_words(cuts, pairs);
    if (!rc) rc = tok.reserve((size_t)rows * 4);
    if (!rc) rc = tab.reserve(words * 4);
    if (!rc) rc = upload_tables(*s, cuts, lens_host, pairs, tab.as<int32_t>(), words, nullptr, batches);
    if (!rc) rc = launch_assemble_packed(*s, cand.as<int64_t>(), pairs, depth, id_base, q_off_dev, q_tok_dev, max_len, tab.as<int32_t>(),
                                         tok.as<int32_t>(), nullptr);
    if (rc) { (void)hipDeviceSynchronize(); return rc; }
    HR_CHECK_HIP(hipMemcpy(out_tokens_host, tok.p, (size_t)rows * 4, hipMemcpyDeviceToHost));
    std::copy(cuts[0].lay.row_off.begin(), cuts[0].lay.row_off.end(), out_row_off_host);
    std::copy(lens_host, lens_host + pairs, out_lens_host);
    s->pk_rows = rows;
    s->pk_batches = 0;
    *out_Tp = (int32_t)rows;
    return HIPRAG_OK;
}

int32_t hiprerank_info(uint64_t tok_h, int64_t* out4)
{
    HR_REQUIRE(out4, "null out");
    GET_TOK(s, tok_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_CHECK_HIP(hipDeviceSynchronize());
    int32_t c[2] = {0, 0};
    if (s->counters.p) HR_CHECK_HIP(hipMemcpy(c, s->counters.p, sizeof(c), hipMemcpyDeviceToHost));
    out4[0] = c[0];
    out4[1] = c[1];
    out4[2] = s->last_S;
    out4[3] = s->last_batches;
    return HIPRAG_OK;
}

int32_t hiprerank_assemble(uint64_t tok_h, const int32_t* q_tokens_host, const int32_t* q_offsets_host, int32_t nq,
                           const int64_t* cand_ids_host, int32_t depth, int64_t id_base, int32_t max_len, int32_t* out_tokens_host,
                           int32_t* out_lens_host, int32_t* out_S)
{
    HR_REQUIRE(nq >= 1, "nq must be at least 1 (got %d)", nq);
    HR_REQUIRE(1 <= depth && depth <= kMaxDepth, "depth must be in 1..%d (got %d)", kMaxDepth, depth);
    HR_REQUIRE(cand_ids_host && out_tokens_host && out_lens_host && out_S, "null argument");
    HR_REQUIRE(max_len >= 5, "max_len must be at least 5 (got %d): four special tokens and one of text", max_len);
    HR_REQUIRE(id_base >= 0, "id_base must not be negative (got %lld)", (long long)id_base);
    GET_TOK(s, tok_h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    int lq = 0;
    int32_t rc;
    if ((rc = check_queries(q_tokens_host, q_offsets_host, nq, s->vocab, &lq))) return rc;
    const int64_t pairs = (int64_t)nq * depth;
    const int S = bound_S(*s, max_len, lq, nullptr, 0, id_base);   // the store-wide bound, as hiprerank_dev has it
    DevBuf cand, tok, lens;
    if ((rc = cand.reserve((size_t)pairs * 8)) || (rc = tok.reserve((size_t)pairs * S * 4)) || (rc = lens.reserve((size_t)pairs * 4))) return rc;
    HR_CHECK_HIP(hipMemcpy(cand.p, cand_ids_host, (size_t)pairs * 8, hipMemcpyHostToDevice));
    const int32_t *q_off_dev = nullptr, *q_tok_dev = nullptr;
    rc = stage_queries(*s, q_tokens_host, q_offsets_host, nq, nullptr, &q_off_dev, &q_tok_dev);
    if (!rc) rc = launch_assemble(*s, cand.as<int64_t>(), pairs, depth, id_base, q_off_dev, q_tok_dev, max_len, S, tok.as<int32_t>(),
                                  lens.as<int32_t>(), nullptr);
    if (rc) { (void)hipDeviceSynchronize(); return rc; }
    HR_CHECK_HIP(hipMemcpy(out_tokens_host, tok.p, (size_t)pairs * S * 4, hipMemcpyDeviceToHost));
    HR_CHECK_HIP(hipMemcpy(out_lens_host, lens.p, (size_t)pairs * 4, hipMemcpyDeviceToHost));
    s->last_S = S;
    s->last_batches = 0;
    *out_S = S;
    return HIPRAG_OK;
}

}  // extern "C"
