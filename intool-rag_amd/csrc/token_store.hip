// token_store.hip -- the passage token store (hiptok_*, include/hiprag.h): a device-resident CSR of the token ids of every
// chunk of a collection, document i = collection row i, bodies only.  It is what the device rerank call (rerank.hip) builds
// its `<s> q </s></s> p </s>` pairs from, so that a query is reranked without tokenising a passage again.  It follows the
// collection as rows, IVF lists and postings do: append at the end, stable compaction on removal.
#include <algorithm>
#include <cstring>

#include "token_store.h"

namespace hiprag {

Registry<TokenStore>& tok_reg()
{
    static Registry<TokenStore> r;
    return r;
}
size_t clear_token_registry() { return tok_reg().clear(); }

namespace {

constexpr int kMoveThreads = 256;
constexpr int64_t kMoveChunk = 32ll << 20;   // elements per pass of a removal: 128 MiB of staging whatever the store holds

// stage[i - d0] = data[source of destination element i], d0 <= i < d1.  One thread per element; the run is found by bisection.
__global__ __launch_bounds__(kMoveThreads) void tok_gather_kernel(const int32_t* __restrict__ tokens, const MoveRun* __restrict__ moves,
                                                                  int n_moves, int64_t d0, int64_t d1, int32_t* __restrict__ stage)
{
    const int64_t i = d0 + (int64_t)blockIdx.x * kMoveThreads + threadIdx.x;
    if (i >= d1) return;
    int lo = 0, hi = n_moves - 1;   // the last run with dst <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (moves[mid].dst <= i) lo = mid; else hi = mid - 1;
    }
    const MoveRun m = moves[lo];
    stage[i - d0] = tokens[m.src + (i - m.dst)];
}

int64_t grown(int64_t need, int64_t cap) { return std::max(need, cap + cap / 2); }

// a larger buffer with the first `keep` bytes of the old one
int32_t regrow(DevBuf& buf, size_t bytes, size_t keep)
{
    DevBuf nb;
    int32_t rc;
    if ((rc = nb.reserve(bytes))) return rc;
    if (keep) HR_CHECK_HIP(hipMemcpy(nb.p, buf.p, keep, hipMemcpyDeviceToDevice));
    std::swap(nb.p, buf.p);
    std::swap(nb.bytes, buf.bytes);
    return HIPRAG_OK;
}

}  // namespace

int32_t move_runs_down_i32(int32_t* data, const std::vector<MoveRun>& moves, int64_t d_begin, int64_t d_end)
{
    if (moves.empty() || d_end <= d_begin) return HIPRAG_OK;
    int32_t rc;
    DevBuf moves_dev, stage;       // freed behind the synchronisation below
    if ((rc = moves_dev.reserve(moves.size() * sizeof(MoveRun)))) return rc;
    if ((rc = stage.reserve((size_t)std::min(kMoveChunk, d_end - d_begin) * sizeof(int32_t)))) return rc;
    HR_CHECK_HIP(hipMemcpy(moves_dev.p, moves.data(), moves.size() * sizeof(MoveRun), hipMemcpyHostToDevice));
    // Every element moves DOWN (dst <= src), so the sources of the destinations behind a chunk lie behind that chunk too:
    // chunks in ascending order, each gathered into the staging buffer and copied into place, never overwrite a source.
    for (int64_t d0 = d_begin; d0 < d_end; d0 += kMoveChunk) {
        const int64_t d1 = std::min(d_end, d0 + kMoveChunk);
        hipLaunchKernelGGL(tok_gather_kernel, dim3((unsigned)((d1 - d0 + kMoveThreads - 1) / kMoveThreads)), dim3(kMoveThreads), 0,
                           nullptr, (const int32_t*)data, (const MoveRun*)moves_dev.as<MoveRun>(), (int)moves.size(), d0, d1,
                           stage.as<int32_t>());
        HR_CHECK_HIP(hipGetLastError());
        HR_CHECK_HIP(hipMemcpyAsync(data + d0, stage.p, (size_t)(d1 - d0) * sizeof(int32_t), hipMemcpyDeviceToDevice, nullptr));
    }
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    return HIPRAG_OK;
}

}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hiptok_create(int32_t vocab, int32_t bos, int32_t eos, int32_t pad, int32_t max_doc_tokens, int32_t device,
                      uint64_t* out_handle)
{
    HR_REQUIRE(out_handle, "null out");
    HR_REQUIRE(vocab > 0, "vocab must be positive (got %d)", vocab);
    HR_REQUIRE(bos >= 0 && bos < vocab && eos >= 0 && eos < vocab && pad >= 0 && pad < vocab,
               "bos %d, eos %d and pad %d must lie in [0, vocab = %d)", bos, eos, pad, vocab);
    HR_REQUIRE(max_doc_tokens >= 1, "max_doc_tokens must be at least 1 (got %d)", max_doc_tokens);
    HR_CHECK_HIP(hipSetDevice(device));
    auto s = std::make_shared<TokenStore>();
    s->device = device;
    s->vocab = vocab; s->bos = bos; s->eos = eos; s->pad = pad; s->max_doc_tokens = max_doc_tokens;
    int32_t rc;
    if ((rc = s->offsets.reserve(sizeof(int64_t)))) return rc;   // offsets[0] = 0 exists from the start
    HR_CHECK_HIP(hipMemset(s->offsets.p, 0, sizeof(int64_t)));
    *out_handle = tok_reg().put(s);
    return HIPRAG_OK;
}

int32_t hiptok_destroy(uint64_t h)
{
    GET_TOK(s, h);
    {
        std::lock_guard<std::mutex> guard(s->mu);
        (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();
    }
    tok_reg().erase(h);
    return HIPRAG_OK;
}

int32_t hiptok_append(uint64_t h, const int32_t* tokens_host, const int64_t* offsets_host, int64_t n_docs)
{
    GET_TOK(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    // every check before anything is touched
    HR_REQUIRE(n_docs >= 0, "n_docs must not be negative (got %lld)", (long long)n_docs);
    HR_REQUIRE(offsets_host, "offsets is null");
    HR_REQUIRE(offsets_host[0] == 0, "offsets must start at 0 (got %lld)", (long long)offsets_host[0]);
    for (int64_t i = 0; i < n_docs; ++i)
        HR_REQUIRE(offsets_host[i] <= offsets_host[i + 1], "offsets descend at document %lld", (long long)i);
    const int64_t total = offsets_host[n_docs];
    HR_REQUIRE(tokens_host || total == 0, "tokens is null");
    for (int64_t t = 0; t < total; ++t)
        HR_REQUIRE(tokens_host[t] >= 0 && tokens_host[t] < s->vocab, "token %lld = %d lies outside [0, vocab = %d)", (long long)t,
                   tokens_host[t], s->vocab);
    HR_REQUIRE(s->n_docs + n_docs < (1ll << 31), "the store would hold %lld documents: the limit is 2^31 - 1",
               (long long)(s->n_docs + n_docs));
    if (n_docs == 0) return HIPRAG_OK;
    // the batch as it is stored: every document cut to the cap
    std::vector<int64_t> off((size_t)n_docs + 1);
    std::vector<int32_t> lens((size_t)n_docs);
    std::vector<int32_t> body;
    body.reserve((size_t)std::min<int64_t>(total, n_docs * (int64_t)s->max_doc_tokens));
    off[0] = s->n_tokens;
    int32_t longest = s->longest;
    for (int64_t i = 0; i < n_docs; ++i) {
        const int64_t len = std::min<int64_t>(offsets_host[i + 1] - offsets_host[i], s->max_doc_tokens);
        body.insert(body.end(), tokens_host + offsets_host[i], tokens_host + offsets_host[i] + len);
        lens[(size_t)i] = (int32_t)len;
        off[(size_t)i + 1] = off[(size_t)i] + len;
        longest = std::max(longest, (int32_t)len);
    }
    const int64_t docs_after = s->n_docs + n_docs, tokens_after = off[(size_t)n_docs];
    int32_t rc;
    if (docs_after > s->cap_docs) {
        const int64_t cap = grown(docs_after, s->cap_docs);
        if ((rc = regrow(s->offsets, (size_t)(cap + 1) * sizeof(int64_t), (size_t)(s->n_docs + 1) * sizeof(int64_t)))) return rc;
        s->cap_docs = cap;
    }
    if (tokens_after > s->cap_tokens) {
        const int64_t cap = grown(tokens_after, s->cap_tokens);
        if ((rc = regrow(s->tokens, (size_t)cap * sizeof(int32_t), (size_t)s->n_tokens * sizeof(int32_t)))) return rc;
        s->cap_tokens = cap;
    }
    if (!body.empty())
        HR_CHECK_HIP(hipMemcpy(s->tokens.as<int32_t>() + s->n_tokens, body.data(), body.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HR_CHECK_HIP(hipMemcpy(s->offsets.as<int64_t>() + s->n_docs, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    s->len_host.insert(s->len_host.end(), lens.begin(), lens.end());
    s->n_docs = docs_after;
    s->n_tokens = tokens_after;
    s->longest = longest;
    return HIPRAG_OK;
}

int32_t hiptok_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges)
{
    GET_TOK(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_REQUIRE(n_ranges >= 0, "n_ranges must not be negative (got %d)", n_ranges);
    HR_REQUIRE(ranges_host || n_ranges == 0, "ranges is null");
    std::vector<std::pair<int64_t, int64_t>> tab;   // non-empty ranges, touching ones joined
    for (int j = 0; j < n_ranges; ++j) {
        const int64_t lo = ranges_host[2 * j], hi = ranges_host[2 * j + 1];
        HR_REQUIRE(0 <= lo && lo <= hi && hi <= s->n_docs, "ranges[%d] = [%lld, %lld) is not within 0 <= lo <= hi <= n_docs = %lld", j,
                   (long long)lo, (long long)hi, (long long)s->n_docs);
        HR_REQUIRE(j == 0 || lo >= ranges_host[2 * j - 1], "ranges[%d] = [%lld, %lld) starts before the end %lld of the range before it: "
                   "the ranges ascend and do not overlap", j, (long long)lo, (long long)hi, (long long)ranges_host[2 * j - 1]);
        if (hi == lo) continue;
        if (!tab.empty() && tab.back().second == lo) tab.back().second = hi;
        else tab.emplace_back(lo, hi);
    }
    if (tab.empty()) return HIPRAG_OK;
    // The host knows every length, so it knows where every surviving run of tokens lies and where it goes.  Offsets of the
    // documents behind the first removed one are written from the host; the tokens themselves move on the device.
    const int64_t first = tab[0].first;
    int64_t t_first = 0;
    for (int64_t i = 0; i < first; ++i) t_first += s->len_host[(size_t)i];
    std::vector<MoveRun> moves;
    std::vector<int64_t> off;          // new offsets of the documents first .. n_new
    std::vector<int32_t> lens_after(s->len_host.begin(), s->len_host.begin() + first);
    off.push_back(t_first);
    int64_t src = t_first, dst = t_first;
    int32_t longest = 0;
    for (size_t j = 0; j < tab.size(); ++j) {
        for (int64_t i = tab[j].first; i < tab[j].second; ++i) src += s->len_host[(size_t)i];   // removed: skipped
        const int64_t keep_hi = j + 1 < tab.size() ? tab[j + 1].first : s->n_docs;
        int64_t run = 0;
        for (int64_t i = tab[j].second; i < keep_hi; ++i) {
            const int32_t len = s->len_host[(size_t)i];
            run += len;
            lens_after.push_back(len);
            off.push_back(dst + run);
        }
        if (run > 0) moves.push_back(MoveRun{src, dst, run});
        src += run;
        dst += run;
    }
    for (int32_t len : lens_after) longest = std::max(longest, len);
    const int64_t tokens_after = dst, n_after = (int64_t)lens_after.size();
    int32_t rc;
    if ((rc = move_runs_down_i32(s->tokens.as<int32_t>(), moves, t_first, tokens_after))) return rc;
    HR_CHECK_HIP(hipMemcpy(s->offsets.as<int64_t>() + first, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    s->len_host.swap(lens_after);
    s->n_docs = n_after;
    s->n_tokens = tokens_after;
    s->longest = longest;
    return HIPRAG_OK;
}

int32_t hiptok_export(uint64_t h, int64_t* offsets, int32_t* tokens)
{
    GET_TOK(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    if (offsets) HR_CHECK_HIP(hipMemcpy(offsets, s->offsets.p, (size_t)(s->n_docs + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (tokens && s->n_tokens) HR_CHECK_HIP(hipMemcpy(tokens, s->tokens.p, (size_t)s->n_tokens * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hiptok_sizes(uint64_t h, int64_t* out4)
{
    HR_REQUIRE(out4, "null out");
    GET_TOK(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    out4[0] = s->n_docs;
    out4[1] = s->n_tokens;
    out4[2] = s->max_doc_tokens;
    out4[3] = s->longest;
    return HIPRAG_OK;
}

}  // extern "C"
