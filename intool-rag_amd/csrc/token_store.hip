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
    s->vocab = vocab; s->bos = bos; s->eos = eos; s->pad = pad;
    int32_t rc;
    if ((rc = s->csr.init(max_doc_tokens))) return rc;
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
    DocCsr& c = s->csr;
    HR_REQUIRE(c.n_docs + n_docs < (1ll << 31), "the store would hold %lld documents: the limit is 2^31 - 1",
               (long long)(c.n_docs + n_docs));
    if (n_docs == 0) return HIPRAG_OK;
    // the batch as it is stored: every document cut to the cap
    std::vector<int64_t> off;
    std::vector<int32_t> lens;
    c.plan_append(n_docs, [&](int64_t i) { return offsets_host[i + 1] - offsets_host[i]; }, off, lens);
    std::vector<int32_t> body;
    body.reserve((size_t)(off.back() - c.n_items));
    for (int64_t i = 0; i < n_docs; ++i)
        body.insert(body.end(), tokens_host + offsets_host[i], tokens_host + offsets_host[i] + lens[(size_t)i]);
    int32_t rc;
    if ((rc = c.ensure_capacity(s->parts(), c.n_docs + n_docs, off.back()))) return rc;
    if (!body.empty())
        HR_CHECK_HIP(hipMemcpy(s->tokens.as<int32_t>() + c.n_items, body.data(), body.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = c.write_offsets(off))) return rc;
    c.commit_append(off, lens);
    return HIPRAG_OK;
}

int32_t hiptok_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges)
{
    GET_TOK(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    RangeTable tab;
    int32_t rc;
    if ((rc = range_table(ranges_host, n_ranges, s->csr.n_docs, "n_docs", true, tab))) return rc;
    if (tab.empty()) return HIPRAG_OK;
    // Offsets of the documents behind the first removed one are written from the host; the tokens themselves move on the device.
    return s->csr.remove(s->parts(), tab);
}

int32_t hiptok_export(uint64_t h, int64_t* offsets, int32_t* tokens)
{
    GET_TOK(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    if (offsets) HR_CHECK_HIP(hipMemcpy(offsets, s->csr.offsets.p, (size_t)(s->csr.n_docs + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (tokens && s->csr.n_items) HR_CHECK_HIP(hipMemcpy(tokens, s->tokens.p, (size_t)s->csr.n_items * sizeof(int32_t), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hiptok_sizes(uint64_t h, int64_t* out4)
{
    HR_REQUIRE(out4, "null out");
    GET_TOK(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    out4[0] = s->csr.n_docs;
    out4[1] = s->csr.n_items;
    out4[2] = s->csr.doc_cap;
    out4[3] = s->csr.longest;
    return HIPRAG_OK;
}

}  // extern "C"
