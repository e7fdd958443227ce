// multivec.hip -- the multi-vector store (hipmv_*, include/hiprag.h): a device-resident CSR of the per-token (ColBERT)
// vectors of every chunk of a collection, document i = collection row i: offsets int64 [docs + 1], vecs bf16 [stored][dim].
// It is what the late-interaction call (maxsim.hip) scores candidates from.  It follows the collection as rows, IVF lists,
// postings, passage tokens and pages do -- append at the end, stable compaction on removal -- under the rules of the token
// store (token_store.hip), whose mover it shares.  Unlike tokens, these vectors cannot be rebuilt without encoding the
// collection again: the store has a file (HIPMV001).
#include <algorithm>
#include <cstring>

#include "multivec.h"
#include "token_store.h"

namespace hiprag {

Registry<MultiVecStore>& mv_reg()
{
    static Registry<MultiVecStore> r;
    return r;
}
size_t clear_multivec_registry() { return mv_reg().clear(); }

namespace {

constexpr int kPackThreads = 64;
constexpr int kMaxDim = 1024;
constexpr size_t kIoChunk = 64u << 20;   // bytes of host staging for save / load
constexpr char kMagic[8] = {'H', 'I', 'P', 'M', 'V', '0', '0', '1'};
constexpr int32_t kVersion = 1;

// One workgroup per stored vector v0 <= v < v1 of the batch: its document is the last one of the batch with off[doc] <= v
// (`off` = the store's offsets from the first new document on, n_docs + 1 entries, already final), its source row
// src[doc][v - off[doc]].  16 bytes per thread and step.
__global__ __launch_bounds__(kPackThreads) void mv_pack_kernel(const uint4* __restrict__ src, int64_t row_stride, int pieces,
                                                               const int64_t* __restrict__ off, int64_t n_docs, int64_t v0,
                                                               uint4* __restrict__ vecs)
{
    const int64_t v = v0 + blockIdx.x;
    int64_t lo = 0, hi = n_docs - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid - 1;
    }
    const uint4* s = src + (lo * row_stride + (v - off[lo])) * pieces;
    uint4* d = vecs + v * pieces;
    for (int p = threadIdx.x; p < pieces; p += kPackThreads) d[p] = s[p];
}

int64_t grown(int64_t need, int64_t cap) { return std::max(need, cap + cap / 2); }

// a larger buffer with the first `keep` bytes of the old one; HIPRAG_E_NOMEM leaves the old one in place
int32_t regrow(DevBuf& buf, size_t bytes, size_t keep)
{
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        set_error("out of device memory growing the multi-vector store to %zu bytes", bytes);
        return HIPRAG_E_NOMEM;
    }
    HR_CHECK_HIP(e);
    if (keep) {
        const hipError_t c = hipMemcpy(p, buf.p, keep, hipMemcpyDeviceToDevice);
        if (c != hipSuccess) { (void)hipFree(p); HR_CHECK_HIP(c); }
    }
    if (buf.p) (void)hipFree(buf.p);
    buf.p = p;
    buf.bytes = bytes;
    return HIPRAG_OK;
}

// room for docs_after documents and vecs_after vectors; the contents stay
int32_t ensure_capacity(MultiVecStore& s, int64_t docs_after, int64_t vecs_after)
{
    int32_t rc;
    if (docs_after > s.cap_docs) {
        const int64_t cap = grown(docs_after, s.cap_docs);
        if ((rc = regrow(s.offsets, (size_t)(cap + 1) * sizeof(int64_t), (size_t)(s.n_docs + 1) * sizeof(int64_t)))) return rc;
        s.cap_docs = cap;
    }
    if (vecs_after > s.cap_vecs) {
        const int64_t cap = grown(vecs_after, s.cap_vecs);
        if ((rc = regrow(s.vecs, (size_t)cap * s.dim * 2, (size_t)s.n_vecs * s.dim * 2))) return rc;
        s.cap_vecs = cap;
    }
    return HIPRAG_OK;
}

int32_t check_shape(int32_t dim, int32_t max_doc_vectors)
{
    HR_REQUIRE(dim >= 64 && dim <= kMaxDim && dim % 64 == 0, "dim must be a multiple of 64 in 64..%d (got %d)", kMaxDim, dim);
    HR_REQUIRE(max_doc_vectors >= 1, "max_doc_vectors must be at least 1 (got %d)", max_doc_vectors);
    return HIPRAG_OK;
}

int32_t new_store(int32_t dim, int32_t max_doc_vectors, int32_t device, std::shared_ptr<MultiVecStore>* out)
{
    HR_CHECK_HIP(hipSetDevice(device));
    auto s = std::make_shared<MultiVecStore>();
    s->device = device;
    s->dim = dim;
    s->max_doc_vectors = max_doc_vectors;
    int32_t rc;
    if ((rc = s->offsets.reserve(sizeof(int64_t)))) return rc;   // offsets[0] = 0 exists from the start
    HR_CHECK_HIP(hipMemset(s->offsets.p, 0, sizeof(int64_t)));
    *out = s;
    return HIPRAG_OK;
}

// The bookkeeping of an append whose vectors are already in place behind the stored ones: `lens` are the stored lengths.
int32_t commit_append(MultiVecStore& s, const std::vector<int64_t>& off, const std::vector<int32_t>& lens)
{
    s.len_host.insert(s.len_host.end(), lens.begin(), lens.end());
    for (int32_t l : lens) s.longest = std::max(s.longest, l);
    s.n_docs += (int64_t)lens.size();
    s.n_vecs = off.back();
    return HIPRAG_OK;
}

struct FileCloser {
    FILE* f;
    ~FileCloser() { if (f) fclose(f); }
};

}  // namespace
}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipmv_create(int32_t dim, int32_t max_doc_vectors, int32_t device, uint64_t* out_handle)
{
    HR_REQUIRE(out_handle, "null out");
    int32_t rc;
    if ((rc = check_shape(dim, max_doc_vectors))) return rc;
    std::shared_ptr<MultiVecStore> s;
    if ((rc = new_store(dim, max_doc_vectors, device, &s))) return rc;
    *out_handle = mv_reg().put(s);
    return HIPRAG_OK;
}

int32_t hipmv_destroy(uint64_t h)
{
    GET_MV(s, h);
    {
        std::lock_guard<std::mutex> guard(s->mu);
        (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();
    }
    mv_reg().erase(h);
    return HIPRAG_OK;
}

int32_t hipmv_append_dev(uint64_t h, const void* vecs_dev, int32_t row_stride, const int32_t* counts_host, int64_t n_docs,
                         void* stream)
{
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    // every check before anything is touched
    HR_REQUIRE(n_docs >= 0, "n_docs must not be negative (got %lld)", (long long)n_docs);
    HR_REQUIRE(row_stride >= 1, "row_stride must be at least 1 (got %d)", row_stride);
    HR_REQUIRE(counts_host || n_docs == 0, "counts is null");
    HR_REQUIRE(vecs_dev || n_docs == 0, "vecs is null");
    HR_REQUIRE(((uintptr_t)vecs_dev & 15) == 0, "vecs must be aligned to 16 bytes");
    for (int64_t i = 0; i < n_docs; ++i)
        HR_REQUIRE(counts_host[i] >= 0 && counts_host[i] <= row_stride, "counts[%lld] = %d lies outside [0, row_stride = %d]",
                   (long long)i, counts_host[i], row_stride);
    HR_REQUIRE(s->n_docs + n_docs < (1ll << 31), "the store would hold %lld documents: the limit is 2^31 - 1",
               (long long)(s->n_docs + n_docs));
    if (n_docs == 0) return HIPRAG_OK;
    std::vector<int64_t> off((size_t)n_docs + 1);
    std::vector<int32_t> lens((size_t)n_docs);
    off[0] = s->n_vecs;
    for (int64_t i = 0; i < n_docs; ++i) {
        lens[(size_t)i] = std::min(counts_host[i], s->max_doc_vectors);
        off[(size_t)i + 1] = off[(size_t)i] + lens[(size_t)i];
    }
    const int64_t added = off[(size_t)n_docs] - s->n_vecs;
    int32_t rc;
    if ((rc = ensure_capacity(*s, s->n_docs + n_docs, off[(size_t)n_docs]))) return rc;
    HR_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));   // the producer of vecs_dev has finished
    HR_CHECK_HIP(hipMemcpy(s->offsets.as<int64_t>() + s->n_docs, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    const int pieces = s->dim / 8;
    constexpr int64_t kMaxGrid = 1ll << 30;
    for (int64_t v0 = 0; v0 < added; v0 += kMaxGrid) {
        const int64_t n = std::min(kMaxGrid, added - v0);
        hipLaunchKernelGGL(mv_pack_kernel, dim3((unsigned)n), dim3(kPackThreads), 0, nullptr, (const uint4*)vecs_dev, (int64_t)row_stride,
                           pieces, (const int64_t*)(s->offsets.as<int64_t>() + s->n_docs), n_docs, s->n_vecs + v0, s->vecs.as<uint4>());
        HR_CHECK_HIP(hipGetLastError());
    }
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    return commit_append(*s, off, lens);
}

int32_t hipmv_append(uint64_t h, const void* vecs_host, const int64_t* offsets_host, int64_t n_docs)
{
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_REQUIRE(n_docs >= 0, "n_docs must not be negative (got %lld)", (long long)n_docs);
    HR_REQUIRE(offsets_host, "offsets is null");
    HR_REQUIRE(offsets_host[0] == 0, "offsets must start at 0 (got %lld)", (long long)offsets_host[0]);
    for (int64_t i = 0; i < n_docs; ++i)
        HR_REQUIRE(offsets_host[i] <= offsets_host[i + 1], "offsets descend at document %lld", (long long)i);
    HR_REQUIRE(vecs_host || offsets_host[n_docs] == 0, "vecs is null");
    HR_REQUIRE(s->n_docs + n_docs < (1ll << 31), "the store would hold %lld documents: the limit is 2^31 - 1",
               (long long)(s->n_docs + n_docs));
    if (n_docs == 0) return HIPRAG_OK;
    std::vector<int64_t> off((size_t)n_docs + 1);
    std::vector<int32_t> lens((size_t)n_docs);
    off[0] = s->n_vecs;
    for (int64_t i = 0; i < n_docs; ++i) {
        lens[(size_t)i] = (int32_t)std::min<int64_t>(offsets_host[i + 1] - offsets_host[i], s->max_doc_vectors);
        off[(size_t)i + 1] = off[(size_t)i] + lens[(size_t)i];
    }
    int32_t rc;
    if ((rc = ensure_capacity(*s, s->n_docs + n_docs, off[(size_t)n_docs]))) return rc;
    // Consecutive documents that lose nothing to the cap are one contiguous run of the source: one copy per run.
    const size_t vb = (size_t)s->dim * 2;
    const char* src = (const char*)vecs_host;
    char* dst = s->vecs.as<char>();
    for (int64_t i = 0; i < n_docs;) {
        int64_t j = i;
        while (j + 1 < n_docs && offsets_host[j + 1] - offsets_host[j] == lens[(size_t)j]) ++j;
        const int64_t n = offsets_host[j] - offsets_host[i] + lens[(size_t)j];
        if (n) HR_CHECK_HIP(hipMemcpy(dst + (size_t)off[(size_t)i] * vb, src + (size_t)offsets_host[i] * vb, (size_t)n * vb, hipMemcpyHostToDevice));
        i = j + 1;
    }
    HR_CHECK_HIP(hipMemcpy(s->offsets.as<int64_t>() + s->n_docs, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    return commit_append(*s, off, lens);
}

int32_t hipmv_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges)
{
    GET_MV(s, h);
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
    // The plan of hiptok_remove_ranges in vectors; the mover works in int32 words, dim / 2 of them per vector.
    const int64_t first = tab[0].first, words = s->dim / 2;
    int64_t v_first = 0;
    for (int64_t i = 0; i < first; ++i) v_first += s->len_host[(size_t)i];
    std::vector<MoveRun> moves;
    std::vector<int64_t> off;          // new offsets of the documents first .. n_new
    std::vector<int32_t> lens_after(s->len_host.begin(), s->len_host.begin() + first);
    off.push_back(v_first);
    int64_t src = v_first, dst = v_first;
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
        if (run > 0) moves.push_back(MoveRun{src * words, dst * words, run * words});
        src += run;
        dst += run;
    }
    int32_t longest = 0;
    for (int32_t len : lens_after) longest = std::max(longest, len);
    int32_t rc;
    if ((rc = move_runs_down_i32(s->vecs.as<int32_t>(), moves, v_first * words, dst * words))) return rc;
    HR_CHECK_HIP(hipMemcpy(s->offsets.as<int64_t>() + first, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    s->n_docs = (int64_t)lens_after.size();
    s->len_host.swap(lens_after);
    s->n_vecs = dst;
    s->longest = longest;
    return HIPRAG_OK;
}

int32_t hipmv_export(uint64_t h, int64_t* offsets, void* vecs)
{
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    if (offsets) HR_CHECK_HIP(hipMemcpy(offsets, s->offsets.p, (size_t)(s->n_docs + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (vecs && s->n_vecs) HR_CHECK_HIP(hipMemcpy(vecs, s->vecs.p, (size_t)s->n_vecs * s->dim * 2, hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hipmv_sizes(uint64_t h, int64_t* out4)
{
    HR_REQUIRE(out4, "null out");
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    out4[0] = s->n_docs;
    out4[1] = s->n_vecs;
    out4[2] = s->dim;
    out4[3] = s->longest;
    return HIPRAG_OK;
}

/* HIPMV001, little-endian, no gaps: char magic[8] | int32 version = 1 | int32 dim | int32 max_doc_vectors | int64 docs |
 * int64 stored vectors | int64 offsets[docs + 1] | bf16 vecs[stored][dim]. */
int32_t hipmv_save(uint64_t h, const char* path)
{
    HR_REQUIRE(path, "null path");
    GET_MV(s, h);
    std::lock_guard<std::mutex> guard(s->mu);
    HR_CHECK_HIP(hipSetDevice(s->device));
    HR_CHECK_HIP(hipDeviceSynchronize());
    std::vector<int64_t> off((size_t)s->n_docs + 1);
    HR_CHECK_HIP(hipMemcpy(off.data(), s->offsets.p, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    const std::string tmp = std::string(path) + ".tmp";
    bool ok;
    {
        FileCloser fc{fopen(tmp.c_str(), "wb")};
        if (!fc.f) { set_error("cannot open %s for writing", tmp.c_str()); return HIPRAG_E_IO; }
        const int32_t head[3] = {kVersion, s->dim, s->max_doc_vectors};
        const int64_t counts[2] = {s->n_docs, s->n_vecs};
        ok = fwrite(kMagic, 1, 8, fc.f) == 8 && fwrite(head, 4, 3, fc.f) == 3 && fwrite(counts, 8, 2, fc.f) == 2 &&
             fwrite(off.data(), 8, off.size(), fc.f) == off.size();
        const size_t total = (size_t)s->n_vecs * s->dim * 2;
        std::vector<char> buf(std::min(total, kIoChunk));
        for (size_t o = 0; ok && o < total; o += kIoChunk) {
            const size_t n = std::min(kIoChunk, total - o);
            HR_CHECK_HIP(hipMemcpy(buf.data(), s->vecs.as<char>() + o, n, hipMemcpyDeviceToHost));
            ok = fwrite(buf.data(), 1, n, fc.f) == n;
        }
        ok = ok && fflush(fc.f) == 0;
    }
    if (!ok || rename(tmp.c_str(), path) != 0) {
        (void)remove(tmp.c_str());
        set_error("write to %s failed", path);
        return HIPRAG_E_IO;
    }
    return HIPRAG_OK;
}

int32_t hipmv_load(const char* path, int32_t device, uint64_t* out_handle)
{
    HR_REQUIRE(path && out_handle, "null argument");
    FileCloser fc{fopen(path, "rb")};
    if (!fc.f) { set_error("cannot open %s", path); return HIPRAG_E_IO; }
    char magic[8];
    int32_t head[3];
    int64_t counts[2];
    if (fread(magic, 1, 8, fc.f) != 8 || memcmp(magic, kMagic, 8) != 0 || fread(head, 4, 3, fc.f) != 3 || fread(counts, 8, 2, fc.f) != 2) {
        set_error("%s is not a HIPMV001 file", path);
        return HIPRAG_E_IO;
    }
    // sizes and offsets are validated before anything is allocated on the device
    if (head[0] != kVersion) { set_error("%s: HIPMV001 version %d is not supported", path, head[0]); return HIPRAG_E_IO; }
    const int32_t dim = head[1], cap = head[2];
    const int64_t n_docs = counts[0], n_vecs = counts[1];
    if (dim < 64 || dim > kMaxDim || dim % 64 || cap < 1 || n_docs < 0 || n_docs >= (1ll << 31) || n_vecs < 0 || n_vecs > n_docs * (int64_t)cap) {
        set_error("%s: bad header (dim %d, cap %d, %lld documents, %lld vectors)", path, dim, cap, (long long)n_docs, (long long)n_vecs);
        return HIPRAG_E_IO;
    }
    const int64_t body = 36 + (n_docs + 1) * 8 + n_vecs * dim * 2;
    if (fseek(fc.f, 0, SEEK_END) != 0 || (int64_t)ftell(fc.f) != body || fseek(fc.f, 36, SEEK_SET) != 0) {
        set_error("%s: the file does not have the %lld bytes its header asks for", path, (long long)body);
        return HIPRAG_E_IO;
    }
    std::vector<int64_t> off((size_t)n_docs + 1);
    if (fread(off.data(), 8, off.size(), fc.f) != off.size()) { set_error("%s: short read", path); return HIPRAG_E_IO; }
    std::vector<int32_t> lens((size_t)n_docs);
    bool ok = off[0] == 0 && off[(size_t)n_docs] == n_vecs;
    for (int64_t i = 0; ok && i < n_docs; ++i) {
        const int64_t len = off[(size_t)i + 1] - off[(size_t)i];
        ok = len >= 0 && len <= cap;
        lens[(size_t)i] = (int32_t)len;
    }
    if (!ok) { set_error("%s: the offsets do not start at 0, descend, exceed the cap or do not end at the vector count", path); return HIPRAG_E_IO; }
    std::shared_ptr<MultiVecStore> s;
    int32_t rc;
    if ((rc = new_store(dim, cap, device, &s))) return rc;
    if ((rc = ensure_capacity(*s, n_docs, n_vecs))) return rc;
    const size_t total = (size_t)n_vecs * dim * 2;
    std::vector<char> buf(std::min(total, kIoChunk));
    for (size_t o = 0; o < total; o += kIoChunk) {
        const size_t n = std::min(kIoChunk, total - o);
        if (fread(buf.data(), 1, n, fc.f) != n) { set_error("%s: short read", path); return HIPRAG_E_IO; }
        HR_CHECK_HIP(hipMemcpy(s->vecs.as<char>() + o, buf.data(), n, hipMemcpyHostToDevice));
    }
    HR_CHECK_HIP(hipMemcpy(s->offsets.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    std::vector<int64_t> end(1, n_vecs);
    commit_append(*s, end, lens);
    *out_handle = mv_reg().put(s);
    return HIPRAG_OK;
}

}  // extern "C"
