// bm25_impacts.hip -- updatable IMPACT postings (hipbm25_create_impacts / _append_impacts / _append_rows_dev, and
// hipbm25_remove_ranges on such a handle; include/hiprag.h).
//
// An impact handle is a Bm25Index that keeps impacts as given -- BGE-M3's lexical weights, which depend on the document
// alone, not on N, df or avgdl.  So an append or a removal changes structure only: the impacts travel with their postings as
// the 32-bit stream the structure passes of bm25_update.hip carry beside doc_ids (append_kernel, rm_scatter_kernel: the tf
// path's kernels, unchanged, moving bits), the skip tables are rebuilt behind every change, and the handle is never dirty.
// Defining property: after any sequence of updates the handle equals, bit for bit, hipbm25_create over
// hiprag.lexical.transpose_doc_weights of the surviving documents' rows in order.
//
// What is new here is the TRANSPOSITION of document-major rows (what hipenc_forward_lexical writes) into the term-major
// batch CSR the merge takes, on the device, a slice of at most 8192 rows at a time:
//   rows_check_kernel   every row check of the whole batch, before anything of the handle changes
//   rows_count_kernel   postings per term (integer atomic add)
//   rm_scan_kernel      exclusive scan of the counts = the batch offsets (the removal's scan)
//   rows_place_kernel   every (term, row, weight) to offsets[term] + a per-term integer cursor: the SET of a list's entries is
//                       fixed, their order inside the list is whatever the atomics gave
//   list_sort_*_kernel  every list sorted by row id.  Row ids inside a list are unique, so the sorted list -- hence every
//                       byte of the result -- does not depend on the order of the atomics.  Lists of up to 64 entries: one
//                       wave each, rank by shuffles; longer ones: one workgroup each, bitonic network in LDS over
//                       (row << 32 | weight bits), which a slice of 8192 rows bounds at 64 KiB.
// No float atomics anywhere.
#include <cmath>
#include <cstring>
#include <vector>

#include "bm25_internal.h"

namespace hiprag {
namespace {

constexpr int kSliceRows = 8192;        // rows per transposition: a list of one slice fits the LDS of list_sort_long_kernel
constexpr int kSortThreads = 1024;
constexpr u32 kShortList = 64;          // lists up to this length are sorted by one wave

struct RowsArgs {
    const int32_t* terms;               // [n][stride]
    const float* wts;                   // [n][stride]
    const int32_t* counts;              // [n]
    i64 n;                              // rows of this launch, starting at row0
    i64 row0;
    i64 stride;
    u32 n_terms;
};

// One wave per row.  err = the smallest (row, entry, reason) key of a violated rule, integer min: the same refusal every run.
// reasons: 0 count outside [0, stride], 1 id outside [0, n_terms), 2 ids not strictly ascending, 3 weight not finite or <= 0
__global__ __launch_bounds__(256) void rows_check_kernel(RowsArgs a, unsigned long long* __restrict__ err)
{
    const i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= a.n) return;
    const i64 row = a.row0 + r;
    const int32_t c = a.counts[row];
    const u64 key0 = (u64)row * (u64)(a.stride + 1);
    if (c < 0 || (i64)c > a.stride) {
        if (lane == 0) atomicMin(err, (unsigned long long)(key0 << 2));
        return;
    }
    const int32_t* t = a.terms + row * a.stride;
    const float* w = a.wts + row * a.stride;
    for (int j = lane; j < c; j += 64) {
        const int32_t id = t[j];
        const float x = w[j];
        int bad = -1;
        if (id < 0 || (u32)id >= a.n_terms) bad = 1;
        else if (j > 0 && t[j - 1] >= id) bad = 2;
        else if (!(x > 0.f) || !(x <= 3.402823466e+38f)) bad = 3;
        if (bad >= 0) atomicMin(err, (unsigned long long)(((key0 + (u64)j) << 2) | (u64)bad));
    }
}

__global__ __launch_bounds__(256) void rows_count_kernel(RowsArgs a, u32* __restrict__ cnt)
{
    const i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= a.n) return;
    const i64 row = a.row0 + r;
    const int32_t c = a.counts[row];
    const int32_t* t = a.terms + row * a.stride;
    for (int j = lane; j < c; j += 64) atomicAdd(&cnt[t[j]], 1u);
}

// ids of the batch CSR are local to the slice (the merge adds n_docs); wbits = the weight as given
__global__ __launch_bounds__(256) void rows_place_kernel(RowsArgs a, const u64* __restrict__ boff, u32* __restrict__ cursor,
                                                         u32* __restrict__ ids, u32* __restrict__ wbits)
{
    const i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= a.n) return;
    const i64 row = a.row0 + r;
    const int32_t c = a.counts[row];
    const int32_t* t = a.terms + row * a.stride;
    const float* w = a.wts + row * a.stride;
    for (int j = lane; j < c; j += 64) {
        const u32 term = (u32)t[j];
        const u64 p = boff[term] + atomicAdd(&cursor[term], 1u);
        ids[p] = (u32)r;
        wbits[p] = __float_as_uint(w[j]);
    }
}

// one wave per term: lists of 2 .. 64 entries, an entry's place = the entries of the list with a smaller row id
__global__ __launch_bounds__(256) void list_sort_short_kernel(const u64* __restrict__ boff, u32 n_terms, u32* __restrict__ ids,
                                                              u32* __restrict__ wbits)
{
    const u64 t = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= n_terms) return;
    const u64 lo = boff[t];
    const u32 len = (u32)(boff[t + 1] - lo);
    if (len < 2 || len > kShortList) return;
    const bool live = (u32)lane < len;
    const u32 id = live ? ids[lo + lane] : 0xffffffffu;
    const u32 wb = live ? wbits[lo + lane] : 0u;
    u32 rank = 0;
    for (u32 j = 0; j < len; ++j) rank += (u32)__shfl((int)id, (int)j) < id ? 1u : 0u;
    if (live) {
        ids[lo + rank] = id;
        wbits[lo + rank] = wb;
    }
}

// one workgroup per long list (65 .. 8192 entries)
__global__ __launch_bounds__(kSortThreads) void list_sort_long_kernel(const u64* __restrict__ boff, const u32* __restrict__ long_terms,
                                                                      u32* __restrict__ ids, u32* __restrict__ wbits)
{
    __shared__ u64 key[kSliceRows];
    const u32 t = long_terms[blockIdx.x];
    const u64 lo = boff[t];
    const u32 len = (u32)(boff[t + 1] - lo);   // <= kSliceRows: one posting per (term, row) of the slice
    u32 n2 = 128;
    while (n2 < len) n2 <<= 1;
    for (u32 i = threadIdx.x; i < n2; i += kSortThreads) key[i] = i < len ? ((u64)ids[lo + i] << 32 | wbits[lo + i]) : ~0ull;
    __syncthreads();
    for (u32 k = 2; k <= n2; k <<= 1)
        for (u32 j = k >> 1; j > 0; j >>= 1) {
            for (u32 i = threadIdx.x; i < n2; i += kSortThreads) {
                const u32 x = i ^ j;
                if (x > i) {
                    const u64 p = key[i], q = key[x];
                    if ((p > q) == ((i & k) == 0)) { key[i] = q; key[x] = p; }
                }
            }
            __syncthreads();
        }
    for (u32 i = threadIdx.x; i < len; i += kSortThreads) {
        ids[lo + i] = (u32)(key[i] >> 32);
        wbits[lo + i] = (u32)key[i];
    }
}

bool impact_ok(float x) { return std::isfinite(x) && x > 0.f; }

// every check of a CSR with impacts (hipbm25_create_impacts, the batch of hipbm25_append_impacts): ids below n_docs
int32_t check_csr_impacts(const char* what, i64 n_docs, i64 n_terms, const uint64_t* off, const uint32_t* ids, const float* imp)
{
    HR_REQUIRE(off, "%soffsets is null", what);
    HR_REQUIRE(off[0] == 0, "%soffsets must start at 0 (got %llu)", what, (unsigned long long)off[0]);
    for (i64 t = 0; t < n_terms; ++t)
        HR_REQUIRE(off[t] <= off[t + 1], "%soffsets descends at term %lld", what, (long long)t);
    const uint64_t P = off[n_terms];
    HR_REQUIRE(P == 0 || (ids && imp), "%sdoc_ids or impacts is null", what);
    for (i64 t = 0; t < n_terms; ++t)
        for (uint64_t i = off[t]; i < off[t + 1]; ++i) {
            HR_REQUIRE((i64)ids[i] < n_docs, "%sposting %llu has doc id %u, not below %lld", what, (unsigned long long)i, ids[i], (long long)n_docs);
            HR_REQUIRE(i == off[t] || ids[i - 1] < ids[i], "%sposting list of term %lld is not strictly ascending by doc id", what, (long long)t);
            HR_REQUIRE(impact_ok(imp[i]), "%sposting %llu has impact %g: every impact must be finite and > 0", what, (unsigned long long)i,
                       (double)imp[i]);
        }
    return HIPRAG_OK;
}

int32_t require_impact_handle(const Bm25Index& ix, const char* entry)
{
    if (ix.has_impacts) return HIPRAG_OK;
    set_error("this bm25 handle was made by %s: %s needs a handle of hipbm25_create_impacts", ix.has_tf ? "hipbm25_create_tf" : "hipbm25_create",
              entry);
    return HIPRAG_E_UNSUPPORTED;
}

int32_t check_append_sizes(const Bm25Index& ix, i64 n_new, i64 n_terms_after)
{
    HR_REQUIRE(n_new >= 0, "n_new_docs must not be negative (got %lld)", (long long)n_new);
    HR_REQUIRE(n_terms_after >= ix.n_terms, "n_terms_after = %lld is below the handle's n_terms = %lld: the vocabulary only grows",
               (long long)n_terms_after, (long long)ix.n_terms);
    HR_REQUIRE(n_terms_after < (1ll << 32), "term ids are u32: n_terms_after must be < 2^32");
    HR_REQUIRE(ix.n_docs + n_new < (1ll << 32), "doc ids are u32: %lld + %lld documents pass 2^32", (long long)ix.n_docs, (long long)n_new);
    return HIPRAG_OK;
}

}  // namespace

int32_t Bm25Index::append_impacts(i64 n_new, i64 n_terms_after, const uint64_t* boff, const uint32_t* bids, const float* bimp)
{
    int32_t rc;
    if ((rc = require_impact_handle(*this, "hipbm25_append_impacts"))) return rc;
    if ((rc = check_append_sizes(*this, n_new, n_terms_after))) return rc;
    if ((rc = check_csr_impacts("batch_", n_new, n_terms_after, boff, bids, bimp))) return rc;
    const i64 P_old = n_postings, Pb = (i64)boff[n_terms_after], docs_before = n_docs;
    std::vector<uint64_t> noff;
    if ((rc = plan_merge(n_terms_after, boff, noff))) return rc;
    if (prev_ev_set) HR_CHECK_HIP(hipEventSynchronize(prev_ev));
    i64 extra = 0, moved = 0;
    bool grew = false;
    DevBuf b_ids, b_imp, b_off;     // freed behind the synchronisation of rebuild_skips
    if (Pb > 0) {
        if ((rc = b_ids.reserve((size_t)Pb * sizeof(u32))) || (rc = b_imp.reserve((size_t)Pb * sizeof(float))) ||
            (rc = b_off.reserve(noff.size() * sizeof(u64))))
            return rc;
        extra += (i64)(b_ids.bytes + b_imp.bytes + b_off.bytes);
        HR_CHECK_HIP(hipMemcpy(b_ids.p, bids, (size_t)Pb * sizeof(u32), hipMemcpyHostToDevice));
        HR_CHECK_HIP(hipMemcpy(b_imp.p, bimp, (size_t)Pb * sizeof(float), hipMemcpyHostToDevice));
        HR_CHECK_HIP(hipMemcpy(b_off.p, boff, noff.size() * sizeof(u64), hipMemcpyHostToDevice));
    }
    if ((rc = merge_batch(impacts, n_terms_after, noff, boff, b_off.as<u64>(), b_ids.as<u32>(), b_imp.as<u32>(), &grew, &extra, &moved))) return rc;
    n_docs += n_new;
    drop_doc_workspaces();
    if ((rc = rebuild_skips())) return rc;
    const i64 info[8] = {5, P_old, n_postings, moved, docs_before, n_docs, extra, grew ? 1 : 0};
    memcpy(upd_info, info, sizeof(info));
    return HIPRAG_OK;
}

int32_t Bm25Index::append_rows_dev(const int32_t* terms_dev, const float* weights_dev, const int32_t* counts_dev, i64 n_new, i64 row_stride,
                                   i64 n_terms_after, hipStream_t stream)
{
    int32_t rc;
    if ((rc = require_impact_handle(*this, "hipbm25_append_rows_dev"))) return rc;
    if ((rc = check_append_sizes(*this, n_new, n_terms_after))) return rc;
    HR_REQUIRE(row_stride >= 1 && row_stride < (1ll << 31), "row_stride must be in 1 .. 2^31 - 1 (got %lld)", (long long)row_stride);
    HR_REQUIRE(n_new == 0 || (terms_dev && weights_dev && counts_dev), "terms, weights or counts is null");
    HR_CHECK_HIP(hipStreamSynchronize(stream));   // the producer of the rows has finished
    if (prev_ev_set) HR_CHECK_HIP(hipEventSynchronize(prev_ev));
    i64 extra = 0, moved = 0;
    bool grew = false;
    const i64 P_old = n_postings, docs_before = n_docs;
    RowsArgs a;
    a.terms = terms_dev; a.wts = weights_dev; a.counts = counts_dev;
    a.n = n_new; a.row0 = 0; a.stride = row_stride; a.n_terms = (u32)n_terms_after;
    // every row check, over the whole batch, before anything of the handle changes
    if (n_new > 0) {
        DevBuf err;
        if ((rc = err.reserve(sizeof(u64)))) return rc;
        extra += (i64)err.bytes;
        u64 e = ~0ull;
        HR_CHECK_HIP(hipMemcpy(err.p, &e, sizeof(e), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(rows_check_kernel, dim3((unsigned)((n_new + 3) / 4)), dim3(256), 0, nullptr, a,
                           reinterpret_cast<unsigned long long*>(err.p));
        HR_CHECK_HIP(hipGetLastError());
        HR_CHECK_HIP(hipMemcpy(&e, err.p, sizeof(e), hipMemcpyDeviceToHost));
        if (e != ~0ull) {
            const u64 at = e >> 2, row = at / (u64)(row_stride + 1), j = at % (u64)(row_stride + 1);
            switch ((int)(e & 3)) {
            case 0: set_error("counts[%llu] lies outside [0, row_stride = %lld]", (unsigned long long)row, (long long)row_stride); break;
            case 1: set_error("row %llu, entry %llu: the term id lies outside [0, n_terms_after = %lld)", (unsigned long long)row,
                              (unsigned long long)j, (long long)n_terms_after); break;
            case 2: set_error("row %llu, entry %llu: term ids must ascend strictly within a row", (unsigned long long)row,
                              (unsigned long long)j); break;
            default: set_error("row %llu, entry %llu: every weight must be finite and > 0", (unsigned long long)row, (unsigned long long)j);
            }
            return HIPRAG_E_INVALID;
        }
    }
    // the batch in slices of at most kSliceRows rows, each transposed and merged; a batch of no rows is one empty slice (the
    // vocabulary may still grow)
    const size_t nt1 = (size_t)n_terms_after + 1;
    DevBuf cnt, b_off, b_ids, b_w, longs_dev;   // freed behind the synchronisation of rebuild_skips
    std::vector<uint64_t> boff(nt1), noff;
    std::vector<u32> longs;
    if ((rc = cnt.reserve(std::max<size_t>(16, (size_t)n_terms_after * sizeof(u32)))) || (rc = b_off.reserve(nt1 * sizeof(u64)))) return rc;
    extra += (i64)(cnt.bytes + b_off.bytes);
    for (i64 r0 = 0; r0 == 0 || r0 < n_new; r0 += kSliceRows) {
        a.row0 = r0;
        a.n = std::min<i64>(kSliceRows, n_new - r0);
        const unsigned row_blocks = (unsigned)((a.n + 3) / 4);
        HR_CHECK_HIP(hipMemsetAsync(cnt.p, 0, cnt.bytes, nullptr));
        if (a.n > 0) hipLaunchKernelGGL(rows_count_kernel, dim3(row_blocks), dim3(256), 0, nullptr, a, cnt.as<u32>());
        launch_excl_scan(cnt.as<u32>(), n_terms_after, b_off.as<u64>());
        HR_CHECK_HIP(hipGetLastError());
        HR_CHECK_HIP(hipMemcpy(boff.data(), b_off.p, nt1 * sizeof(u64), hipMemcpyDeviceToHost));   // synchronises the null stream
        const i64 Pb = (i64)boff[(size_t)n_terms_after];
        if ((rc = plan_merge(n_terms_after, boff.data(), noff))) return rc;
        if (Pb > 0) {
            const size_t had = b_ids.bytes + b_w.bytes + longs_dev.bytes;
            if ((rc = b_ids.reserve((size_t)Pb * sizeof(u32))) || (rc = b_w.reserve((size_t)Pb * sizeof(u32)))) return rc;
            longs.clear();
            for (i64 t = 0; t < n_terms_after; ++t)
                if (boff[(size_t)t + 1] - boff[(size_t)t] > kShortList) longs.push_back((u32)t);
            HR_CHECK_HIP(hipMemsetAsync(cnt.p, 0, cnt.bytes, nullptr));   // the counts become the cursors
            hipLaunchKernelGGL(rows_place_kernel, dim3(row_blocks), dim3(256), 0, nullptr, a, (const u64*)b_off.as<u64>(), cnt.as<u32>(),
                               b_ids.as<u32>(), b_w.as<u32>());
            hipLaunchKernelGGL(list_sort_short_kernel, dim3((unsigned)((n_terms_after + 3) / 4)), dim3(256), 0, nullptr,
                               (const u64*)b_off.as<u64>(), (u32)n_terms_after, b_ids.as<u32>(), b_w.as<u32>());
            if (!longs.empty()) {
                if ((rc = longs_dev.reserve(longs.size() * sizeof(u32)))) return rc;
                HR_CHECK_HIP(hipMemcpyAsync(longs_dev.p, longs.data(), longs.size() * sizeof(u32), hipMemcpyHostToDevice, nullptr));
                hipLaunchKernelGGL(list_sort_long_kernel, dim3((unsigned)longs.size()), dim3(kSortThreads), 0, nullptr,
                                   (const u64*)b_off.as<u64>(), (const u32*)longs_dev.as<u32>(), b_ids.as<u32>(), b_w.as<u32>());
            }
            HR_CHECK_HIP(hipGetLastError());
            extra += (i64)(b_ids.bytes + b_w.bytes + longs_dev.bytes - had);
        }
        if ((rc = merge_batch(impacts, n_terms_after, noff, boff.data(), b_off.as<u64>(), b_ids.as<u32>(), b_w.as<u32>(), &grew, &extra, &moved)))
            return rc;
        n_docs += a.n;
    }
    drop_doc_workspaces();
    if ((rc = rebuild_skips())) return rc;
    const i64 info[8] = {6, P_old, n_postings, moved, docs_before, n_docs, extra, grew ? 1 : 0};
    memcpy(upd_info, info, sizeof(info));
    return HIPRAG_OK;
}

}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipbm25_create_impacts(int64_t n_docs, int64_t n_terms, const uint64_t* offsets_host, const uint32_t* doc_ids_host,
                               const float* impacts_host, int32_t device, uint64_t* out_handle)
{
    HR_REQUIRE(out_handle, "out_handle is null");
    HR_REQUIRE(n_docs >= 0 && n_terms >= 0, "negative sizes");
    HR_REQUIRE(n_docs < (1ll << 32), "doc ids are u32: n_docs must be < 2^32 per shard");
    HR_REQUIRE(n_terms < (1ll << 32), "term ids are u32: n_terms must be < 2^32");
    int32_t rc;
    if ((rc = check_csr_impacts("", n_docs, n_terms, offsets_host, doc_ids_host, impacts_host))) return rc;
    for (int64_t t = 0; t < n_terms; ++t) {
        const uint64_t len = offsets_host[t + 1] - offsets_host[t];
        HR_REQUIRE(len < kSkipMinDf || len < (1ull << 32), "posting list of term %lld is too long for u32 skip offsets", (long long)t);
    }
    const uint64_t P = offsets_host[n_terms];
    auto ix = std::make_shared<Bm25Index>();
    ix->device = device;
    ix->has_impacts = true;
    ix->n_docs = n_docs;
    ix->n_terms = n_terms;
    ix->n_postings = (i64)P;
    ix->offsets.assign(offsets_host, offsets_host + n_terms + 1);
    HR_CHECK_HIP(hipSetDevice(device));
    ix->cap_postings = round4((i64)P);
    if ((rc = ix->doc_ids.reserve((size_t)ix->cap_postings * sizeof(u32))) || (rc = ix->impacts.reserve((size_t)ix->cap_postings * sizeof(float))) ||
        (rc = ix->offsets_dev.reserve((size_t)(n_terms + 1) * sizeof(u64))))
        return rc;
    if (P) {
        HR_CHECK_HIP(hipMemcpy(ix->doc_ids.p, doc_ids_host, P * sizeof(u32), hipMemcpyHostToDevice));
        HR_CHECK_HIP(hipMemcpy(ix->impacts.p, impacts_host, P * sizeof(float), hipMemcpyHostToDevice));
    }
    HR_CHECK_HIP(hipMemcpy(ix->offsets_dev.p, ix->offsets.data(), (size_t)(n_terms + 1) * sizeof(u64), hipMemcpyHostToDevice));
    ix->read_env();
    if ((rc = ix->rebuild_skips())) return rc;
    const i64 info[8] = {4, 0, (i64)P, 0, 0, n_docs, 0, 0};
    memcpy(ix->upd_info, info, sizeof(info));
    *out_handle = bm25_reg().put(ix);
    return HIPRAG_OK;
}

int32_t hipbm25_append_impacts(uint64_t h, int64_t n_new_docs, int64_t n_terms_after, const uint64_t* batch_offsets_host,
                               const uint32_t* batch_doc_ids_host, const float* batch_impacts_host)
{
    GET_BM25(h);
    return ix->append_impacts(n_new_docs, n_terms_after, batch_offsets_host, batch_doc_ids_host, batch_impacts_host);
}

int32_t hipbm25_append_rows_dev(uint64_t h, const int32_t* terms_dev, const float* weights_dev, const int32_t* counts_dev,
                                int64_t n_new_docs, int64_t row_stride, int64_t n_terms_after, void* stream)
{
    GET_BM25(h);
    return ix->append_rows_dev(terms_dev, weights_dev, counts_dev, n_new_docs, row_stride, n_terms_after, (hipStream_t)stream);
}

}  // extern "C"
