// bm25_update.hip -- updatable BM25 postings (hipbm25_create_tf / _append / _remove_ranges / _reweigh, include/hiprag.h).
//
// A handle made by hipbm25_create_tf keeps what impacts are made of: per-posting term frequency, per-document length and
// (in the offsets) per-term document frequency.  An append or a removal changes N, df and avgdl, hence every impact, so
// the structure passes (append, remove) only rewrite doc_ids / tf / offsets / doc_len and leave the handle DIRTY; one
// reweigh pass then recomputes every impact and the skip tables.  The search kernels of bm25.hip are untouched: they go on
// reading doc_ids and impacts.  Defining property: after any sequence of updates followed by a reweigh the handle equals,
// bit for bit, hipbm25_create over hiprag.sparse.build_postings of the surviving documents in order.
//
// All three passes are streaming passes over the posting array cut into ITEMS of 4096 postings (256 threads x 16): an item
// is a slice of one long list or a run of short lists.  The workgroup bisects the device copy of the offsets once for the
// terms of its first and last posting; a posting's term is then a bisection inside that (usually one-element) interval --
// never one thread per term, list lengths are Zipfian.  16-byte vector loads and stores of the streams, no LDS beyond the
// scans, no float atomics; the only atomics are integer add / min, whose result does not depend on order, so a run gives
// identical bytes every time.
//
// The append and the removal move tf as a 32-bit stream beside doc_ids without looking at it.  The impact handles of
// bm25_impacts.hip pass their impacts' bits through the same kernels (merge_batch, remove_ranges) and rebuild the skip tables
// with rebuild_skips, the second half of the reweigh.
#include <cmath>
#include <cstring>
#include <vector>

#include "bm25_internal.h"
#include "range_table.h"

namespace hiprag {
namespace {

constexpr int kUpdThreads = 256;
constexpr int kUpdPer = 16;                        // postings per thread: four 16-byte pieces of each stream
constexpr int kUpdChunk = kUpdThreads * kUpdPer;   // postings per item
constexpr int kScanThreads = 1024;

// the last list in [lo, hi] that starts at or before posting p (off[lo] <= p): lists are half-open, so with p below the
// end of list hi this is the non-empty list that holds p
__device__ inline u32 term_of(const u64* __restrict__ off, u32 lo, u32 hi, u64 p)
{
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// terms of the first and the last posting of this workgroup's item, through LDS
__device__ inline void item_terms(const u64* __restrict__ off, u32 n_terms, u64 p0, u64 P, u32* trange)
{
    if (threadIdx.x == 0) {
        const u64 p1 = (p0 + kUpdChunk < P ? p0 + kUpdChunk : P) - 1;
        const u32 tl = term_of(off, 0, n_terms - 1, p0);
        trange[0] = tl;
        trange[1] = term_of(off, tl, n_terms - 1, p1);
    }
    __syncthreads();
}

// exclusive prefix of v over the workgroup (blockDim.x a multiple of 64, at most 1024); total = the sum
__device__ inline u32 block_excl_scan(u32 v, u32* wsum, u32& total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    u32 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 up = (u32)__shfl_up((int)inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    u32 base = 0;
    total = 0;
    for (int w = 0; w < nw; ++w) {
        const u32 s = wsum[w];
        if (w < wv) base += s;
        total += s;
    }
    __syncthreads();   // wsum may be written again
    return base + inc - v;
}

// ---- reweigh: impacts[p] = bm25_impact(idf[term(p)], tf[p], doc_len[doc_ids[p]]) -------------------------------------
struct ReweighArgs {
    const u32* doc_ids;
    const u32* tf;
    const u32* doc_len;
    const u64* off;
    const double* idf;
    float* impacts;
    u64 P;
    u32 n_terms;
    double avgdl, k1, b;
};

__global__ __launch_bounds__(kUpdThreads) void reweigh_kernel(ReweighArgs a)
{
    __shared__ u32 trange[2];
    const u64 p0 = (u64)blockIdx.x * kUpdChunk;
    item_terms(a.off, a.n_terms, p0, a.P, trange);
    u32 t = trange[0];
    const u32 thi = trange[1];
    // unconditional loads (pieces past the end read piece 0: the buffers hold 16 entries at least), all eight in flight
    uint4 d[4], f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u64 i = p0 + (u64)j * (kUpdThreads * 4) + (u64)threadIdx.x * 4;
        const u64 ic = i < a.P ? i : 0;
        d[j] = *reinterpret_cast<const uint4*>(a.doc_ids + ic);
        f[j] = *reinterpret_cast<const uint4*>(a.tf + ic);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u64 i = p0 + (u64)j * (kUpdThreads * 4) + (u64)threadIdx.x * 4;
        if (i >= a.P) break;
        const u32 dd[4] = {d[j].x, d[j].y, d[j].z, d[j].w}, ff[4] = {f[j].x, f[j].y, f[j].z, f[j].w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = 0.f;
            if (i + e < a.P) {    // the capacity is a multiple of four entries: the tail of the last piece is written as 0
                t = term_of(a.off, t, thi, i + e);
                o[e] = bm25_impact(a.idf[t], (double)ff[e], (double)a.doc_len[dd[e]], a.avgdl, a.k1, a.b);
            }
        }
        *reinterpret_cast<float4*>(a.impacts + i) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- skip tables: entry (long list li, tile boundary) = first posting of the list whose document is >= tile * kTileDocs,
//      relative to the list start -- the std::lower_bound loop of hipbm25_create, one thread per entry ---------------------
__global__ __launch_bounds__(256) void skip_kernel(const u32* __restrict__ doc_ids, const u64* __restrict__ off,
                                                   const u32* __restrict__ long_terms, i64 n_long, i64 nt1, u32* __restrict__ skip)
{
    const i64 g = (i64)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_long * nt1) return;
    const u32 t = long_terms[g / nt1];
    const u64 bound = (u64)(g % nt1) * kTileDocs;
    const u64 lo0 = off[t];
    u64 lo = lo0, hi = off[t + 1];
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if ((u64)doc_ids[mid] < bound) lo = mid + 1; else hi = mid;
    }
    skip[g] = (u32)(lo - lo0);
}

// ---- append: destination list = old list, then the batch list with ids + doc_base --------------------------------------
struct AppendArgs {
    const u32* old_ids;
    const u32* old_tf;
    const u64* old_off;     // [n_terms_old + 1]
    const u32* b_ids;
    const u32* b_tf;
    const u64* b_off;       // [n_terms + 1]
    const u64* new_off;     // [n_terms + 1] = old + batch, elementwise
    u32* dst_ids;
    u32* dst_tf;
    u64 P;                  // postings afterwards
    u32 n_terms, n_terms_old, doc_base;
};

__global__ __launch_bounds__(kUpdThreads) void append_kernel(AppendArgs a)
{
    __shared__ u32 trange[2];
    const u64 p0 = (u64)blockIdx.x * kUpdChunk;
    item_terms(a.new_off, a.n_terms, p0, a.P, trange);
    u32 t = trange[0];
    const u32 thi = trange[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u64 i = p0 + (u64)j * (kUpdThreads * 4) + (u64)threadIdx.x * 4;
        if (i >= a.P) break;
        u32 id[4], tf[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            id[e] = 0;
            tf[e] = 0;
            if (i + e < a.P) {
                t = term_of(a.new_off, t, thi, i + e);
                const u64 r = i + e - a.new_off[t];
                u64 old_lo = 0, old_len = 0;
                if (t < a.n_terms_old) { old_lo = a.old_off[t]; old_len = a.old_off[t + 1] - old_lo; }
                if (r < old_len) {
                    id[e] = a.old_ids[old_lo + r];
                    tf[e] = a.old_tf[old_lo + r];
                } else {
                    const u64 s = a.b_off[t] + (r - old_len);
                    id[e] = a.b_ids[s] + a.doc_base;
                    tf[e] = a.b_tf[s];
                }
            }
        }
        *reinterpret_cast<uint4*>(a.dst_ids + i) = make_uint4(id[0], id[1], id[2], id[3]);
        *reinterpret_cast<uint4*>(a.dst_tf + i) = make_uint4(tf[0], tf[1], tf[2], tf[3]);
    }
}

// ---- remove: stable compaction with renumbering ------------------------------------------------------------------------
struct RmRange {   // a removed document range (non-empty, touching ones coalesced), ascending
    u32 lo, hi;
    u32 cum;       // documents removed before it
    u32 pad;
};

// whether document d survives, and its new id = d - the documents removed before it
__device__ inline bool doc_survives(const RmRange* __restrict__ tab, int n, u32 d, u32& nid)
{
    int lo = 0, hi = n;   // the ranges that start at or before d
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].lo <= d) lo = mid + 1; else hi = mid;
    }
    nid = d;
    if (lo == 0) return true;
    const RmRange r = tab[lo - 1];
    if (d < r.hi) return false;
    nid = d - (r.cum + (r.hi - r.lo));
    return true;
}

// block counts: survivors of every item, and the first removed posting (integer min: order does not matter)
__global__ __launch_bounds__(kUpdThreads) void rm_count_kernel(const u32* __restrict__ doc_ids, u64 P, const RmRange* __restrict__ tab,
                                                               int n_tab, u32* __restrict__ counts, u64* __restrict__ first_removed)
{
    __shared__ u32 wsum[kUpdThreads / 64];
    const u64 i0 = (u64)blockIdx.x * kUpdChunk + (u64)threadIdx.x * kUpdPer;
    u32 c = 0;
    u64 fr = ~0ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u64 i = i0 + (u64)j * 4;
        const uint4 d = *reinterpret_cast<const uint4*>(doc_ids + (i < P ? i : 0));
        const u32 dd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i + e >= P) continue;
            u32 nid;
            if (doc_survives(tab, n_tab, dd[e], nid)) ++c;
            else if (fr == ~0ull) fr = i + e;
        }
    }
    u32 total;
    (void)block_excl_scan(c, wsum, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
    if (fr != ~0ull) atomicMin(first_removed, fr);
}

// base[i] = survivors of the items before item i; base[n] = all survivors.  One workgroup walks the counts.
__global__ __launch_bounds__(kScanThreads) void rm_scan_kernel(const u32* __restrict__ counts, i64 n, u64* __restrict__ base)
{
    __shared__ u32 wsum[kScanThreads / 64];
    u64 carry = 0;
    for (i64 i0 = 0; i0 < n; i0 += kScanThreads) {
        const i64 i = i0 + threadIdx.x;
        const u32 v = i < n ? counts[i] : 0u;
        u32 total;
        const u32 ex = block_excl_scan(v, wsum, total);
        if (i < n) base[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) base[n] = carry;
}

struct ScatterArgs {
    const u32* src_ids;
    const u32* src_tf;
    const u64* old_off;   // [n_terms + 1]
    u32* dst_ids;
    u32* dst_tf;
    u64* new_off;         // [n_terms + 1]
    const u64* base;
    const RmRange* tab;
    int n_tab;
    u32 n_terms;
    u64 P;
};

// The scatter.  A thread owns 16 consecutive postings, so the order of survivors is (thread, element): new position = the
// item's base + the exclusive prefix of the keep flags inside the item, kept in LDS for every posting of the item.  The new
// offsets are that prefix evaluated at the old offsets: the workgroup whose item holds posting offsets[t] writes
// new_off[t].  The grid has P / 4096 + 1 items, so position P (the end of the last list, and every empty list behind it) lies
// in an item too.
__global__ __launch_bounds__(kUpdThreads) void rm_scatter_kernel(ScatterArgs a)
{
    __shared__ u32 wsum[kUpdThreads / 64];
    __shared__ u32 pre[kUpdChunk];
    __shared__ u32 trange[2];
    const u64 p0 = (u64)blockIdx.x * kUpdChunk;
    const u64 i0 = p0 + (u64)threadIdx.x * kUpdPer;
    u32 nid[kUpdPer], tf[kUpdPer];
    bool keep[kUpdPer];
    u32 c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const u64 i = i0 + (u64)j * 4;
        const u64 ic = i < a.P ? i : 0;
        const uint4 d = *reinterpret_cast<const uint4*>(a.src_ids + ic);
        const uint4 f = *reinterpret_cast<const uint4*>(a.src_tf + ic);
        const u32 dd[4] = {d.x, d.y, d.z, d.w}, ff[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = j * 4 + e;
            tf[n] = ff[e];
            nid[n] = 0;
            keep[n] = i + e < a.P && doc_survives(a.tab, a.n_tab, dd[e], nid[n]);
            c += keep[n] ? 1u : 0u;
        }
    }
    u32 total;
    u32 run = block_excl_scan(c, wsum, total);
    const u64 b0 = a.base[blockIdx.x];
#pragma unroll
    for (int n = 0; n < kUpdPer; ++n) {
        pre[threadIdx.x * kUpdPer + n] = run;
        if (keep[n]) {
            a.dst_ids[b0 + run] = nid[n];
            a.dst_tf[b0 + run] = tf[n];
            ++run;
        }
    }
    // the lists that start inside this item: [first t with off[t] >= p0, first t with off[t] >= p0 + 4096) of n_terms + 1
    if (threadIdx.x < 2) {
        const u64 key = p0 + (u64)threadIdx.x * kUpdChunk;
        u32 lo = 0, hi = a.n_terms + 1;
        while (lo < hi) {
            const u32 mid = lo + (hi - lo) / 2;
            if (a.old_off[mid] < key) lo = mid + 1; else hi = mid;
        }
        trange[threadIdx.x] = lo;
    }
    __syncthreads();   // pre and trange are written
    for (u32 t = trange[0] + threadIdx.x; t < trange[1]; t += kUpdThreads) a.new_off[t] = b0 + pre[a.old_off[t] - p0];
}

// document lengths of the survivors: new document j reads old document j + the documents removed at or before it -- the
// range table bisected by NEW id (lo - cum ascends strictly: touching ranges are coalesced); their sum by integer atomics
__global__ __launch_bounds__(256) void rm_doclen_kernel(const u32* __restrict__ src, u32* __restrict__ dst, i64 n_new,
                                                        const RmRange* __restrict__ tab, int n_tab, unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long wsum[4];
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    unsigned long long v = 0;
    if (j < n_new) {
        int lo = 0, hi = n_tab;   // the ranges whose first document would have had new id <= j
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((i64)(tab[mid].lo - tab[mid].cum) <= j) lo = mid + 1; else hi = mid;
        }
        i64 shift = 0;
        if (lo > 0) shift = (i64)tab[lo - 1].cum + (tab[lo - 1].hi - tab[lo - 1].lo);
        const u32 x = src[j + shift];
        dst[j] = x;
        v = x;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long s = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (s) atomicAdd(total, s);
    }
}

// buf holds `keep` bytes that must survive and needs room for `want`
int32_t grow_keep(DevBuf& buf, size_t keep, size_t want)
{
    if (want <= buf.bytes) return HIPRAG_OK;
    DevBuf nb;
    int32_t rc;
    if ((rc = nb.reserve(want))) return rc;
    if (keep) HR_CHECK_HIP(hipMemcpy(nb.p, buf.p, keep, hipMemcpyDeviceToDevice));
    swap_buf(buf, nb);
    return HIPRAG_OK;
}

// every check of a CSR with term frequencies (hipbm25_create_tf, the batch of hipbm25_append): ids below n_docs
int32_t check_csr(const char* what, i64 n_docs, i64 n_terms, const uint64_t* off, const uint32_t* ids, const uint32_t* tf)
{
    HR_REQUIRE(off, "%soffsets is null", what);
    HR_REQUIRE(off[0] == 0, "%soffsets must start at 0 (got %llu)", what, (unsigned long long)off[0]);
    for (i64 t = 0; t < n_terms; ++t)
        HR_REQUIRE(off[t] <= off[t + 1], "%soffsets descends at term %lld", what, (long long)t);
    const uint64_t P = off[n_terms];
    HR_REQUIRE(P == 0 || (ids && tf), "%sdoc_ids or tf is null", what);
    for (i64 t = 0; t < n_terms; ++t)
        for (uint64_t i = off[t]; i < off[t + 1]; ++i) {
            HR_REQUIRE((i64)ids[i] < n_docs, "%sposting %llu has doc id %u, not below %lld", what, (unsigned long long)i, ids[i], (long long)n_docs);
            HR_REQUIRE(i == off[t] || ids[i - 1] < ids[i], "%sposting list of term %lld is not strictly ascending by doc id", what, (long long)t);
            HR_REQUIRE(tf[i] >= 1, "%sposting %llu has tf 0: a term frequency is at least 1", what, (unsigned long long)i);
        }
    return HIPRAG_OK;
}

}  // namespace

void swap_buf(DevBuf& x, DevBuf& y)
{
    std::swap(x.p, y.p);
    std::swap(x.bytes, y.bytes);
}

void launch_excl_scan(const u32* counts_dev, i64 n, u64* base_dev)
{
    hipLaunchKernelGGL(rm_scan_kernel, dim3(1), dim3(kScanThreads), 0, nullptr, counts_dev, n, base_dev);
}

void Bm25Index::drop_doc_workspaces()
{
    acc.release();
    ck.release();
    ci.release();
    ws_k = 0;
}

// room for `need` postings in every posting buffer: the live ones keep their content (the caller fills doc_ids2 / tf2 and
// swaps); impacts are rewritten by the reweigh that has to follow, so they are not carried over -- those of an impact handle
// are its live stream and are left alone
int32_t Bm25Index::reserve_postings(i64 need, bool* grew, i64* extra)
{
    int32_t rc;
    i64 cap = cap_postings;
    if (need > cap) {
        cap = round4(std::max(need, cap + cap / 2));
        *grew = true;
    }
    const size_t bytes = (size_t)cap * sizeof(u32);
    for (DevBuf* bf : {&doc_ids2, &tf2, &impacts})
        if (bf->bytes < bytes && (has_tf || bf != &impacts)) {
            *extra += (i64)bytes;
            if ((rc = bf->reserve(bytes))) return rc;
        }
    cap_postings = cap;
    return HIPRAG_OK;
}

int32_t Bm25Index::plan_merge(i64 n_terms_after, const uint64_t* boff, std::vector<uint64_t>& noff) const
{
    const i64 P_old = n_postings;
    noff.resize((size_t)n_terms_after + 1);
    for (i64 t = 0; t <= n_terms_after; ++t) noff[(size_t)t] = (t <= n_terms ? offsets[(size_t)t] : (uint64_t)P_old) + boff[t];
    for (i64 t = 0; t < n_terms_after; ++t) {
        const uint64_t len = noff[(size_t)t + 1] - noff[(size_t)t];
        HR_REQUIRE(len < kSkipMinDf || len < (1ull << 32), "posting list of term %lld would be too long for u32 skip offsets", (long long)t);
    }
    return HIPRAG_OK;
}

int32_t Bm25Index::merge_batch(DevBuf& pay, i64 n_terms_after, std::vector<uint64_t>& noff, const uint64_t* boff, const u64* boff_dev,
                               const u32* bids_dev, const u32* bpay_dev, bool* grew, i64* extra, i64* moved)
{
    int32_t rc;
    const i64 P_old = n_postings, Pb = (i64)boff[n_terms_after], P_new = P_old + Pb;
    if ((rc = offsets2.reserve(noff.size() * sizeof(u64)))) return rc;
    HR_CHECK_HIP(hipMemcpy(offsets2.p, noff.data(), noff.size() * sizeof(u64), hipMemcpyHostToDevice));
    if (Pb > 0) {
        if ((rc = reserve_postings(P_new, grew, extra))) return rc;
        AppendArgs a;
        a.old_ids = doc_ids.as<u32>(); a.old_tf = pay.as<u32>(); a.old_off = offsets_dev.as<u64>();
        a.b_ids = bids_dev; a.b_tf = bpay_dev; a.b_off = boff_dev;
        a.new_off = offsets2.as<u64>();
        a.dst_ids = doc_ids2.as<u32>(); a.dst_tf = tf2.as<u32>();
        a.P = (u64)P_new;
        a.n_terms = (u32)n_terms_after; a.n_terms_old = (u32)n_terms; a.doc_base = (u32)n_docs;
        hipLaunchKernelGGL(append_kernel, dim3((unsigned)((P_new + kUpdChunk - 1) / kUpdChunk)), dim3(kUpdThreads), 0, nullptr, a);
        HR_CHECK_HIP(hipGetLastError());
        HR_CHECK_HIP(hipStreamSynchronize(nullptr));
        swap_buf(doc_ids, doc_ids2);
        swap_buf(pay, tf2);
        // everything before the end of the first list that gains a posting stays where it was
        for (i64 t = 0; t < n_terms_after; ++t)
            if (boff[t + 1] > boff[t]) { *moved += P_new - (i64)(noff[(size_t)t] + (t < n_terms ? offsets[(size_t)t + 1] - offsets[(size_t)t] : 0)); break; }
    }
    swap_buf(offsets_dev, offsets2);
    offsets.swap(noff);
    n_terms = n_terms_after;
    n_postings = P_new;
    skip_index.resize((size_t)n_terms, -1);   // new terms have empty lists; the skip tables are rebuilt behind the update
    return HIPRAG_OK;
}

int32_t Bm25Index::append(i64 n_new, i64 n_terms_after, const uint64_t* boff, const uint32_t* bids, const uint32_t* btf, const uint32_t* bdl)
{
    if (has_impacts) {
        set_error("this bm25 handle was made by hipbm25_create_impacts and holds impacts as given, no term frequencies: append to it "
                  "with hipbm25_append_impacts or hipbm25_append_rows_dev");
        return HIPRAG_E_UNSUPPORTED;
    }
    if (!has_tf) {
        set_error("this bm25 handle was made by hipbm25_create and holds no term frequencies: hipbm25_append needs hipbm25_create_tf");
        return HIPRAG_E_UNSUPPORTED;
    }
    HR_REQUIRE(n_new >= 0, "n_new_docs must not be negative (got %lld)", (long long)n_new);
    HR_REQUIRE(n_terms_after >= n_terms, "n_terms_after = %lld is below the handle's n_terms = %lld: the vocabulary only grows",
               (long long)n_terms_after, (long long)n_terms);
    HR_REQUIRE(n_terms_after < (1ll << 32), "term ids are u32: n_terms_after must be < 2^32");
    HR_REQUIRE(n_docs + n_new < (1ll << 32), "doc ids are u32: %lld + %lld documents pass 2^32", (long long)n_docs, (long long)n_new);
    int32_t rc;
    if ((rc = check_csr("batch_", n_new, n_terms_after, boff, bids, btf))) return rc;
    HR_REQUIRE(n_new == 0 || bdl, "batch_doc_len is null");
    const i64 P_old = n_postings, Pb = (i64)boff[n_terms_after];
    std::vector<uint64_t> noff;
    if ((rc = plan_merge(n_terms_after, boff, noff))) return rc;
    if (prev_ev_set) HR_CHECK_HIP(hipEventSynchronize(prev_ev));
    i64 extra = 0, moved = 0;
    bool grew = false;
    const i64 docs_before = n_docs;
    DevBuf b_ids, b_tf, b_off;     // freed behind the synchronisation below
    if (Pb > 0) {
        if ((rc = b_ids.reserve((size_t)Pb * sizeof(u32))) || (rc = b_tf.reserve((size_t)Pb * sizeof(u32))) ||
            (rc = b_off.reserve(noff.size() * sizeof(u64))))
            return rc;
        extra += (i64)(b_ids.bytes + b_tf.bytes + b_off.bytes);
        HR_CHECK_HIP(hipMemcpy(b_ids.p, bids, (size_t)Pb * sizeof(u32), hipMemcpyHostToDevice));
        HR_CHECK_HIP(hipMemcpy(b_tf.p, btf, (size_t)Pb * sizeof(u32), hipMemcpyHostToDevice));
        HR_CHECK_HIP(hipMemcpy(b_off.p, boff, noff.size() * sizeof(u64), hipMemcpyHostToDevice));
    }
    if ((rc = merge_batch(tf, n_terms_after, noff, boff, b_off.as<u64>(), b_ids.as<u32>(), b_tf.as<u32>(), &grew, &extra, &moved))) return rc;
    const i64 P_new = n_postings;
    if (n_new > 0) {
        if (n_docs + n_new > cap_docs) {
            const i64 cap = round4(std::max(n_docs + n_new, cap_docs + cap_docs / 2));
            const size_t before = doc_len.bytes;
            if ((rc = grow_keep(doc_len, (size_t)n_docs * sizeof(u32), (size_t)cap * sizeof(u32)))) return rc;
            extra += (i64)(doc_len.bytes - before);
            cap_docs = cap;
            grew = true;
        }
        HR_CHECK_HIP(hipMemcpy(doc_len.as<u32>() + n_docs, bdl, (size_t)n_new * sizeof(u32), hipMemcpyHostToDevice));
        for (i64 i = 0; i < n_new; ++i) total_len += bdl[i];
        n_docs += n_new;
        drop_doc_workspaces();
        dirty = true;     // N and avgdl changed: every impact is stale
    }
    const i64 info[8] = {2, P_old, P_new, moved, docs_before, n_docs, extra, grew ? 1 : 0};
    memcpy(upd_info, info, sizeof(info));
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    return HIPRAG_OK;
}

int32_t Bm25Index::remove_ranges(const int64_t* ranges, int32_t n_ranges)
{
    if (!has_tf && !has_impacts) {
        set_error("this bm25 handle was made by hipbm25_create and holds no term frequencies: hipbm25_remove_ranges needs hipbm25_create_tf");
        return HIPRAG_E_UNSUPPORTED;
    }
    DevBuf& pay = has_tf ? tf : impacts;   // the 32-bit stream that travels with doc_ids: tf, or an impact handle's impacts as bits
    RangeTable joined;
    int32_t rc;
    if ((rc = range_table(ranges, n_ranges, n_docs, "n_docs", true, joined))) return rc;
    std::vector<RmRange> tab;
    i64 removed = 0;
    for (const auto& r : joined) {
        tab.push_back(RmRange{(u32)r.first, (u32)r.second, (u32)removed, 0});
        removed += r.second - r.first;
    }
    const i64 P_old = n_postings, docs_before = n_docs, n_new = n_docs - removed;
    const i64 none[8] = {3, P_old, P_old, 0, docs_before, docs_before, 0, 0};
    memcpy(upd_info, none, sizeof(none));
    if (removed == 0) return HIPRAG_OK;    // nothing to remove: the handle stays as it is, clean if it was
    if (prev_ev_set) HR_CHECK_HIP(hipEventSynchronize(prev_ev));
    i64 extra = 0, moved = 0, P_new = P_old;
    bool grew = false;
    DevBuf tab_dev, counts, base, scal, dl2;   // freed behind the synchronisation below
    if ((rc = tab_dev.reserve(tab.size() * sizeof(RmRange)))) return rc;
    HR_CHECK_HIP(hipMemcpy(tab_dev.p, tab.data(), tab.size() * sizeof(RmRange), hipMemcpyHostToDevice));
    if ((rc = scal.reserve(2 * sizeof(u64)))) return rc;    // [0] first removed posting, [1] sum of the surviving doc_len
    const u64 scal0[2] = {~0ull, 0ull};
    HR_CHECK_HIP(hipMemcpy(scal.p, scal0, sizeof(scal0), hipMemcpyHostToDevice));
    extra += (i64)(tab_dev.bytes + scal.bytes);
    if (P_old > 0) {
        const i64 nblk = P_old / kUpdChunk + 1;
        if ((rc = reserve_postings(P_old, &grew, &extra))) return rc;
        if ((rc = offsets2.reserve((size_t)(n_terms + 1) * sizeof(u64)))) return rc;
        if ((rc = counts.reserve((size_t)nblk * sizeof(u32))) || (rc = base.reserve((size_t)(nblk + 1) * sizeof(u64)))) return rc;
        extra += (i64)(counts.bytes + base.bytes);
        hipLaunchKernelGGL(rm_count_kernel, dim3((unsigned)nblk), dim3(kUpdThreads), 0, nullptr, (const u32*)doc_ids.as<u32>(), (u64)P_old,
                           (const RmRange*)tab_dev.as<RmRange>(), (int)tab.size(), counts.as<u32>(), scal.as<u64>());
        hipLaunchKernelGGL(rm_scan_kernel, dim3(1), dim3(kScanThreads), 0, nullptr, (const u32*)counts.as<u32>(), nblk, base.as<u64>());
        ScatterArgs a;
        a.src_ids = doc_ids.as<u32>(); a.src_tf = pay.as<u32>(); a.old_off = offsets_dev.as<u64>();
        a.dst_ids = doc_ids2.as<u32>(); a.dst_tf = tf2.as<u32>(); a.new_off = offsets2.as<u64>();
        a.base = base.as<u64>(); a.tab = tab_dev.as<RmRange>(); a.n_tab = (int)tab.size();
        a.n_terms = (u32)n_terms; a.P = (u64)P_old;
        hipLaunchKernelGGL(rm_scatter_kernel, dim3((unsigned)nblk), dim3(kUpdThreads), 0, nullptr, a);
        HR_CHECK_HIP(hipGetLastError());
    }
    if (has_tf) {
        if ((rc = dl2.reserve((size_t)cap_docs * sizeof(u32)))) return rc;
        extra += (i64)dl2.bytes;
    }
    if (has_tf && n_new > 0) {
        hipLaunchKernelGGL(rm_doclen_kernel, dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, nullptr, (const u32*)doc_len.as<u32>(),
                           dl2.as<u32>(), n_new, (const RmRange*)tab_dev.as<RmRange>(), (int)tab.size(),
                           reinterpret_cast<unsigned long long*>(scal.as<u64>() + 1));
        HR_CHECK_HIP(hipGetLastError());
    }
    u64 scal_h[2];
    HR_CHECK_HIP(hipMemcpy(scal_h, scal.p, sizeof(scal_h), hipMemcpyDeviceToHost));   // synchronises the null stream
    if (P_old > 0) {
        HR_CHECK_HIP(hipMemcpy(offsets.data(), offsets2.p, (size_t)(n_terms + 1) * sizeof(u64), hipMemcpyDeviceToHost));
        P_new = (i64)offsets[(size_t)n_terms];
        if (scal_h[0] != ~0ull) moved = P_new - (i64)scal_h[0];   // the survivors behind the first removed posting
        swap_buf(doc_ids, doc_ids2);
        swap_buf(pay, tf2);
        swap_buf(offsets_dev, offsets2);
    }
    if (has_tf) {
        swap_buf(doc_len, dl2);
        total_len = (i64)scal_h[1];
    }
    n_docs = n_new;
    n_postings = P_new;
    drop_doc_workspaces();
    if (has_tf) dirty = true;
    else if ((rc = rebuild_skips())) return rc;   // impacts do not depend on N, df or avgdl: the handle stays clean
    const i64 info[8] = {3, P_old, P_new, moved, docs_before, n_new, extra, grew ? 1 : 0};
    memcpy(upd_info, info, sizeof(info));
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    return HIPRAG_OK;
}

int32_t Bm25Index::reweigh(const double* idf_host)
{
    if (has_impacts) {
        set_error("this bm25 handle was made by hipbm25_create_impacts: its impacts are kept as given and there is nothing to reweigh");
        return HIPRAG_E_UNSUPPORTED;
    }
    if (!has_tf) {
        set_error("this bm25 handle was made by hipbm25_create and holds no term frequencies: hipbm25_reweigh needs hipbm25_create_tf");
        return HIPRAG_E_UNSUPPORTED;
    }
    if (prev_ev_set) HR_CHECK_HIP(hipEventSynchronize(prev_ev));
    int32_t rc;
    std::vector<double> own;
    if (!idf_host) {   // the expression of build_postings, operation for operation, with the C library's log
        own.resize((size_t)n_terms);
        const double n_all = (double)n_docs;
        for (i64 t = 0; t < n_terms; ++t) {
            const double df = (double)(offsets[(size_t)t + 1] - offsets[(size_t)t]);
            own[(size_t)t] = std::log(1.0 + ((n_all - df) + 0.5) / (df + 0.5));
        }
        idf_host = own.data();
    }
    if (n_postings > 0) {
        if ((rc = idf_dev.reserve((size_t)n_terms * sizeof(double)))) return rc;
        HR_CHECK_HIP(hipMemcpy(idf_dev.p, idf_host, (size_t)n_terms * sizeof(double), hipMemcpyHostToDevice));
        ReweighArgs a;
        a.doc_ids = doc_ids.as<u32>(); a.tf = tf.as<u32>(); a.doc_len = doc_len.as<u32>(); a.off = offsets_dev.as<u64>();
        a.idf = idf_dev.as<double>(); a.impacts = impacts.as<float>();
        a.P = (u64)n_postings; a.n_terms = (u32)n_terms;
        a.avgdl = n_docs ? (double)total_len / (double)n_docs : 1.0;
        a.k1 = k1; a.b = b;
        hipLaunchKernelGGL(reweigh_kernel, dim3((unsigned)((n_postings + kUpdChunk - 1) / kUpdChunk)), dim3(kUpdThreads), 0, nullptr, a);
        HR_CHECK_HIP(hipGetLastError());
    }
    if ((rc = rebuild_skips())) return rc;
    dirty = false;
    return HIPRAG_OK;
}

// skip tables of the lists that are long NOW: ntiles() follows n_docs, lists cross kSkipMinDf in either direction
int32_t Bm25Index::rebuild_skips()
{
    int32_t rc;
    const i64 nt1 = ntiles() + 1;
    std::vector<u32> longs;
    skip_index.assign((size_t)n_terms, -1);
    for (i64 t = 0; t < n_terms; ++t)
        if (offsets[(size_t)t + 1] - offsets[(size_t)t] >= kSkipMinDf) {
            skip_index[(size_t)t] = (i64)longs.size() * nt1;
            longs.push_back((u32)t);
        }
    const i64 n_skip = (i64)longs.size() * nt1;
    if ((rc = skip_dev.reserve(std::max<size_t>(16, (size_t)n_skip * sizeof(u32))))) return rc;
    if (n_skip > 0) {
        if ((rc = long_dev.reserve(longs.size() * sizeof(u32)))) return rc;
        HR_CHECK_HIP(hipMemcpy(long_dev.p, longs.data(), longs.size() * sizeof(u32), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(skip_kernel, dim3((unsigned)((n_skip + 255) / 256)), dim3(256), 0, nullptr, (const u32*)doc_ids.as<u32>(),
                           (const u64*)offsets_dev.as<u64>(), (const u32*)long_dev.as<u32>(), (i64)longs.size(), nt1, skip_dev.as<u32>());
        HR_CHECK_HIP(hipGetLastError());
    }
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    return HIPRAG_OK;
}

}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipbm25_create_tf(int64_t n_docs, int64_t n_terms, const uint64_t* offsets_host, const uint32_t* doc_ids_host,
                          const uint32_t* tf_host, const uint32_t* doc_len_host, double k1, double b, int32_t device,
                          uint64_t* out_handle)
{
    HR_REQUIRE(out_handle, "out_handle is null");
    HR_REQUIRE(n_docs >= 0 && n_terms >= 0, "negative sizes");
    HR_REQUIRE(n_docs < (1ll << 32), "doc ids are u32: n_docs must be < 2^32 per shard");
    HR_REQUIRE(n_terms < (1ll << 32), "term ids are u32: n_terms must be < 2^32");
    HR_REQUIRE(k1 >= 0.0, "k1 must not be negative (got %g)", k1);
    HR_REQUIRE(b >= 0.0 && b <= 1.0, "b must be in 0..1 (got %g)", b);
    int32_t rc;
    if ((rc = check_csr("", n_docs, n_terms, offsets_host, doc_ids_host, tf_host))) return rc;
    HR_REQUIRE(n_docs == 0 || doc_len_host, "doc_len is null");
    for (int64_t t = 0; t < n_terms; ++t) {
        const uint64_t len = offsets_host[t + 1] - offsets_host[t];
        HR_REQUIRE(len < kSkipMinDf || len < (1ull << 32), "posting list of term %lld is too long for u32 skip offsets", (long long)t);
    }
    const uint64_t P = offsets_host[n_terms];
    auto ix = std::make_shared<Bm25Index>();
    ix->device = device;
    ix->has_tf = true;
    ix->k1 = k1;
    ix->b = b;
    ix->n_docs = n_docs;
    ix->n_terms = n_terms;
    ix->n_postings = (i64)P;
    ix->offsets.assign(offsets_host, offsets_host + n_terms + 1);
    for (int64_t i = 0; i < n_docs; ++i) ix->total_len += doc_len_host[i];
    HR_CHECK_HIP(hipSetDevice(device));
    ix->cap_postings = round4((i64)P);
    ix->cap_docs = round4(n_docs);
    if ((rc = ix->doc_ids.reserve((size_t)ix->cap_postings * sizeof(u32))) || (rc = ix->tf.reserve((size_t)ix->cap_postings * sizeof(u32))) ||
        (rc = ix->impacts.reserve((size_t)ix->cap_postings * sizeof(float))) || (rc = ix->doc_len.reserve((size_t)ix->cap_docs * sizeof(u32))) ||
        (rc = ix->offsets_dev.reserve((size_t)(n_terms + 1) * sizeof(u64))))
        return rc;
    if (P) {
        HR_CHECK_HIP(hipMemcpy(ix->doc_ids.p, doc_ids_host, P * sizeof(u32), hipMemcpyHostToDevice));
        HR_CHECK_HIP(hipMemcpy(ix->tf.p, tf_host, P * sizeof(u32), hipMemcpyHostToDevice));
    }
    if (n_docs) HR_CHECK_HIP(hipMemcpy(ix->doc_len.p, doc_len_host, (size_t)n_docs * sizeof(u32), hipMemcpyHostToDevice));
    HR_CHECK_HIP(hipMemcpy(ix->offsets_dev.p, ix->offsets.data(), (size_t)(n_terms + 1) * sizeof(u64), hipMemcpyHostToDevice));
    ix->read_env();
    if ((rc = ix->reweigh(nullptr))) return rc;
    const i64 info[8] = {1, 0, (i64)P, 0, 0, n_docs, 0, 0};
    memcpy(ix->upd_info, info, sizeof(info));
    *out_handle = bm25_reg().put(ix);
    return HIPRAG_OK;
}

int32_t hipbm25_append(uint64_t h, int64_t n_new_docs, int64_t n_terms_after, const uint64_t* batch_offsets_host,
                       const uint32_t* batch_doc_ids_host, const uint32_t* batch_tf_host, const uint32_t* batch_doc_len_host)
{
    GET_BM25(h);
    return ix->append(n_new_docs, n_terms_after, batch_offsets_host, batch_doc_ids_host, batch_tf_host, batch_doc_len_host);
}

int32_t hipbm25_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges)
{
    GET_BM25(h);
    return ix->remove_ranges(ranges_host, n_ranges);
}

int32_t hipbm25_reweigh(uint64_t h, const double* idf_host)
{
    GET_BM25(h);
    return ix->reweigh(idf_host);
}

int32_t hipbm25_export(uint64_t h, uint64_t* offsets, uint32_t* doc_ids, uint32_t* tf, float* impacts, uint32_t* doc_len)
{
    GET_BM25(h);
    if (tf || doc_len) {
        if (!ix->has_tf) {
            set_error("this bm25 handle was made by %s: it holds neither term frequencies nor document lengths",
                      ix->has_impacts ? "hipbm25_create_impacts" : "hipbm25_create");
            return HIPRAG_E_UNSUPPORTED;
        }
    }
    HR_CHECK_HIP(hipDeviceSynchronize());
    const size_t P = (size_t)ix->n_postings;
    if (offsets) memcpy(offsets, ix->offsets.data(), ix->offsets.size() * sizeof(uint64_t));
    if (doc_ids && P) HR_CHECK_HIP(hipMemcpy(doc_ids, ix->doc_ids.p, P * sizeof(u32), hipMemcpyDeviceToHost));
    if (tf && P) HR_CHECK_HIP(hipMemcpy(tf, ix->tf.p, P * sizeof(u32), hipMemcpyDeviceToHost));
    if (impacts && P) HR_CHECK_HIP(hipMemcpy(impacts, ix->impacts.p, P * sizeof(float), hipMemcpyDeviceToHost));
    if (doc_len && ix->n_docs) HR_CHECK_HIP(hipMemcpy(doc_len, ix->doc_len.p, (size_t)ix->n_docs * sizeof(u32), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t hipbm25_update_info(uint64_t h, int64_t* out8)
{
    GET_BM25(h);
    HR_REQUIRE(out8, "out8 is null");
    for (int i = 0; i < 8; ++i) out8[i] = ix->upd_info[i];
    return HIPRAG_OK;
}

int32_t hipbm25_sizes(uint64_t h, int64_t* out4)
{
    GET_BM25(h);
    HR_REQUIRE(out4, "out4 is null");
    out4[0] = ix->n_docs;
    out4[1] = ix->n_terms;
    out4[2] = ix->n_postings;
    out4[3] = (ix->has_tf ? 1 : 0) | (ix->dirty ? 2 : 0) | (ix->has_impacts ? 4 : 0);
    return HIPRAG_OK;
}

/* test hook, no GPU: the impact formula of the reweigh kernel evaluated on the host */
int32_t hipbm25_impacts_host(const double* idf, const uint32_t* tf, const uint32_t* dl, int64_t n, double avgdl, double k1, double b,
                             float* out)
{
    HR_REQUIRE(n >= 0, "n must not be negative (got %lld)", (long long)n);
    HR_REQUIRE(n == 0 || (idf && tf && dl && out), "null argument");
    HR_REQUIRE(k1 >= 0.0, "k1 must not be negative (got %g)", k1);
    HR_REQUIRE(b >= 0.0 && b <= 1.0, "b must be in 0..1 (got %g)", b);
    HR_REQUIRE(avgdl > 0.0, "avgdl must be positive (got %g)", avgdl);
    for (int64_t i = 0; i < n; ++i) out[i] = bm25_impact(idf[i], (double)tf[i], (double)dl[i], avgdl, k1, b);
    return HIPRAG_OK;
}

}  // extern "C"
