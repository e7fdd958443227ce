// ivf_update.hip -- hipivf_from_centroids, hipivf_add(_dev), hipivf_remove_ranges: the membership of the lists of an IVF-Flat
// index changes in place.  The k-means, the layout rule and the searches are ivf_build.hip and ivf_search.hip.
#include <algorithm>
#include <vector>

#include "ivf_internal.h"
#include "range_table.h"

namespace hiprag {
namespace {

// ------------------------------------------------------------------------------------------------------
// An update is a RELAYOUT of the rows index's blocked storage (dense_layout.h) and of `orig`.  The layout rule of the build
// (lists in list order, ascending id within a list, every list padded to whole 32-row blocks with zero rows of id -1) fixes
// the new place of every row, and the host, which knows the length of every list, writes it down as a RUN TABLE: ascending
// first destination rows, and for every run where its rows come from --
//   kRunSkip   they stand where they stood (neither read nor written)
//   kRunOld    stored rows run_src, run_src + 1, ... of the index itself
//   kRunNew    rows run_src, ... of the BATCH: the new rows, sorted by list, tiled once by the ordinary add path into a
//              temporary flat index; their ids are id_base + batch_order[row]
//   kRunZero   padding: zero rows of id -1
// so every stored byte was produced by retile_kernel / retile_bf16_kernel / row_stats_kernel or is a copy of bytes they
// produced.  ivf_relayout_kernel is move_rows_kernel (dense_remove.hip) with that table: one wave per destination block,
// lane (h, r) bisects the table for its row and copies its float4 of every 1 KiB fp32 piece, its 16 B of every piece of the
// bf16 filter copy, the norm (h = 0) and the original id (h = 1).  Plain 16-byte vector loads and stores, eight in flight
// per lane, no LDS, no atomics.  GATHER: sources -> staging (chunk-relative blocks); !GATHER: staging -> index.
// Bound: HBM -- a moved row is read and written twice (through the staging buffer).
// ------------------------------------------------------------------------------------------------------
enum { kRunSkip = 0, kRunOld = 1, kRunNew = 2, kRunZero = 3 };

struct RelayoutArgs {
    const float4* src_xb[2];   // [0] the index (writing back: the staging buffer), [1] the tiled batch
    const float4* src_xh[2];
    const float* src_n[2];
    const i64* src_orig;       // original ids of the index (writing back: of the staging buffer)
    const i64* batch_order;    // batch row -> its position in the caller's array
    i64 id_base;               // id of the caller's row 0
    float4* dst_xb;
    float4* dst_xh;
    float* dst_n;
    i64* dst_orig;
    const i64* run_dst;        // [n_runs] ascending, run_dst[0] == 0
    const i64* run_src;
    const int* run_kind;
    int n_runs;
    i64 blk0, nblk;            // destination blocks [blk0, blk0 + nblk) of the index; staging block = block - blk0
    int P;
};

template <bool GATHER>
__global__ __launch_bounds__(256) void ivf_relayout_kernel(RelayoutArgs a)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const i64 nw = (i64)gridDim.x * 4;
    const int P2 = a.P / 2;
    for (i64 w = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); w < a.nblk; w += nw) {
        const i64 blk = a.blk0 + w;
        const i64 row = blk * kRowsPerBlock + r;
        int lo = 0, hi = a.n_runs;          // the last run that starts at or before `row`
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.run_dst[mid] <= row) lo = mid; else hi = mid;
        }
        const int kind = a.run_kind[lo];
        if (kind == kRunSkip) continue;
        const bool live = !GATHER || kind != kRunZero;
        const int which = (GATHER && kind == kRunNew) ? 1 : 0;
        const i64 srow = live ? (GATHER ? a.run_src[lo] + (row - a.run_dst[lo]) : w * kRowsPerBlock + r) : 0;
        const i64 sblk = srow / kRowsPerBlock, dblk = GATHER ? w : blk;
        const int sr = (int)(srow % kRowsPerBlock);
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4* s = a.src_xb[which] + sblk * a.P * kPieceVec4 + piece_slot(h, sr);
        float4* o = a.dst_xb + dblk * a.P * kPieceVec4 + piece_slot(h, r);
        for (int p = 0; p < a.P; p += 8) {          // P is a multiple of 16
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = live ? s[(p + u) * kPieceVec4] : zero;
#pragma unroll
            for (int u = 0; u < 8; ++u) o[(p + u) * kPieceVec4] = v[u];
        }
        s = a.src_xh[which] + sblk * P2 * 64 + h * 32 + sr;
        o = a.dst_xh + dblk * P2 * 64 + lane;
        for (int p = 0; p < P2; p += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = live ? s[(p + u) * 64] : zero;
#pragma unroll
            for (int u = 0; u < 8; ++u) o[(p + u) * 64] = v[u];
        }
        if (h == 0) {
            a.dst_n[dblk * kRowsPerBlock + r] = live ? a.src_n[which][srow] : 0.f;
        } else {
            i64 id = -1;
            if (live) id = which ? a.id_base + a.batch_order[srow] : a.src_orig[srow];
            a.dst_orig[dblk * kRowsPerBlock + r] = id;
        }
    }
}

// len[l] = members of list l, read off the layout: a list's padding is the tail of its last block.  bad[0] = 1 when a
// non-empty list ends in a block of padding only.
__global__ void ivf_list_len_kernel(const i64* __restrict__ orig, const i64* __restrict__ offs, int nlist, i64* __restrict__ len,
                                    int* __restrict__ bad)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nlist) return;
    const i64 rows = offs[l + 1] - offs[l];
    i64 cnt = 0;
    if (rows > 0) {
        for (int r = 0; r < kRowsPerBlock; ++r) cnt += orig[offs[l + 1] - kRowsPerBlock + r] >= 0;
        if (cnt == 0) bad[0] = 1;
    }
    len[l] = rows > 0 ? rows - kRowsPerBlock + cnt : 0;
}

// bad[0] = 1 unless every list is its len[l] members in ascending id followed by padding (every thread stores the same 1)
__global__ void ivf_layout_check_kernel(const i64* __restrict__ orig, const i64* __restrict__ offs, const i64* __restrict__ len,
                                        int nlist, i64 stored, int* __restrict__ bad)
{
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < stored; j += (i64)gridDim.x * blockDim.x) {
        int lo = 0, hi = nlist;             // the last list that starts at or before j: the one that holds it
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offs[mid] <= j) lo = mid; else hi = mid;
        }
        const i64 id = orig[j];
        const bool ok = j < offs[lo] + len[lo] ? (id >= 0 && (j == offs[lo] || orig[j - 1] < id)) : id == -1;
        if (!ok) bad[0] = 1;
    }
}

// pos[l][b] = members of list l whose id is below bounds[b] (ids ascend within a list: a bisection)
__global__ void ivf_range_pos_kernel(const i64* __restrict__ orig, const i64* __restrict__ offs, const i64* __restrict__ len,
                                     const i64* __restrict__ bounds, int nb, int nlist, i64* __restrict__ pos)
{
    const i64 total = (i64)nlist * nb;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (i64)gridDim.x * blockDim.x) {
        const int l = (int)(t / nb);
        const i64 bound = bounds[t - (i64)l * nb];
        const i64* ids = orig + offs[l];
        i64 lo = 0, hi = len[l];            // ids[lo - 1] < bound <= ids[hi]
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (ids[mid] < bound) lo = mid + 1; else hi = mid;
        }
        pos[t] = lo;
    }
}

// new id = old id minus the ids removed before it: cut[j] = ids removed by ranges 0..j, range_lo ascending
__global__ void ivf_renumber_kernel(i64* __restrict__ orig, i64 stored, const i64* __restrict__ range_lo, const i64* __restrict__ cut,
                                    int nr)
{
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < stored; j += (i64)gridDim.x * blockDim.x) {
        const i64 id = orig[j];
        if (id < range_lo[0]) continue;     // padding (-1) included
        int lo = 0, hi = nr;                // the last range that starts at or before id
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (range_lo[mid] <= id) lo = mid; else hi = mid;
        }
        orig[j] = id - cut[lo];
    }
}

// the two certificate maxima after an add: max(the index's, the batch's)
__global__ void ivf_max_scalars_kernel(unsigned* __restrict__ dst, const unsigned* __restrict__ src)
{
    if (threadIdx.x < 2) dst[threadIdx.x] = max(dst[threadIdx.x], src[threadIdx.x]);
}

unsigned flat_grid(i64 n) { return (unsigned)std::max<i64>(1, std::min<i64>((n + 255) / 256, 4096)); }

struct RunTable {
    std::vector<i64> dst, src;
    std::vector<int> kind;
    i64 moved = 0;             // rows of kRunOld runs
    void push(i64 d, i64 s, int k, i64 rows)
    {
        if (rows <= 0) return;
        if (k == kRunOld && s == d) k = kRunSkip;
        if (k == kRunOld) moved += rows;
        if (k == kRunSkip && !kind.empty() && kind.back() == kRunSkip) return;   // the run before extends over these rows
        dst.push_back(d); src.push_back(s); kind.push_back(k);
    }
};

const char* const kCannotUpdate = "it can be searched but not updated";

i64 pad32(i64 v) { return (v + kRowsPerBlock - 1) / kRowsPerBlock * kRowsPerBlock; }

}  // namespace

// The members of every list, on first use: read off `orig`, and the layout checked to be the build's (a HIPIVF01 file
// need not be: hipivf_load accepts any padding; neither need the lists of a hipivf_create handle).  The lengths stay on the
// device as lens_dev for the scope-aware probing (ivf_scoped.hip).
int32_t ensure_lens(IvfIndex& iv, const char* cannot)
{
    const int nlist = iv.nlist;
    int32_t rc;
    if (iv.lens_known) {                         // hipivf_from_centroids knows its lengths without a device copy
        if (iv.lens_dev.p) return HIPRAG_OK;
        if ((rc = iv.lens_dev.reserve((size_t)nlist * 8))) return rc;
        HR_CHECK_HIP(hipMemcpy(iv.lens_dev.p, iv.lens_host.data(), (size_t)nlist * 8, hipMemcpyHostToDevice));
        return HIPRAG_OK;
    }
    const i64 stored = iv.rows->ntotal;
    bool bad_host_layout = false;            // hipivf_create: lists start on 32-row blocks, the last may end anywhere
    for (int l = 0; l < nlist; ++l) bad_host_layout |= (iv.offs_host[(size_t)l + 1] - iv.offs_host[(size_t)l]) % kRowsPerBlock != 0;
    DevBuf len, bad;
    int bad_host = bad_host_layout ? 1 : 0;
    std::vector<i64> lens((size_t)nlist);
    if (!bad_host_layout) {
        if ((rc = len.reserve((size_t)nlist * 8)) || (rc = bad.reserve(4)) || (rc = iv.lens_dev.reserve((size_t)nlist * 8))) return rc;
        HR_CHECK_HIP(hipMemsetAsync(bad.p, 0, 4, nullptr));
        hipLaunchKernelGGL(ivf_list_len_kernel, dim3((unsigned)((nlist + 255) / 256)), dim3(256), 0, nullptr, iv.orig.as<i64>(),
                           iv.offs.as<i64>(), nlist, len.as<i64>(), bad.as<int>());
        if (stored > 0)
            hipLaunchKernelGGL(ivf_layout_check_kernel, dim3(flat_grid(stored)), dim3(256), 0, nullptr, iv.orig.as<i64>(), iv.offs.as<i64>(),
                               len.as<i64>(), nlist, stored, bad.as<int>());
        HR_CHECK_HIP(hipGetLastError());
        HR_CHECK_HIP(hipMemcpy(&bad_host, bad.p, 4, hipMemcpyDeviceToHost));
        HR_CHECK_HIP(hipMemcpy(lens.data(), len.p, (size_t)nlist * 8, hipMemcpyDeviceToHost));
    }
    if (bad_host) {
        set_error("the lists of this IVF index are not in the build's layout (ascending id within a list, padding only behind "
                  "the members, less than a block of it): %s", cannot);
        return HIPRAG_E_UNSUPPORTED;
    }
    HR_CHECK_HIP(hipMemcpy(iv.lens_dev.p, lens.data(), (size_t)nlist * 8, hipMemcpyHostToDevice));
    iv.lens_host = std::move(lens);
    iv.lens_known = true;
    return HIPRAG_OK;
}

namespace {

int32_t require_owned(const IvfIndex& iv)
{
    if (!iv.attached) return HIPRAG_OK;
    set_error("this IVF handle was made by hipivf_create over the caller's own flat indexes: the caller owns those rows, and "
              "an update would move them under the caller's handles (build, load or hipivf_from_centroids give an index that "
              "can be updated)");
    return HIPRAG_E_UNSUPPORTED;
}

// `orig` holds at least `need` ids, its first `keep` kept
int32_t grow_orig(IvfIndex& iv, i64 keep, i64 need)
{
    if ((size_t)need * 8 <= iv.orig.bytes) return HIPRAG_OK;
    const i64 cap = (i64)(iv.orig.bytes / 8);
    DevBuf nb;
    int32_t rc = nb.reserve((size_t)std::max(need, cap + cap / 2) * 8);
    if (rc) return rc;
    if (keep > 0) HR_CHECK_HIP(hipMemcpy(nb.p, iv.orig.p, (size_t)keep * 8, hipMemcpyDeviceToDevice));
    std::swap(nb.p, iv.orig.p);
    std::swap(nb.bytes, iv.orig.bytes);
    return HIPRAG_OK;
}

// Moves the rows as the table says, in chunks of destination blocks that are gathered completely into the staging buffer
// and then written back.  An add only moves rows up (dst >= src), so its chunks DESCEND: what a write-back overwrites can
// only be the source of destinations inside the chunk or above it -- all gathered already.  A removal only moves rows down
// and its chunks ASCEND, as in dense_remove.hip.  Staging + table <= DenseIndex::kRemoveBudget whatever N is.
int32_t relayout(IvfIndex& iv, const RunTable& t, i64 stored_new, bool descending, const DenseIndex* batch, const i64* batch_order,
                 i64 id_base, hipStream_t st, DevBuf& stage, DevBuf& tab)
{
    DenseIndex& R = *iv.rows;
    const int n_runs = (int)t.dst.size();
    int first = 0, last = n_runs - 1;
    while (first < n_runs && t.kind[(size_t)first] == kRunSkip) ++first;
    while (last >= 0 && t.kind[(size_t)last] == kRunSkip) --last;
    if (first > last) return HIPRAG_OK;          // every row stands where it stood
    const i64 lo_blk = t.dst[(size_t)first] / kRowsPerBlock;
    const i64 hi_row = last + 1 < n_runs ? t.dst[(size_t)last + 1] : stored_new;
    const i64 hi_blk = (hi_row + kRowsPerBlock - 1) / kRowsPerBlock;
    const size_t xb_blk = (size_t)R.P * kPieceFloats * sizeof(float), xh_blk = xb_blk / 2, n_blk = kRowsPerBlock * sizeof(float),
                 id_blk = kRowsPerBlock * sizeof(i64);
    const size_t per_blk = xb_blk + xh_blk + n_blk + id_blk;
    const size_t tab_bytes = (size_t)n_runs * 20;
    const size_t budget = DenseIndex::kRemoveBudget;
    const i64 cb = std::max<i64>(1, std::min<i64>(hi_blk - lo_blk, (i64)((budget - std::min(tab_bytes, budget)) / per_blk)));
    int32_t rc;
    if ((rc = stage.reserve((size_t)cb * per_blk)) || (rc = tab.reserve(tab_bytes))) return rc;
    i64* tab_dst = tab.as<i64>();
    i64* tab_src = tab_dst + n_runs;
    int* tab_kind = reinterpret_cast<int*>(tab_src + n_runs);
    HR_CHECK_HIP(hipMemcpyAsync(tab_dst, t.dst.data(), (size_t)n_runs * 8, hipMemcpyHostToDevice, st));
    HR_CHECK_HIP(hipMemcpyAsync(tab_src, t.src.data(), (size_t)n_runs * 8, hipMemcpyHostToDevice, st));
    HR_CHECK_HIP(hipMemcpyAsync(tab_kind, t.kind.data(), (size_t)n_runs * 4, hipMemcpyHostToDevice, st));
    float4* st_xb = stage.as<float4>();
    float4* st_xh = reinterpret_cast<float4*>(stage.as<char>() + (size_t)cb * xb_blk);
    float* st_n = reinterpret_cast<float*>(stage.as<char>() + (size_t)cb * (xb_blk + xh_blk));
    i64* st_id = reinterpret_cast<i64*>(stage.as<char>() + (size_t)cb * (xb_blk + xh_blk + n_blk));
    RelayoutArgs g, s;                           // gather, write-back
    g.run_dst = tab_dst; g.run_src = tab_src; g.run_kind = tab_kind; g.n_runs = n_runs; g.P = R.P;
    g.batch_order = batch_order; g.id_base = id_base;
    s = g;
    g.src_xb[0] = R.xb.as<float4>(); g.src_xh[0] = R.xh.as<float4>(); g.src_n[0] = R.norms.as<float>(); g.src_orig = iv.orig.as<i64>();
    g.src_xb[1] = batch ? batch->xb.as<float4>() : nullptr;
    g.src_xh[1] = batch ? batch->xh.as<float4>() : nullptr;
    g.src_n[1] = batch ? batch->norms.as<float>() : nullptr;
    g.dst_xb = st_xb; g.dst_xh = st_xh; g.dst_n = st_n; g.dst_orig = st_id;
    s.src_xb[0] = s.src_xb[1] = st_xb; s.src_xh[0] = s.src_xh[1] = st_xh; s.src_n[0] = s.src_n[1] = st_n; s.src_orig = st_id;
    s.dst_xb = R.xb.as<float4>(); s.dst_xh = R.xh.as<float4>(); s.dst_n = R.norms.as<float>(); s.dst_orig = iv.orig.as<i64>();
    auto grid = [](i64 nblk) { return dim3((unsigned)std::max<i64>(1, std::min<i64>((nblk + 3) / 4, 4096))); };
    const i64 nchunks = (hi_blk - lo_blk + cb - 1) / cb;
    for (i64 c = 0; c < nchunks; ++c) {
        // descending: the chunks are cut from the top, so the lowest one is the short one
        const i64 b_hi = descending ? hi_blk - c * cb : std::min(hi_blk, lo_blk + (c + 1) * cb);
        const i64 b_lo = descending ? std::max(lo_blk, b_hi - cb) : lo_blk + c * cb;
        g.blk0 = s.blk0 = b_lo;
        g.nblk = s.nblk = b_hi - b_lo;
        hipLaunchKernelGGL(ivf_relayout_kernel<true>, grid(g.nblk), dim3(256), 0, st, g);
        hipLaunchKernelGGL(ivf_relayout_kernel<false>, grid(s.nblk), dim3(256), 0, st, s);
    }
    HR_CHECK_HIP(hipGetLastError());
    iv.up_info[2] += t.moved;
    iv.up_info[3] += nchunks;
    return HIPRAG_OK;
}

// the handle's own state behind an update whose kernels are enqueued on `st`; returns with `st` drained
int32_t refresh(IvfIndex& iv, std::vector<i64>& new_offs, std::vector<i64>& new_lens, i64 n_new, hipStream_t st)
{
    iv.offs_host.swap(new_offs);
    iv.lens_host.swap(new_lens);
    iv.n_rows = n_new;
    iv.maxlen = 0;
    for (int l = 0; l < iv.nlist; ++l) iv.maxlen = std::max(iv.maxlen, iv.offs_host[(size_t)l + 1] - iv.offs_host[(size_t)l]);
    iv.list_tab.release();                       // the batch search remakes it from offs_host
    HR_CHECK_HIP(hipMemcpyAsync(iv.offs.p, iv.offs_host.data(), (size_t)(iv.nlist + 1) * 8, hipMemcpyHostToDevice, st));
    HR_CHECK_HIP(hipMemcpyAsync(iv.lens_dev.p, iv.lens_host.data(), (size_t)iv.nlist * 8, hipMemcpyHostToDevice, st));   // ensure_lens made it
    HR_CHECK_HIP(hipStreamSynchronize(st));
    return HIPRAG_OK;
}

// rows of one pass of an add: the sorted copy of the batch and its tiled form stay within a few hundred MiB
i64 add_step(int d) { return std::max<i64>(1024, (i64)(128ll << 20) / ((i64)d * 4)); }

// One pass of hipivf_add_dev: m <= add_step rows x (device, ordered on st) get the ids n_rows .. n_rows + m - 1.
int32_t add_pass(IvfIndex& iv, const float* x, i64 m, hipStream_t st)
{
    DenseIndex& R = *iv.rows;
    DenseIndex& C = *iv.cents;
    const int nlist = iv.nlist, d = R.d;
    DevBuf s64, ids, order, tiles, len, offs, chunks, sorted, stage, tab;
    int32_t rc;
    if ((rc = s64.reserve((size_t)m * 8)) || (rc = ids.reserve((size_t)m * 8)) || (rc = order.reserve((size_t)m * 8))) return rc;
    {   // the build's assignment: the exact k = 1 search among the centroids, ties to the lower list
        std::lock_guard<std::mutex> gc(C.mu);
        const i64 step = 1 << 16;
        for (i64 o = 0; o < m; o += step) {
            const int mm = (int)std::min(step, m - o);
            if ((rc = C.search_dev(x + o * d, mm, 1, s64.as<double>() + o, nullptr, ids.as<int64_t>() + o, st))) return rc;
        }
    }
    // the batch by list, ascending position (= id) within a list, and how many rows every list gets
    if ((rc = ivf_counting_sort(ids.as<i64>(), m, nlist, 1, tiles, len, offs, chunks, order.as<i64>(), st))) return rc;
    std::vector<i64> add_len((size_t)nlist), add_offs((size_t)nlist + 1);
    HR_CHECK_HIP(hipMemcpyAsync(add_len.data(), len.p, (size_t)nlist * 8, hipMemcpyDeviceToHost, st));
    HR_CHECK_HIP(hipMemcpyAsync(add_offs.data(), offs.p, (size_t)(nlist + 1) * 8, hipMemcpyDeviceToHost, st));
    HR_CHECK_HIP(hipStreamSynchronize(st));
    HR_REQUIRE(add_offs[(size_t)nlist] == m, "%lld of the %lld new rows have no nearest centroid (NaN?): nothing was added",
               (long long)(m - add_offs[(size_t)nlist]), (long long)m);
    // tiled once through the ordinary add path
    std::shared_ptr<DenseIndex> batch;
    if ((rc = sorted.reserve((size_t)m * d * 4)) || (rc = ivf_gather_rows(x, m, d, order.as<i64>(), m, sorted.as<float>(), st)) ||
        (rc = create_dense(d, R.metric, R.device, batch)) || (rc = batch->add_dev(sorted.as<float>(), m, st)))
        return rc;
    // the new layout and where its rows come from
    std::vector<i64> new_lens((size_t)nlist), new_offs((size_t)nlist + 1, 0);
    RunTable t;
    for (int l = 0; l < nlist; ++l) {
        const i64 old_len = iv.lens_host[(size_t)l], old_off = iv.offs_host[(size_t)l], add = add_len[(size_t)l];
        const i64 off = new_offs[(size_t)l], end = off + pad32(old_len + add);
        new_lens[(size_t)l] = old_len + add;
        new_offs[(size_t)l + 1] = end;
        t.push(off, old_off, kRunOld, old_len);
        t.push(off + old_len, add_offs[(size_t)l], kRunNew, add);
        const bool same_pad = add == 0 && off == old_off;
        t.push(off + old_len + add, 0, same_pad ? kRunSkip : kRunZero, end - (off + old_len + add));
    }
    const i64 stored_old = R.ntotal, stored_new = new_offs[(size_t)nlist];
    if ((rc = R.grow(stored_new / kRowsPerBlock)) || (rc = grow_orig(iv, stored_old, stored_new))) return rc;
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));   // their copies ran on the null stream, the relayout runs on the caller's
    if ((rc = relayout(iv, t, stored_new, true, batch.get(), order.as<i64>(), iv.n_rows, st, stage, tab))) return rc;
    hipLaunchKernelGGL(ivf_max_scalars_kernel, dim3(1), dim3(64), 0, st, R.max_norm2_bits(), batch->max_norm2_bits());
    HR_CHECK_HIP(hipGetLastError());
    R.ntotal = stored_new;
    R.update_launch_q();
    iv.up_info[0] += m;
    iv.up_info[4] = std::max<i64>(iv.up_info[4], (i64)(stage.bytes + tab.bytes + sorted.bytes + batch->xb.bytes + batch->xh.bytes +
                                                        batch->norms.bytes));
    return refresh(iv, new_offs, new_lens, iv.n_rows + m, st);   // synchronises: the buffers above are done with
}

// One pass of hipivf_remove_ranges: nr non-empty ranges (ascending, disjoint) of the current ids, on the null stream.
int32_t remove_pass(IvfIndex& iv, const i64* ranges, int nr)
{
    DenseIndex& R = *iv.rows;
    const int nlist = iv.nlist, nb = 2 * nr;
    DevBuf bounds, lens, pos, stage, tab, cuts;
    int32_t rc;
    if ((rc = bounds.reserve((size_t)nb * 8)) || (rc = lens.reserve((size_t)nlist * 8)) || (rc = pos.reserve((size_t)nlist * nb * 8)) ||
        (rc = cuts.reserve((size_t)nb * 8)))
        return rc;
    HR_CHECK_HIP(hipMemcpy(bounds.p, ranges, (size_t)nb * 8, hipMemcpyHostToDevice));
    HR_CHECK_HIP(hipMemcpy(lens.p, iv.lens_host.data(), (size_t)nlist * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(ivf_range_pos_kernel, dim3(flat_grid((i64)nlist * nb)), dim3(256), 0, nullptr, iv.orig.as<i64>(), iv.offs.as<i64>(),
                       lens.as<i64>(), bounds.as<i64>(), nb, nlist, pos.as<i64>());
    HR_CHECK_HIP(hipGetLastError());
    std::vector<i64> p((size_t)nlist * nb);
    HR_CHECK_HIP(hipMemcpy(p.data(), pos.p, p.size() * 8, hipMemcpyDeviceToHost));
    // the surviving runs of every list, the new layout
    std::vector<i64> new_lens((size_t)nlist), new_offs((size_t)nlist + 1, 0);
    RunTable t;
    i64 removed = 0;
    for (int l = 0; l < nlist; ++l) {
        const i64 old_len = iv.lens_host[(size_t)l], old_off = iv.offs_host[(size_t)l], off = new_offs[(size_t)l];
        const i64* pl = p.data() + (size_t)l * nb;
        i64 cur = 0, dst = off;                  // members of the list looked at; next destination row
        for (int j = 0; j <= nr; ++j) {
            const i64 a = j < nr ? pl[2 * j] : old_len, b = j < nr ? pl[2 * j + 1] : old_len;
            t.push(dst, old_off + cur, kRunOld, a - cur);
            dst += a - cur;
            cur = b;
        }
        const i64 len = dst - off, end = off + pad32(len);
        removed += old_len - len;
        new_lens[(size_t)l] = len;
        new_offs[(size_t)l + 1] = end;
        const bool same_pad = len == old_len && off == old_off;
        t.push(dst, 0, same_pad ? kRunSkip : kRunZero, end - dst);
    }
    i64 want = 0;
    std::vector<i64> lo_cut((size_t)nb);         // [0, nr) range starts | [nr, 2 nr) ids removed by the ranges up to it
    for (int j = 0; j < nr; ++j) {
        want += ranges[2 * j + 1] - ranges[2 * j];
        lo_cut[(size_t)j] = ranges[2 * j];
        lo_cut[(size_t)nr + j] = want;
    }
    if (removed != want) {
        set_error("IVF removal: the lists hold %lld of the %lld ids to remove", (long long)removed, (long long)want);
        return HIPRAG_E_HIP;
    }
    const i64 stored_old = R.ntotal, stored_new = new_offs[(size_t)nlist];
    if ((rc = relayout(iv, t, stored_new, false, nullptr, nullptr, 0, nullptr, stage, tab))) return rc;
    if (stored_new > 0) {
        HR_CHECK_HIP(hipMemcpy(cuts.p, lo_cut.data(), (size_t)nb * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(ivf_renumber_kernel, dim3(flat_grid(stored_new)), dim3(256), 0, nullptr, iv.orig.as<i64>(), stored_new,
                           cuts.as<i64>(), cuts.as<i64>() + nr, nr);
        HR_CHECK_HIP(hipGetLastError());
    }
    const size_t xb_blk = (size_t)R.P * kPieceFloats * sizeof(float);
    // vacated blocks back to zero, the two maxima recomputed over the survivors, the new stored row count; synchronises
    if ((rc = R.finish_removal(stored_old / kRowsPerBlock, stored_new / kRowsPerBlock, stored_new, xb_blk, xb_blk / 2,
                               kRowsPerBlock * sizeof(float))))
        return rc;
    iv.up_info[1] += removed;
    iv.up_info[4] = std::max<i64>(iv.up_info[4], (i64)(stage.bytes + tab.bytes + pos.bytes + bounds.bytes + lens.bytes + cuts.bytes));
    return refresh(iv, new_offs, new_lens, iv.n_rows - removed, nullptr);
}

}  // namespace
}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipivf_from_centroids(const float* centroids_host, int32_t nlist, int32_t d, int32_t metric, int32_t device,
                              uint64_t* out_handle)
{
    HR_REQUIRE(out_handle && centroids_host, "null argument");
    HR_REQUIRE(nlist >= 1, "nlist must be positive (got %d)", nlist);
    HR_CHECK_HIP(hipSetDevice(device));
    auto iv = std::make_shared<IvfIndex>();
    int32_t rc;
    if ((rc = create_dense(d, metric, device, iv->cents)) || (rc = iv->cents->add_host(centroids_host, nlist))) return rc;
    if ((rc = create_dense(d, metric, device, iv->rows))) return rc;
    if ((rc = iv->offs.reserve((size_t)(nlist + 1) * 8)) || (rc = iv->orig.reserve(kRowsPerBlock * 8))) return rc;
    HR_CHECK_HIP(hipMemset(iv->offs.p, 0, (size_t)(nlist + 1) * 8));
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    iv->nlist = nlist;
    iv->offs_host.assign((size_t)nlist + 1, 0);
    iv->lens_host.assign((size_t)nlist, 0);
    iv->lens_known = true;
    *out_handle = ivf_reg().put(iv);
    return HIPRAG_OK;
}

int32_t hipivf_add_dev(uint64_t h, const float* x_dev, int64_t n_add, void* stream)
{
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    int32_t rc = require_owned(*iv);
    if (rc) return rc;
    HR_REQUIRE(n_add >= 0, "n_add must not be negative (got %lld)", (long long)n_add);
    HR_REQUIRE(x_dev || n_add == 0, "x is null");
    HR_REQUIRE(iv->n_rows + n_add < (1ll << 31), "n + n_add must stay below 2^31 (n %lld, n_add %lld)", (long long)iv->n_rows,
               (long long)n_add);
    DenseIndex& R = *iv->rows;
    std::lock_guard<std::mutex> gr(R.mu);
    HR_CHECK_HIP(hipSetDevice(R.device));
    if ((rc = ensure_lens(*iv, kCannotUpdate))) return rc;
    for (int i = 0; i < 5; ++i) iv->up_info[i] = 0;
    if (n_add == 0) return HIPRAG_OK;
    if ((rc = R.wait_adds_host())) return rc;
    const i64 step = add_step(R.d);
    for (i64 o = 0; o < n_add; o += step)
        if ((rc = add_pass(*iv, x_dev + o * R.d, std::min<i64>(step, n_add - o), (hipStream_t)stream))) return rc;
    return HIPRAG_OK;
}

int32_t hipivf_add(uint64_t h, const float* x_host, int64_t n_add)
{
    int32_t d = 0, device = 0;
    i64 n = 0;
    {
        GET_IVF(h);
        std::lock_guard<std::mutex> guard(iv->mu);
        const int32_t rc = require_owned(*iv);
        if (rc) return rc;
        d = iv->rows->d;
        device = iv->rows->device;
        n = iv->n_rows;
    }
    HR_REQUIRE(n_add >= 0, "n_add must not be negative (got %lld)", (long long)n_add);
    HR_REQUIRE(x_host || n_add == 0, "x is null");
    HR_REQUIRE(n + n_add < (1ll << 31), "n + n_add must stay below 2^31 (n %lld, n_add %lld)", (long long)n, (long long)n_add);
    if (n_add == 0) return hipivf_add_dev(h, nullptr, 0, nullptr);
    HR_CHECK_HIP(hipSetDevice(device));
    const i64 step = add_step(d);                // a pass of the device form at a time: the staging stays small
    DevBuf x;
    int32_t rc = x.reserve((size_t)std::min<i64>(step, n_add) * d * sizeof(float));
    if (rc) return rc;
    int64_t info[5] = {0, 0, 0, 0, 0};
    for (i64 o = 0; o < n_add; o += step) {
        const i64 m = std::min<i64>(step, n_add - o);
        HR_CHECK_HIP(hipMemcpy(x.p, x_host + o * d, (size_t)m * d * sizeof(float), hipMemcpyHostToDevice));
        if ((rc = hipivf_add_dev(h, x.as<float>(), m, nullptr))) return rc;
        int64_t part[5];
        if ((rc = hipivf_update_info(h, part))) return rc;
        for (int i = 0; i < 4; ++i) info[i] += part[i];
        info[4] = std::max<int64_t>(info[4], part[4] + (int64_t)x.bytes);
    }
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    for (int i = 0; i < 5; ++i) iv->up_info[i] = info[i];
    return HIPRAG_OK;
}

int32_t hipivf_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges)
{
    GET_IVF(h);
    std::lock_guard<std::mutex> guard(iv->mu);
    int32_t rc = require_owned(*iv);
    if (rc) return rc;
    RangeTable tab;                              // not joined: the passes are cut, and up_info[4] is sized, by range count
    if ((rc = range_table(ranges_host, n_ranges, iv->n_rows, "n", false, tab))) return rc;
    std::vector<i64> live;                       // the non-empty ranges, lo and hi in turn
    for (const auto& r : tab) { live.push_back(r.first); live.push_back(r.second); }
    DenseIndex& R = *iv->rows;
    std::lock_guard<std::mutex> gr(R.mu);
    HR_CHECK_HIP(hipSetDevice(R.device));
    if ((rc = ensure_lens(*iv, kCannotUpdate))) return rc;
    for (int i = 0; i < 5; ++i) iv->up_info[i] = 0;
    if (live.empty()) return HIPRAG_OK;
    if ((rc = R.wait_adds_host())) return rc;
    // A pass takes as many ranges as keep its tables (lists x range ends) small, the LAST ranges first: the ids of the
    // ranges before them are not renumbered by it.
    const i64 nr = (i64)live.size() / 2;
    const i64 per_pass = std::max<i64>(1, (i64)(1 << 20) / iv->nlist);
    for (i64 hi = nr; hi > 0; hi -= per_pass) {
        const i64 lo = std::max<i64>(0, hi - per_pass);
        if ((rc = remove_pass(*iv, live.data() + 2 * lo, (int)(hi - lo)))) return rc;
    }
    return HIPRAG_OK;
}

int32_t hipivf_update_info(uint64_t h, int64_t* out5)
{
    GET_IVF(h);
    HR_REQUIRE(out5, "out5 is null");
    std::lock_guard<std::mutex> guard(iv->mu);
    for (int i = 0; i < 5; ++i) out5[i] = iv->up_info[i];
    return HIPRAG_OK;
}

}  // extern "C"
