// group_partials.hip -- what the two list-major searches share on the host side.  Both the IVF batch search
// (ivf_search.hip: entries = inverted lists, pairs = (query, probe rank)) and the scoped search (dense_scoped.hip: entries =
// scopes, pairs = queries) sort their pairs by entry with the IVF build's stable counting sort, cut every entry into work
// items = (slice of 256 rows, group of up to 16 pairs), prefill the partial lists [parts][queries][k] and hand them to the
// canonical merge.  Cold kernels only: the kernels that score rows stay with their searches.  Also the one upload of a scope
// image (ScopeUpload) and the chunk driver of the three sliced scoped searches (slice_plan / slice_begin / slice_chunk).
#include <algorithm>
#include <cfloat>
#include <cstring>

#include "dense_internal.h"

namespace hiprag {
namespace {

constexpr int kSortTile = 1024;          // rows per tile of the counting sort (grown while tiles x nlist > kSortCells)
constexpr i64 kSortCells = 1ll << 24;

__global__ __launch_bounds__(256) void ivf_hist_kernel(const i64* __restrict__ assign, i64 n, int tile, int nlist,
                                                       int* __restrict__ tile_count)
{
    const i64 t = blockIdx.x, lo = t * tile, hi = min(n, lo + tile);
    for (i64 i = lo + threadIdx.x; i < hi; i += 256) {
        const i64 l = assign[i];
        if (l >= 0 && l < nlist) atomicAdd(&tile_count[t * nlist + l], 1);   // integer counts: independent of arrival order
    }
}

// per list: counts of the tiles -> their exclusive prefix (in place); len[l] = members of list l
__global__ __launch_bounds__(256) void ivf_tile_prefix_kernel(int* __restrict__ tile_count, int ntiles, int nlist,
                                                              i64* __restrict__ len)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nlist) return;
    int run = 0;
    for (int t = 0; t < ntiles; ++t) {
        const int c = tile_count[(i64)t * nlist + l];
        tile_count[(i64)t * nlist + l] = run;
        run += c;
    }
    len[l] = run;
}

// one workgroup: offs[l] = sum over l' < l of len[l'] rounded up to `pad` rows, offs[nlist] = the total;
// chunk_start[l] = sum over l' < l of ceil(len[l'] / kSumRows), chunk_start[nlist] = the chunk count
__global__ __launch_bounds__(256) void ivf_list_scan_kernel(const i64* __restrict__ len, int nlist, int pad,
                                                            i64* __restrict__ offs, int* __restrict__ chunk_start)
{
    __shared__ i64 s_off[256], s_ch[256];
    const int tid = threadIdx.x;
    i64 carry_off = 0, carry_ch = 0;
    for (int base = 0; base < nlist; base += 256) {
        const int l = base + tid;
        i64 v = 0, c = 0;
        if (l < nlist) {
            const i64 L = len[l];
            v = (L + pad - 1) / pad * pad;
            c = (L + kSumRows - 1) / kSumRows;
        }
        s_off[tid] = v;
        s_ch[tid] = c;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {      // inclusive scan (Hillis-Steele)
            const i64 a = tid >= s ? s_off[tid - s] : 0, b = tid >= s ? s_ch[tid - s] : 0;
            __syncthreads();
            s_off[tid] += a;
            s_ch[tid] += b;
            __syncthreads();
        }
        if (l < nlist) {
            offs[l] = carry_off + s_off[tid] - v;
            chunk_start[l] = (int)(carry_ch + s_ch[tid] - c);
        }
        carry_off += s_off[255];
        carry_ch += s_ch[255];
        __syncthreads();
    }
    if (tid == 0) {
        offs[nlist] = carry_off;
        chunk_start[nlist] = (int)carry_ch;
    }
}

// stable scatter: out[offs[l] + (members of l in earlier tiles) + (members of l before row i in its tile)] = i
__global__ __launch_bounds__(256) void ivf_scatter_kernel(const i64* __restrict__ assign, i64 n, int tile, int nlist,
                                                          int* __restrict__ tile_prefix, const i64* __restrict__ offs,
                                                          i64* __restrict__ out)
{
    __shared__ int win[256];
    const int tid = threadIdx.x;
    const i64 t = blockIdx.x, lo = t * tile, hi = min(n, lo + tile);
    int* cur = tile_prefix + t * nlist;          // this tile's running position inside every list (this workgroup only)
    for (i64 base = lo; base < hi; base += 256) {
        const i64 i = base + tid;
        i64 li = i < hi ? assign[i] : -1;
        const int l = li >= 0 && li < nlist ? (int)li : -1;
        win[tid] = l;
        __syncthreads();
        int before = 0, after = 0;
        if (l >= 0) {
            for (int j = 0; j < 256; ++j) {
                const int v = win[j];
                before += (v == l) & (j < tid);
                after += (v == l) & (j > tid);
            }
            out[offs[l] + cur[l] + before] = i;
        }
        __syncthreads();                         // every lane has read cur[] for this window
        if (l >= 0 && after == 0) cur[l] += before + 1;
        __syncthreads();
    }
}

// one workgroup: item_start = exclusive prefix over the entries (lists, scopes) of their work items, groups x slices, where
// groups = the entry's pairs in groups of `group`; an entry without pairs has no items.  rows_read += the rows of every entry
// with pairs -- once (IVF: the stored rows of the probed lists) or once per group (scoped: groups x rows of the scope).
__global__ __launch_bounds__(256) void group_item_scan_kernel(const i64* __restrict__ pair_len, const i64* __restrict__ slices,
                                                              const i64* __restrict__ rows_of, int group, int rows_per_group, int n,
                                                              i64* __restrict__ item_start, i64* __restrict__ rows_read)
{
    __shared__ i64 s_it[256], s_rows[256];
    const int tid = threadIdx.x;
    i64 carry = 0, carry_rows = 0;
    for (int base = 0; base < n; base += 256) {
        const int e = base + tid;
        i64 v = 0, rows = 0;
        if (e < n && pair_len[e] > 0) {
            const i64 groups = (pair_len[e] + group - 1) / group;
            v = groups * slices[e];
            rows = (rows_per_group ? groups : 1) * rows_of[e];
        }
        s_it[tid] = v;
        s_rows[tid] = rows;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {      // inclusive scan (Hillis-Steele)
            const i64 a = tid >= s ? s_it[tid - s] : 0, b = tid >= s ? s_rows[tid - s] : 0;
            __syncthreads();
            s_it[tid] += a;
            s_rows[tid] += b;
            __syncthreads();
        }
        if (e < n) item_start[e] = carry + s_it[tid] - v;
        carry += s_it[255];
        carry_rows += s_rows[255];
        __syncthreads();
    }
    if (tid == 0) {
        item_start[n] = carry;
        rows_read[0] += carry_rows;               // stream-ordered, one writer
    }
}

// the partial-list slots nobody writes (slices past the end of an entry, -1 probes, ranks past the rows of a slice)
template <int METRIC>
__global__ __launch_bounds__(256) void ivf_pad_fill_kernel(double* __restrict__ ps, i64* __restrict__ pi, i64 n)
{
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        ps[i] = METRIC == HIPRAG_METRIC_IP ? -DBL_MAX : DBL_MAX;
        pi[i] = -1;
    }
}

}  // namespace

// stable counting sort of the m entries of a[] by list (entries outside 0..nlist-1 belong to no list): offs / len / chunks,
// and out[offs[l] ..] = the indices of the members of l ascending, every list rounded up to `pad` slots (out must be
// prefilled with -1 when pad > 1).  The build sorts rows by assigned list, the batch search sorts (query, j) pairs by
// probed list.
int32_t ivf_counting_sort(const i64* a, i64 m, int nlist, int pad, DevBuf& tiles, DevBuf& len, DevBuf& offs, DevBuf& chunks,
                          i64* out, hipStream_t st)
{
    int tile = kSortTile;
    while ((m + tile - 1) / tile * (i64)nlist > kSortCells && tile < (1 << 30)) tile *= 2;
    const i64 ntiles = std::max<i64>(1, (m + tile - 1) / tile);
    int32_t rc;
    if ((rc = tiles.reserve((size_t)ntiles * nlist * 4)) || (rc = len.reserve((size_t)nlist * 8)) ||
        (rc = offs.reserve((size_t)(nlist + 1) * 8)) || (rc = chunks.reserve((size_t)(nlist + 1) * 4)))
        return rc;
    HR_CHECK_HIP(hipMemsetAsync(tiles.p, 0, (size_t)ntiles * nlist * 4, st));
    hipLaunchKernelGGL(ivf_hist_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, a, m, tile, nlist, tiles.as<int>());
    hipLaunchKernelGGL(ivf_tile_prefix_kernel, dim3((unsigned)((nlist + 255) / 256)), dim3(256), 0, st, tiles.as<int>(),
                       (int)ntiles, nlist, len.as<i64>());
    hipLaunchKernelGGL(ivf_list_scan_kernel, dim3(1), dim3(256), 0, st, len.as<i64>(), nlist, pad, offs.as<i64>(),
                       chunks.as<int>());
    hipLaunchKernelGGL(ivf_scatter_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, a, m, tile, nlist, tiles.as<int>(),
                       offs.as<i64>(), out);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

// the work items of the n entries behind the counting sort (pair_len = its `len`): group_item_scan_kernel
int32_t group_item_scan(const i64* pair_len, const i64* slices, const i64* rows, int group, bool rows_per_group, int n,
                        i64* item_start, i64* rows_read, hipStream_t st)
{
    hipLaunchKernelGGL(group_item_scan_kernel, dim3(1), dim3(256), 0, st, pair_len, slices, rows, group, rows_per_group ? 1 : 0, n,
                       item_start, rows_read);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

// n slots of partial lists -> the padding the canonical merge skips (worst score of the metric, id -1)
int32_t fill_partials(int metric, double* ps, i64* pi, i64 n, hipStream_t st)
{
    const unsigned grid = (unsigned)std::max<i64>(1, std::min<i64>((n + 255) / 256, 4096));
    if (metric == HIPRAG_METRIC_IP) hipLaunchKernelGGL(ivf_pad_fill_kernel<HIPRAG_METRIC_IP>, dim3(grid), dim3(256), 0, st, ps, pi, n);
    else hipLaunchKernelGGL(ivf_pad_fill_kernel<HIPRAG_METRIC_L2>, dim3(grid), dim3(256), 0, st, ps, pi, n);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

// queries per chunk of a call: the partial lists [parts][chunk][k] (score + id), and whatever else the call keeps per query
// (extra_per_query bytes), stay within the budget; a chunk is one query at least and max_chunk at most
int queries_per_chunk(int nq, i64 parts, int k, i64 budget, int max_chunk, i64 extra_per_query)
{
    return (int)std::max<i64>(1, std::min<i64>(std::min(nq, max_chunk), budget / (parts * k * 16 + extra_per_query)));
}

// The scope image of a call goes to `meta` through the next buffer of the pinned ring; the buffer is rewritten only after
// the copy that last read it, kRing calls ago, has run.  The one upload of every scoped search.
int32_t ScopeUpload::upload(const int64_t* img, size_t words, hipStream_t st)
{
    int32_t rc;
    if ((rc = meta.reserve(words * 8))) return rc;
    const int slot = pin_next;
    pin_next = (slot + 1) % kRing;
    if (!pin_ev[slot]) HR_CHECK_HIP(hipEventCreateWithFlags(&pin_ev[slot], hipEventDisableTiming));
    if (pin_used[slot]) HR_CHECK_HIP(hipEventSynchronize(pin_ev[slot]));
    if ((rc = pin[slot].reserve(words * 8))) return rc;
    memcpy(pin[slot].p, img, words * 8);
    HR_CHECK_HIP(hipMemcpyAsync(meta.p, pin[slot].p, words * 8, hipMemcpyHostToDevice, st));
    HR_CHECK_HIP(hipEventRecord(pin_ev[slot], st));
    pin_used[slot] = true;
    return HIPRAG_OK;
}

int32_t slice_plan(const int64_t* ranges, const int32_t* scope_offsets, int n_scopes, const int32_t* scope_of_query, int nq, i64 n,
                   const char* name_of_n, int slice_rows, int group, int depth, const char* name_of_depth, SlicePlan& out)
{
    int32_t rc;
    if ((rc = check_scope_tables(ranges, scope_offsets, n_scopes, scope_of_query, nq, n, name_of_n))) return rc;
    build_scope_image(ranges, scope_offsets, n_scopes, scope_of_query, nq, slice_rows, group, out.im);
    out.n_scopes = n_scopes; out.group = group;
    out.smax = std::max<i64>(out.im.smax, 1); out.bound = out.im.bound; out.kp = std::min(depth, slice_rows);
    HR_REQUIRE(out.smax * out.kp < (1ll << 31), "a scope of %lld slices at %s = %d is beyond the merge", (long long)out.smax, name_of_depth,
               depth);
    return HIPRAG_OK;
}

int32_t slice_begin(ScopeUpload& S, const SlicePlan& P, int qchunk, hipStream_t st)
{
    GroupWorkspace& W = S.gw;
    int32_t rc;
    const size_t part = (size_t)P.smax * qchunk * P.kp * 8;
    if ((rc = W.ps.reserve(part)) || (rc = W.pi.reserve(part)) || (rc = W.order.reserve((size_t)qchunk * 8)) ||
        (rc = W.items.reserve((size_t)(P.n_scopes + 1) * 8)) || (rc = W.stat.reserve(8)) || (rc = S.upload(P.im.img.data(), P.im.words, st)))
        return rc;
    HR_CHECK_HIP(hipMemsetAsync(W.stat.p, 0, 8, st));
    return HIPRAG_OK;
}

int32_t slice_chunk(ScopeUpload& S, const SlicePlan& P, int metric, int o, int m, SliceTables& out, hipStream_t st)
{
    GroupWorkspace& W = S.gw;
    const i64* meta = S.meta.as<i64>();
    int32_t rc;
    if ((rc = ivf_counting_sort(meta + P.im.o_soq + o, m, P.n_scopes, 1, W.tiles, W.len, W.offs, W.chunks, W.order.as<i64>(), st))) return rc;
    if ((rc = group_item_scan(W.len.as<i64>(), meta + P.im.o_sl, meta + P.im.o_rows, P.group, true, P.n_scopes, W.items.as<i64>(),
                              W.stat.as<i64>(), st)))
        return rc;
    if ((rc = fill_partials(metric, W.ps.as<double>(), W.pi.as<i64>(), P.smax * m * P.kp, st))) return rc;
    out = SliceTables{meta, meta + P.im.o_slice, meta + P.im.o_off, W.offs.as<i64>(), W.order.as<i64>(), W.items.as<i64>(), P.n_scopes};
    return HIPRAG_OK;
}

}  // namespace hiprag
