// ivf_build.hip -- the IVF-Flat k-means build on the GPU, and HIPIVF01 save / load.  The searches are ivf_search.hip.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "ivf_internal.h"

namespace hiprag {
namespace {

// ------------------------------------------------------------------------------------------------------
// IVF build (hipivf_build_dev): k-means on the GPU, specified in include/hiprag.h.  Assignment is the flat index's exact
// k = 1 search (DenseIndex::search_dev over the centroids, dense_index.hip); the kernels below are the rest, and none of them sums floats
// with atomics, so a build is the same bits from run to run:
//   ivf_hist / ivf_tile_prefix / ivf_list_scan / ivf_scatter (group_partials.hip)   a STABLE counting sort of row -> list: integer histogram per
//       tile of rows, exclusive prefix over the tiles of every list and over the lists (optionally padded to 32-row blocks),
//       then every tile scatters its rows, ranked inside a 256-row window by an LDS compare, behind its own tile prefix
//   ivf_chunk_sum / ivf_update   the segmented fp64 mean: every list is cut into chunks of kSumRows members (ascending row
//       id), one workgroup sums a chunk (a row is one coalesced float4 per lane at d = 1024), and one workgroup per list adds
//       its chunk partials in chunk order, divides, normalises under IP and rounds to fp32
//   ivf_gather   rows by index (-1 = a zero row): the training sample, the initial centroids, and the final layout, written
//       chunk by chunk into a staging buffer that the rows index's ordinary add path re-tiles.
// Bound: HBM.  A round reads the training rows twice (scan of the assignment + the sum), the layout reads x once more.
// ------------------------------------------------------------------------------------------------------
// partial[w][c] = fp64 sum of x[order[r]][c] over the members r of chunk w (kSumRows consecutive members of one list)
__global__ __launch_bounds__(256) void ivf_chunk_sum_kernel(const float* __restrict__ x, int d, int vec,
                                                            const i64* __restrict__ order, const i64* __restrict__ offs,
                                                            const int* __restrict__ chunk_start, int nlist,
                                                            double* __restrict__ partial)
{
    __shared__ i64 rows[kSumRows];
    const int w = blockIdx.x, tid = threadIdx.x;
    if (w >= chunk_start[nlist]) return;         // the grid is sized by an upper bound of the chunk count
    int lo = 0, hi = nlist - 1;                  // the list of chunk w: the last l with chunk_start[l] <= w (never empty)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_start[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    const i64 r0 = offs[lo] + (i64)(w - chunk_start[lo]) * kSumRows;
    const int m = (int)min((i64)kSumRows, offs[lo + 1] - r0);
    if (tid < m) rows[tid] = order[r0 + tid];
    __syncthreads();
    double* out = partial + (i64)w * d;
    if (vec) {                                   // d % 4 == 0, x 16-byte aligned: one float4 column group per lane
        const int dv = d >> 2;
        if (tid < dv) {
            const float4* x4 = reinterpret_cast<const float4*>(x);
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 8
            for (int r = 0; r < m; ++r) {
                const float4 v = x4[rows[r] * dv + tid];
                s0 += (double)v.x;
                s1 += (double)v.y;
                s2 += (double)v.z;
                s3 += (double)v.w;
            }
            out[4 * tid + 0] = s0;
            out[4 * tid + 1] = s1;
            out[4 * tid + 2] = s2;
            out[4 * tid + 3] = s3;
        }
    } else {
        for (int c = tid; c < d; c += 256) {
            double s = 0.0;
            for (int r = 0; r < m; ++r) s += (double)x[rows[r] * d + c];
            out[c] = s;
        }
    }
}

// next[l] = (sum of list l's chunk partials, in chunk order) / len[l], under IP divided by its fp64 norm, rounded to fp32;
// an empty list keeps prev[l].  d <= 1024: four columns per lane.
template <int METRIC>
__global__ __launch_bounds__(256) void ivf_update_kernel(const double* __restrict__ partial, const int* __restrict__ chunk_start,
                                                         const i64* __restrict__ len, int d, const float* __restrict__ prev,
                                                         float* __restrict__ next)
{
    __shared__ double red[256];
    const int l = blockIdx.x, tid = threadIdx.x;
    const i64 cnt = len[l];
    const float* p = prev + (i64)l * d;
    float* o = next + (i64)l * d;
    if (cnt == 0) {
        for (int c = tid; c < d; c += 256) o[c] = p[c];
        return;
    }
    const int w0 = chunk_start[l], w1 = chunk_start[l + 1];
    double m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = tid + 256 * j;
        double s = 0.0;
        if (c < d)
            for (int w = w0; w < w1; ++w) s += partial[(i64)w * d + c];
        m[j] = s / (double)cnt;
    }
    if (METRIC == HIPRAG_METRIC_IP) {            // spherical k-means: the assignment maximises <x, c>
        red[tid] = m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + m[3] * m[3];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        const double nrm = sqrt(red[0]);
        if (nrm > 0.0)
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] /= nrm;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = tid + 256 * j;
        if (c < d) o[c] = (float)m[j];
    }
}

// out[r] = src[idx[r]] for r in [0, m); idx[r] < 0 -> a zero row.  idx == nullptr: idx[r] = floor(r * n_src / m)
// (the training sample).  vec: d % 4 == 0 and both pointers 16-byte aligned.
__global__ __launch_bounds__(256) void ivf_gather_kernel(const float* __restrict__ src, i64 n_src, int d, int vec,
                                                         const i64* __restrict__ idx, i64 m, float* __restrict__ out)
{
    const int dv = vec ? d >> 2 : d;
    const i64 total = m * dv;
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < total; e += (i64)gridDim.x * 256) {
        const i64 r = e / dv, c = e - r * dv;
        const i64 id = idx ? idx[r] : r * n_src / m;
        if (vec) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (id >= 0) v = reinterpret_cast<const float4*>(src)[id * dv + c];
            reinterpret_cast<float4*>(out)[e] = v;
        } else {
            out[e] = id >= 0 ? src[id * dv + c] : 0.f;
        }
    }
}

// splitmix64 (Steele, Lea, Flood 2014): the documented generator of the initial centroids
inline uint64_t splitmix64(uint64_t& s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

unsigned gather_grid(i64 elems) { return (unsigned)std::max<i64>(1, std::min<i64>((elems + 255) / 256, 8192)); }

}  // namespace

int32_t ivf_gather_rows(const float* src, i64 n_src, int d, const i64* idx, i64 m, float* out, hipStream_t st)
{
    const int vec = (d % 4 == 0) && ((uintptr_t)src % 16 == 0) && ((uintptr_t)out % 16 == 0);
    const i64 elems = m * (vec ? d / 4 : d);
    hipLaunchKernelGGL(ivf_gather_kernel, dim3(gather_grid(elems)), dim3(256), 0, st, src, n_src, d, vec, idx, m, out);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

namespace {

struct IvfBuilder {
    int d = 0, metric = 0, device = 0, nlist = 0;
    hipStream_t st = nullptr;
    DevBuf s64, ids, tiles, len, offs, chunks, order, partial, cent[2], train, init_idx, stage;

    int32_t gather(const float* src, i64 n_src, const i64* idx, i64 m, float* out) { return ivf_gather_rows(src, n_src, d, idx, m, out, st); }

    // ids[0..m) = the list of every row of xq: the exact k = 1 search among the centroids, ties to the lower list
    int32_t assign(DenseIndex& C, const float* xq, i64 m)
    {
        int32_t rc;
        if ((rc = s64.reserve((size_t)m * 8)) || (rc = ids.reserve((size_t)m * 8))) return rc;
        const i64 step = 1 << 16;
        for (i64 o = 0; o < m; o += step) {
            const int mm = (int)std::min(step, m - o);
            if ((rc = C.search_dev(xq + o * d, mm, 1, s64.as<double>() + o, nullptr, ids.as<int64_t>() + o, st))) return rc;
        }
        return HIPRAG_OK;
    }

    // stable counting sort of the m rows by ids[] (ivf_counting_sort, group_partials.hip)
    int32_t sort(i64 m, int pad, i64* out)
    {
        return ivf_counting_sort(ids.as<i64>(), m, nlist, pad, tiles, len, offs, chunks, out, st);
    }

    // one k-means update of the centroids cent[cur] over the training rows xt -> cent[cur ^ 1]
    int32_t update(const float* xt, i64 m, int cur)
    {
        const i64 max_chunks = (m + kSumRows - 1) / kSumRows + nlist;
        int32_t rc;
        if ((rc = partial.reserve((size_t)max_chunks * d * 8))) return rc;
        const int vec = (d % 4 == 0) && ((uintptr_t)xt % 16 == 0);
        hipLaunchKernelGGL(ivf_chunk_sum_kernel, dim3((unsigned)max_chunks), dim3(256), 0, st, xt, d, vec, order.as<i64>(),
                           offs.as<i64>(), chunks.as<int>(), nlist, partial.as<double>());
        if (metric == HIPRAG_METRIC_IP)
            hipLaunchKernelGGL(ivf_update_kernel<HIPRAG_METRIC_IP>, dim3(nlist), dim3(256), 0, st, partial.as<double>(),
                               chunks.as<int>(), len.as<i64>(), d, cent[cur].as<float>(), cent[cur ^ 1].as<float>());
        else
            hipLaunchKernelGGL(ivf_update_kernel<HIPRAG_METRIC_L2>, dim3(nlist), dim3(256), 0, st, partial.as<double>(),
                               chunks.as<int>(), len.as<i64>(), d, cent[cur].as<float>(), cent[cur ^ 1].as<float>());
        HR_CHECK_HIP(hipGetLastError());
        return HIPRAG_OK;
    }

    int32_t centroid_index(int cur, std::shared_ptr<DenseIndex>& C)
    {
        int32_t rc = create_dense(d, metric, device, C);
        if (rc) return rc;
        return C->add_dev(cent[cur].as<float>(), nlist, st);
    }
};

// the whole build (hipivf_build_dev); x_dev [n, d] on `device`, ordered on `st`; returns with `st` drained
int32_t ivf_build(const float* x, i64 n, int32_t d, int32_t metric, int32_t nlist, int32_t iters, uint64_t seed,
                  i64 max_train_rows, int32_t device, hipStream_t st, std::shared_ptr<IvfIndex>& out)
{
    HR_REQUIRE(x, "x is null");
    HR_REQUIRE(n > 0 && n < (1ll << 31), "n must be in 1..2^31-1 (got %lld)", (long long)n);
    HR_REQUIRE(iters >= 0, "iters must be >= 0 (got %d)", iters);
    const i64 m = (max_train_rows <= 0 || max_train_rows >= n) ? n : max_train_rows;
    HR_REQUIRE(nlist >= 1 && nlist <= m, "nlist must be in 1..%lld, the number of training rows (got %d)", (long long)m, nlist);
    HR_CHECK_HIP(hipSetDevice(device));
    auto iv = std::make_shared<IvfIndex>();
    int32_t rc = create_dense(d, metric, device, iv->rows);   // also checks d and the metric
    if (rc) return rc;
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<float, std::milli>(clk::now() - t0).count(); };
    IvfBuilder b;
    b.d = d; b.metric = metric; b.device = device; b.nlist = nlist; b.st = st;
    const float* xt = x;                                       // the training rows
    if (m < n) {
        if ((rc = b.train.reserve((size_t)m * d * 4)) || (rc = b.gather(x, n, nullptr, m, b.train.as<float>()))) return rc;
        xt = b.train.as<float>();
    }
    {   // initial centroids: training rows perm[0..nlist) of a partial Fisher-Yates shuffle driven by splitmix64 from seed + 1
        std::vector<i64> perm((size_t)m);
        for (i64 i = 0; i < m; ++i) perm[(size_t)i] = i;
        uint64_t s = seed + 1;
        for (int i = 0; i < nlist; ++i) {
            const i64 j = i + (i64)(splitmix64(s) % (uint64_t)(m - i));
            std::swap(perm[(size_t)i], perm[(size_t)j]);
        }
        if ((rc = b.init_idx.reserve((size_t)nlist * 8)) || (rc = b.cent[0].reserve((size_t)nlist * d * 4)) ||
            (rc = b.cent[1].reserve((size_t)nlist * d * 4)))
            return rc;
        HR_CHECK_HIP(hipMemcpyAsync(b.init_idx.p, perm.data(), (size_t)nlist * 8, hipMemcpyHostToDevice, st));
        if ((rc = b.gather(xt, m, b.init_idx.as<i64>(), nlist, b.cent[0].as<float>()))) return rc;
        HR_CHECK_HIP(hipStreamSynchronize(st));                // perm leaves scope
    }
    int cur = 0;
    if ((rc = b.order.reserve((size_t)m * 8))) return rc;
    for (int it = 0; it < iters; ++it) {
        std::shared_ptr<DenseIndex> C;
        clk::time_point t0 = clk::now();
        if ((rc = b.centroid_index(cur, C)) || (rc = b.assign(*C, xt, m))) return rc;
        HR_CHECK_HIP(hipStreamSynchronize(st));
        iv->build_ms[0] += ms_since(t0);
        t0 = clk::now();
        if ((rc = b.sort(m, 1, b.order.as<i64>())) || (rc = b.update(xt, m, cur))) return rc;
        HR_CHECK_HIP(hipStreamSynchronize(st));                // C (freed here) and the buffers are done with
        iv->build_ms[1] += ms_since(t0);
        cur ^= 1;
    }
    // final layout: every row to its nearest final centroid, lists padded to 32-row blocks, stored through the add path
    clk::time_point t0 = clk::now();
    if ((rc = b.centroid_index(cur, iv->cents)) || (rc = b.assign(*iv->cents, x, n))) return rc;
    HR_CHECK_HIP(hipStreamSynchronize(st));
    iv->build_ms[0] += ms_since(t0);
    t0 = clk::now();
    const i64 cap = n + (i64)(kRowsPerBlock - 1) * nlist;
    if ((rc = iv->orig.reserve((size_t)cap * 8)) || (rc = iv->offs.reserve((size_t)(nlist + 1) * 8))) return rc;
    HR_CHECK_HIP(hipMemsetAsync(iv->orig.p, 0xff, (size_t)cap * 8, st));   // padding: original id -1
    if ((rc = b.sort(n, kRowsPerBlock, iv->orig.as<i64>()))) return rc;
    HR_CHECK_HIP(hipMemcpyAsync(iv->offs.p, b.offs.p, (size_t)(nlist + 1) * 8, hipMemcpyDeviceToDevice, st));
    iv->offs_host.resize((size_t)nlist + 1);
    std::vector<i64> lens((size_t)nlist);
    HR_CHECK_HIP(hipMemcpyAsync(iv->offs_host.data(), b.offs.p, (size_t)(nlist + 1) * 8, hipMemcpyDeviceToHost, st));
    HR_CHECK_HIP(hipMemcpyAsync(lens.data(), b.len.p, (size_t)nlist * 8, hipMemcpyDeviceToHost, st));
    HR_CHECK_HIP(hipStreamSynchronize(st));
    i64 members = 0;
    for (i64 v : lens) members += v;
    if (members != n) { set_error("IVF build: %lld of %lld rows were assigned to a list", (long long)members, (long long)n); return HIPRAG_E_HIP; }
    const i64 stored = iv->offs_host[(size_t)nlist];
    DenseIndex& R = *iv->rows;
    if ((rc = R.grow((stored + kRowsPerBlock - 1) / kRowsPerBlock))) return rc;
    const i64 step = std::max<i64>(1024, (i64)(128ll << 20) / ((i64)d * 4)) / kRowsPerBlock * kRowsPerBlock;
    if ((rc = b.stage.reserve((size_t)std::min(step, stored) * d * 4))) return rc;
    for (i64 o = 0; o < stored; o += step) {    // the stage is reused: its gather is ordered behind the previous add on `st`
        const i64 mm = std::min(step, stored - o);
        if ((rc = b.gather(x, n, iv->orig.as<i64>() + o, mm, b.stage.as<float>())) || (rc = R.add_dev(b.stage.as<float>(), mm, st)))
            return rc;
    }
    HR_CHECK_HIP(hipStreamSynchronize(st));
    iv->build_ms[2] = ms_since(t0);
    iv->nlist = nlist;
    iv->n_rows = n;
    for (int l = 0; l < nlist; ++l) iv->maxlen = std::max(iv->maxlen, iv->offs_host[(size_t)l + 1] - iv->offs_host[(size_t)l]);
    out = iv;
    return HIPRAG_OK;
}

}  // namespace
}  // namespace hiprag

using namespace hiprag;

extern "C" {

int32_t hipivf_build_dev(const float* x_dev, int64_t n, int32_t d, int32_t metric, int32_t nlist, int32_t iters, uint64_t seed,
                         int64_t max_train_rows, int32_t device, void* stream, uint64_t* out_handle)
{
    HR_REQUIRE(out_handle, "out_handle is null");
    std::shared_ptr<IvfIndex> iv;
    const int32_t rc = ivf_build(x_dev, n, d, metric, nlist, iters, seed, max_train_rows, device, (hipStream_t)stream, iv);
    if (rc) return rc;
    *out_handle = ivf_reg().put(iv);
    return HIPRAG_OK;
}

int32_t hipivf_build(const float* x_host, int64_t n, int32_t d, int32_t metric, int32_t nlist, int32_t iters, uint64_t seed,
                     int64_t max_train_rows, int32_t device, void* stream, uint64_t* out_handle)
{
    HR_REQUIRE(out_handle && x_host, "null argument");
    HR_REQUIRE(n > 0 && d > 0, "bad shape [%lld, %d]", (long long)n, d);
    if (d > kMaxDPad) {   // the answer create_dense gives the device entry, before the rows are copied
        set_error("d=%d: the flat index under the lists supports d <= %d", d, kMaxDPad);
        return HIPRAG_E_UNSUPPORTED;
    }
    HR_CHECK_HIP(hipSetDevice(device));
    DevBuf x;
    int32_t rc = x.reserve((size_t)n * d * sizeof(float));
    if (rc) return rc;
    HR_CHECK_HIP(hipMemcpy(x.p, x_host, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice));
    rc = hipivf_build_dev(x.as<float>(), n, d, metric, nlist, iters, seed, max_train_rows, device, stream, out_handle);
    HR_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    return rc;
}

// File format "HIPIVF01" (include/hiprag.h): magic[8], int32 version, d, metric, nlist, int64 n, stored rows, then fp32
// centroids [nlist][d], int64 offsets [nlist + 1], int64 original ids [stored], fp32 stored rows [stored][d].
int32_t hipivf_save(uint64_t h, const char* path)
{
    GET_IVF(h);
    HR_REQUIRE(path, "null path");
    std::lock_guard<std::mutex> guard(iv->mu);
    DenseIndex& R = *iv->rows;
    DenseIndex& C = *iv->cents;
    std::lock_guard<std::mutex> gr(R.mu), gc(C.mu);
    HR_CHECK_HIP(hipSetDevice(R.device));
    const i64 stored = R.ntotal;
    std::vector<float> cents((size_t)iv->nlist * R.d);
    std::vector<i64> orig((size_t)stored);
    DevBuf tmp;
    int32_t rc = read_rows_host(C, 0, iv->nlist, tmp, cents.data());
    if (rc) return rc;
    HR_CHECK_HIP(hipMemcpy(orig.data(), iv->orig.p, (size_t)stored * 8, hipMemcpyDeviceToHost));
    FILE* f = fopen(path, "wb");
    if (!f) { set_error("cannot open %s for writing", path); return HIPRAG_E_IO; }
    const char magic[8] = {'H', 'I', 'P', 'I', 'V', 'F', '0', '1'};
    const int32_t hd[4] = {1, R.d, R.metric, iv->nlist};
    const int64_t sz[2] = {iv->n_rows, stored};
    bool ok = fwrite(magic, 1, 8, f) == 8 && fwrite(hd, 4, 4, f) == 4 && fwrite(sz, 8, 2, f) == 2 &&
              fwrite(cents.data(), 4, cents.size(), f) == cents.size() &&
              fwrite(iv->offs_host.data(), 8, iv->offs_host.size(), f) == iv->offs_host.size() &&
              fwrite(orig.data(), 8, orig.size(), f) == orig.size();
    const i64 chunk = std::max<i64>(1, (64ll << 20) / ((i64)R.d * 4));
    std::vector<float> host((size_t)std::min(chunk, std::max<i64>(stored, 1)) * R.d);
    for (i64 o = 0; ok && o < stored; o += chunk) {
        const i64 m = std::min(chunk, stored - o);
        if ((rc = read_rows_host(R, o, m, tmp, host.data()))) { fclose(f); return rc; }
        ok = fwrite(host.data(), sizeof(float), (size_t)m * R.d, f) == (size_t)m * R.d;
    }
    ok = (fclose(f) == 0) && ok;
    if (!ok) { set_error("write to %s failed", path); return HIPRAG_E_IO; }
    return HIPRAG_OK;
}

int32_t hipivf_load(const char* path, int32_t device, uint64_t* out_handle)
{
    HR_REQUIRE(path && out_handle, "null argument");
    FILE* f = fopen(path, "rb");
    if (!f) { set_error("cannot open %s", path); return HIPRAG_E_IO; }
    std::unique_ptr<FILE, int (*)(FILE*)> closer(f, fclose);
    char magic[8];
    int32_t hd[4];
    int64_t sz[2];
    if (fread(magic, 1, 8, f) != 8) { set_error("%s is not a HIPIVF01 file", path); return HIPRAG_E_IO; }
    if (memcmp(magic, "HIPIDX01", 8) == 0) {
        set_error("%s is a flat index file (HIPIDX01), not an IVF one: open it with hipidx_load", path);
        return HIPRAG_E_IO;
    }
    if (memcmp(magic, "HIPIVF01", 8) != 0 || fread(hd, 4, 4, f) != 4 || fread(sz, 8, 2, f) != 2) {
        set_error("%s is not a HIPIVF01 file", path);
        return HIPRAG_E_IO;
    }
    const int32_t version = hd[0], d = hd[1], metric = hd[2], nlist = hd[3];
    const i64 n = sz[0], stored = sz[1];
    HR_REQUIRE(version == 1, "%s: unknown HIPIVF01 version %d", path, version);
    HR_REQUIRE(d > 0 && d <= kMaxDPad && nlist > 0 && n >= 0 && n < (1ll << 31) && stored >= n && stored < (1ll << 36),
               "%s: inconsistent header (d %d, nlist %d, n %lld, stored rows %lld)", path, d, nlist, (long long)n, (long long)stored);
    {   // the size the header implies must be the file's size: a truncated file is rejected before anything is allocated
        const i64 want = 40 + (i64)nlist * d * 4 + ((i64)nlist + 1) * 8 + stored * 8 + stored * d * 4;
        if (fseeko(f, 0, SEEK_END) != 0 || ftello(f) != want || fseeko(f, 40, SEEK_SET) != 0) {
            set_error("%s is truncated or inconsistent with its header", path);
            return HIPRAG_E_IO;
        }
    }
    std::vector<float> cents((size_t)nlist * d);
    std::vector<i64> offs((size_t)nlist + 1), orig((size_t)stored);
    if (fread(cents.data(), 4, cents.size(), f) != cents.size() || fread(offs.data(), 8, offs.size(), f) != offs.size() ||
        fread(orig.data(), 8, orig.size(), f) != orig.size()) {
        set_error("%s is truncated", path);
        return HIPRAG_E_IO;
    }
    HR_REQUIRE(offs[0] == 0 && offs[(size_t)nlist] == stored, "%s: list offsets must cover the stored rows [0, %lld)", path,
               (long long)stored);
    for (int l = 0; l < nlist; ++l)
        HR_REQUIRE(offs[(size_t)l + 1] >= offs[(size_t)l] && offs[(size_t)l] % kRowsPerBlock == 0,
                   "%s: list offsets must ascend on 32-row blocks (list %d)", path, l);
    {
        std::vector<char> seen((size_t)n, 0);
        i64 ids = 0;
        for (i64 r = 0; r < stored; ++r) {
            const i64 id = orig[(size_t)r];
            HR_REQUIRE(id >= -1 && id < n, "%s: original id %lld of stored row %lld is outside [-1, %lld)", path, (long long)id,
                       (long long)r, (long long)n);
            if (id < 0) continue;
            HR_REQUIRE(!seen[(size_t)id], "%s: original id %lld is stored twice", path, (long long)id);
            seen[(size_t)id] = 1;
            ++ids;
        }
        HR_REQUIRE(ids == n, "%s: %lld of the %lld original ids are stored", path, (long long)ids, (long long)n);
    }
    HR_CHECK_HIP(hipSetDevice(device));
    auto iv = std::make_shared<IvfIndex>();
    int32_t rc;
    if ((rc = create_dense(d, metric, device, iv->cents)) || (rc = iv->cents->add_host(cents.data(), nlist))) return rc;
    if ((rc = create_dense(d, metric, device, iv->rows)) || (rc = iv->rows->grow((stored + kRowsPerBlock - 1) / kRowsPerBlock)))
        return rc;
    const i64 chunk = std::max<i64>(1, (64ll << 20) / ((i64)d * 4));
    std::vector<float> host((size_t)std::min(chunk, std::max<i64>(stored, 1)) * d);
    for (i64 o = 0; o < stored; o += chunk) {   // the ordinary add path: bf16 filter copy and row statistics recomputed
        const i64 m = std::min(chunk, stored - o);
        if (fread(host.data(), sizeof(float), (size_t)m * d, f) != (size_t)m * d) { set_error("%s is truncated", path); return HIPRAG_E_IO; }
        if ((rc = iv->rows->add_host(host.data(), m))) return rc;
    }
    if ((rc = iv->offs.reserve((size_t)(nlist + 1) * 8)) || (rc = iv->orig.reserve((size_t)std::max<i64>(stored, 1) * 8))) return rc;
    HR_CHECK_HIP(hipMemcpy(iv->offs.p, offs.data(), (size_t)(nlist + 1) * 8, hipMemcpyHostToDevice));
    HR_CHECK_HIP(hipMemcpy(iv->orig.p, orig.data(), (size_t)stored * 8, hipMemcpyHostToDevice));
    iv->nlist = nlist;
    iv->n_rows = n;
    for (int l = 0; l < nlist; ++l) iv->maxlen = std::max(iv->maxlen, offs[(size_t)l + 1] - offs[(size_t)l]);
    iv->offs_host = std::move(offs);
    *out_handle = ivf_reg().put(iv);
    return HIPRAG_OK;
}

int32_t hipivf_build_times(uint64_t h, float* out_ms3)
{
    GET_IVF(h);
    HR_REQUIRE(out_ms3, "null out");
    for (int i = 0; i < 3; ++i) out_ms3[i] = iv->build_ms[i];
    return HIPRAG_OK;
}

}  // extern "C"
