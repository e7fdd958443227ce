// dense_index.hip -- flat (brute-force) vector index for MI355X / gfx950.
//
// Replaces faiss.IndexFlatL2 / IndexFlatIP as used by the reference:
//   build   rag/storage/faiss_index.py:121-124   (np.array(float32) -> IndexFlatL2(d).add)
//   search  rag/storage/faiss_index.py:81-83     (index.search(float32[1,d], k))
//
// Data layout in HBM (ours, not FAISS's): rows are stored in 32-row BLOCKS, each block as P = d_pad/8 PIECES of
// 1 KiB.  Piece p of block B holds, for lane = h*32 + r (h in {0,1}, r in 0..31), the four floats
// X[32B + r][8p + 4h + 0..3] at float4 position piece_slot(h, r).  d_pad is d rounded up to 128 floats (zero filled).
// Beside the fp32 rows lives a bf16 FILTER COPY (retile_bf16_kernel): the same blocks with P/2 pieces of 1 KiB, piece p
// holding for lane (h, r) the eight values bf16(X[32B + r][16p + 8h + 0..7]) -- the A fragment of one
// v_mfma_f32_32x32x16_bf16, read with fully coalesced 16-B-per-lane loads straight into MFMA operand registers: no LDS
// staging, no transposes, one wave's work is one contiguous run per block.
//
// One search launch answers up to 1024 queries, 64 per PASS over the index:
//   K1  scan_bf16_kernel (default) / scan_split_kernel   every wave streams a contiguous range of blocks once per pass;
//       queries sit in LDS as bf16 B fragments; two 32 x 32 score tiles per block; per 16-row GROUP only the best and the
//       second-best quad maximum survive, and only for groups that reach a per-query bound the scan itself maintains
//       (class-slot maxima, see "the scan" below) -> a CANDIDATE LIST per query, a few hundred entries
//   K2  fin_kernel   per query: rank the list, re-score the best groups in fp64 from the fp32 rows, extend the re-scored
//       prefix until nothing listed can still reach the top k, exact top-k under (score, id); then a CERTIFICATE: every row
//       that was not re-scored has scan value <= m, hence exact score <= m + eps, eps a worst-case bound of the scan's
//       arithmetic.  If the k-th exact score is not > m + eps the query is flagged and
//   K3  exhaustive_kernel (launched always, exits at once unless a query is flagged) re-scores EVERY row in fp64.
// So results are exact for any input (ties, duplicates, zero vectors), and the common case reads the index once per pass.
//
// Bound: HBM.  Algorithmic bytes per pass = nblocks * P * 512 (bf16 copy) or * 1024 (q64: fp32 rows), + norms in L2 mode
// -- hipidx_stats.bytes_per_pass.  Launches of 256 queries or more on an index of at least one 256-row tile per scan workgroup take scan_wide_kernel
// (scan_wide.h) instead of K1: a tiled MFMA kernel that reads the filter copy once per 256 queries and leaves the same lists.
//
// This file: the layout kernels and the bodies of struct DenseIndex; it is the one translation unit that includes the kernel
// headers dense_scan.h (K1, and scan_wide.h behind it) and dense_finish.h (K2, K3, the start gate's wait), so every kernel is
// compiled once.  Which kernel a launch gets and in what shape: dense_plan.h.  The hipidx_* entries, save / load, the
// registry and the statistics: dense_api.hip.
// The rest of the dense subsystems: dense_layout.h (the layout constants and the fp64 re-score every exact path shares),
// dense_internal.h (struct DenseIndex), dense_remove.hip (in-place removal), dense_scoped.hip (scoped search),
// ivf_search.hip and ivf_build.hip (IVF-Flat on top of this index), group_partials.hip (what the two list-major searches
// share on the host side).
#include <atomic>
#include <cfloat>
#include <cmath>
#include <chrono>
#include <cstring>
#include <vector>

#include "common.h"
#include "topk_device.h"
#include "dense_internal.h"

namespace hiprag {
namespace {

// ------------------------------------------------------------------------------------------------------
// build: row-major -> blocked layout, squared norms
// ------------------------------------------------------------------------------------------------------
__global__ void retile_kernel(const float* __restrict__ src, int64_t row0, int64_t n, int d, int P,
                              float4* __restrict__ xb)
{
    const int64_t blk0 = row0 / kRowsPerBlock;
    const int64_t nblk = (row0 + n - 1) / kRowsPerBlock - blk0 + 1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nblk * P * kPieceVec4) return;
    const int lane = (int)(t & 63);
    const int64_t pp = t >> 6;
    const int p = (int)(pp % P);
    const int64_t blk = blk0 + pp / P;
    const int r = lane & 31, h = lane >> 5;
    const int64_t row = blk * kRowsPerBlock + r;
    if (row < row0 || row >= row0 + n) return;
    const int col = 8 * p + 4 * h;
    const float* s = src + (row - row0) * (int64_t)d + col;
    float4 v;
    v.x = col + 0 < d ? s[0] : 0.f;
    v.y = col + 1 < d ? s[1] : 0.f;
    v.z = col + 2 < d ? s[2] : 0.f;
    v.w = col + 3 < d ? s[3] : 0.f;
    xb[(blk * P + p) * kPieceVec4 + piece_slot(h, r)] = v;
}

__global__ void untile_kernel(const float4* __restrict__ xb, int64_t row0, int64_t n, int d, int P,
                              float* __restrict__ dst)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_row = (int64_t)P * 2;
    if (t >= n * per_row) return;
    const int64_t row = row0 + t / per_row;
    const int ph = (int)(t % per_row);
    const int p = ph >> 1, h = ph & 1;
    const int64_t blk = row / kRowsPerBlock;
    const int r = (int)(row % kRowsPerBlock);
    float4 v = xb[(blk * P + p) * kPieceVec4 + piece_slot(h, r)];
    const int col = 8 * p + 4 * h;
    float* o = dst + (row - row0) * (int64_t)d + col;
    if (col + 0 < d) o[0] = v.x;
    if (col + 1 < d) o[1] = v.y;
    if (col + 2 < d) o[2] = v.z;
    if (col + 3 < d) o[3] = v.w;
}

// Row statistics of one add: |x|^2 (fp64 sum -> float, stored per row; its running maximum rounded UP) and
// |x - bf16(x)|^2 (running maximum, rounded up: the certificate of the bf16 scan bounds |<x - x^, q^>| by |x - x^| |q^|).
// One wave per row at a time, rows grid-strided, each row read ONCE for both sums; a wave keeps its maxima in registers
// and issues two atomics when it is done (one atomicMax per ROW on a single address serialised 125 k of them per
// 125 k-row add: 1.4 ms for a kernel that reads 512 MB).
__global__ __launch_bounds__(256) void row_stats_kernel(const float* __restrict__ src, int64_t row0, int64_t n, int d,
                                                        float* __restrict__ norms, unsigned* __restrict__ max_norm2_bits,
                                                        unsigned* __restrict__ max_dx2_bits)
{
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
    float mx_n = 0.f, mx_d = 0.f;
    for (int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); row < n; row += nw) {
        const float* s = src + row * (int64_t)d;
        double acc = 0.0, dcc = 0.0;
#pragma unroll 8
        for (int c = lane; c < d; c += 64) {
            const float f = s[c];
            const double v = (double)f, dv = v - (double)(float)(__bf16)f;
            acc += v * v;
            dcc += dv * dv;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { acc += __shfl_xor(acc, off); dcc += __shfl_xor(dcc, off); }
        float f = (float)acc;
        if (lane == 0) norms[row0 + row] = f;
        // round up so the stored maxima are upper bounds of the exact values
        if ((double)f < acc) f = nextafterf(f, INFINITY);
        float g = (float)dcc;
        if ((double)g < dcc) g = nextafterf(g, INFINITY);
        mx_n = fmaxf(mx_n, f);
        mx_d = fmaxf(mx_d, g);
    }
    if (lane == 0) {
        atomicMax(max_norm2_bits, __float_as_uint(mx_n));
        atomicMax(max_dx2_bits, __float_as_uint(mx_d));
    }
}

// bf16 FILTER copy of the rows (scan operand of the default mode): block of 32 rows = P/2 pieces of 1 KiB, piece p holds
// for lane l = h*32 + r the eight values bf16(X[32B + r][16p + 8h + 0..7]) -- the A fragment of one
// v_mfma_f32_32x32x16_bf16, 16 bytes per lane, so the scan streams 2 bytes per element straight into MFMA registers.
// The fp32 blocked copy above stays the source of every exact (fp64) re-score.
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
__global__ void retile_bf16_kernel(const float* __restrict__ src, int64_t row0, int64_t n, int d, int P2,
                                   bf16x8_t* __restrict__ xh)
{
    const int64_t blk0 = row0 / kRowsPerBlock;
    const int64_t nblk = (row0 + n - 1) / kRowsPerBlock - blk0 + 1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nblk * P2 * 64) return;
    const int lane = (int)(t & 63);
    const int64_t pp = t >> 6;
    const int p = (int)(pp % P2);
    const int64_t blk = blk0 + pp / P2;
    const int r = lane & 31, h = lane >> 5;
    const int64_t row = blk * kRowsPerBlock + r;
    if (row < row0 || row >= row0 + n) return;
    const int col = 16 * p + 8 * h;
    const float* s = src + (row - row0) * (int64_t)d + col;
    bf16x8_t v;
    if ((d & 3) == 0 && col + 8 <= d) {   // the usual case: two 16-B loads (eight predicated scalar loads cost a round trip each)
        const float4 a = *reinterpret_cast<const float4*>(s), b = *reinterpret_cast<const float4*>(s + 4);
        v[0] = (__bf16)a.x; v[1] = (__bf16)a.y; v[2] = (__bf16)a.z; v[3] = (__bf16)a.w;
        v[4] = (__bf16)b.x; v[5] = (__bf16)b.y; v[6] = (__bf16)b.z; v[7] = (__bf16)b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (__bf16)(col + j < d ? s[j] : 0.f);
    }
    xh[(blk * P2 + p) * 64 + lane] = v;
}

#include "dense_scan.h"
#include "dense_finish.h"

}  // namespace

// ------------------------------------------------------------------------------------------------------
// host object
// ------------------------------------------------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (function, size) instead of on every launch
int32_t ensure_lds(const void* fn, size_t bytes)
{
    static std::mutex mu;
    static std::unordered_map<const void*, size_t> done;
    std::lock_guard<std::mutex> g(mu);
    auto it = done.find(fn);
    if (it != done.end() && it->second >= bytes) return HIPRAG_OK;
    HR_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done[fn] = bytes;
    return HIPRAG_OK;
}

DenseIndex::~DenseIndex()
{
    if (pipe_in) (void)hipEventDestroy(pipe_in);
    for (int i = 0; i < kSlots; ++i) {
        if (pipe_scanned[i]) (void)hipEventDestroy(pipe_scanned[i]);
        if (pipe_done[i]) (void)hipEventDestroy(pipe_done[i]);
    }
    if (add_ev) (void)hipEventDestroy(add_ev);
}

int32_t DenseIndex::init()
{
    HR_CHECK_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    HR_CHECK_HIP(hipGetDeviceProperties(&prop, device));
    n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    scan_cus = n_cu;
    if (const char* ms = getenv("HIPRAG_SCAN_MODE")) {
        if (!strcmp(ms, "bf16")) scan_mode = kScanBf16;
        else if (!strcmp(ms, "q64")) scan_mode = kScanQ64;
        else { set_error("HIPRAG_SCAN_MODE=%s: the scan has two operand modes, bf16 (default) and q64", ms); return HIPRAG_E_INVALID; }
    }
    if (const char* sw = getenv("HIPRAG_SCAN_WIDE")) {
        if (!strcmp(sw, "0")) scan_wide = 0;
        else if (!strcmp(sw, "1")) scan_wide = 1;
        else { set_error("HIPRAG_SCAN_WIDE=%s: 0 (never the wide scan kernel) or 1 (whenever a launch is eligible)", sw); return HIPRAG_E_INVALID; }
    }
    if (const char* fe = getenv("HIPRAG_WIDE_FOLD_EVERY")) {
        char* end = nullptr;
        const long n = strtol(fe, &end, 10);
        if (end == fe || *end || !wide_fold_every_ok(n)) {
            set_error("HIPRAG_WIDE_FOLD_EVERY=%s: a power of two in 1..%d (the wide scan recomputes a unit's bound in one tile out of so many; 1 = in every tile)", fe, kWideFoldMax);
            return HIPRAG_E_INVALID;
        }
        wide_fold_every = (int)n;
    }
    const char* lq = getenv("HIPRAG_LAUNCH_QUERIES");
    launch_env = lq ? atoi(lq) : 0;
    update_launch_q();
    int32_t rc = scalars.reserve(64);
    if (rc) return rc;
    if ((rc = started.reserve(256))) return rc;
    HR_CHECK_HIP(hipMemset(started.p, 0, 256));
    gate = started.as<unsigned long long>() + 16;   // its own 128-byte line
    HR_CHECK_HIP(hipMemset(scalars.p, 0, 64));
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));   // hipMemset of device memory may return before the fill has run
    return HIPRAG_OK;
}

int32_t DenseIndex::grow(int64_t need_blocks)
{
    if (need_blocks <= cap_blocks) return HIPRAG_OK;
    {   // the copies below run on the null stream: rows a previous add is still writing must have landed
        const int32_t wrc = wait_adds_host();
        if (wrc) return wrc;
    }
    int64_t nc = cap_blocks == 0 ? need_blocks : std::max(need_blocks, cap_blocks + cap_blocks / 2);
    size_t xbytes = (size_t)nc * P * kPieceFloats * sizeof(float);
    size_t nbytes = (size_t)nc * kRowsPerBlock * sizeof(float);
    size_t hbytes = xbytes / 2;   // bf16 filter copy
    void* nx = nullptr;
    void* nn = nullptr;
    void* nh = nullptr;
    // The buffer the scan STREAMS is allocated first.  How fast 2048 waves stream a buffer depends on which physical pages
    // it got: the same binary scanned 1M rows at 2.77-2.94 ms per launch with the filter copy allocated behind the 4 GB
    // of fp32 rows and at 2.60-2.66 with it allocated first (A/B in fresh processes, several boxes; the "allocation
    // lottery" of rounds 1-2, which blamed the scan's output).  Probing several candidate allocations and keeping the
    // fastest was measured too and bought nothing beyond this order.
    const bool stream_h = scan_mode == kScanBf16;
    HR_CHECK_HIP(hipMalloc(stream_h ? &nh : &nx, stream_h ? hbytes : xbytes));
    hipError_t e = hipMalloc(stream_h ? &nx : &nh, stream_h ? xbytes : hbytes);
    if (e == hipSuccess) e = hipMalloc(&nn, nbytes);
    if (e != hipSuccess) { if (nx) (void)hipFree(nx); if (nh) (void)hipFree(nh); if (nn) (void)hipFree(nn); HR_CHECK_HIP(e); }
    HR_CHECK_HIP(hipMemset(nx, 0, xbytes));
    HR_CHECK_HIP(hipMemset(nn, 0, nbytes));
    HR_CHECK_HIP(hipMemset(nh, 0, hbytes));
    // hipMemset of device memory is ordered on the null stream but may return before the fill has run, and the kernels
    // that write and read these buffers run on the callers' (non-blocking) streams
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    if (xb.p) {
        HR_CHECK_HIP(hipMemcpy(nx, xb.p, (size_t)cap_blocks * P * kPieceFloats * sizeof(float), hipMemcpyDeviceToDevice));
        HR_CHECK_HIP(hipMemcpy(nn, norms.p, (size_t)cap_blocks * kRowsPerBlock * sizeof(float), hipMemcpyDeviceToDevice));
        HR_CHECK_HIP(hipMemcpy(nh, xh.p, (size_t)cap_blocks * P * kPieceFloats * sizeof(float) / 2, hipMemcpyDeviceToDevice));
    }
    xb.release();
    norms.release();
    xh.release();
    xb.p = nx; xb.bytes = xbytes;
    norms.p = nn; norms.bytes = nbytes;
    xh.p = nh; xh.bytes = hbytes;
    cap_blocks = nc;
    return HIPRAG_OK;
}

int32_t DenseIndex::add_dev(const float* x_dev, int64_t n, hipStream_t st)
{
    if (n == 0) return HIPRAG_OK;
    int32_t rc = grow((ntotal + n + kRowsPerBlock - 1) / kRowsPerBlock);
    if (rc) return rc;
    const int64_t blk0 = ntotal / kRowsPerBlock;
    const int64_t nblk = (ntotal + n - 1) / kRowsPerBlock - blk0 + 1;
    const int64_t threads = nblk * P * kPieceVec4;
    hipLaunchKernelGGL(retile_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, x_dev, ntotal, n, d, P,
                       xb.as<float4>());
    hipLaunchKernelGGL(row_stats_kernel, dim3((unsigned)std::min<int64_t>((n + 3) / 4, 4096)), dim3(256), 0, st, x_dev,
                       ntotal, n, d, norms.as<float>(), max_norm2_bits(), max_dx2_bits());
    hipLaunchKernelGGL(retile_bf16_kernel, dim3((unsigned)((nblk * (P / 2) * 64 + 255) / 256)), dim3(256), 0, st, x_dev, ntotal, n,
                       d, P / 2, xh.as<bf16x8_t>());
    HR_CHECK_HIP(hipGetLastError());
    if (!add_ev) HR_CHECK_HIP(hipEventCreateWithFlags(&add_ev, hipEventDisableTiming));
    HR_CHECK_HIP(hipEventRecord(add_ev, st));
    add_pending = true;
    ntotal += n;
    update_launch_q();
    return HIPRAG_OK;
}

int32_t DenseIndex::add_host(const float* x, int64_t n)
{
    if (n == 0) return HIPRAG_OK;
    const int64_t chunk_rows = std::max<int64_t>(1, (int64_t)(256ll << 20) / ((int64_t)d * 4));
    DevBuf stage;
    int32_t rc = stage.reserve((size_t)std::min(chunk_rows, n) * d * sizeof(float));
    if (rc) return rc;
    rc = grow((ntotal + n + kRowsPerBlock - 1) / kRowsPerBlock);
    if (rc) return rc;
    for (int64_t o = 0; o < n; o += chunk_rows) {
        const int64_t m = std::min(chunk_rows, n - o);
        HR_CHECK_HIP(hipMemcpy(stage.p, x + o * d, (size_t)m * d * sizeof(float), hipMemcpyHostToDevice));
        rc = add_dev(stage.as<float>(), m, nullptr);
        if (rc) return rc;
        HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    }
    return HIPRAG_OK;
}

// Workspace of one slot for (up to launch_q queries, k), allocated on first use: an unused slot costs nothing.
int32_t DenseIndex::reserve_slot(int slot, int k)
{
    Workspace& w = ws[slot];
    const int64_t nb = std::max<int64_t>(nblocks(), 1);
    if (k <= w.k && nb <= w.blocks && launch_q <= w.q) return HIPRAG_OK;
    const int kk = std::max(k, w.k);
    const int64_t nbb = std::max(nb, w.blocks);
    const int64_t nslices = (nbb * kRowsPerBlock + kExRows - 1) / kExRows;
    const int ekk = std::min(kk, kExRows);
    const size_t Q = (size_t)std::max(launch_q, w.q);
    int32_t rc;
    if ((rc = w.list.reserve(Q * kCandCap * sizeof(Cand)))) return rc;
    const size_t state_bytes = state_words(Q) * sizeof(u32);
    const bool fresh = w.state.bytes < state_bytes;
    if ((rc = w.state.reserve(state_bytes))) return rc;
    if (fresh) {   // the finish keeps it clean from here on
        // the fill is ordered on the null stream only and may still be pending when hipMemset returns; the scan that reads
        // this state runs on a non-blocking stream (a garbage bound drops candidates: seen once as a two-rank mismatch)
        HR_CHECK_HIP(hipMemset(w.state.p, 0, w.state.bytes));
        HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    }
    if ((rc = w.flags.reserve(2 * Q * sizeof(int)))) return rc;  // flags[Q] + arrivals[Q]
    if (uses_qtile_images(shape()) && (rc = w.qtile.reserve((Q / 64) * (size_t)P * 64 * 16))) return rc;   // passes x (2 * P2 * 64) fragments
    if ((rc = w.ek.reserve(Q * nslices * ekk * sizeof(u64)))) return rc;
    if ((rc = w.ei.reserve(Q * nslices * ekk * sizeof(i64)))) return rc;
    w.k = kk;
    w.blocks = nbb;
    w.q = (int)Q;
    return HIPRAG_OK;
}

size_t DenseIndex::state_words(size_t Q) { return 2 * Q + (Q / 64) * kClasses * 64; }

// create-on-first-use of what timing needs (prepare)
int32_t ScanTiming::ensure(int n_cu_, int device)
{
    if (!on || !evs.empty()) return HIPRAG_OK;
    n_cu = n_cu_;
    evs.resize(2 * kEvRing);
    ev_set.assign(kEvRing, 0);
    ev_waves.assign(kEvRing, 0);
    for (auto& e : evs) HR_CHECK_HIP(hipEventCreate(&e));
    int32_t src = stamps.reserve((size_t)kEvRing * n_cu * kMaxScanWaves * 2 * sizeof(unsigned long long));
    if (src) return src;
    (void)hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, device);
    if (wall_khz <= 0) wall_khz = 100000;
    return HIPRAG_OK;
}

int ScanTiming::note(bool bracketed, int waves)
{
    if (!on) return -1;
    const int ev = slot();
    ev_set[ev] = bracketed;
    ev_waves[ev] = waves;
    ++count;
    return ev;
}

int32_t ScanTiming::summarise(bool have_rows, hipidx_stats* out) const
{
    out->avg_scan_ms = -1.f;
    out->avg_scan_wall_ms = -1.f;
    out->avg_scan_gap_ms = 0.f;
    out->timed_passes = 0;
    if (evs.empty() || count <= 0) return HIPRAG_OK;
    const int64_t n = std::min<int64_t>(count, kEvRing);
    double sum = 0.0;
    int64_t ok = 0;
    for (int64_t i = 0; i < n; ++i) {
        float ms = 0.f;
        if (ev_set[(size_t)i] && hipEventElapsedTime(&ms, evs[2 * i], evs[2 * i + 1]) == hipSuccess) { sum += ms; ++ok; }
    }
    if (ok) { out->avg_scan_ms = (float)(sum / ok); out->timed_passes = ok; }
    // the same launches on the GPU's own wall clock: first wave in -> last wave out, and the idle time between the
    // last wave of one scan and the first wave of the next (negative = the next scan started on CUs already free)
    if (!stamps.p || !have_rows) return HIPRAG_OK;
    const size_t per = (size_t)n_cu * kMaxScanWaves * 2;
    std::vector<unsigned long long> hst((size_t)n * per);
    HR_CHECK_HIP(hipMemcpy(hst.data(), stamps.p, hst.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::vector<std::pair<unsigned long long, unsigned long long>> se((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        unsigned long long lo = ~0ull, hi = 0;
        const size_t nwaves = std::min<size_t>((size_t)std::max(ev_waves[(size_t)i], 0), per / 2);   // the launch's own waves
        for (size_t w = 0; w < nwaves; ++w) {
            lo = std::min(lo, hst[(size_t)i * per + 2 * w]);
            hi = std::max(hi, hst[(size_t)i * per + 2 * w + 1]);
        }
        se[(size_t)i] = {lo, hi};
    }
    double dsum = 0.0, gsum = 0.0;
    for (int64_t i = 0; i < n; ++i) dsum += (double)(se[(size_t)i].second - se[(size_t)i].first);
    const bool ordered = count <= kEvRing;
    for (int64_t i = 0; ordered && i + 1 < n; ++i) gsum += (double)((long long)se[(size_t)i + 1].first - (long long)se[(size_t)i].second);
    out->avg_scan_wall_ms = (float)(dsum / n / wall_khz);
    out->avg_scan_gap_ms = ordered && n > 1 ? (float)(gsum / (n - 1) / wall_khz) : 0.f;
    return HIPRAG_OK;
}

// the kernel of a plan
using ScanKernel = void (*)(ScanArgs);
template <int METRIC>
static ScanKernel scan_kernel_of(const ScanPlan& p, ScanMode mode)
{
    if (p.wide) return scan_wide_kernel<METRIC>;
    if (mode == kScanQ64) return p.multi_pass ? scan_split_kernel<METRIC, 8, 16, true> : scan_split_kernel<METRIC, 8, 16, false>;
    if (p.waves == 4) return p.multi_pass ? scan_bf16_kernel<METRIC, 4, 16, true> : scan_bf16_kernel<METRIC, 4, 16, false>;
    if (p.ring == 16) return p.multi_pass ? scan_bf16_kernel<METRIC, 8, 16, true> : scan_bf16_kernel<METRIC, 8, 16, false>;
    return p.multi_pass ? scan_bf16_kernel<METRIC, 8, 8, true> : scan_bf16_kernel<METRIC, 8, 8, false>;
}

// phase 1 of a launch (<= launch_q queries): the scan, on `cus` workgroups, into workspace `slot`
template <int METRIC>
int32_t DenseIndex::scan_pass(const float* q_dev, int nq, int k, int slot, int cus, hipStream_t st)
{
    Workspace& w = ws[slot];
    const ScanPlan pl = plan(nq, k, cus);
    const bool use_ev = timing.bracket() && pl.run;
    w.seq = 0;
    if (pl.run) {
        if (w.dirty) HR_CHECK_HIP(hipMemsetAsync(w.state.p, 0, w.state.bytes, st));   // a scan without its finish came before
        w.dirty = true;
        w.waves = pl.waves;
        ScanArgs sa;
        sa.xb = xb.as<float4>(); sa.xh = xh.p; sa.q = q_dev; sa.norms = norms.as<float>();
        sa.slots = st_slots(w); sa.thetac = st_thetac(w); sa.count = st_count(w);
        sa.list = w.list.as<Cand>();
        sa.nblocks = nblocks(); sa.ntotal = ntotal; sa.nq = nq; sa.d = d; sa.P = P;
        sa.filter = pl.filter ? 1 : 0;
        sa.ncls = pl.ncls;
        // (no fill of the stamp slot ahead of the launch -- a kernel of its own between two scans, 5-15 us: the host knows
        // how many waves the launch has and reads exactly their words)
        sa.stamps = timing.launch_stamps();
        w.seq = ++scan_seq;
        started_total += (unsigned long long)cus;
        sa.started = started.as<unsigned long long>(); sa.target = started_total; sa.seq = w.seq; sa.gate = gate;
        sa.fold_every = wide_fold_every; sa.folds = fold_counter();
        sa.qtile = nullptr;
        if (pl.qtile_image) {
            const int npass = (nq + kPassQ - 1) / kPassQ, per_pass = P * 64;   // 2 * P2 * 64 fragments of 16 B
            hipLaunchKernelGGL(qtile_kernel, dim3((unsigned)((per_pass + 255) / 256), (unsigned)npass), dim3(256), 0, st, q_dev, nq, d,
                               P / 2, w.qtile.as<bf16x8>());
            sa.qtile = w.qtile.p;
        }
        const ScanKernel scan = scan_kernel_of<METRIC>(pl, scan_mode);
        if (pl.wide) ++wide_launches;
        { int32_t lrc = ensure_lds(reinterpret_cast<const void*>(scan), pl.lds_bytes); if (lrc) return lrc; }
        if (use_ev) HR_CHECK_HIP(hipEventRecord(timing.edge(0), st));
        hipLaunchKernelGGL(scan, dim3(cus), dim3(pl.waves * 64), pl.lds_bytes, st, sa);
        if (use_ev) HR_CHECK_HIP(hipEventRecord(timing.edge(1), st));
    }
    w.ev_idx = timing.note(use_ev, pl.run ? cus * w.waves : 0);
    HR_CHECK_HIP(hipGetLastError());
    passes += (nq + kPassQ - 1) / kPassQ;
    ++launches;
    queries += nq;
    return HIPRAG_OK;
}

// phase 2: the finish (list ranking, fp64 re-score, extension, certificate) + the exhaustive path; reads workspace `slot`
// host_flags (pinned host memory, nq ints) != null: the finish also writes the queries' flags there and the exhaustive
// check is NOT launched -- the caller synchronises, looks at the flags and calls exhaustive_pass only if one is set
// (hipidx_search's few-query path: one launch and one kernel's run time less on the way to the host)
template <int METRIC>
int32_t DenseIndex::finish_pass(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st,
                    int* host_flags)
{
    Workspace& w = ws[slot];
    const ScanPlan pl = plan(nq, k, scan_cus);   // `run` and `filter` do not depend on the grid
    int* flags = w.flags.as<int>();
    int* arrivals = flags + w.q;
    if (pl.run) {
        FinArgs fa;
        fa.xb = xb.as<float4>(); fa.q = q_dev; fa.max_norm2_bits = max_norm2_bits();
        fa.out64 = o64p; fa.out32 = o32p; fa.out_ids = oidp; fa.flags = flags; fa.host_flags = host_flags; fa.arrivals = arrivals;
        fa.fallback_counter = fallback_counter(); fa.extend_counter = extend_counter(); fa.work_counters = work_counters();
        fa.slots = st_slots(w); fa.thetac = st_thetac(w); fa.count = st_count(w);
        fa.list = w.list.as<Cand>();
        fa.ntotal = ntotal; fa.id_base = id_base; fa.d = d; fa.P = P; fa.k = k; fa.mode = scan_mode;
        fa.filter = pl.filter ? 1 : 0;
        if (k >= 32) hipLaunchKernelGGL((fin_kernel<METRIC, 1024>), dim3(nq), dim3(1024), 0, st, fa);
        else hipLaunchKernelGGL((fin_kernel<METRIC, kFinThreads>), dim3(nq), dim3(kFinThreads), 0, st, fa);
        w.dirty = false;
    } else {
        hipLaunchKernelGGL(flag_all_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, flags, arrivals, fallback_counter(), nq);
        host_flags = nullptr;   // every query is flagged: nothing to look at first
    }
    if (host_flags) { HR_CHECK_HIP(hipGetLastError()); return HIPRAG_OK; }
    return exhaustive_pass<METRIC>(q_dev, nq, k, slot, o64p, o32p, oidp, st);
}

template <int METRIC>
int32_t DenseIndex::exhaustive_pass(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st)
{
    Workspace& w = ws[slot];
    int* flags = w.flags.as<int>();
    int* arrivals = flags + w.q;
    ExArgs ea;
    ea.xb = xb.as<float4>(); ea.q = q_dev; ea.flags = flags; ea.arrivals = arrivals;
    ea.ek = w.ek.as<u64>(); ea.ei = w.ei.as<i64>();
    ea.out64 = o64p; ea.out32 = o32p; ea.out_ids = oidp; ea.ntotal = ntotal; ea.id_base = id_base;
    ea.d = d; ea.P = P; ea.k = k; ea.kk = std::min(k, kExRows); ea.nq = nq;
    ea.nslices = (int)std::max<int64_t>(1, (ntotal + kExRows - 1) / kExRows);
    const size_t ex_lds = (size_t)kExRows * 16 + (size_t)k * 16 + 2 * (kSelThreads / 64) * sizeof(KeyId) +
                          (size_t)P * 8 * sizeof(float) + 16;
    auto exk = exhaustive_kernel<METRIC>;
    { int32_t lrc = ensure_lds(reinterpret_cast<const void*>(exk), ex_lds); if (lrc) return lrc; }
    hipLaunchKernelGGL(exk, dim3(std::min(ea.nslices, n_cu)), dim3(kSelThreads), ex_lds, st, ea);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

int32_t DenseIndex::prepare(int k, int slot)
{
    int32_t rc = reserve_slot(slot, k);
    if (rc) return rc;
    return timing.ensure(n_cu, device);
}

int32_t DenseIndex::begin_dev(const float* q_dev, int nq, int k, int slot, int cus, hipStream_t st)
{
    if (add_pending) {   // rows of the last add may still be in flight on another stream
        if (hipEventQuery(add_ev) == hipSuccess) add_pending = false;
        else { const int32_t wrc = wait_adds_stream(st); if (wrc) return wrc; }
    }
    return metric == HIPRAG_METRIC_IP ? scan_pass<HIPRAG_METRIC_IP>(q_dev, nq, k, slot, cus, st)
                                      : scan_pass<HIPRAG_METRIC_L2>(q_dev, nq, k, slot, cus, st);
}

int32_t DenseIndex::finish_dev(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st,
                   int* host_flags)
{
    return metric == HIPRAG_METRIC_IP ? finish_pass<HIPRAG_METRIC_IP>(q_dev, nq, k, slot, o64p, o32p, oidp, st, host_flags)
                                      : finish_pass<HIPRAG_METRIC_L2>(q_dev, nq, k, slot, o64p, o32p, oidp, st, host_flags);
}

int32_t DenseIndex::exhaustive_dev(const float* q_dev, int nq, int k, int slot, double* o64p, float* o32p, int64_t* oidp, hipStream_t st)
{
    return metric == HIPRAG_METRIC_IP ? exhaustive_pass<HIPRAG_METRIC_IP>(q_dev, nq, k, slot, o64p, o32p, oidp, st)
                                      : exhaustive_pass<HIPRAG_METRIC_L2>(q_dev, nq, k, slot, o64p, o32p, oidp, st);
}

// hipidx_search for a handful of queries (the reference's call shape: ONE, rag/storage/faiss_index.py:81-83): what is
// not the scan has to be short.  Query up through pinned staging with an asynchronous copy; the finish writes scores,
// ids and its flags straight into pinned host memory; one synchronise; the exhaustive check is launched only if the
// finish flagged a query (it almost never does) -- against the general path: two blocking D2H copies, one blocking H2D
// copy and one kernel less between the scan and the caller.
int32_t DenseIndex::search_few_host(const float* q_host, int nq, int k, float* out_scores, int64_t* out_ids)
{
    int32_t rc;
    const size_t nk = (size_t)nq * k;
    if ((rc = qbuf.reserve((size_t)nq * d * sizeof(float)))) return rc;
    if ((rc = o64.reserve(nk * sizeof(double)))) return rc;
    if ((rc = pin_q.reserve((size_t)nq * d * sizeof(float)))) return rc;
    if ((rc = pin_o32.reserve(nk * sizeof(float)))) return rc;
    if ((rc = pin_oid.reserve(nk * sizeof(int64_t)))) return rc;
    if ((rc = pin_flags.reserve((size_t)nq * sizeof(int)))) return rc;
    if ((rc = prepare(k, 0))) return rc;
    memcpy(pin_q.p, q_host, (size_t)nq * d * sizeof(float));
    HR_CHECK_HIP(hipMemcpyAsync(qbuf.p, pin_q.p, (size_t)nq * d * sizeof(float), hipMemcpyHostToDevice, nullptr));
    int* hf = reinterpret_cast<int*>(pin_flags.p);
    float* h32 = reinterpret_cast<float*>(pin_o32.p);
    int64_t* hid = reinterpret_cast<int64_t*>(pin_oid.p);
    if ((rc = begin_dev(qbuf.as<float>(), nq, k, 0, scan_cus, nullptr))) return rc;
    for (int i = 0; i < nq; ++i) hf[i] = 1;   // a finish that does not write them (k beyond the fast path) launches the check itself
    if ((rc = finish_dev(qbuf.as<float>(), nq, k, 0, o64.as<double>(), h32, hid, nullptr, hf))) return rc;
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    if (nblocks() > 0 && fast_k(k)) {
        int any = 0;
        for (int i = 0; i < nq; ++i) any |= hf[i];
        if (any) {
            if ((rc = exhaustive_dev(qbuf.as<float>(), nq, k, 0, o64.as<double>(), h32, hid, nullptr))) return rc;
            HR_CHECK_HIP(hipStreamSynchronize(nullptr));
        }
    }
    memcpy(out_scores, h32, nk * sizeof(float));
    memcpy(out_ids, hid, nk * sizeof(int64_t));
    return HIPRAG_OK;
}

int32_t DenseIndex::pipe_init()
{
    if (pipe_tail) return HIPRAG_OK;
    {   // the device's tail stream 0 (library-owned, shared by every index of the device: lib.cpp)
        void* t = nullptr;
        const int32_t trc = hiprag_tail_stream(device, 0, &t);
        if (trc) return trc;
        pipe_tail = (hipStream_t)t;
    }
    HR_CHECK_HIP(hipEventCreateWithFlags(&pipe_in, hipEventDisableTiming));
    for (int i = 0; i < kSlots; ++i) {
        HR_CHECK_HIP(hipEventCreateWithFlags(&pipe_scanned[i], hipEventDisableTiming));
        HR_CHECK_HIP(hipEventCreateWithFlags(&pipe_done[i], hipEventDisableTiming));
    }
    return HIPRAG_OK;
}

// A batch of several launches, pipelined the way hiprag/sharded.py pipelines steps: the scans chained on the
// device's high-priority scan stream with CUs left out of their grids, the finish of launch j on the index's tail stream
// behind the end of scan j AND the start of scan j + 1 (the start gate), the last one ungated; `st` -- where the queries
// come from and the results are wanted -- is ahead of the first scan and behind the last finish.  Nothing synchronises
// the host.  Uses every workspace slot: not to be mixed with a begin / finish pipeline in flight on the same index.
int32_t DenseIndex::search_dev_pipelined(const float* q_dev, int nq, int k, double* o64p, float* o32p, int64_t* oidp, hipStream_t st)
{
    int32_t rc = pipe_init();
    if (rc) return rc;
    void* hpv = nullptr;
    if ((rc = hiprag_scan_stream(device, &hpv))) return rc;
    hipStream_t hp = (hipStream_t)hpv;
    HR_CHECK_HIP(hipEventRecord(pipe_in, st));
    HR_CHECK_HIP(hipStreamWaitEvent(hp, pipe_in, 0));
    HR_CHECK_HIP(hipStreamWaitEvent(pipe_tail, pipe_in, 0));   // (the output buffers: whatever `st` still does with them is ahead)
    const int cus = std::min(scan_cus, std::max(1, n_cu - pipe_spare_cus()));
    const int L = (nq + launch_q - 1) / launch_q;
    auto tails = [&](int j, bool gated) -> int32_t {
        const int slot = j % kSlots, o = j * launch_q, m = std::min(launch_q, nq - o);
        HR_CHECK_HIP(hipStreamWaitEvent(pipe_tail, pipe_scanned[slot], 0));
        if (gated) { const int32_t grc = gate_tail(slot, pipe_tail); if (grc) return grc; }
        const int32_t frc = finish_dev(q_dev + (int64_t)o * d, m, k, slot, o64p + (int64_t)o * k, o32p ? o32p + (int64_t)o * k : nullptr,
                                       oidp + (int64_t)o * k, pipe_tail);
        if (frc) return frc;
        HR_CHECK_HIP(hipEventRecord(pipe_done[slot], pipe_tail));
        return HIPRAG_OK;
    };
    rc = HIPRAG_OK;
    int launched = 0;
    for (int j = 0; j < L && !rc; ++j) {
        const int slot = j % kSlots, o = j * launch_q, m = std::min(launch_q, nq - o);
        if (j >= kSlots) rc = hipStreamWaitEvent(hp, pipe_done[slot], 0) == hipSuccess ? HIPRAG_OK : HIPRAG_E_HIP;   // the slot's previous finish
        if (!rc) rc = prepare(k, slot);
        if (!rc) rc = begin_dev(q_dev + (int64_t)o * d, m, k, slot, cus, hp);
        if (!rc) rc = hipEventRecord(pipe_scanned[slot], hp) == hipSuccess ? HIPRAG_OK : HIPRAG_E_HIP;
        if (!rc) { launched = j + 1; if (j >= 1) rc = tails(j - 1, true); }
    }
    // the last launched scan's finish has no scan behind it: no gate (nothing would open it)
    if (launched > 0) { const int32_t trc = tails(launched - 1, false); if (!rc) rc = trc; }
    if (launched > 0) HR_CHECK_HIP(hipStreamWaitEvent(st, pipe_done[(launched - 1) % kSlots], 0));   // the tail stream is in order: the last finish is behind all others
    if (rc == HIPRAG_E_HIP) set_error("a HIP call failed while enqueueing a pipelined search: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

int32_t DenseIndex::search_dev(const float* q_dev, int nq, int k, double* o64p, float* o32p, int64_t* oidp, hipStream_t st)
{
    int32_t rc = prepare(k, 0);
    if (rc) return rc;
    if (nq > launch_q && nblocks() > 0 && fast_k(k)) return search_dev_pipelined(q_dev, nq, k, o64p, o32p, oidp, st);
    for (int o = 0; o < nq; o += launch_q) {
        const int m = std::min(launch_q, nq - o);
        const float* qo = q_dev + (int64_t)o * d;
        if ((rc = begin_dev(qo, m, k, 0, scan_cus, st))) return rc;
        if ((rc = finish_dev(qo, m, k, 0, o64p + (int64_t)o * k, o32p ? o32p + (int64_t)o * k : nullptr,
                             oidp + (int64_t)o * k, st)))
            return rc;
    }
    return HIPRAG_OK;
}

// rows [o, o + m) of a flat index, row-major fp32, to host memory (null stream; tmp: m * d floats)
int32_t read_rows_host(DenseIndex& ix, i64 o, i64 m, DevBuf& tmp, float* host)
{
    int32_t rc = tmp.reserve((size_t)std::max<i64>(m, 1) * ix.d * sizeof(float));
    if (rc) return rc;
    if ((rc = ix.wait_adds_host())) return rc;
    const i64 threads = m * ix.P * 2;
    hipLaunchKernelGGL(untile_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, nullptr, ix.xb.as<float4>(), (int64_t)o,
                       (int64_t)m, ix.d, ix.P, tmp.as<float>());
    HR_CHECK_HIP(hipGetLastError());
    HR_CHECK_HIP(hipMemcpy(host, tmp.p, (size_t)m * ix.d * sizeof(float), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

int32_t DenseIndex::gate_tail(int slot, hipStream_t st)
{
    const unsigned long long seq = ws[slot].seq;
    if (!gate || seq == 0) return HIPRAG_OK;
    // only a scan that is already on its way can open the gate: a wait for one that has not been launched is a mistake of the
    // caller's (it would merely run into the wait's time limit)
    HR_REQUIRE(scan_seq > seq, "hipidx_gate_tail_dev: no scan has been launched after the one of slot %d", slot);
    hipLaunchKernelGGL(gate_wait_kernel, dim3(1), dim3(64), 0, st, gate, seq + 1);
    HR_CHECK_HIP(hipGetLastError());
    return HIPRAG_OK;
}

}  // namespace hiprag
