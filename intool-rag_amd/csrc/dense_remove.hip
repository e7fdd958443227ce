// dense_remove.hip -- hipidx_remove_ranges: faiss.IndexFlat.remove_ids on local row ranges, a stable compaction of the
// blocked layout of the flat index (dense_index.hip, dense_layout.h) in place.
#include <algorithm>
#include <cmath>
#include <vector>

#include "dense_internal.h"
#include "range_table.h"

namespace hiprag {
namespace {

// ------------------------------------------------------------------------------------------------------
// removal (hipidx_remove_ranges): stable compaction of the blocked layout, in place
// ------------------------------------------------------------------------------------------------------
// Destination row j >= `first` (the first removed row) takes source row j + shift, shift = the rows removed at or before
// its source: the surviving runs behind `first` are a table (run_dst ascending, run_shift), a lane bisects it once per
// block for its row -- the item lookup of the scoped search.  One wave moves one destination block: for every 1 KiB fp32
// piece lane (h, r) reads its float4 at the SOURCE row's piece_slot and writes it at its own; the bf16 filter copy moves
// the same way (16 B per lane, lane-linear pieces: bf16(x) is a function of x alone, so moving it equals recomputing it);
// the norms are a gather of floats.  Plain 16-byte vector loads and stores, eight in flight per lane, no LDS.
// GATHER: index -> staging (chunk-relative blocks), rows >= ntotal_new become zero; !GATHER: staging -> index, identity.
// Lanes of rows < first do nothing in either direction: the prefix is neither read nor written.
struct MoveArgs {
    const float4* src_xb;
    const float4* src_xh;
    const float* src_n;
    float4* dst_xb;
    float4* dst_xh;
    float* dst_n;
    const i64* run_dst;      // [n_runs] first destination row of every surviving run behind `first` (run_dst[0] == first)
    const i64* run_shift;    // [n_runs] source row - destination row
    int n_runs;
    i64 blk0, nblk;          // destination blocks [blk0, blk0 + nblk) of the index
    i64 src_blk_off, dst_blk_off;   // block number of the first block of the src / dst buffers (staging: the chunk's blk0)
    i64 first, ntotal_new;
    int P;
};

template <bool GATHER>
__global__ __launch_bounds__(256) void move_rows_kernel(MoveArgs a)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const i64 nw = (i64)gridDim.x * 4;
    const int P2 = a.P / 2;
    for (i64 w = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); w < a.nblk; w += nw) {
        const i64 blk = a.blk0 + w;
        const i64 row = blk * kRowsPerBlock + r;
        if (row < a.first) continue;
        const bool live = !GATHER || row < a.ntotal_new;
        i64 srow = row;
        if (GATHER && live) {
            int lo = 0, hi = a.n_runs;      // the last run that starts at or before `row`
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (a.run_dst[mid] <= row) lo = mid; else hi = mid;
            }
            srow = row + a.run_shift[lo];
        }
        const i64 sblk = srow / kRowsPerBlock - a.src_blk_off, dblk = blk - a.dst_blk_off;
        const int sr = (int)(srow % kRowsPerBlock);
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4* s = a.src_xb + sblk * a.P * kPieceVec4 + piece_slot(h, sr);
        float4* o = a.dst_xb + dblk * a.P * kPieceVec4 + piece_slot(h, r);
        for (int p = 0; p < a.P; p += 8) {          // P is a multiple of 16
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = live ? s[(p + u) * kPieceVec4] : zero;
#pragma unroll
            for (int u = 0; u < 8; ++u) o[(p + u) * kPieceVec4] = v[u];
        }
        s = a.src_xh + sblk * P2 * 64 + h * 32 + sr;
        o = a.dst_xh + dblk * P2 * 64 + lane;
        for (int p = 0; p < P2; p += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = live ? s[(p + u) * 64] : zero;
#pragma unroll
            for (int u = 0; u < 8; ++u) o[(p + u) * 64] = v[u];
        }
        if (h == 0) a.dst_n[dblk * kRowsPerBlock + r] = live ? a.src_n[sblk * kRowsPerBlock + sr] : 0.f;
    }
}

// The two maxima of `scalars` over the blocked rows, with the bits row_stats_kernel gives a fresh add of the same rows.
// There lane c sums columns c, c + 64, ... in fp64 (every product of two floats is exact in fp64, so a fused multiply-add
// and a multiply followed by an add are the same number) and an xor butterfly (offsets 32 .. 1) adds the 64 partial sums.
// Here one wave takes a block: lane (h, r) holds, of row r, the columns 8p + 4h + j of every piece p, i.e. the partial
// sums of the column classes c = 8 (p mod 8) + 4h + j, accumulated over p in ascending order -- the same 64 sums in the same
// order, 32 per lane -- and adds them along the butterfly's tree: offsets 32, 16, 8 pair classes inside the lane, offset 4
// is the other half-row's lane, offsets 2 and 1 are inside the lane again.  Floating-point addition commutes, so which
// side of a pair a lane stands on does not matter.  Padding columns and the rows past ntotal are zero and add +0.0.
// One streaming read of the fp32 rows, 16 bytes per lane; the norms are not written (the move carried them).
__global__ __launch_bounds__(256) void tiled_stats_kernel(const float4* __restrict__ xb, i64 nblocks, int P,
                                                          unsigned* __restrict__ max_norm2_bits, unsigned* __restrict__ max_dx2_bits)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const i64 nw = (i64)gridDim.x * 4;
    float mx_n = 0.f, mx_d = 0.f;
    for (i64 blk = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); blk < nblocks; blk += nw) {
        const float4* s = xb + blk * P * kPieceVec4 + piece_slot(h, r);
        double acc[8][4], dcc[8][4];
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j) { acc[m][j] = 0.0; dcc[m][j] = 0.0; }
        for (int p = 0; p < P; p += 8) {
            float4 v[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = s[(p + m) * kPieceVec4];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const float f4[4] = {v[m].x, v[m].y, v[m].z, v[m].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float f = f4[j];
                    const double x = (double)f, dx = x - (double)(float)(__bf16)f;
                    acc[m][j] += x * x;
                    dcc[m][j] += dx * dx;
                }
            }
        }
        double un[4], ud[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // offsets 32, 16, 8: classes c and c ^ 32 are pieces m and m + 4, then m + 2, then m + 1
            const double n0 = acc[0][j] + acc[4][j], n1 = acc[1][j] + acc[5][j], n2 = acc[2][j] + acc[6][j], n3 = acc[3][j] + acc[7][j];
            const double d0 = dcc[0][j] + dcc[4][j], d1 = dcc[1][j] + dcc[5][j], d2 = dcc[2][j] + dcc[6][j], d3 = dcc[3][j] + dcc[7][j];
            un[j] = (n0 + n2) + (n1 + n3);
            ud[j] = (d0 + d2) + (d1 + d3);
            un[j] += __shfl_xor(un[j], 32);     // offset 4: the other half-row
            ud[j] += __shfl_xor(ud[j], 32);
        }
        const double sn = (un[0] + un[2]) + (un[1] + un[3]), sd = (ud[0] + ud[2]) + (ud[1] + ud[3]);   // offsets 2, 1
        float f = (float)sn;
        if ((double)f < sn) f = nextafterf(f, INFINITY);
        float g = (float)sd;
        if ((double)g < sd) g = nextafterf(g, INFINITY);
        mx_n = fmaxf(mx_n, f);
        mx_d = fmaxf(mx_d, g);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { mx_n = fmaxf(mx_n, __shfl_xor(mx_n, off)); mx_d = fmaxf(mx_d, __shfl_xor(mx_d, off)); }
    if (lane == 0) {
        atomicMax(max_norm2_bits, __float_as_uint(mx_n));
        atomicMax(max_dx2_bits, __float_as_uint(mx_d));
    }
}

}  // namespace

// hipidx_remove_ranges (include/hiprag.h), under the mutex.  Every check runs before anything is touched.
// Order of the move: ascending CHUNKS of destination blocks; a chunk is gathered completely into the staging buffer, then
// written back.  dst <= src for every row, so what a chunk's write-back overwrites (destinations inside the chunk) can
// only be the source of destinations at or before it -- all gathered already -- and the sources of every later chunk
// lie at or beyond the end of this one.  Staging + table <= kRemoveBudget whatever N is.
int32_t DenseIndex::remove_ranges(const int64_t* ranges, int32_t n_ranges)
{
    int32_t rc = check_range_args(ranges, n_ranges);
    if (rc) return rc;
    if (ivf_refs.load() > 0) {
        set_error("this index is referenced by %d live IVF handle(s): removing rows would leave their list offsets stale "
                  "(destroy the IVF index first)", ivf_refs.load());
        return HIPRAG_E_UNSUPPORTED;
    }
    RangeTable rm;     // the non-empty ranges, touching ones joined
    if ((rc = range_table(ranges, n_ranges, ntotal, "ntotal", true, rm))) return rc;
    i64 removed = 0;
    for (const auto& r : rm) removed += r.second - r.first;
    if ((rc = wait_adds_host())) return rc;
    rm_info[0] = removed; rm_info[1] = 0; rm_info[2] = 0; rm_info[3] = 0;
    if (removed == 0) return HIPRAG_OK;
    // the surviving runs behind the first removed row: where each lands, and how many rows were cut in front of it
    const i64 first = rm[0].first;
    std::vector<i64> tab_dst, tab_shift;
    {
        i64 cut = 0;
        for (size_t j = 0; j < rm.size(); ++j) {
            cut += rm[j].second - rm[j].first;
            const i64 next_lo = j + 1 < rm.size() ? rm[j + 1].first : ntotal;
            if (next_lo > rm[j].second) { tab_dst.push_back(rm[j].second - cut); tab_shift.push_back(cut); }
        }
    }
    const i64 n_new = ntotal - removed, moved = n_new - first;
    const i64 nb_old = nblocks(), nb_new = (n_new + kRowsPerBlock - 1) / kRowsPerBlock;
    const i64 bf = first / kRowsPerBlock;
    const size_t xb_blk = (size_t)P * kPieceFloats * sizeof(float), xh_blk = xb_blk / 2, n_blk = kRowsPerBlock * sizeof(float);
    MoveArgs a;
    a.P = P;
    a.first = first;
    a.ntotal_new = n_new;
    a.n_runs = (int)tab_dst.size();
    a.run_dst = a.run_shift = nullptr;
    auto grid = [](i64 nblk) { return dim3((unsigned)std::max<i64>(1, std::min<i64>((nblk + 3) / 4, 4096))); };
    DevBuf stage, tab;     // freed behind the synchronisation of finish_removal
    if (moved == 0) {
        // only a tail goes: nothing moves, the rows of the last kept block behind n_new become zero where they stand
        if (nb_new > bf) {
            a.src_xb = xb.as<float4>(); a.src_xh = xh.as<float4>(); a.src_n = norms.as<float>();
            a.dst_xb = xb.as<float4>(); a.dst_xh = xh.as<float4>(); a.dst_n = norms.as<float>();
            a.blk0 = bf; a.nblk = nb_new - bf; a.src_blk_off = a.dst_blk_off = 0;
            hipLaunchKernelGGL(move_rows_kernel<true>, grid(a.nblk), dim3(256), 0, nullptr, a);
        }
    } else {
        const size_t tab_bytes = tab_dst.size() * 16;
        const size_t per_blk = xb_blk + xh_blk + n_blk;
        const i64 cb = std::max<i64>(1, std::min<i64>(nb_new - bf, (i64)((kRemoveBudget - std::min(tab_bytes, kRemoveBudget)) / per_blk)));
        if ((rc = stage.reserve((size_t)cb * per_blk))) return rc;
        if ((rc = tab.reserve(tab_bytes))) return rc;
        HR_CHECK_HIP(hipMemcpy(tab.p, tab_dst.data(), tab_bytes / 2, hipMemcpyHostToDevice));
        HR_CHECK_HIP(hipMemcpy(tab.as<char>() + tab_bytes / 2, tab_shift.data(), tab_bytes / 2, hipMemcpyHostToDevice));
        a.run_dst = tab.as<i64>();
        a.run_shift = tab.as<i64>() + tab_dst.size();
        float4* st_xb = stage.as<float4>();
        float4* st_xh = reinterpret_cast<float4*>(stage.as<char>() + (size_t)cb * xb_blk);
        float* st_n = reinterpret_cast<float*>(stage.as<char>() + (size_t)cb * (xb_blk + xh_blk));
        for (i64 b = bf; b < nb_new; b += cb) {
            a.blk0 = b; a.nblk = std::min(cb, nb_new - b);
            a.src_xb = xb.as<float4>(); a.src_xh = xh.as<float4>(); a.src_n = norms.as<float>();
            a.dst_xb = st_xb; a.dst_xh = st_xh; a.dst_n = st_n;
            a.src_blk_off = 0; a.dst_blk_off = b;
            hipLaunchKernelGGL(move_rows_kernel<true>, grid(a.nblk), dim3(256), 0, nullptr, a);
            a.src_xb = st_xb; a.src_xh = st_xh; a.src_n = st_n;
            a.dst_xb = xb.as<float4>(); a.dst_xh = xh.as<float4>(); a.dst_n = norms.as<float>();
            a.src_blk_off = b; a.dst_blk_off = 0;
            hipLaunchKernelGGL(move_rows_kernel<false>, grid(a.nblk), dim3(256), 0, nullptr, a);
            ++rm_info[2];
        }
        rm_info[1] = moved;
        rm_info[3] = (i64)(stage.bytes + tab.bytes);
    }
    HR_CHECK_HIP(hipGetLastError());
    return finish_removal(nb_old, nb_new, n_new, xb_blk, xh_blk, n_blk);
}

// behind the move: vacated blocks back to zero (grow leaves them zero, add writes only its own rows), the two maxima
// recomputed over the survivors, the new row count; synchronises
int32_t DenseIndex::finish_removal(i64 nb_old, i64 nb_new, i64 n_new, size_t xb_blk, size_t xh_blk, size_t n_blk)
{
    if (nb_old > nb_new) {
        const size_t nv = (size_t)(nb_old - nb_new);
        HR_CHECK_HIP(hipMemsetAsync(xb.as<char>() + (size_t)nb_new * xb_blk, 0, nv * xb_blk, nullptr));
        HR_CHECK_HIP(hipMemsetAsync(xh.as<char>() + (size_t)nb_new * xh_blk, 0, nv * xh_blk, nullptr));
        HR_CHECK_HIP(hipMemsetAsync(norms.as<char>() + (size_t)nb_new * n_blk, 0, nv * n_blk, nullptr));
    }
    HR_CHECK_HIP(hipMemsetAsync(scalars.p, 0, 2 * sizeof(unsigned), nullptr));
    if (nb_new > 0) {
        hipLaunchKernelGGL(tiled_stats_kernel, dim3((unsigned)std::min<i64>((nb_new + 3) / 4, 4096)), dim3(256), 0, nullptr,
                           xb.as<float4>(), nb_new, P, max_norm2_bits(), max_dx2_bits());
        HR_CHECK_HIP(hipGetLastError());
    }
    ntotal = n_new;
    update_launch_q();
    HR_CHECK_HIP(hipStreamSynchronize(nullptr));
    return HIPRAG_OK;
}
}  // namespace hiprag

using namespace hiprag;

extern "C" {

/* faiss.IndexFlat.remove_ids on local row ranges (include/hiprag.h): stable compaction of the blocked layout in place */
int32_t hipidx_remove_ranges(uint64_t h, const int64_t* ranges_host, int32_t n_ranges)
{
    GET_INDEX(h);
    return ix->remove_ranges(ranges_host, n_ranges);
}

int32_t hipidx_remove_info(uint64_t h, int64_t* out4)
{
    GET_INDEX(h);
    HR_REQUIRE(out4, "out4 is null");
    for (int i = 0; i < 4; ++i) out4[i] = ix->rm_info[i];
    return HIPRAG_OK;
}

int32_t hipidx_row_bounds(uint64_t h, float* out2)
{
    GET_INDEX(h);
    HR_REQUIRE(out2, "out2 is null");
    { const int32_t wrc = ix->wait_adds_host(); if (wrc) return wrc; }
    HR_CHECK_HIP(hipMemcpy(out2, ix->scalars.p, 2 * sizeof(float), hipMemcpyDeviceToHost));
    return HIPRAG_OK;
}

}  // extern "C"
