// scan_wide.h -- the WIDE scan of the bf16 filter copy: a tiled MFMA kernel that answers 256 queries per read of the
// index instead of 64.  Included by dense_index.hip behind the narrow kernels, inside its namespaces: it uses their
// ScanArgs, block_lane_top2, append_direct and the class-slot / thetac protocol, and leaves exactly what they leave
// (candidate lists, count, thetac, class slots), so the finish does not know which scan ran.
//
// Why: scan_bf16_kernel keeps a whole-K query tile in LDS, which holds 64 queries (128 KiB at d_pad = 1024); a 512-query
// launch therefore streams the filter copy eight times and sits at the HBM rate while the matrix pipe idles.  This kernel
// is a GEMM that stages K-SLICES of both operands in LDS and keeps the whole K in the accumulators, so the number of
// queries per read is set by registers, not by LDS.
//
// Tile: 256 rows (8 blocks) x 256 queries (8 query tiles of 32), K in steps of 64 (4 pieces).  Both operands are stored as
// 1 KiB lane-linear fragments of v_mfma_f32_32x32x16_bf16 already -- block B, piece p of the filter copy; the images
// qtile_kernel writes -- so staging is global_load_lds of whole pieces and a fragment read is one lane-linear
// ds_read_b128: no swizzle.  LDS = 2 buffers x (32 KiB rows + 32 KiB queries), ONE object.
// A wave owns 4 blocks x 2 query tiles = 8 accumulators (128 registers): wave w -> blocks 4 (w & 1) + 0..3, query tiles
// 2 (w >> 1) + 0..1, i.e. ONE 64-query unit (the unit of the class slots and of the finish).  Per piece 4 + 2 fragment
// reads feed 8 MFMAs.  `first` / `second` are the same bits as the narrow kernel's: same MFMA, A = rows, B = queries, one
// accumulator per 32 x 32 sub-tile, pieces 0 .. P2 - 1 in that order, then block_lane_top2.
//
// Schedule (the plain one): k-step s + 1 is staged into the other buffer while k-step s is computed; per step
//     s_waitcnt vmcnt(0); barrier; issue(s + 1 -> buffer (s + 1) & 1); compute(s from buffer s & 1)
// Hazards: buffer (s + 1) & 1 was last read by compute(s - 1), which every wave has left when it reaches the barrier of
// step s; buffer s & 1 is read after that barrier, which every wave reaches after ITS OWN share of step s has landed
// (vmcnt(0)).  The step sequence is flat over (row tile, column, k-step), so the staging runs on into the next tile while
// the epilogue of this one runs.
//
// Persistent workgroups, one per scan CU: workgroup i takes row tiles i, i + G, ...; per row tile all columns in turn (the
// re-read of the 512 KiB row tile by the second column can hit the Infinity Cache).  Every (row tile, column) pair is
// computed exactly once.
//
// Epilogue of a tile, per wave, no workgroup barrier:
//   (i)   block_lane_top2 per sub-tile (the L2 norms of the wave's four blocks are loaded here);
//   (ii)  the per-query maxima of the wave's 128 rows -> class slot cls = (2 row_tile + row_half) % 64 of its unit
//         (atomicMax).  The class follows the ROW TILE, so row tiles 0..31 give every class a publisher whatever the grid;
//         the host sends a launch here only when those all fall into the first round (G >= 32) and the filter is on
//         (more than 64 row tiles);
//   (iii) theta of the unit's 64 queries = min over the classes, folded into thetac (atomicMax) BEFORE use, and joined with
//         what thetac already holds.  While a live query has no bound yet -- the first tile of a column -- the wave waits,
//         bounded, for the publishers of the other workgroups;
//   (iv)  first >= bound -> append_direct.
// Invariants:
//   * a value is dropped only against a bound that is already folded into thetac (or was read from it): the FINAL thetac[q]
//     bounds everything that is not on q's list, and exactness never depends on timing -- a late publisher or a wait that
//     ran out makes lists longer, never wrong;
//   * nothing is read, published, counted or appended for queries >= nq: a 64-query unit without a live query is skipped
//     altogether (no image of it is staged -- this launch wrote none -- and its waves only stage and keep the barriers);
//     inside a live unit the dead queries' images are the zeros qtile_kernel wrote, and their lanes do nothing;
//   * nothing is published or appended for blocks >= nblocks: staging loads of the partial last row tile are CLAMPED to the
//     last block, their sub-tiles are computed and thrown away; padded rows of the last block get -FLT_MAX in
//     block_lane_top2, as in the narrow kernel.
#pragma once

constexpr int kWideBlocks = 8;     // blocks per row tile (256 rows)
constexpr int kWideQTiles = 8;     // 32-query tiles per column (256 queries)
constexpr int kWideKP = 4;         // pieces per k-step (64 k-values)
constexpr int kWideBufFrags = (kWideBlocks + kWideQTiles) * kWideKP * 64;   // 16-byte fragments per buffer (64 KiB)
constexpr size_t kWideLds = (size_t)2 * kWideBufFrags * 16;
constexpr int kWideQ = kWideQTiles * 32;         // queries per column
constexpr int kWideMinCus = 32;                  // row tiles 0..31 (all 64 classes) must fall into the first round
constexpr unsigned long long kWideWaitTicks = 20000ull;   // 200 us at the 100 MHz wall clock: a few tile times

// theta of unit `unit` (lane = query) from its class slots, folded into thetac, joined with what thetac holds; 0 = none
template <bool FRESH>
__device__ __forceinline__ u32 wide_theta(const ScanArgs& a, int unit, int lane, bool live)
{
    u32 m = 0;
    if (live) {
        u32* s = a.slots + (size_t)unit * kClasses * 64 + lane;
        u32 mn = 0xFFFFFFFFu;
#pragma unroll 16
        for (int c = 0; c < kClasses; ++c) mn = min(mn, FRESH ? load_memside_u32(s + c * 64) : load_agent_u32(s + c * 64));
        u32* t = a.thetac + unit * 64 + lane;
        if (mn != 0) atomicMax(t, mn);   // BEFORE anything is dropped against it
        m = max(mn, FRESH ? load_memside_u32(t) : load_agent_u32(t));
    }
    return m;
}

template <int METRIC>
__device__ __forceinline__ void wide_epilogue(const ScanArgs& a, const f32x16 (&acc)[4][2], int64_t rt, int unit, int bh, int lane)
{
    const int h = lane >> 5, b = lane & 31;
    const int64_t blk0 = rt * kWideBlocks + 4 * bh;
    if (blk0 >= a.nblocks) return;   // (wave-uniform) this half of the partial last row tile does not exist
    float f[4][2], s[4][2];
    float pm0 = -INFINITY, pm1 = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t blk = blk0 + i;
        f[i][0] = f[i][1] = s[i][0] = s[i][1] = -FLT_MAX;
        if (blk < a.nblocks) {
            f32x4 nrm[4];
            if (METRIC == HIPRAG_METRIC_L2) {
#pragma unroll
                for (int g = 0; g < 4; ++g) nrm[g] = *reinterpret_cast<const f32x4*>(a.norms + blk * kRowsPerBlock + 8 * g + 4 * h);
            }
            f[i][0] = block_lane_top2<METRIC>(acc[i][0], nrm, blk, h, a, s[i][0]);
            f[i][1] = block_lane_top2<METRIC>(acc[i][1], nrm, blk, h, a, s[i][1]);
            pm0 = fmaxf(pm0, f[i][0]);
            pm1 = fmaxf(pm1, f[i][1]);
        }
    }
    // (ii) publish: lane l ends up with the maximum of query 64 unit + l over the wave's live blocks
    const bool live = unit * 64 + lane < a.nq;
    {
        const float x0 = fmaxf(pm0, __shfl_xor(pm0, 32)), x1 = fmaxf(pm1, __shfl_xor(pm1, 32));
        const float v = lane < 32 ? x0 : x1;
        const int cls = (int)((2 * rt + bh) & (kClasses - 1));
        if (live) atomicMax(a.slots + ((size_t)unit * kClasses + cls) * 64 + lane, ord32(v));
    }
    // (iii) the bound
    u32 m = wide_theta<false>(a, unit, lane, live);
    if (__ballot(live && m == 0)) {
        const unsigned long long t0 = wall_clock64();
        for (int it = 0;; ++it) {
            if (live && m == 0) m = load_memside_u32(a.thetac + unit * 64 + lane);   // another workgroup may have formed it
            if (it && __ballot(live && m == 0)) m = max(m, wide_theta<true>(a, unit, lane, live && m == 0));
            if (!__ballot(live && m == 0)) break;
            if (wall_clock64() - t0 > kWideWaitTicks) break;   // go on without: everything of this tile is appended
            __builtin_amdgcn_s_sleep(127);
        }
    }
    // (iv) test and append
    const u32 th0 = (u32)__shfl((int)m, b), th1 = (u32)__shfl((int)m, 32 + b);
    const int q0 = unit * 64 + b, q1 = q0 + 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t blk = blk0 + i;
        if (blk < a.nblocks) {
            const bool p0 = q0 < a.nq && ord32(f[i][0]) >= th0;
            const bool p1 = q1 < a.nq && ord32(f[i][1]) >= th1;
            const u32 gid = (u32)(2 * blk + h);
            if (p0) append_direct(a, pack_key(f[i][0], gid), s[i][0], (u32)q0);
            if (p1) append_direct(a, pack_key(f[i][1], gid), s[i][1], (u32)q1);
        }
    }
}

template <int METRIC>
__global__ __launch_bounds__(512) void scan_wide_kernel(ScanArgs a)
{
    extern __shared__ float4 qs[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    __builtin_amdgcn_s_setprio(3);
    const int64_t gw = (int64_t)blockIdx.x * 8 + wave;
    if (a.stamps && lane == 0) a.stamps[2 * gw] = wall_clock64();
    if (a.gate && tid == 0) {   // once per workgroup, whether or not it owns a tile
        const unsigned long long was = __hip_atomic_fetch_add(a.started, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (was + 1 == a.target) __hip_atomic_fetch_max(a.gate, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int P2 = a.P / 2;               // pieces per block and per query tile (a multiple of 8)
    const int KS = P2 / kWideKP;          // k-steps per tile (>= 2)
    const int nunits = (a.nq + 63) / 64;  // 64-query units this launch has images of
    const int ncol = (a.nq + kWideQ - 1) / kWideQ;
    const int64_t nrt = (a.nblocks + kWideBlocks - 1) / kWideBlocks;
    const int bh = wave & 1, qp = wave >> 1;
    const bf16x8* xh = reinterpret_cast<const bf16x8*>(a.xh);
    const bf16x8* qimg = reinterpret_cast<const bf16x8*>(a.qtile);
    bf16x8* lds = reinterpret_cast<bf16x8*>(qs);

    // one k-step of one tile -> buffer `buf`: 64 pieces of 1 KiB, eight per wave (four of the rows, four of the queries)
    auto stage = [&](int64_t rt, int col, int ks, int buf) {
        bf16x8* dst = lds + buf * kWideBufFrags;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = wave + 8 * i;   // piece slot: [0, 32) rows (block c >> 2, piece c & 3), [32, 64) queries likewise
            const int pc = ks * kWideKP + (c & 3);
            if (i < 4) {
                const int64_t blk = min(rt * kWideBlocks + (c >> 2), a.nblocks - 1);   // clamped, never out of range
                __builtin_amdgcn_global_load_lds((const void*)(xh + ((size_t)blk * P2 + pc) * 64 + lane), (scan_lds_ptr_t)(dst + c * 64), 16, 0, 0);
            } else {
                const int qt = col * kWideQTiles + ((c - 32) >> 2);
                if ((qt >> 1) < nunits)   // a unit this launch wrote an image of
                    __builtin_amdgcn_global_load_lds((const void*)(qimg + ((size_t)qt * P2 + pc) * 64 + lane), (scan_lds_ptr_t)(dst + c * 64), 16, 0, 0);
            }
        }
    };

    f32x16 acc[4][2];
    int64_t rt = blockIdx.x;
    int col = 0, ks = 0, buf = 0;
    bool have = rt < nrt;
    if (have) stage(rt, 0, 0, 0);
    while (have) {
        int64_t nr = rt;
        int nc = col, nk = ks + 1;
        if (nk == KS) {
            nk = 0;
            if (++nc == ncol) { nc = 0; nr += gridDim.x; }
        }
        const bool more = nr < nrt;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of step s has landed
        __syncthreads();                                   // ... everyone's has, and everyone has left compute(s - 1)
        if (more) stage(nr, nc, nk, buf ^ 1);
        const int unit = col * (kWideQTiles / 2) + qp;
        if (unit < nunits) {
            if (ks == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) { acc[i][0][e] = 0.f; acc[i][1][e] = 0.f; }
            }
            const bf16x8* A = lds + buf * kWideBufFrags + (4 * bh) * kWideKP * 64 + lane;
            const bf16x8* B = lds + buf * kWideBufFrags + (kWideBlocks + 2 * qp) * kWideKP * 64 + lane;
#pragma unroll
            for (int pc = 0; pc < kWideKP; ++pc) {
                bf16x8 av[4], bv[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) av[i] = A[(i * kWideKP + pc) * 64];
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[j] = B[(j * kWideKP + pc) * 64];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[0], acc[i][0], 0, 0, 0);
                    acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[1], acc[i][1], 0, 0, 0);
                }
            }
            if (ks == KS - 1) {
                int lane_e = lane;
                asm volatile("" : "+v"(lane_e));   // keeps the epilogue's lane arithmetic out of the k-loop's live set
                wide_epilogue<METRIC>(a, acc, rt, unit, bh, lane_e);
            }
        }
        rt = nr; col = nc; ks = nk; have = more; buf ^= 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (a.stamps && lane == 0) a.stamps[2 * gw + 1] = wall_clock64();
}
