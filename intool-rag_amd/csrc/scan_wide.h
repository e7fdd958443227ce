// scan_wide.h -- the WIDE scan of the bf16 filter copy: a tiled MFMA kernel that answers 256 queries per read of the
// index instead of 64.  Included by dense_scan.h behind the narrow kernels, inside dense_index.hip's namespaces: it uses their
// ScanArgs, block_lane_top2, the list format and the class-slot / thetac protocol, and leaves exactly what they leave
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
// the epilogue of this one runs -- and the epilogue itself is cut into phases that run under the next tile's k-steps:
//     s_waitcnt vmcnt(0); barrier; wide_issue(phase); issue(s + 1); compute(s); wide_land(phase)
// A phase only ISSUES its memory operations, just ahead of the staging, and consumes them behind the step's last MFMA, where
// the next instruction is the next step's vmcnt(0) anyway; between a step's staging and its last MFMA stands no wait.
// The staging stands at the HEAD of the step on purpose: issued in slices among the step's MFMAs instead (four placements,
// DESIGN 3.4) every launch is slower, the more so the later the loads go out -- a step lasts about as long as a row piece
// takes to land, and with two buffers a piece has one step for it.
//
// Persistent workgroups, one per scan CU: workgroup i takes row tiles i, i + G, ...; per row tile all columns in turn (the
// re-read of the 512 KiB row tile by the second column can hit the Infinity Cache).  Every (row tile, column) pair is
// computed exactly once.
//
// Epilogue of a tile, per wave, no workgroup barrier, in two parts.
// At the end of the tile (wide_park), register work only:
//   (i)   block_lane_top2 per sub-tile (the L2 norms of the wave's four blocks are loaded here);
//   (ii)  the per-query maxima of the wave's 128 rows -> class slot cls = (2 row_tile + row_half) % 64 of its unit
//         (atomicMax, returns nothing).  The class follows the ROW TILE, so row tiles 0..31 give every class a publisher
//         whatever the grid; the host sends a launch here only when those all fall into the first round (G >= 32) and the
//         filter is on (more than 64 row tiles);
//   the 8 (first, second) pairs and (row tile, unit) are parked as the wave's PENDING tile.
// Under the next tile's k-steps, one phase per step (wide_issue / wide_land):
//   (iii) B0 .. B3: theta of the unit's 64 queries = min over the classes, 16 slot loads per phase;
//         T: theta folded into thetac BEFORE use by a returning atomicMax, whose answer is what thetac held (memory-side,
//         never stale): bound = the larger.  While a live query has no bound yet the wave waits, bounded, for the publishers
//         of the other workgroups -- five k-steps after its own publish, so hardly ever;
//   (iv)  A: first >= bound, counted per lane and query half: ONE atomicAdd(count, n) per half instead of one per entry;
//         behind the step's MFMAs the entries go to positions p, p + 1, ... (each guarded by kCandCap; count = entries
//         offered, as before).
// Six phases.  A tile of fewer k-steps (d_pad 128 / 256: 2 / 4), and the last tile of a wave, run the remaining phases in
// a row before the next tile is parked / after the loop (wide_drain): the same code, the compiler's waits doing the
// waiting.  A wave whose unit is dead in the tile being computed (a short last column) still takes a phase of its pending
// tile per k-step: liveness is the pending tile's.  Both row halves of a unit still recompute theta (the duplicate of
// DESIGN 3.2): its loads are hidden now, and a half that only read thetac would test against an older bound wherever the
// other half's fold is not ordered before its read -- in every drain.
// Invariants:
//   * a value is dropped only against a bound that is already folded into thetac (or was read from it): the FINAL thetac[q]
//     bounds everything that is not on q's list, and exactness never depends on timing -- a late publisher or a wait that
//     ran out makes lists longer, never wrong; a test that runs later only sees a higher bound: lists get shorter;
//   * nothing is read, published, counted or appended for queries >= nq: a 64-query unit without a live query is skipped
//     altogether (no image of it is staged -- this launch wrote none -- and its waves only stage and keep the barriers);
//     inside a live unit the dead queries' images are the zeros qtile_kernel wrote, and their lanes do nothing;
//   * nothing is published or appended for blocks >= nblocks: staging loads of the partial last row tile are CLAMPED to the
//     last block, their sub-tiles are computed and thrown away; padded rows of the last block get -FLT_MAX in
//     block_lane_top2, as in the narrow kernel.
#pragma once

// the tile (kWideBlocks, kWideQTiles, kWideKP), kWideBufFrags, kWideLds and kWideMinCus: dense_plan.h
constexpr int kWideQ = kWideQTiles * 32;         // queries per column
constexpr unsigned long long kWideWaitTicks = 20000ull;   // 200 us at the 100 MHz wall clock: a few tile times

constexpr int kWideBatch = 16;                          // class slots a phase loads
constexpr int kWidePhaseT = kClasses / kWideBatch + 1;   // phases 1 .. 4 = B0 .. B3, then T, then A (with S as its second half)
constexpr int kWidePhaseA = kWidePhaseT + 1;

// The pending tile of a wave: what wide_park left of the tile it finished last, and how far the phases have taken it.
// rt, unit and phase are wave-uniform.
struct WidePend {
    float f[4][2], s[4][2];   // first / second of the wave's 4 blocks x 2 query tiles (lane = (row half h, query b))
    u32 mn;                   // running minimum over the class slots (lane = query); behind phase T: the bound
    int64_t rt;
    int unit;
    int phase;                // the phase that runs next; 0 = nothing pending
};
// what a phase has in flight between its two halves.  It lives inside ONE k-step -- nothing that a load writes is carried
// round the loop, where the compiler would copy it into the carried register and wait for it first -- and every kind of
// round trip has registers of its own, each written at one place only: the compiler's counter bookkeeping joins the paths
// of wide_issue, and a register that a slot load of one path and an atomic of another both wrote would draw a wait in
// front of the second, in the middle of a k-step.
struct WideFlight {
    u32 ld[kWideBatch];   // B: 16 class slots (0xFFFFFFFF where nothing was loaded)
    u32 tc;               // T: thetac as the fold returned it
    u32 pos0, pos1;       // A: the list positions of the two query halves
};

// theta of unit `unit` (lane = query) from its class slots, all reads memory-side, folded into thetac; 0 = none.  Only the
// bounded wait of phase T calls it.
__device__ __forceinline__ u32 wide_theta_fresh(const ScanArgs& a, int unit, int lane, bool live)
{
    u32 m = 0;
    if (live) {
        u32* s = a.slots + (size_t)unit * kClasses * 64 + lane;
        u32 mn = 0xFFFFFFFFu;
#pragma unroll 16
        for (int c = 0; c < kClasses; ++c) mn = min(mn, load_memside_u32(s + c * 64));
        if (mn != 0) atomicMax(a.thetac + unit * 64 + lane, mn);   // BEFORE anything is dropped against it
        m = mn;
    }
    return m;
}

// the 8 parked pairs of the pending tile against the bound m (lane = query): which pass, per query half
__device__ __forceinline__ void wide_test(const ScanArgs& a, const WidePend& P, int bh, int lane, u32 m, bool (&p0)[4], bool (&p1)[4])
{
    const int b = lane & 31;
    const u32 th0 = (u32)__shfl((int)m, b), th1 = (u32)__shfl((int)m, 32 + b);
    const int q0 = P.unit * 64 + b, q1 = q0 + 32;
    const int64_t blk0 = P.rt * kWideBlocks + 4 * bh;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool there = blk0 + i < a.nblocks;
        p0[i] = there && q0 < a.nq && ord32(P.f[i][0]) >= th0;
        p1[i] = there && q1 < a.nq && ord32(P.f[i][1]) >= th1;
    }
}

// A phase of the pending tile has two halves inside one k-step of the NEXT tile.  wide_issue runs right behind the step's
// barrier and only ISSUES: 16 slot loads, or one returning atomic, or two.  It stands AHEAD of the step's staging: the
// memory pipe is empty there (everything has landed), whereas behind the staging the few loads of a phase queue behind
// the workgroup's 64 KiB and the wave sits in the issue instead of starting its MFMAs -- measured, both placements in one
// call: 1.333 against 1.365 ms per 512-query step.  wide_land runs behind the step's MFMAs and consumes what
// came back.  The compiler's wait for those values therefore stands behind the last MFMA, where the next
// instruction is the loop's own vmcnt(0) anyway: every round trip of the epilogue runs under the MFMAs of a step, and no
// wait stands between a step's staging and its last MFMA.  Called in a row (wide_drain) the two halves are the same code
// with the compiler's waits doing the waiting.  No barrier in either, and nothing of the tile the wave computes
// meanwhile: liveness is the pending tile's.
//   B0 .. B3  load 16 class slots | fold them into the running minimum
//   T         theta -> thetac by a RETURNING atomicMax: the fold that must precede every drop and a memory-side (never
//             stale) read of what the other workgroups have folded, in one round trip | bound = max(theta, what came
//             back); the bounded wait while a live query still has none
//   A (+ S)   test the 8 parked pairs; ONE atomicAdd per query half for all the blocks that passed | the list stores
// Invariants (those of the file header; this is where they are kept):
//   * a value is dropped only against a bound that T (or the wait) folded into thetac or read from it;
//   * queries >= nq: `live` masks every slot load, fold and wait, wide_test every count and store; blocks >= nblocks:
//     wide_test again (wide_park parks -FLT_MAX for them and publishes nothing);
//   * the stores test against the very bound the counts were taken with, so a lane stores exactly the entries it took
//     positions for; a later tile only sees a higher thetac: lists get shorter, never wrong.
__device__ __forceinline__ void wide_issue(const ScanArgs& a, const WidePend& P, WideFlight& X, int bh, int lane)
{
    const bool live = P.unit * 64 + lane < a.nq;
#pragma unroll
    for (int i = 0; i < kWideBatch; ++i) X.ld[i] = 0xFFFFFFFFu;
    X.tc = X.pos0 = X.pos1 = 0;
    if (P.phase < kWidePhaseT) {
        if (live) {
            const u32* sl = a.slots + ((size_t)P.unit * kClasses + (size_t)(P.phase - 1) * kWideBatch) * 64 + lane;
#pragma unroll
            for (int i = 0; i < kWideBatch; ++i) X.ld[i] = load_agent_u32(sl + i * 64);
        }
    }
    if (P.phase == kWidePhaseT) {
        // BEFORE anything is dropped against it; an empty class (mn = 0) folds nothing and still reads
        if (live) X.tc = __hip_atomic_fetch_max(a.thetac + P.unit * 64 + lane, P.mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (P.phase == kWidePhaseA) {
        bool p0[4], p1[4];
        wide_test(a, P, bh, lane, P.mn, p0, p1);
        const u32 n0 = (u32)p0[0] + (u32)p0[1] + (u32)p0[2] + (u32)p0[3], n1 = (u32)p1[0] + (u32)p1[1] + (u32)p1[2] + (u32)p1[3];
        const int q0 = P.unit * 64 + (lane & 31);
        // count = entries OFFERED, as append_direct counts them; the two atomics go out back to back: one round trip
        if (n0) X.pos0 = atomicAdd(a.count + q0, n0);
        if (n1) X.pos1 = atomicAdd(a.count + q0 + 32, n1);
    }
}

__device__ __forceinline__ void wide_land(const ScanArgs& a, WidePend& P, const WideFlight& X, int bh, int lane)
{
#pragma unroll
    for (int i = 0; i < kWideBatch; ++i) P.mn = min(P.mn, X.ld[i]);   // behind B only, the 0xFFFFFFFF of wide_issue
    if (P.phase == kWidePhaseT) {
        const bool live = P.unit * 64 + lane < a.nq;
        u32 m = live ? max(P.mn, X.tc) : 0u;
        if (__ballot(live && m == 0)) {   // no bound yet: the publishers of the other workgroups' first tiles are still out
            const unsigned long long t0 = wall_clock64();
            for (int it = 0;; ++it) {
                if (live && m == 0) m = load_memside_u32(a.thetac + P.unit * 64 + lane);   // another workgroup may have formed it
                if (it && __ballot(live && m == 0)) m = max(m, wide_theta_fresh(a, P.unit, lane, live && m == 0));
                if (!__ballot(live && m == 0)) break;
                if (wall_clock64() - t0 > kWideWaitTicks) break;   // go on without: everything of this tile is appended
                __builtin_amdgcn_s_sleep(127);
            }
        }
        P.mn = m;
    }
    if (P.phase == kWidePhaseA) {
        bool p0[4], p1[4];
        wide_test(a, P, bh, lane, P.mn, p0, p1);
        const int h = lane >> 5;
        const u32 q0 = (u32)(P.unit * 64 + (lane & 31)), q1 = q0 + 32;
        const int64_t blk0 = P.rt * kWideBlocks + 4 * bh;
        u32 pos0 = X.pos0, pos1 = X.pos1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u32 gid = (u32)(2 * (blk0 + i) + h);
            if (p0[i]) {
                if (pos0 < (u32)kCandCap) a.list[(size_t)q0 * kCandCap + pos0] = Cand{pack_key(P.f[i][0], gid), P.s[i][0], q0};
                ++pos0;
            }
            if (p1[i]) {
                if (pos1 < (u32)kCandCap) a.list[(size_t)q1 * kCandCap + pos1] = Cand{pack_key(P.f[i][1], gid), P.s[i][1], q1};
                ++pos1;
            }
        }
    }
    P.phase = P.phase == kWidePhaseA ? 0 : P.phase + 1;
}

// every remaining phase of the pending tile, at once
__device__ __forceinline__ void wide_drain(const ScanArgs& a, WidePend& P, int bh, int lane)
{
    while (P.phase) {
        WideFlight X;
        wide_issue(a, P, X, bh, lane);
        wide_land(a, P, X, bh, lane);
    }
}

// End of a tile: the register work only.  block_lane_top2 of the wave's 8 sub-tiles, the publish (an atomicMax that returns
// nothing), and the tile becomes the pending one; the wave goes straight on to the next tile's first k-step.
template <int METRIC>
__device__ __forceinline__ void wide_park(const ScanArgs& a, const f32x16 (&acc)[4][2], WidePend& P, int64_t rt, int unit, int bh, int lane)
{
    const int h = lane >> 5;
    const int64_t blk0 = rt * kWideBlocks + 4 * bh;
    if (blk0 >= a.nblocks) return;   // (wave-uniform) this half of the partial last row tile does not exist
    float pm0 = -INFINITY, pm1 = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t blk = blk0 + i;
        P.f[i][0] = P.f[i][1] = P.s[i][0] = P.s[i][1] = -FLT_MAX;
        if (blk < a.nblocks) {
            f32x4 nrm[4];
            if (METRIC == HIPRAG_METRIC_L2) {
#pragma unroll
                for (int g = 0; g < 4; ++g) nrm[g] = *reinterpret_cast<const f32x4*>(a.norms + blk * kRowsPerBlock + 8 * g + 4 * h);
            }
            P.f[i][0] = block_lane_top2<METRIC>(acc[i][0], nrm, blk, h, a, P.s[i][0]);
            P.f[i][1] = block_lane_top2<METRIC>(acc[i][1], nrm, blk, h, a, P.s[i][1]);
            pm0 = fmaxf(pm0, P.f[i][0]);
            pm1 = fmaxf(pm1, P.f[i][1]);
        }
    }
    // publish: lane l ends up with the maximum of query 64 unit + l over the wave's live blocks
    {
        const float x0 = fmaxf(pm0, __shfl_xor(pm0, 32)), x1 = fmaxf(pm1, __shfl_xor(pm1, 32));
        const float v = lane < 32 ? x0 : x1;
        const int cls = (int)((2 * rt + bh) & (kClasses - 1));
        if (unit * 64 + lane < a.nq) atomicMax(a.slots + ((size_t)unit * kClasses + cls) * 64 + lane, ord32(v));
    }
    P.mn = 0xFFFFFFFFu;
    P.rt = rt;
    P.unit = unit;
    P.phase = 1;
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
    WidePend P;
    P.phase = 0;
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
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));   // keeps the epilogue's lane arithmetic out of the k-loop's live set
        const bool pend = P.phase != 0;    // a phase of the tile before this one: issued here, landed behind the MFMAs
        WideFlight X;
        if (pend) wide_issue(a, P, X, bh, lane_e);   // AHEAD of the staging: see wide_issue
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
        }
        __builtin_amdgcn_sched_barrier(0);   // nothing of wide_land, its wait least of all, moves up among the MFMAs
        if (pend) wide_land(a, P, X, bh, lane_e);
        if (unit < nunits && ks == KS - 1) {
            wide_drain(a, P, bh, lane_e);   // fewer k-steps per tile than phases: the rest of them, now
            wide_park<METRIC>(a, acc, P, rt, unit, bh, lane_e);
        }
        rt = nr; col = nc; ks = nk; have = more; buf ^= 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wide_drain(a, P, bh, lane);   // the last tile of the wave
    if (a.stamps && lane == 0) a.stamps[2 * gw + 1] = wall_clock64();
}
