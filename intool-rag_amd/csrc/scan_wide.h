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
// Tile: 256 rows (8 blocks) x 256 queries (8 query tiles of 32), K in steps of 32 (2 pieces).  Both operands are stored as
// 1 KiB lane-linear fragments of v_mfma_f32_32x32x16_bf16 already -- block B, piece p of the filter copy; the images
// qtile_kernel writes -- so staging is global_load_lds of whole pieces and a fragment read is one lane-linear
// ds_read_b128: no swizzle.  A k-step's 16 row pieces and its 16 query pieces are 16 KiB each, and the 128 KiB of LDS, ONE
// object, are eight such slots: a ROW RING of 5 and a QUERY RING of 3, indexed by the flat step counter mod 5 and mod 3.
// A wave owns 4 blocks x 2 query tiles = 8 accumulators (128 registers): wave w -> blocks 4 (w & 1) + 0..3, query tiles
// 2 (w >> 1) + 0..1, i.e. ONE 64-query unit (the unit of the class slots and of the finish).  Per piece 4 + 2 fragment
// reads feed 8 MFMAs.  `first` / `second` are the same bits as the narrow kernel's: same MFMA, A = rows, B = queries, one
// accumulator per 32 x 32 sub-tile, pieces 0 .. P2 - 1 in that order, then block_lane_top2.
//
// Why two rings of unequal length: the query images of a launch are 1 MiB, shared by every workgroup and read again for
// every row tile -- they come from the XCD's L2; the row pieces come from HBM or the Infinity Cache, and a k-step of 64 in
// two symmetric buffers gave them one step (0.85 us of MFMAs) to land where they take 1-2 us under this load (DESIGN
// 3.4).  A third 64 KiB buffer does not fit, a fifth quarter-size row slot does.
//
// Schedule.  The step sequence of a workgroup is flat over (pair of its walk, k-step) -- a pair is a (row tile, column),
// below: Persistent workgroups -- with d_pad / 32 = 4, 8, 12, ... steps per tile, so the rings wrap at every phase against
// the tile boundaries, and the staging runs on into the next tile, whichever row tile and column that is, while the
// epilogue of this one runs.  Step s, every wave:
//     W1: s_waitcnt vmcnt(6); raw s_barrier; [wide_issue(phase)]; issue queries(s + 2); issue rows(s + 4);
//     the books of step s + 1; compute(s) from row slot s % 5 and query slot s % 3; [W2: wide_land(phase)]
// A step finds what its staging and its reads need ready behind the barrier: the two M0 values are one addition each, the
// four addresses and the two fragment addresses stand in registers.  The books -- the two staging cursors a step on (and
// the walk's division where one enters a pair), the ring slots, the fragment addresses of the next step, in a tile's last
// step the walk's next pair -- are kept behind the staging and ahead of the fragment reads, by live and dead waves
// alike (the k-loop says what the other places measured).
// The tile loop is written out as first step | KS - 2 middle steps | last step (KS = d_pad / 32, a multiple of 4): the
// first step's eight piece-0 MFMAs take an inline 0 as C (no accumulator is cleared: that was 128 v_mov per wave and
// tile, ahead of the MFMAs), the last step parks the tile, and the middle steps come in pairs (odd, even): phases run in
// the EVEN steps of a tile, which are the even steps of the flat sequence, and the odd steps carry no phase code.  The
// flat sequence itself does not change: the staging cursors, the rings and the phases run on across tiles.
// Every wave issues exactly 2 + 2 LDS-DMA instructions per step, queries first, with no branch around any of them: row
// blocks past the index are clamped to the last block, a query tile of a unit without an image to the last tile that has
// one, and past the end of the workgroup's sequence the cursors run on into slots nobody reads any more.  The prologue
// issues, in the order steps -4 .. -1 would have, r0 | r1 | q0 r2 | q1 r3.  A workgroup without a tile issues nothing.
// Hazards (vector-memory LOADS of one wave return in order; "younger" = issued later):
//   loads in flight at the top of step s, oldest first:  ... q(s) r(s+2) | q(s+1) r(s+3)      (issued in steps s-2 | s-1)
//   W1  vmcnt(6): the six youngest are r(s+2), q(s+1), r(s+3) -> q(s), and with it r(s), r(s+1) and all before, have landed
//       -- this wave's share; the barrier behind it makes that everyone's.
//   write-after-read: row slot (s+4) % 5 = (s-1) % 5 and query slot (s+2) % 3 = (s-1) % 3 were last read by
//       compute(s-1); a wave's fragment reads are complete before its last MFMAs issue, hence before it reaches the
//       barrier of step s, and the loads of step s are issued behind that barrier.
//   W2  a phase's round trips (16 slot loads, or one returning atomic, or two; inline asm, the compiler counts none of
//       them) are issued AHEAD of the step's staging and waited for behind its last MFMA with vmcnt(4): the four
//       staging loads are the only younger loads.  Everything older has landed then, too: r(s+3) a step early -- a
//       phase costs its step one step of the ring's lead, six steps per fold tile, two per no-fold tile (an idle phase
//       issues nothing and waits for nothing).
//   stores (the list stores of phase A behind W2, the publish of wide_park, the stamps) are never counted: a store's
//       acknowledgement may overtake an older load, so an outstanding store can only make W1 or W2 wait longer.
//   the loop's exit waits with vmcnt(0).
//   ordinary code, the compiler's own waits (which do not know the asm loads and therefore only wait longer): wide_drain
//       (every phase with vmcnt(0), right whatever of the ring is in flight), the bounded wait of phase T,
//       wide_theta_fresh, wide_park's norm loads (L2).  They drain the ring; once per tile at the most.
// No wait on vmcnt stands between the barrier and the last MFMA of a step, and none with count 0 in the k-loop outside
// the paths just named (read in the disassembly of both instantiations).  __syncthreads() is not used: its fence puts
// vmcnt(0) in front of the barrier.
// The fragment reads of a step are ordered by hand as well (the k-loop says how): left to the compiler every pair of
// MFMAs waits with lgkmcnt(0) for two reads issued just ahead of it, five exposed LDS round trips per 16 MFMAs.
// The staging cursors are running pointers; only a new tile computes them afresh.  With a k-step of 16 MFMAs per wave the
// scalar work of a step is no longer small beside it: recomputing the four addresses from (row tile, column, k-step)
// in every step cost 9 % of the launch.  A cursor's own state is (pair number, k-step): a step counts the
// k-step up and compares, and the walk's arithmetic (one division) runs where a cursor enters a pair, once per tile.
// The computing cursor is the tile loop itself plus the pair number; its row tile is asked of the walk again in the
// tile's last step and not carried (the k-loop has no SGPR to spare: wave-uniform constants that only a per-tile path
// uses are made opaque there -- `fresh` -- so that what the compiler derives from them is not held across the loop).
// The clocks of the phases: a phase runs in every SECOND step (kWidePhaseEvery), so the six phases take 12 steps of 32
// k-values where they took 6 of 64 -- the test runs as late as before and sees the same bound; one per step measured
// 1 % slower and no shorter lists.
//
// Persistent workgroups, one per scan CU, each on its WALK (wide_walk / wide_walk_pair, dense_plan.h: one definition for
// this kernel, the host and the tests).  The floor(row tiles / G) full rounds: workgroup i takes row tiles i, i + G, ...,
// per row tile all columns in turn (the re-read of the 512 KiB row tile by the second column can hit the Infinity Cache).
// The row tiles left over, fewer than G: their (row tile, column) pairs are numbered row tile first and dealt round the
// workgroups, i, i + G, ..., so the tail lasts ceil(left-over pairs / G) pair-times on all CUs instead of one per column
// on some of them -- the idle CUs could run nothing else: the next scan is behind this one in stream order and needs a
// CU's whole LDS.  A workgroup's tail pairs are tiles of different row tiles, and the columns of a tail row tile run on
// neighbouring workgroups at once.  Fewer row tiles than workgroups (a forced launch): workgroup i < row tiles takes row
// tile i and all its columns, nothing is spread.  Every (row tile, column) pair is computed exactly once, and all three
// cursors of a workgroup go through the same sequence of pairs.
//
// Epilogue of a tile, per wave, no workgroup barrier, in two parts.
// At the end of the tile (wide_park), register work only:
//   (i)   block_lane_top2 per sub-tile (the L2 norms of the wave's four blocks are loaded here);
//   (ii)  the per-query maxima of the wave's 128 rows -> class slot cls = (2 row_tile + row_half) % 64 of its unit
//         (atomicMax, returns nothing).  The class follows the ROW TILE, so row tiles 0..31 give every class a publisher
//         whatever the grid; the host sends a launch here only when those all fall into the first round (G >= 32) and the
//         filter is on (more than 64 row tiles);
//   the 8 (first, second) pairs and (row tile, unit) are parked as the wave's PENDING tile.
// Under the next tile's k-steps, one phase per second step (wide_issue / wide_land):
//   (iii) B0 .. B3, on a FOLD tile: theta of the unit's 64 queries = min over the classes, 16 slot loads per phase; on a
//         no-fold tile four idle phases in their place (the fold schedule, below);
//         T: theta folded into thetac BEFORE use by a returning atomicMax, whose answer is what thetac held (memory-side,
//         never stale): bound = the larger; on a no-fold tile theta is 0, "none": the atomic folds nothing and only
//         reads.  While a live query has no bound yet the wave waits, bounded, for the publishers of the other
//         workgroups -- ten k-steps after its own publish, so hardly ever -- and recomputes theta itself
//         (wide_theta_fresh), fold tile or not;
//   (iv)  A: first >= bound, counted per lane and query half: ONE atomicAdd(count, n) per half instead of one per entry;
//         behind the step's MFMAs the entries go to positions p, p + 1, ... (each guarded by kCandCap; count = entries
//         offered, as before).
// Six phases, every tile: the idle phases keep T and A of a no-fold tile in the k-steps they have on a fold tile (8 and
// 10; in 0 and 2 they test against an older bound: longer lists, no shorter launches).  A tile of fewer than 12 k-steps (d_pad 128 / 256: 4 / 8), and the last tile of a wave, run the remaining
// phases in a row before the next tile is parked / after the loop (wide_drain): the same code, each phase waiting with
// vmcnt(0).  A wave whose unit is dead in the tile being computed (a short last column) still takes a phase of its
// pending tile per second k-step: liveness is the pending tile's.
// The fold schedule (wide_fold, dense_plan.h: one definition for this kernel, the host and the tests).  Recomputing theta
// is 64 agent-scope loads per wave and tile, a third of the vector-memory instructions a CU issues, for a bound that
// hardly moves after a launch's first tiles.  So wide_park asks wide_fold with the pair number of the tile it parks: the
// first kWideFoldFirst pairs of a walk are fold tiles (the bound forms there; an index of few pairs per workgroup folds
// in every tile), and from there one pair in N = ScanArgs::fold_every (HIPRAG_WIDE_FOLD_EVERY, default kWideFoldEvery; 1
// = every tile), at an offset that counts through (workgroup, row half) and shifts with the query pair, so that in
// every pair-time 2 G / N waves refresh thetac of every unit.  A no-fold tile tests against what thetac holds: every
// fold of every workgroup up to T's round trip, at most a little older than its own theta would be -- by about one visit
// of the unit's column.  The final thetac, which the finish ranks against, is what the waves fold behind their LAST
// tiles: a wave whose last tile is a no-fold tile folds once more at the exit (the kernel's end says why).
// Invariants:
//   * a value is dropped only against a bound that is already folded into thetac (or was read from it): the FINAL thetac[q]
//     bounds everything that is not on q's list, and exactness never depends on timing -- a late publisher, a wait that
//     ran out or a tile that does not fold makes lists longer, never wrong; a test that runs later only sees a higher
//     bound: lists get shorter;
//   * nothing is read, published, counted or appended for queries >= nq: a 64-query unit without a live query is skipped
//     altogether (no image of it is staged -- this launch wrote none -- and its waves only stage and keep the barriers);
//     inside a live unit the dead queries' images are the zeros qtile_kernel wrote, and their lanes do nothing;
//   * nothing is published or appended for blocks >= nblocks: staging loads of the partial last row tile are CLAMPED to the
//     last block, their sub-tiles are computed and thrown away; padded rows of the last block get -FLT_MAX in
//     block_lane_top2, as in the narrow kernel.
#pragma once

// the tile (kWideBlocks, kWideQTiles, kWideKP), the rings (kWideBufFrags, kWideRowRing, kWideQRing), kWideLds and kWideMinCus: dense_plan.h
constexpr int kWideQ = kWideQTiles * 32;         // queries per column
constexpr unsigned long long kWideWaitTicks = 20000ull;   // 200 us at the 100 MHz wall clock: a few tile times

constexpr int kWideBatch = 16;                          // class slots a phase loads
constexpr int kWidePhaseT = kClasses / kWideBatch + 1;   // phases 1 .. 4 = B0 .. B3, then T, then A (with S as its second half)
constexpr int kWidePhaseA = kWidePhaseT + 1;
// A no-fold tile (wide_fold) has no B0 .. B3; in their place it passes through as many IDLE phases, I0 .. I3, which issue
// and land nothing, so that its T and A run in the k-steps they run in on a fold tile -- and the k-loop asks nothing new
// of a step: a hold state tested beside `pend` cost every step 14 scalar instructions ahead of its staging
constexpr int kWidePhaseIdle = kWidePhaseA + 1;
constexpr int kWidePhaseIdleLast = kWidePhaseIdle + kClasses / kWideBatch - 1;
constexpr int kWidePhaseEvery = 2;   // a phase runs in every second k-step (a power of two): the clocks of the phases, below
// T and A of a no-fold tile run in the k-steps they have on a fold tile (8 and 10), not in 0 and 2: the early placement
// tests against an older bound and measured longer lists and no shorter launches
constexpr bool kWideFoldLate = true;

// a fragment read and the wait for it, by hand (the k-loop says why)
#define WIDE_DSR(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory")
#define WIDE_LGKM1(n, x) asm volatile("s_waitcnt lgkmcnt(%[c])" : "+v"(x) : [c] "n"(n) : "memory")
#define WIDE_LGKM3(n, x, y, z) asm volatile("s_waitcnt lgkmcnt(%[c])" : "+v"(x), "+v"(y), "+v"(z) : [c] "n"(n) : "memory")

// raw barrier: __syncthreads() would put `s_waitcnt vmcnt(0) lgkmcnt(0)` in front of it and drain the ring
#define WIDE_BAR()                                \
    do {                                          \
        __builtin_amdgcn_sched_barrier(0);        \
        __builtin_amdgcn_s_barrier();             \
        __builtin_amdgcn_sched_barrier(0);        \
    } while (0)

// The pending tile of a wave: what wide_park left of the tile it finished last, and how far the phases have taken it.
// rt, unit and phase are wave-uniform.
struct WidePend {
    float f[4][2], s[4][2];   // first / second of the wave's 4 blocks x 2 query tiles (lane = (row half h, query b))
    u32 mn;                   // running minimum over the class slots (lane = query); behind phase T: the bound
    uint32_t rt;              // (32 bits: a row tile number is below 2^28, and the k-loop has no SGPR to spare)
    int unit;
    int phase;                // the phase that runs next; 0 = nothing pending
};
// what a phase has in flight between its two halves.  It lives inside ONE k-step.  Every value is the output of an inline-asm
// memory instruction and goes through the one hand-written wait of its phase before it is used (wide_land): the compiler
// knows nothing of these round trips and places no wait of its own for them.
struct WideFlight {
    u32 ld[kWideBatch];   // B: 16 class slots
    u32 tc;               // T: thetac as the fold returned it
    u32 pos0, pos1;       // A: the list positions of the two query halves
};

// the 16 agent-scope slot loads of a phase B (global_load_dword ... sc1, as __hip_atomic_load at agent scope compiles)
template <int I>
__device__ __forceinline__ void wide_slot_loads(WideFlight& X, const u32* sl)
{
    asm volatile("global_load_dword %0, %1, off offset:%2 sc1" : "=v"(X.ld[I]) : "v"(sl), "n"(I * 256) : "memory");
    if constexpr (I + 1 < kWideBatch) wide_slot_loads<I + 1>(X, sl);
}
// returning agent-scope atomics (sc0 = return the value before the operation), relaxed
__device__ __forceinline__ void wide_fetch_max(u32& out, u32* p, u32 v)
{
    asm volatile("global_atomic_umax %0, %1, %2, off sc0" : "=v"(out) : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void wide_fetch_add(u32& out, u32* p, u32 v)
{
    asm volatile("global_atomic_add %0, %1, %2, off sc0" : "=v"(out) : "v"(p), "v"(v) : "memory");
}
// The wait of a phase's round trips: `s_waitcnt vmcnt(YOUNGER)`, YOUNGER = the vector-memory LOADS this wave has issued
// behind them.  The values are tied into it so that no use moves above it.
#define WIDE_WAIT1(younger, a) asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(a) : [n] "n"(younger) : "memory")
#define WIDE_WAIT2(younger, a, b) asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(a), "+v"(b) : [n] "n"(younger) : "memory")
#define WIDE_WAIT8(younger, r, o) \
    asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(r[o]), "+v"(r[o + 1]), "+v"(r[o + 2]), "+v"(r[o + 3]), "+v"(r[o + 4]), "+v"(r[o + 5]), "+v"(r[o + 6]), "+v"(r[o + 7]) : [n] "n"(younger) : "memory")

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
    const int64_t blk0 = (int64_t)P.rt * kWideBlocks + 4 * bh;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool there = blk0 + i < a.nblocks;
        p0[i] = there && q0 < a.nq && ord32(P.f[i][0]) >= th0;
        p1[i] = there && q1 < a.nq && ord32(P.f[i][1]) >= th1;
    }
}

// A phase of the pending tile has two halves inside one k-step of the NEXT tile.  wide_issue runs right behind the step's
// barrier and only ISSUES: 16 slot loads, or one returning atomic, or two.  It stands AHEAD of the step's staging, where
// it stood when a step's staging was 64 KiB at once and the few loads of a phase queued behind it (1.333 against 1.365 ms
// per 512-query step) -- and where the wait for it needs to count no more than the step's own four staging
// loads.  wide_land runs behind the step's MFMAs: one hand-written s_waitcnt vmcnt(YOUNGER) into which the phase's
// values are tied, then it consumes them.  Every round trip of the epilogue runs under the MFMAs of a step, and no wait
// stands between a step's staging and its last MFMA.  Called in a row (wide_drain) the two halves are the same code with
// YOUNGER = 0.  No barrier in either, and nothing of the tile the wave computes meanwhile: liveness is the pending tile's.
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
    // every lane issues, under the wave-uniform phase alone: a dead lane (query >= nq) goes to the unit's query 0, which is
    // live -- it loads that query's slots and folds 0 into its thetac, which changes nothing -- and its answer is dropped
    const bool live = P.unit * 64 + lane < a.nq;
    const int ql = P.unit * 64 + (live ? lane : 0);
    if (P.phase < kWidePhaseT) {
        wide_slot_loads<0>(X, a.slots + ((size_t)P.unit * kClasses + (size_t)(P.phase - 1) * kWideBatch) * 64 + (ql & 63));
    }
    if (P.phase == kWidePhaseT) {
        // BEFORE anything is dropped against it; an empty class (mn = 0) folds nothing and still reads
        wide_fetch_max(X.tc, a.thetac + ql, live ? P.mn : 0u);
    }
    if (P.phase == kWidePhaseA) {
        bool p0[4], p1[4];
        wide_test(a, P, bh, lane, P.mn, p0, p1);
        const u32 n0 = (u32)p0[0] + (u32)p0[1] + (u32)p0[2] + (u32)p0[3], n1 = (u32)p1[0] + (u32)p1[1] + (u32)p1[2] + (u32)p1[3];
        const int q0 = P.unit * 64 + (lane & 31);
        // count = entries OFFERED, as append_direct counts them; the two atomics go out back to back: one round trip.
        // Only lanes with entries take part (an atomic per lane of every tile would be traffic for nothing), so whether
        // an instruction goes out at all depends on the data: no wait may count these, and none does (wide_land)
        X.pos0 = X.pos1 = 0;
        if (n0) wide_fetch_add(X.pos0, a.count + q0, n0);
        if (n1) wide_fetch_add(X.pos1, a.count + q0 + 32, n1);
    }
}

// YOUNGER: the loads the wave has issued behind the phase's own operations -- the 4 staging loads of the step inside the
// k-loop, none in a drain.  Everything OLDER than the phase (the ring) has landed behind this wait as well: a phase costs
// its step the ring's lead.  The list stores of phase A stand behind the wait; a store's acknowledgement may overtake an
// older load, so stores are never counted: outstanding they only make the next wait stricter.
template <bool DRAIN>
__device__ __forceinline__ void wide_land(const ScanArgs& a, WidePend& P, WideFlight& X, int bh, int lane)
{
    constexpr int YOUNGER = DRAIN ? 0 : 4;
    const bool live = P.unit * 64 + lane < a.nq;
    if (P.phase < kWidePhaseT) {
        WIDE_WAIT8(YOUNGER, X.ld, 0);
        WIDE_WAIT8(YOUNGER, X.ld, 8);
        if (live) {
#pragma unroll
            for (int i = 0; i < kWideBatch; ++i) P.mn = min(P.mn, X.ld[i]);
        }
    }
    if (P.phase == kWidePhaseT) {
        WIDE_WAIT1(YOUNGER, X.tc);
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
        WIDE_WAIT2(YOUNGER, X.pos0, X.pos1);
        bool p0[4], p1[4];
        wide_test(a, P, bh, lane, P.mn, p0, p1);
        const int h = lane >> 5;
        const u32 q0 = (u32)(P.unit * 64 + (lane & 31)), q1 = q0 + 32;
        const int64_t blk0 = (int64_t)P.rt * kWideBlocks + 4 * bh;
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
    P.phase = P.phase == kWidePhaseA ? 0 : P.phase == kWidePhaseIdleLast ? kWidePhaseT : P.phase + 1;
}

// every remaining phase of the pending tile, at once: each phase waits with vmcnt(0), which is right whatever of the ring
// is in flight -- and drains it.  Once per tile at the most (a tile of fewer k-steps than the phases need, the last tile)
__device__ __forceinline__ void wide_drain(const ScanArgs& a, WidePend& P, int bh, int lane)
{
    if (P.phase >= kWidePhaseIdle) P.phase = kWidePhaseT;   // nothing to wait for in a drain
    while (P.phase) {
        WideFlight X;
        wide_issue(a, P, X, bh, lane);
        wide_land<true>(a, P, X, bh, lane);
    }
}

// End of a tile: the register work only.  block_lane_top2 of the wave's 8 sub-tiles, the publish (an atomicMax that returns
// nothing), and the tile becomes the pending one; the wave goes straight on to the next tile's first k-step.
template <int METRIC>
__device__ __forceinline__ void wide_park(const ScanArgs& a, const f32x16 (&acc)[4][2], WidePend& P, int64_t rt, int unit, bool fold, int bh, int lane)
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
        if (unit * 64 + lane < a.nq) atomicMax(a.slots + (u32)((unit * kClasses + cls) * 64 + lane), ord32(v));   // (a 32-bit index: units x 4096 slots)
    }
    // a fold tile starts the running minimum and goes through B0 .. B3; a no-fold tile starts at T with theta = 0, "none":
    // T folds nothing, reads thetac, and the bound is what came back
    P.mn = fold ? 0xFFFFFFFFu : 0u;
    P.rt = (uint32_t)rt;
    P.unit = unit;
    P.phase = fold ? 1 : kWideFoldLate ? kWidePhaseIdle : kWidePhaseT;
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
    const int KS = P2 / kWideKP;          // k-steps per tile (a multiple of 4)
    const int nunits = (a.nq + 63) / 64;  // 64-query units this launch has images of
    const int ncol = (a.nq + kWideQ - 1) / kWideQ;
    const int64_t nrt = (a.nblocks + kWideBlocks - 1) / kWideBlocks;
    const int bh = wave & 1, qp = wave >> 1;
    const bf16x8* xh = reinterpret_cast<const bf16x8*>(a.xh);
    const bf16x8* qimg = reinterpret_cast<const bf16x8*>(a.qtile);
    bf16x8* lds = reinterpret_cast<bf16x8*>(qs);

    // The flat step sequence of this workgroup, (pair of the walk, k-step), walked by three cursors: the step being
    // computed, the query pieces two steps ahead of it and the row pieces four steps ahead.  A cursor is (pair number,
    // k-step) and nothing else: which (row tile, column) a pair is, wide_walk_pair says when the cursor enters it, once per
    // KS steps.  The two staging cursors run on past the end of the sequence (pairs >= npairs are a row tile past the
    // index, their addresses are clamped), so every step issues the same four loads.
    const WideWalk W = wide_walk((uint32_t)nrt, (uint32_t)ncol, gridDim.x, blockIdx.x);
    struct Cursor { uint32_t p; int ks; };
    auto advance = [&](Cursor& c) -> bool {   // true: the cursor has entered another pair
        if (++c.ks < KS) return false;
        c.ks = 0;
        ++c.p;
        return true;
    };
    // A wave's share of a k-step's 16 row pieces / 16 query pieces (1 KiB each): pieces wave and wave + 8 of the slot, piece
    // c = (block or query tile c >> 1, piece c & 1 of the step).  A staging cursor keeps the fragment offset of its first
    // piece and the distance to its second; a k-step on is kWideKP pieces on, and only a new tile computes them afresh.
    struct Stream { const bf16x8* p; u32 d; };   // d in BYTES, never negative: the second piece is the later one, or the same when clamped
    auto row_stream = [&](uint32_t rt) {
        // clamped, never out of range; in 32 bits, unsigned: a block number is below 2^31 (a group id is 32 bits).  The row
        // tile of a pair past the walk is kWideNoTile = 0xFFFFFFFF: times 8 that WRAPS, to 0xFFFFFFF8, and the 0 .. 3 + 4
        // added to it reach 0xFFFFFFFF at the most and do not wrap again, so it is still above every block: clamped to the last
        const uint32_t last = (uint32_t)(a.nblocks - 1);
        const uint32_t b0 = min(rt * (uint32_t)kWideBlocks + (uint32_t)(wave >> 1), last);
        const uint32_t b1 = min(rt * (uint32_t)kWideBlocks + (uint32_t)(wave >> 1) + 4u, last);
        return Stream{xh + ((size_t)b0 * P2 + (wave & 1)) * 64, (b1 - b0) * (u32)P2 * 1024u};
    };
    auto query_stream = [&](int col) {
        const int t0 = min(col * kWideQTiles + (wave >> 1), 2 * nunits - 1);   // clamped to the last tile this launch wrote an image of
        const int t1 = min(col * kWideQTiles + (wave >> 1) + 4, 2 * nunits - 1);
        return Stream{qimg + ((size_t)t0 * P2 + (wave & 1)) * 64, (u32)(t1 - t0) * (u32)P2 * 1024u};
    };
    // LDS byte addresses: the wave's first piece of ring slot `slot` (the M0 of its staging), its second piece 8 KiB on
    constexpr u32 kSlotBytes = (u32)kWideBufFrags * 16u;
    const u32 ldsw = (u32)(uintptr_t)(scan_lds_ptr_t)(lds + wave * 64);
    auto stage = [&](const Stream& S, u32 dst) {
        __builtin_amdgcn_global_load_lds((const void*)(S.p + lane), (scan_lds_ptr_t)(uintptr_t)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const void*)(reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(S.p) + S.d) + lane),
                                         (scan_lds_ptr_t)(uintptr_t)(dst + 8u * 1024u), 16, 0, 0);
    };

    // The wave's key of the fold schedule (wide_fold_key: its offset and N - 1), wave-uniform but kept in a VGPR: the k-loop
    // has no SGPR to spare (every one it is given comes back as a spill inside the loop), 11 VGPRs are free,
    // and wide_park reads it once per tile.
    u32 fold_key = wide_fold_key(blockIdx.x, (uint32_t)wave, (uint32_t)a.fold_every);
    asm volatile("" : "+v"(fold_key));
    f32x16 acc[4][2];
    WidePend P;
    P.phase = 0;
    if (W.npairs) {   // a workgroup without a tile issues nothing
        // the pair being computed: pair 0 of every walk is (row tile w, column 0)
        uint32_t cp = 0;
        int unit = qp;   // the wave's 64-query unit of the pair's column
        Cursor rc{0, 0}, qc{0, 0};
        Stream R = row_stream(blockIdx.x), Q = query_stream(0);
        auto next_rows = [&]() {
            R.p += kWideKP * 64;
            if (advance(rc)) R = row_stream(wide_walk_pair(W, rc.p).rt);
        };
        auto next_queries = [&]() {
            Q.p += kWideKP * 64;
            if (advance(qc)) Q = query_stream((int)wide_walk_pair(W, qc.p).col);
        };
        // prologue, in the order the steps -4 .. -1 would have issued them: r0 | r1 | q0 r2 | q1 r3
        stage(R, ldsw + 0 * kSlotBytes); next_rows();
        stage(R, ldsw + 1 * kSlotBytes); next_rows();
        stage(Q, ldsw + (kWideRowRing + 0) * kSlotBytes); next_queries();
        stage(R, ldsw + 2 * kSlotBytes); next_rows();
        stage(Q, ldsw + (kWideRowRing + 1) * kSlotBytes); next_queries();
        stage(R, ldsw + 3 * kSlotBytes); next_rows();
        // What a step needs at its head is computed in the step BEFORE it, behind that step's staging (the books, below),
        // and stands ready behind the barrier: Q and R (the streams of its two stagings), rst and qst (the byte offsets of
        // the ring slots it stages into; M0 is one addition away), A and B (the fragment addresses of its reads).  A step
        // stages into the slot the step before it computed from and computes from the slot behind that: one offset per
        // ring is all the state there is, as before.
        constexpr u32 kRowEnd = (u32)kWideRowRing * kSlotBytes, kQEnd = (u32)(kWideRowRing + kWideQRing) * kSlotBytes;
        auto row_next = [](u32 o) { return o + kSlotBytes == kRowEnd ? 0u : o + kSlotBytes; };
        auto q_next = [](u32 o) { return o + kSlotBytes == kQEnd ? kRowEnd : o + kSlotBytes; };
        u32 rst = kRowEnd - kSlotBytes, qst = kQEnd - kSlotBytes;   // step 0 stages into the last slot of either ring ...
        const unsigned A0 = (unsigned)(uintptr_t)(scan_lds_ptr_t)(lds + (4 * bh) * kWideKP * 64 + lane);
        const unsigned B0 = (unsigned)(uintptr_t)(scan_lds_ptr_t)(lds + (2 * qp) * kWideKP * 64 + lane);
        unsigned A = A0 + row_next(rst), B = B0 + q_next(qst);      // ... and computes from the first
        // a wave-uniform constant made opaque where a per-tile path uses it: what the compiler derives from it (4 bh as 64
        // bits, KS / 2 - 1, ...) is then computed there, in an instruction or two, and not carried through the k-loop in
        // an SGPR the loop does not have (it comes back as a spill read inside the loop)
        auto fresh = [](int v) { asm volatile("" : "+s"(v)); return v; };
        // One k-step.  FIRST / LAST: the first / last step of a tile, written out (the tile loop, below).  PHASE: a step in
        // which a phase of the pending tile runs -- the even k-steps (kWidePhaseEvery), the step counter of a tile being
        // even at its first step whatever the tile, since KS is a multiple of 4.
        static_assert(kWidePhaseEvery == 2, "the tile loop below writes the phases' clock out: every second step");
        static_assert(kWideKP == 2, "the read order below is written out for two pieces per k-step");
        auto step = [&](auto first_, auto last_, auto phase_) __attribute__((always_inline)) {
            constexpr bool FIRST = decltype(first_)::value, LAST = decltype(last_)::value, PHASE = decltype(phase_)::value;
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");   // W1: this wave's share of step s has landed
            WIDE_BAR();                                        // ... everyone's has, and everyone has left compute(s - 1)
            int lane_e = lane;
            asm volatile("" : "+v"(lane_e));   // keeps the epilogue's lane arithmetic out of the k-loop's live set
            // a phase of the tile before this one: issued here, landed behind the MFMAs
            const bool pend = PHASE && P.phase != 0;
            WideFlight X;
            if (pend) wide_issue(a, P, X, fresh(bh), lane_e);   // AHEAD of the staging: see wide_issue
            stage(Q, ldsw + qst);   // step s + 2
            stage(R, ldsw + rst);   // step s + 4, last: the youngest
            uint32_t rt = 0;   // (the last step: the row tile of the pair, for wide_park -- asked of the walk again, not carried)
            int unit_next = 0;
            // The books of step s + 1, behind the step's staging and ahead of its fragment reads (which keep this step's
            // addresses, Ac and Bc), by live and dead waves alike: a wave whose unit is dead in this pair runs no MFMA and
            // keeps the same books in the same step.  Nothing here touches memory or LDS.  Other places were measured
            // (DESIGN 3.4): behind the step's last MFMA, ahead of the next barrier, +0.3 % at 1M rows and +0.7 % at 125 k
            // between the means, NOT clear of the run-to-run spread by the project's bar and therefore not taken; spread
            // among the step's MFMA pairs, or as one block behind the last fragment read, 1.0 - 1.5 % SLOWER than here.
            const unsigned Ac = A, Bc = B;
            __builtin_amdgcn_sched_barrier(0);
            next_queries();
            next_rows();
            rst = row_next(rst);   // the slot this step computed from is the one the next step stages into ...
            qst = q_next(qst);
            A = A0 + row_next(rst);   // ... and the next step computes from the slot behind it
            B = B0 + q_next(qst);
            if constexpr (LAST) {   // the computing cursor enters the next pair of the walk
                rt = wide_walk_pair(W, cp).rt;
                unit_next = (int)wide_walk_pair(W, cp + 1).col * (kWideQTiles / 2) + qp;
            }
            __builtin_amdgcn_sched_barrier(0);
            if (unit < nunits) {
                // The 12 fragment reads of the step in an order of their own, by hand: the six of piece 0 at once, those of
                // piece 1 behind the MFMAs that free their registers, every MFMA pair behind a counted lgkmcnt -- one exposed
                // LDS round trip per step.  Left to the compiler each pair of MFMAs waits with lgkmcnt(0) for the two reads
                // issued just ahead of it: five round trips per step.
                bf16x8 a0, a1, a2, a3, b0, b1, c0, c1;   // a: row fragments of blocks 0 .. 3; b / c: the two query tiles, piece 0 / 1
                const f32x16 zero = {};   // a tile's first MFMAs take an inline 0 as C: no accumulator is cleared
#define WIDE_PAIR0(i, av, q0, q1)                                                                                  \
                acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, q0, FIRST ? zero : acc[i][0], 0, 0, 0);    \
                acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, q1, FIRST ? zero : acc[i][1], 0, 0, 0)
#define WIDE_PAIR(i, av, q0, q1)                                                                 \
                acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, q0, acc[i][0], 0, 0, 0); \
                acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, q1, acc[i][1], 0, 0, 0)
                WIDE_DSR(b0, Bc, 0); WIDE_DSR(b1, Bc, 2048);
                WIDE_DSR(a0, Ac, 0); WIDE_DSR(a1, Ac, 2048); WIDE_DSR(a2, Ac, 4096); WIDE_DSR(a3, Ac, 6144);
                WIDE_LGKM3(3, b0, b1, a0); WIDE_PAIR0(0, a0, b0, b1);
                WIDE_DSR(c0, Bc, 1024);     // in flight: a1 a2 a3 c0
                WIDE_LGKM1(3, a1); WIDE_PAIR0(1, a1, b0, b1);
                WIDE_DSR(c1, Bc, 3072);     // a2 a3 c0 c1
                WIDE_LGKM1(3, a2); WIDE_PAIR0(2, a2, b0, b1);
                WIDE_DSR(a0, Ac, 1024);     // a3 c0 c1 a0
                WIDE_LGKM1(3, a3); WIDE_PAIR0(3, a3, b0, b1);
                WIDE_DSR(a1, Ac, 3072); WIDE_DSR(a2, Ac, 5120); WIDE_DSR(a3, Ac, 7168);   // c0 c1 a0 a1 a2 a3
                // (the scheduling barriers keep each pair in front of the next wait, which the compiler otherwise gathers)
                WIDE_LGKM3(3, c0, c1, a0); WIDE_PAIR(0, a0, c0, c1); __builtin_amdgcn_sched_barrier(0);
                WIDE_LGKM1(2, a1); WIDE_PAIR(1, a1, c0, c1); __builtin_amdgcn_sched_barrier(0);
                WIDE_LGKM1(1, a2); WIDE_PAIR(2, a2, c0, c1); __builtin_amdgcn_sched_barrier(0);
                WIDE_LGKM1(0, a3); WIDE_PAIR(3, a3, c0, c1); __builtin_amdgcn_sched_barrier(0);
#undef WIDE_PAIR
#undef WIDE_PAIR0
            }
            __builtin_amdgcn_sched_barrier(0);   // nothing of wide_land, its wait least of all, moves up among the MFMAs
            if (pend) wide_land<false>(a, P, X, fresh(bh), lane_e);   // W2
            if constexpr (LAST) {
                if (unit < nunits) {
                    wide_drain(a, P, fresh(bh), lane_e);   // fewer k-steps per tile than the phases take: the rest of them, now
                    asm volatile("" : "+v"(fold_key));   // (read from its VGPR here, once per tile, not kept in an SGPR)
                    wide_park<METRIC>(a, acc, P, (int64_t)rt, unit, wide_fold_at(cp, (uint32_t)__builtin_amdgcn_readfirstlane((int)fold_key)), fresh(bh), lane_e);
                }
                ++cp;
                unit = unit_next;
            }
        };
        // The tile loop: first step | KS - 2 middle steps | last step (KS >= 4, a multiple of 4).  The step sequence stays
        // flat for the staging cursors and the rings, which run on across tiles; phases run in the even steps.
        const std::false_type no;
        const std::true_type yes;
        do {
            step(yes, no, yes);
            for (int k = fresh(KS) / 2 - 1; k > 0; --k) {
                step(no, no, no);
                step(no, no, yes);
            }
            step(no, yes, no);
        } while (cp < W.npairs);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wide_drain(a, P, bh, lane);   // the last tile of the wave
    // The last word on the bound.  The finish ranks what stands at or above the FINAL thetac, in LDS, and sends a query whose
    // ranked entries do not fit there to the exhaustive path; the final thetac of a unit is what the waves fold behind
    // their LAST tiles, when every class slot is as good as complete.  Under a schedule a wave whose last tile is a no-fold
    // tile therefore folds theta of that tile's unit once more here, as its last drain did when every tile folded (without
    // it: 100-600 of 225,000 queries on the exhaustive path at 125 k rows and N = 8-16).  Nothing is tested
    // against it and it is no fold tile.  The last tile the wave parked is found from the walk, backwards: no state.
    if (a.fold_every > 1) {
        const uint32_t key = (uint32_t)__builtin_amdgcn_readfirstlane((int)fold_key);
        for (uint32_t p = W.npairs; p-- > 0;) {
            const WidePair pr = wide_walk_pair(W, p);
            const int u = (int)pr.col * (kWideQTiles / 2) + qp;
            if (u < nunits && (int64_t)pr.rt * kWideBlocks + 4 * bh < a.nblocks) {
                if (!wide_fold_at(p, key)) (void)wide_theta_fresh(a, u, lane, u * 64 + lane < a.nq);
                break;
            }
        }
    }
    if (a.stamps && lane == 0) a.stamps[2 * gw + 1] = wall_clock64();
    // statistics (wide_theta_folds): the fold tiles the workgroup's waves have completed, in closed form from the walk --
    // the tiles wide_park parked (a live unit, an existing row half) with wide_fold true; every one of them goes through T
    // before its wave leaves.  Counted here and not in T: a counter carried through the k-loop costs it a spilled SGPR
    // (DESIGN 3.4).  Wave 0 counts for all eight, lane = (pair number mod 8, wave), and adds once: one atomic per wave
    // would be 1,800 atomics on one word at the end of every launch.
    if (wave == 0) {
        const uint32_t wv = (uint32_t)lane & 7u;
        const uint32_t key = wide_fold_key(blockIdx.x, wv, (uint32_t)a.fold_every);
        u32 nf = 0;
        for (uint32_t p = (uint32_t)lane >> 3; p < W.npairs; p += 8) {
            const WidePair pr = wide_walk_pair(W, p);
            const bool parked = (int)pr.col * (kWideQTiles / 2) + (int)(wv >> 1) < nunits && (int64_t)pr.rt * kWideBlocks + 4 * (int)(wv & 1u) < a.nblocks;
            nf += parked && wide_fold_at(p, key) ? 1u : 0u;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) nf += (u32)__shfl_xor((int)nf, off);
        if (lane == 0 && nf) atomicAdd(a.folds, (unsigned long long)nf);
    }
}
