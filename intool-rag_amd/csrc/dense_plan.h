// dense_plan.h -- the launch policy of the dense scan: which kernel a launch gets and in what shape, how many queries a
// launch takes, how many CUs a pipelined scan leaves free, which tiles a workgroup of the wide kernel walks.  Plain C++17
// (no HIP header, no HIP type): pure functions of a ScanShape, so that DenseIndex (dense_index.hip), the statistics
// (dense_api.hip) and a test on a machine without a GPU (hiprag_scan_plan, hiprag_wide_walk, hiprag_wide_fold) all ask the same code.  The
// kernels and scan_wide.h take their policy constants from here, and the wide kernel calls the walk itself (the only
// functions here that carry a device qualifier, behind a macro that is empty for a host compiler); oracle/width_cases.py
// restates the rules for the tests that compare the two.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/hiprag.h"

namespace hiprag {

constexpr int kPassQ = 64;         // queries that share one read of the index
constexpr int kMaxQ = 1024;        // most queries per LAUNCH (16 passes of 64): see launch_queries
constexpr int kMaxKFast = 128;     // deepest k of the scan + finish path; beyond: exhaustive path for every query
constexpr int kClasses = 64;       // theta slots per query
constexpr int kNoFilterGroups = 1024;   // indexes with at most this many groups list every group (= the finish's LDS list)

// LDS of the narrow kernels: query tile (P KiB) | Cand stage[2][kStageHalf] | u32 ctl[16] | u32 bound[kThetaBack][64]
constexpr int kStageHalf = 896;   // staged appends per workgroup and pass (two alternating halves of 14 KiB of LDS); beyond that: direct global appends
constexpr int kThetaBack = 8;     // passes a value can lag behind the pass its wave is in (kAge blocks / >= 1 block per pass)
constexpr int kCandBytes = 16;    // sizeof(Cand): one staged or listed candidate

// The wide kernel (scan_wide.h)
constexpr int kWideBlocks = 8;     // blocks per row tile (256 rows)
constexpr int kWideQTiles = 8;     // 32-query tiles per column (256 queries)
constexpr int kWideKP = 2;         // pieces per k-step (32 k-values)
constexpr int kWideBufFrags = kWideBlocks * kWideKP * 64;   // 16-byte fragments per ring slot (16 KiB): a k-step's row pieces, or its query pieces
static_assert(kWideBlocks == kWideQTiles, "one slot size serves both rings");
constexpr int kWideRowRing = 5;    // row pieces are issued four k-steps ahead: HBM / Infinity Cache
constexpr int kWideQRing = 3;      // query pieces two k-steps ahead: the XCD's L2
constexpr size_t kWideLds = (size_t)(kWideRowRing + kWideQRing) * kWideBufFrags * 16;
static_assert(kWideLds == 131072, "eight 16 KiB slots, one LDS object");
constexpr int kWideMinCus = 32;    // row tiles 0..31 (all 64 classes) must fall into the first round
// Default threshold of the wide kernel, measured one launch at a time, ms narrow / wide (profiles/wide_threshold_probe*.jsonl):
// at 1M x 1024 128 queries 0.74 / 0.81, 192 queries 1.09 / 0.88, 256 queries 1.39 / 0.94; at 125 k x 1024 192 queries
// 0.210 / 0.234, 256 queries 0.267 / 0.248: 256 is the smallest size at which the wide kernel wins on both.
constexpr int kWideMinQ = 256;

// CUs a pipelined scan leaves to the finish of the launch before it (search_dev's own pipeline, and hiprag/sharded.py
// through hipidx_pipe_spare_cus).  The narrow scan is HBM-bound and 32-64 measure the same: 48.  The wide scan is bound by
// its CUs: workgroup i walks row tiles i, i + G, ... and the last, partial round is split by column over all of them
// (wide_walk), so a launch lasts floor(row tiles / G) ncol + ceil((row tiles mod G) ncol / G) pair-times, and CUs that
// save a round are worth more to the scan than to the finish -- down to 32, below which the finish no longer fits beside
// the scan (fin_kernel 0.38 ms at 32 spare CUs, 1.29 ms at 26).  The rule below still counts whole rounds,
// ceil(row tiles / G), as it was measured: 1M x 1024, 512 queries: 19 rounds on 208 workgroups, 18 on 224, +2.4 %;
// 125 k x 1024, 1024 queries: 3 rounds either way, and 32 is 1.6 % SLOWER than 48.  (In pair-times the larger grid would
// now save one at 250 k and 125 k rows as well, 18 against 19 and 9 against 10: DESIGN 9.2.)
constexpr int kPipeSpareCus = 48;
constexpr int kPipeSpareCusWide = 32;

// Launch size (launch_queries): a launch should last about as long as kLaunchPasses passes over kLaunchRefBytes, a 1M x 1024
// fp32 index (2.6 ms), between kMinLaunchPasses and kMaxQ / kPassQ passes.
constexpr double kLaunchPasses = 4.0;
constexpr double kLaunchRefBytes = 4.096e9;
constexpr int kMinLaunchPasses = 4;

// HIPRAG_SCAN_MODE: the operands the scan streams.  The values are what FinArgs::mode (scan_eps) receives.
enum ScanMode : int {
    kScanQ64 = 2,    // fp32 rows split on the fly
    kScanBf16 = 3,   // bf16 filter copy (default)
};

// All the policy depends on: nblocks, P, mode (a ScanMode), wide_env (HIPRAG_SCAN_WIDE: 0 = never the wide kernel, 1 =
// whenever a launch is eligible, -1 = unset: from kWideMinQ queries), n_cu, launch_env (HIPRAG_LAUNCH_QUERIES, 0 = size
// launches by the index).  The C struct of hipidx_scan_shape itself, so the entry and the tests see what the policy sees.
using ScanShape = hipidx_scan_shape_t;

// One scan launch.  Everything but `run` and `filter` is meaningful only where `run` is set.
struct ScanPlan {
    bool run = false;          // a scan is launched at all (rows, and k within the finish's reach)
    bool wide = false;         // scan_wide_kernel
    int waves = 8;             // per workgroup
    int ring = 16;             // depth of the narrow kernels' load ring (0: wide)
    bool multi_pass = false;   // more than kPassQ queries
    bool filter = false;       // the scan keeps a bound and lists only what reaches it
    int ncls = 1;              // theta classes in use: every class needs a publisher, or theta never forms
    size_t lds_bytes = 0;      // dynamic LDS of the launch
    bool qtile_image = false;  // the query tiles come from qtile_kernel's images
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline bool filter_on(const ScanShape& s) { return 2 * s.nblocks > kNoFilterGroups; }
inline bool uses_qtile_images(const ScanShape& s) { return s.mode == kScanBf16; }   // multi-pass launches of the bf16 kernels

// Small shards (an 8-GPU row split of 1M rows leaves 125 k per GPU): with 8 waves per workgroup a wave streams two or
// three 32-row blocks per pass; 4-wave workgroups stream twice as many each and leave half of every SIMD's registers to
// the tail kernels of earlier steps.  Measured in rounds 1-2 (1024 queries per launch, pipelined): 125 k rows 945 -> 902
// us per step, 250 k 1640 -> 1590, 500 k about equal, 1M equal: 4 waves below 9 blocks per wave of the 8-wave partition.
inline int scan_waves(const ScanShape& s, int cus)
{
    return (s.mode == kScanBf16 && s.P % 32 == 0 && s.nblocks < (int64_t)cus * 8 * 9) ? 4 : 8;
}

// Which launches take scan_wide_kernel (scan_wide.h), if the scan had `cus` workgroups: the bf16 copy, the filter on (more
// than 64 row tiles of 256 rows, so that row tiles 0..31 publish all 64 classes), at least 32 workgroups (those row tiles
// all fall into the first round) and enough queries.  Forced (HIPRAG_SCAN_WIDE=1): more than one 64-query pass.  Default:
// at least kWideMinQ queries -- and at least one row tile per workgroup: on a smaller index part of the grid owns no tile
// while every narrow wave still streams its share (not measured, so not taken).
inline bool wide_launch_on(const ScanShape& s, int nq, int cus)
{
    if (s.mode != kScanBf16 || s.wide_env == 0 || !filter_on(s) || cus < kWideMinCus) return false;
    if (s.wide_env == 1) return nq > kPassQ;
    return nq >= kWideMinQ && ceil_div(s.nblocks, kWideBlocks) >= cus;
}

// Bytes of index one pass (64 queries) reads, algorithmically: the operand stream, + the norms in L2 mode.  The wide kernel
// reads both once per 256 queries.
inline int64_t stream_bytes_per_pass(const ScanShape& s) { return s.nblocks * s.P * (s.mode == kScanBf16 ? 512 : 1024); }
inline int64_t bytes_per_pass(const ScanShape& s, int metric, bool wide = false)
{
    return (stream_bytes_per_pass(s) + (metric == HIPRAG_METRIC_L2 ? s.nblocks * 32 * 4 : 0)) / (wide ? 4 : 1);
}

// Queries per launch.  A launch chained behind its predecessor pays ~45-60 us of dispatch bubble and the tail of a
// launch is a fixed cost too, so launches are sized to last about as long as four passes over a 1M x 1024 fp32 index
// (2.6 ms) whatever the index size: 8 passes of the bf16 copy there, 16 (the cap) at half a million rows and below --
// where a short launch would spend a quarter of its time outside the scan.  HIPRAG_LAUNCH_QUERIES fixes the size.
inline int launch_queries(const ScanShape& s)
{
    if (s.launch_env > 0) return std::max(kPassQ, std::min(kMaxQ, s.launch_env / kPassQ * kPassQ));
    ScanShape t = s;
    t.nblocks = std::max<int64_t>(s.nblocks, 1);
    const int np = (int)std::lround(kLaunchPasses * kLaunchRefBytes / (double)stream_bytes_per_pass(t));
    return std::max(kMinLaunchPasses, std::min(kMaxQ / kPassQ, np)) * kPassQ;
}

// See kPipeSpareCus: 32 where a full launch goes wide on either grid and the larger grid saves it a round, 48 otherwise.
inline int pipe_spare_cus(const ScanShape& s, int launch_q)
{
    const int g48 = std::max(1, s.n_cu - kPipeSpareCus), g32 = std::max(1, s.n_cu - kPipeSpareCusWide);
    if (!wide_launch_on(s, launch_q, g48) || !wide_launch_on(s, launch_q, g32)) return kPipeSpareCus;
    const int64_t nrt = ceil_div(s.nblocks, kWideBlocks);
    return ceil_div(nrt, g32) < ceil_div(nrt, g48) ? kPipeSpareCusWide : kPipeSpareCus;
}

// The WALK of the wide kernel: which (row tile, column) pairs workgroup w of G computes, and in what order.  One definition
// for the kernel (scan_wide.h), the host and a test on a machine without a GPU (hiprag_wide_walk); HIPRAG_HD is empty
// outside hipcc.  A pair is one 256-row tile against one 256-query column, d_pad / 32 k-steps.  With F = nrt / G full
// rounds and L = nrt - F G row tiles left over:
//   * pairs 0 .. F ncol - 1, the full rounds: row tile w + (p / ncol) G, column p % ncol.  Row tiles 0..31 fall into the
//     first round (every class gets its publisher), and the columns of a row tile follow one another on one workgroup
//     (the re-read of the row tile comes from the Infinity Cache);
//   * the tail, split by COLUMN over all the workgroups: the L ncol left-over pairs are numbered row tile first, and
//     workgroup w takes numbers t = w, w + G, ... < L ncol: row tile F G + t / ncol, column t % ncol.  By row tile the
//     tail would last ncol pair-times on L workgroups while G - L CUs idle; like this it lasts ceil(L ncol / G);
//   * F == 0 (fewer row tiles than workgroups; only a forced wide launch gets here): workgroup w < nrt takes row tile w
//     and all its columns, nothing is spread -- row tiles 0..31 publish all 64 classes in every column's first pair.
// A workgroup runs F ncol + ceil((L ncol - w) / G) pairs (the last term not below 0); the longest sequence is
// ceil(nrt ncol / G) wherever F > 0: the best that whole pairs allow.  32-bit throughout (the kernel walks with it):
// nrt < 2^28 (a group id is 32 bits), ncol <= kMaxQ / 256.
#if defined(__HIPCC__)
#define HIPRAG_HD __attribute__((host)) __attribute__((device))
#else
#define HIPRAG_HD
#endif
struct WideWalk {
    uint32_t ncol, G, w;
    uint32_t full;     // pairs of the full rounds, F ncol (F == 0: ncol)
    uint32_t tail0;    // first row tile of the tail, F G
    uint32_t npairs;   // pairs of this workgroup
};
struct WidePair {
    uint32_t rt, col;
};
constexpr uint32_t kWideNoTile = 0xFFFFFFFFu;   // the row tile of a pair past the end of a walk: past any index
HIPRAG_HD inline WideWalk wide_walk(uint32_t nrt, uint32_t ncol, uint32_t G, uint32_t w)
{
    const uint32_t F = nrt / G, L = nrt - F * G;
    const uint32_t tail = F ? L * ncol : 0u;   // pairs of the whole tail
    WideWalk W;
    W.ncol = ncol; W.G = G; W.w = w;
    W.full = (F ? F : 1u) * ncol;
    W.tail0 = F * G;
    W.npairs = w >= nrt ? 0u : W.full + (tail > w ? (tail - w + G - 1) / G : 0u);
    return W;
}
// pair p of the walk; p >= npairs: (kWideNoTile, 0) -- the kernel's staging cursors run on into it, with clamped addresses
HIPRAG_HD inline WidePair wide_walk_pair(const WideWalk& W, uint32_t p)
{
    if (p >= W.npairs) return WidePair{kWideNoTile, 0u};
    const bool in_full = p < W.full;
    const uint32_t t = in_full ? p : W.w + (p - W.full) * W.G;   // the tail's t < L ncol, by npairs
    const uint32_t r = t / W.ncol;                               // one division serves both parts
    return WidePair{in_full ? W.w + r * W.G : W.tail0 + r, t - r * W.ncol};
}

// The FOLD SCHEDULE of the wide kernel: does wave `wave` of workgroup `wg` recompute theta of its 64-query unit (phases
// B0..B3 of scan_wide.h: 64 class-slot loads, folded into thetac by phase T) behind pair number p of its walk, or does it
// only read thetac (phase T alone)?  One definition for the kernel, the host (hiprag_wide_fold) and the tests.
//   * every pair p < kWideFoldFirst folds: the bound forms in a launch's first tiles and the lists are longest there --
//     and an index of few pairs per workgroup folds in every tile, as it did before there was a schedule;
//   * from there a wave folds in one pair out of N (a power of two <= kWideFoldMax: the test is a mask), at an offset that
//     counts through (workgroup, row half) and shifts with the query pair: any N consecutive pairs hold exactly one fold
//     of every wave, and at any pair number the waves that fold for one query pair are floor or ceil(2 G / N) of the 2 G
//     (workgroup, row half) -- somebody refreshes thetac of every unit in every pair-time.
// Exactness does not depend on the schedule (scan_wide.h, Invariants): a wave that skips its recomputation tests against
// what thetac holds memory-side, which every fold of every workgroup has gone into.  N = 1 folds always.
constexpr int kWideFoldFirst = 4;
constexpr int kWideFoldMax = 64;
constexpr int kWideFoldEvery = 8;   // the default of HIPRAG_WIDE_FOLD_EVERY, measured over 1, 2, 4, 8, 16; 1 = every tile folds
inline bool wide_fold_every_ok(int64_t N) { return N >= 1 && N <= kWideFoldMax && (N & (N - 1)) == 0; }
// In two steps, because the kernel keeps a wave's part of the question in one register: the KEY of a wave = its offset
// (mod kWideFoldMax, which is all a mask of at most kWideFoldMax - 1 sees) in bits 0..7, N - 1 in bits 8..15.
HIPRAG_HD inline uint32_t wide_fold_key(uint32_t wg, uint32_t wave, uint32_t N)
{
    const uint32_t bh = wave & 1u, qp = wave >> 1;   // the wave's row half and query pair, as the kernel assigns them
    return ((2u * wg + bh + qp) & (uint32_t)(kWideFoldMax - 1)) | ((N - 1u) << 8);
}
HIPRAG_HD inline bool wide_fold_at(uint32_t p, uint32_t key)
{
    return p < (uint32_t)kWideFoldFirst || ((p + (key & 0xFFu)) & (key >> 8)) == 0u;
}
HIPRAG_HD inline bool wide_fold(uint32_t p, uint32_t wg, uint32_t wave, uint32_t N) { return wide_fold_at(p, wide_fold_key(wg, wave, N)); }

// The launch that `nq` queries at depth k get on a grid of `cus` workgroups.
inline ScanPlan plan_scan(const ScanShape& s, int nq, int k, int cus)
{
    ScanPlan p;
    p.filter = filter_on(s);
    p.run = s.nblocks > 0 && k <= kMaxKFast;   // deeper k: every query takes the exhaustive path, nothing to scan for
    if (!p.run) return p;
    p.wide = wide_launch_on(s, nq, cus);
    p.waves = p.wide ? 8 : scan_waves(s, cus);
    p.multi_pass = nq > kPassQ;
    // ring depth: 16 pieces where that divides the pieces of a block of the filter copy (d_pad / 16), else 8; q64 runs 16
    p.ring = p.wide ? 0 : (s.mode == kScanQ64 || (s.P / 2) % 16 == 0) ? 16 : 8;
    const int64_t bpw = ceil_div(s.nblocks, (int64_t)cus * p.waves);   // the kernels' scan_blocks_per_wave
    p.ncls = (int)std::max<int64_t>(1, std::min<int64_t>(kClasses, ceil_div(s.nblocks, bpw)));   // waves that own blocks
    // narrow: query tile + staged appends + control words + bounds
    p.lds_bytes = p.wide ? kWideLds : (size_t)s.P * 1024 + (size_t)2 * kStageHalf * kCandBytes + 64 + (size_t)kThetaBack * 64 * 4;
    p.qtile_image = uses_qtile_images(s) && p.multi_pass;
    return p;
}

}  // namespace hiprag
