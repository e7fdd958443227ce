// encoder_plan.h -- the policy of the encoder's forward: which GEMM family a batch takes (small-batch, 256-tile, 128-tile),
// how the tiled path splits K in its N = H products, how many partials the heads and the LayerNorms sum, how large the
// pre-LayerNorm buffer is.  Host-only plain C++17 (no HIP header, no HIP type): pure functions of an EncShape, so that
// Encoder::run_forward, the test hooks (hipenc_colbert_rows, hipenc_linear_ex; all in encoder.hip) and a test on a machine
// without a GPU (hipenc_forward_plan) ask the same code.  The kernel headers assert that their tile geometry is the one
// assumed here; oracle/encoder_cases.py and oracle/linear_cases.py restate the rules for the tests that compare the two.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/hiprag.h"

namespace hiprag {

// Tile geometry the rules depend on
constexpr int kTileM = 128, kTileN = 128, kTileK = 64;   // gemm_bf16_kernel (encoder_gemm.h)
constexpr int kBigTile = 256, kBigK = 64;                // gemm256_kernel (gemm256.h): square tiles, k-tiles taken in pairs
constexpr int kSkinnyMaxK = 1024;                        // gemm_skinny_kernel: K range of a workgroup, at most ...
constexpr int kSkinnyKGrain = 128;                       // ... and a multiple of (4 waves x one 32-deep MFMA step)
constexpr int kSkinnyRows = 64;                          // its row block; S is a multiple of it, so every T is

// Batches of at most this many (padded) token rows take the small-batch GEMM; 0 = never (HIPENC_SMALL_ROWS).  Measured
// crossover with the split-K tiled GEMM: 256 rows 1.72 vs 2.11 ms, 512 rows 2.37 vs 2.17 ms.
constexpr int kSmallRowsDefault = 384;
constexpr int kSmallMaxHidden = 1024;   // the small-batch and the 256-tile path exist for H <= 1024 (registers, LayerNorm16)
constexpr int kMaxPartials = 4;         // partial products a LayerNorm<PARTS> row sums at most

// The tile split aims at about this many workgroups per launch, and leaves every split at least kTileSplitMinK of K
constexpr int kTileSplitWorkgroups = 512;
constexpr int kTileSplitMinK = 256;

// All the policy depends on: the model's widths, the device's CUs, HIPENC_SMALL_ROWS and HIPENC_GEMM256 as read at
// creation.  The C struct of hipenc_shape itself, so the entry and the tests see what the policy sees.
using EncShape = hipenc_shape_t;

enum class EncPath : int { small = HIPENC_PATH_SMALL, big = HIPENC_PATH_BIG, tiled = HIPENC_PATH_TILED };

// One forward over nseq rows of S tokens
struct EncPlan {
    int T = 0;             // token rows, nseq * S
    int M = 0;             // rows the GEMMs run over: T padded to whole tiles of the path's family (small: 128, as tiled)
    EncPath path = EncPath::tiled;
    int osplit = 1;        // tiled: K split of the out-projection (K = H); 1 on the other paths
    int dsplit = 1;        // tiled: K split of FFN-down (K = F); 1 on the other paths
    int fsplit = 1;        // skinny_split(F): the partials of the small path's FFN-down
    int head_split = 1;    // partials of the ColBERT head's product on this path: 1 on small and big, osplit on tiled
    size_t pre_bytes = 0;  // the pre-LayerNorm buffer: M x H floats times the most partials any product of the path writes
};

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// ---- small-batch kernel: K range per workgroup = K / split, a multiple of kSkinnyKGrain and at most kSkinnyMaxK ----------
inline int skinny_split(int K) { return (K + kSkinnyMaxK - 1) / kSkinnyMaxK; }
inline bool skinny_ok(int K) { return K % (skinny_split(K) * kSkinnyKGrain) == 0; }

// ---- 128-tile kernel: the split of an N = H product over K.  With few row tiles the (H/128) x (M/128) workgroups leave
// most CUs idle while each walks K serially (F -> H at 2560 rows: 160 workgroups x 64 k-tiles = 64 us of a 165 us layer):
// split K, in powers of two, until the launch has about 512 workgroups; the LayerNorm sums the partials.
inline int tile_ksplit(int H, int M, int K)
{
    int ks = 1;
    while (ks < kMaxPartials && (H / kTileN) * (M / kTileM) * ks < kTileSplitWorkgroups && K % (ks * 2 * kTileK) == 0 &&
           K / (ks * 2) >= kTileSplitMinK)
        ks *= 2;
    return ks;
}

// ---- 256-tile persistent kernel: whole tiles in M and N and an even number of k-tiles ...
inline bool tile256_shape_ok(int M, int N, int K) { return M % kBigTile == 0 && N % kBigTile == 0 && K % (2 * kBigK) == 0; }
inline int tile256_tiles(int M, int N) { return (M / kBigTile) * (N / kBigTile); }
// ... and enough tiles.  There are TWO fill rules, and they are different on purpose:
//   the forward  takes the 256-tile path for ALL of a layer's products or none: every product must give at least half the
//                CUs a tile, and the narrowest one (N = H) every CU;
//   the hook     (hipenc_linear_ex, impl 0 = auto) judges ONE product: at least one tile per CU.
inline bool tile256_fills_forward_product(int M, int N, int n_cu) { return tile256_tiles(M, N) >= n_cu / 2; }
inline bool tile256_fills_forward_narrowest(int M, int H, int n_cu) { return tile256_tiles(M, H) >= n_cu; }
inline bool tile256_fills_auto(int M, int N, int cus) { return tile256_tiles(M, N) >= cus; }

inline bool big_ok(const EncShape& s, int M, int N, int K)
{
    return s.use256 && tile256_shape_ok(M, N, K) && tile256_fills_forward_product(M, N, s.n_cu);
}

inline EncPlan plan_forward(const EncShape& s, int nseq, int S)
{
    const int H = s.hidden, F = s.ffn;
    EncPlan p;
    p.T = nseq * S;
    // one query / a few short texts: weight-streaming GEMMs instead of 128 x 128 tiles
    const bool small = s.small_rows > 0 && p.T <= s.small_rows && H <= kSmallMaxHidden && skinny_ok(H) && skinny_ok(F) &&
                       skinny_split(F) <= kMaxPartials;
    // big batches: 256 x 256 persistent tiles once the narrowest GEMM (N = H) fills every CU
    const int M256 = round_up(p.T, kBigTile);
    const bool big = H <= kSmallMaxHidden && big_ok(s, M256, H, H) && big_ok(s, M256, F, H) && big_ok(s, M256, H, F) &&
                     tile256_fills_forward_narrowest(M256, H, s.n_cu);
    p.path = small ? EncPath::small : big ? EncPath::big : EncPath::tiled;   // small wins where both hold
    p.M = big ? M256 : round_up(p.T, kTileM);
    p.fsplit = skinny_split(F);
    if (p.path == EncPath::tiled) {
        p.osplit = tile_ksplit(H, p.M, H);
        p.dsplit = tile_ksplit(H, p.M, F);
        p.head_split = p.osplit;
    }
    p.pre_bytes = (size_t)p.M * H * 4 * (small ? p.fsplit : std::max(p.osplit, p.dsplit));
    return p;
}

}  // namespace hiprag
