"""
oracle/encoder_cases.py -- the inputs of the encoder's kernel-level and every-row tests, shared by the GPU tests
(tests/test_encoder_kernels_gpu.py) and by the CPU tests that prove the bars can fail (tests/test_encoder_reference_cpu.py).

TEST INFRASTRUCTURE ONLY (see oracle/hybrid_oracle.py header).  Nothing here depends on the code under test: the attention
cases are built from seeded random numbers and checked in float64, the model cases are plain configurations.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch

# ---- attention2_kernel ----------------------------------------------------------------------------------------------
ATT_S = (64, 128, 192, 512)
ATT_HEADS = 4
ATT_LENS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192)
ATT_REGIMES = ("peaked", "rising", "first_tile", "interleaved", "huge")
POISON = 3.0e4           # finite: 0 * NaN is NaN inside an MFMA, and the model never produces NaN there either
U_BF16 = 2.0 ** -8       # unit roundoff of bf16 (8 significant bits, round to nearest even)
TILE_STEP = 4.0          # logit step between 64-key tiles in the ordered regimes


def attention_lens(S: int) -> List[int]:
    return sorted({n for n in ATT_LENS if n <= S} | {S})


def attention_case(regime: str, S: int, seed: int = 0) -> Dict[str, object]:
    """bf16 q (carrying the 1/8 scale: logits are q . k), k [nseq, 4, S, 64], vt [nseq, 4, 64, S] and lens, one sequence
    per length of attention_lens(S), different data for every (sequence, head).
      peaked       random logits of standard deviation 6
      rising       keys ordered so that EVERY query's maximum rises in EVERY 64-key tile (checked below in float64)
      first_tile   keys ordered so that every query's maximum lies in tile 0 and never rises again (checked)
      interleaved  even queries as `rising`, odd queries as `first_tile`: inside one wave of 32 queries the rescale
                   branch is taken in every tile, and half of its lanes must come through it with a factor of exactly 1
      huge         random logits of standard deviation 40 (|logit| ~ 80 and beyond): exp() of them overflows fp32 unless the
                   row maximum is subtracted first
    K rows and V^T columns at positions >= len hold POISON."""
    assert regime in ATT_REGIMES and S % 64 == 0
    lens = attention_lens(S)
    n, h = len(lens), ATT_HEADS
    g = torch.Generator().manual_seed(1000 * ATT_REGIMES.index(regime) + S + seed)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    k, v = rn(n, h, S, 64), rn(n, h, S, 64)
    if regime == "peaked":
        q = rn(n, h, S, 64) * 0.75
    elif regime == "huge":
        q = rn(n, h, S, 64) * 5.0
    else:
        # coordinate 0 carries the order (logit = sign * TILE_STEP * tile + noise of standard deviation 0.32), the rest noise
        q = rn(n, h, S, 64) * 0.04
        tile = (torch.arange(S) // 64).to(torch.float32)
        sign = {"rising": torch.ones(S), "first_tile": -torch.ones(S),
                "interleaved": torch.where(torch.arange(S) % 2 == 0, 1.0, -1.0)}[regime]
        q[..., 0] = sign
        k[..., 0] = TILE_STEP * tile
    q, k, v = (t.to(torch.bfloat16) for t in (q, k, v))
    if regime in ("rising", "first_tile", "interleaved"):
        _check_order(regime, q, k, lens)
    vt = v.transpose(-1, -2).contiguous()
    for i, n_i in enumerate(lens):
        k[i, :, n_i:, :] = POISON
        vt[i, :, :, n_i:] = POISON
    return {"q": q, "k": k, "vt": vt, "lens": np.asarray(lens, dtype=np.int32), "S": S, "heads": h}


def _check_order(regime, q, k, lens):
    """float64 proof that the keys are ordered as the regime says, for every real query and every tile with a real key."""
    s = q.double() @ k.double().transpose(-1, -2)
    for i, n_i in enumerate(lens):
        nt = (n_i + 63) // 64
        if nt < 2:
            continue
        tmax = torch.stack([s[i, :, :n_i, 64 * t:min(64 * t + 64, n_i)].max(-1).values for t in range(nt)], -1)   # [h, query, tile]
        rises = tmax[..., 1:] > torch.cummax(tmax, -1).values[..., :-1]
        up = torch.ones(n_i, dtype=torch.bool) if regime == "rising" else torch.zeros(n_i, dtype=torch.bool) \
            if regime == "first_tile" else (torch.arange(n_i) % 2 == 0)
        assert bool(rises[:, up].all()) and not bool(rises[:, ~up].any()), (regime, n_i)


def attention_bound(ctx_ref: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """Element-wise bound on |ctx_gpu - ctx_ref|.  q, k, v are bf16-exact and their products exact in fp32, so the only bf16
    roundings are the probabilities (numerator only: relative error <= u each, <= u * A in the quotient) and the output
    (<= u * |ctx|); the factor 1 + 2^-6 and the 1e-6 cover fp32 accumulation over <= 512 keys and the 1-ulp hardware exp2."""
    return U_BF16 * (A + ctx_ref.abs()) * (1.0 + 2.0 ** -6) + 1e-6


# ---- whole model, every row ------------------------------------------------------------------------------------------
MIXED_LENS = (200, 129, 65, 64, 16, 1)      # cross 64 and 128; 200 and 129 leave a half-filled second 128-query tile
YARDSTICK_FACTOR = 3.0                      # a different realisation of the same roundings + fp32 instead of fp64 sums

# path: which GEMM / LayerNorm forms Encoder::forward takes (csrc/encoder.hip).  env: switches read at hipenc_create.
# sample: indices of the sequences compared against the CPU reference (None = all).
MODEL_CASES = {
    "small_h256": dict(cfg=dict(vocab=1000, hidden=256, layers=2, heads=4, ffn=1024, max_pos=300), std=0.08, seed=21,
                       lens=MIXED_LENS, env={"HIPENC_SMALL_ROWS": "2048"}, path="small", sample=None),
    "tiled_h256": dict(cfg=dict(vocab=1000, hidden=256, layers=2, heads=4, ffn=1024, max_pos=300), std=0.08, seed=21,
                       lens=MIXED_LENS, env={"HIPENC_SMALL_ROWS": "0"}, path="tiled_splitk", sample=None),
    "tiled_splitk_h1024": dict(cfg=dict(vocab=3000, hidden=1024, layers=2, heads=16, ffn=4096, max_pos=300), std=0.05, seed=22,
                               lens=MIXED_LENS, env={"HIPENC_SMALL_ROWS": "0"}, path="tiled_splitk", sample=None),
    "tiled_nosplit_h1024": dict(cfg=dict(vocab=3000, hidden=1024, layers=2, heads=16, ffn=4096, max_pos=300), std=0.05, seed=23,
                                lens=MIXED_LENS * 7, env={}, path="tiled", sample=(0, 1, 2, 3, 4, 5, 36, 41)),
    "big_h1024": dict(cfg=dict(vocab=3000, hidden=1024, layers=2, heads=16, ffn=4096, max_pos=300), std=0.05, seed=24,
                      lens=(191, 129, 65, 64, 16, 1) * 14 + (192, 130, 2), env={}, path="big", sample=(0, 1, 5, 40, 84, 85, 86)),
    "tiled_h384": dict(cfg=dict(vocab=1000, hidden=384, layers=2, heads=6, ffn=1536, max_pos=300), std=0.08, seed=25,
                       lens=MIXED_LENS, env={}, path="tiled_splitk", sample=None),
    "tiled_h2048": dict(cfg=dict(vocab=1000, hidden=2048, layers=1, heads=32, ffn=2048, max_pos=300), std=0.035, seed=26,
                        lens=MIXED_LENS, env={}, path="tiled_splitk", sample=None),
}


def model_tokens(case: Dict[str, object]) -> List[List[int]]:
    rng = np.random.default_rng(case["seed"])
    vocab = case["cfg"]["vocab"]
    return [([0] + rng.integers(3, vocab, size=max(0, n - 2)).tolist() + [2])[:n] for n in case["lens"]]


def forward_path(hidden: int, ffn: int, rows: int, small_rows: int, use256: bool, n_cu: int) -> str:
    """Which path the encoder's forward takes for `rows` = nseq * S padded token rows -- the selection rules of
    csrc/encoder_plan.h (plan_forward) restated, so that a test can assert that the sizes and switches it chose reach the path
    it means to test.  Kept as the independent statement of the rule: tests/test_encoder_plan_cpu.py holds it equal to what
    the library itself answers (hipenc_forward_plan), so a drift of either shows:
      small         weight-streaming GEMMs, split-K partials summed by the LayerNorm
      big           persistent 256 x 256 tiles, bf16 pre-LayerNorm rows
      tiled_splitk  128 x 128 tiles, at least one of the two N = H products split over K
      tiled         128 x 128 tiles, no split"""
    H, F, T = hidden, ffn, rows
    skinny_split = lambda K: (K + 1023) // 1024
    skinny_ok = lambda K: K % (skinny_split(K) * 128) == 0
    if small_rows > 0 and T <= small_rows and H <= 1024 and skinny_ok(H) and skinny_ok(F) and skinny_split(F) <= 4:
        return "small"
    M256 = -(-T // 256) * 256
    big_ok = lambda M, N, K: use256 and M % 256 == 0 and N % 256 == 0 and K % 128 == 0 and (M // 256) * (N // 256) >= n_cu // 2
    if H <= 1024 and big_ok(M256, H, H) and big_ok(M256, F, H) and big_ok(M256, H, F) and (M256 // 256) * (H // 256) >= n_cu:
        return "big"
    M = -(-T // 128) * 128

    def tile_split(K):
        ks = 1
        while ks < 4 and (H // 128) * (M // 128) * ks < 512 and K % (ks * 128) == 0 and K // (ks * 2) >= 256:
            ks *= 2
        return ks
    return "tiled_splitk" if max(tile_split(H), tile_split(F)) > 1 else "tiled"
