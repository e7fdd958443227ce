"""
oracle/linear_cases.py -- cases, float64 references, derived bounds and mutants for the encoder's three GEMM kernels and three
LayerNorm kernels (csrc/encoder.hip, csrc/gemm256.h), shared by tests/test_encoder_linear_gpu.py (the kernels, through
hipenc_linear_ex / hipenc_layernorm) and tests/test_linear_cases_cpu.py (which proves on the CPU that the checks can fail).

TEST INFRASTRUCTURE ONLY (see oracle/hybrid_oracle.py header): pure numpy / torch-CPU; the product package never imports it.
Nothing here is fitted to what the GPU gives: every bound below comes from the float64 reference and the number formats.

Notation: u32 = 2^-24 and u16 = 2^-8 are the unit roundoffs of fp32 and bf16 (round to nearest even).  hulp16(v) is half a
bf16 ulp at magnitude v, 2^(floor(log2 v) - 8).  A value y that is computed in fp32 with error <= e and then rounded once to
bf16 lands within  hulp16(|y| + e) + e  of y.

DATA REGIMES of the GEMMs
  exact   A and the residual are integers in [-8, 8], W and the bias integers in [-8, 8] * 2^-6: all bf16-exact.  Every
          product is an integer multiple of 2^-6 of at most 64 units, so with K <= 4096 every partial sum over any subset,
          in any order, is a multiple of 2^-6 below 2^18 + 2^10 units < 2^24: fp32 accumulation is EXACT whatever the
          kernel's order or split (linear_data asserts the precondition).  The float64 matmul of the same integers is exact
          too.  Hence fp32 outputs and raw partials must equal the reference bit for bit, and bf16 outputs must equal ONE
          round-to-nearest-even of the exact value, bit for bit.  Only GELU is compared within a bound (below).
  random  Gaussian A (std 0.5), W (0.03), bias (0.1), residual (1): realistic magnitudes and the GELU range.  c = sum_k a_k w_k
          accumulated in fp32 in any order (any tree over the K_r terms of a K range has depth < K_r) is within
              acc = K_r * u32 * sum_k |a_k w_k|                     (first order; all bounds carry a factor 1.001 for the rest)
          of the exact c.  Epilogues:
            partials      acc over the split's own K range, nothing else
            f32 residual  (c + b) + r: two fp32 adds           e = acc + 2 u32 (|c| + |b| + |r|)
            bf16 residual the same, then one bf16 rounding     hulp16(|y| + e) + e
            q, k, v       c + b: one add, * 1/8 exact          e = (acc + u32 (|c| + |b|)) * scale, then hulp16(|y| + e) + e
            GELU          x = c + b with e_x = acc + u32 (|c| + |b|); |gelu'| <= 1.13, so gelu64 moves by <= 1.13 e_x;
                          gelu_exact(x) itself is within delta(x) of gelu64(x):
                              5.1e-7                      the fit, as gelu_exact's comment documents
                            + |x| Phi(-z) (ln2 * 16 u32 * P(z) + 2 u32)
                                                          the fp32 evaluation of t = exp2(p(z)), z = min(|x|, 6): Horner with
                                                          eight fma (seven for the polynomial and the clamp's ordering give at
                                                          most 16 u32 relative to P(z) = sum |c_i| z^i), error of p enters
                                                          t relatively as ln2 * dp, the hardware exp2 adds 1 ulp = 2 u32; the
                                                          GELU value carries it as |x| * dt with t = Phi(-z) <= 1/2
                            + 3 u32 |gelu(x)|             1 - t, the product with x
                            + 1e-9 |x| beyond |x| = 6     the clamped tail, Phi(-6) = 1e-9
                          e = 1.13 e_x + delta(x), then hulp16(|g| + e) + e.  In the exact regime e_x = 0.

LAYERNORM  y = (v - mean) * rstd * gamma + beta in fp32 (two passes over registers), one bf16 rounding.  The inputs of form 1
  (partials + bias + residual) are multiples of 2^-10 whose sums stay below 2^24 units, so v is exact in fp32 in any order and
  the reference takes v in float64 from the same numbers (layernorm_data asserts it).  Counting the kernel's operations, with
  D = 16 the depth of its sums (<= 10 lane-local adds, 6 butterfly steps; 9 + 6 in the bf16-row kernel):
      mean:   H-term sum of depth D and a division           dm  <= (D + 1) u32 * mean|v|
      dev:    d_i = v_i - mean, one rounding                 |dd_i| <= dm + u32 |d_i|
      var:    squares (1), sum (D), the 2 u32 relative error of the d_i, division, + eps: (D + 7) u32 relative, and the common
              shift dm of every d_i, which cancels to first order (sum d_i = 0) and leaves dm^2:
                                                             theta <= (D + 7) u32 + dm^2 / (var + eps)
      rstd:   rsqrtf within 1 ulp                            rho <= theta / 2 + 2 u32
      y:      two products and one add (or one fma)          e = |gamma| rstd (dm + u32 |d|) + |d rstd gamma| (rho + 2 u32) + u32 |y|
  and the bound is hulp16(|y| + e) + e.  Rows of one constant c with c * H exact in fp32 have mean = c and d = 0 exactly, so
  the output must be bf16(beta) bit for bit.

MUTANTS are wrong versions of the reference (MUTANTS, LN_MUTANTS): tests/test_linear_cases_cpu.py shows that each one fails --
different bits in the exact regime, >= 3 x the bound in the random one.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

U32 = 2.0 ** -24
U16 = 2.0 ** -8
SLACK = 1.001                 # second-order terms of the first-order bounds: K u32 <= 2.5e-4
FILL32 = 0x7FC12345           # quiet-NaN payloads no kernel produces: the pre-fill of every output
FILL16 = 0x7FC5
EPI_QKV, EPI_GELU, EPI_RESID, EPI_RESID16, EPI_PART = 0, 1, 2, 3, 4        # hipenc_linear_ex's `epilogue`
EPI_NAMES = {0: "qkv", 1: "gelu", 2: "resid", 3: "resid16", 4: "part"}
REGIMES = ("exact", "random")
LN_REGIMES = ("random", "offset", "constant")
LN_SUM_DEPTH = 16
LN_EPS = 1e-5
GELU_LIPSCHITZ = 1.13         # max |d/dx x Phi(x)| = 1.1290
GELU_FIT = 5.1e-7
GELU_COEF = (-1.9448814327915898e-06, 6.385969027178362e-05, -0.0009488638024777174, 0.008582341484725475,
             -0.05411824584007263, -0.4582975208759308, -1.1513246297836304, -0.9999869465827942)   # gelu_exact, highest first


# ---- dispatch, restated from csrc/encoder_plan.h, csrc/encoder_gemm.h and csrc/gemm256.h ------------------------------------------------------------
def skinny_split(K: int) -> int:
    return (K + 1023) // 1024


def skinny_ok(K: int) -> bool:
    return K % (skinny_split(K) * 128) == 0


def skinny_plan(M: int, N: int, K: int) -> Dict[str, int]:
    """launch_skinny: split count, 16-column tiles per wave (NT), the all-loads-first form (FULL), row blocks per workgroup."""
    assert M % 64 == 0 and N % 16 == 0 and skinny_ok(K)
    sp = skinny_split(K)
    kc = K // sp
    steps = kc // 128
    wide = M >= 128 and N % 32 == 0
    gx = (N // (32 if wide else 16)) * sp
    mblocks = M // 64
    mb = max(1, (gx * mblocks + 1023) // 1024)
    gy = (mblocks + mb - 1) // mb
    return dict(split=sp, kc=kc, steps=steps, NT=2 if wide else 1, FULL=int(steps == 8), mb_per_wg=mb, gx=gx, gy=gy,
                last_group=mblocks - (gy - 1) * mb)


def tiled_plan(M: int, N: int, K: int, ksplit: int = 1) -> Dict[str, object]:
    """gemm_bf16_kernel's grid: tiles per split, the XCD remainder, the widths of its 8-column-tile groups, k-tiles per split."""
    assert M % 128 == 0 and N % 128 == 0 and K % (64 * ksplit) == 0
    nbn, nbm = N // 128, M // 128
    nblk = nbn * nbm
    groups = [min(8, nbn - g * 8) for g in range((nbn + 7) // 8)]
    return dict(tiles=nblk, xcd_rem=nblk & 7, groups=groups, nk=K // ksplit // 64, grid=nblk * ksplit)


def tile_split(H: int, M: int, K: int) -> int:
    """forward's split of the N = H products on the tiled path."""
    ks = 1
    while ks < 4 and (H // 128) * (M // 128) * ks < 512 and K % (ks * 128) == 0 and K // (ks * 2) >= 256:
        ks *= 2
    return ks


def g256_plan(M: int, N: int, K: int, n_cu: int, max_wg: int = 0) -> Dict[str, object]:
    """gemm256_kernel's persistent walk: grid, tile order, and how many tiles the workgroups own."""
    assert M % 256 == 0 and N % 256 == 0 and K % 128 == 0
    tiles = (M // 256) * (N // 256)
    grid = min(tiles, n_cu)
    if max_wg > 0:
        grid = min(grid, max_wg)
    owned = [len(range(v, tiles, grid)) for v in range(grid)]
    return dict(tiles=tiles, grid=grid, xcd_order=int(grid % 8 == 0), max_owned=max(owned), min_owned=min(owned), nk=K // 64)


# ---- number formats ---------------------------------------------------------------------------------------------------------
def bf16_bits(x) -> np.ndarray:
    """ONE round-to-nearest-even of fp32-representable values to bf16, as uint16 bit patterns."""
    x32 = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def bf16_values(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def f32_bits(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)).view(np.uint32).copy()


def f32_values(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint32).view(np.float32).astype(np.float64)


def hulp16(v) -> np.ndarray:
    v = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return np.exp2(np.floor(np.log2(v)) - 8.0)


def round_bound(y, e) -> np.ndarray:
    """|bf16(y_fp32) - y| for |y_fp32 - y| <= e."""
    return hulp16(np.abs(y) + e) + e


# ---- GELU -------------------------------------------------------------------------------------------------------------------
def gelu64(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    return x * 0.5 * torch.erfc(torch.from_numpy(-x / math.sqrt(2.0))).numpy()


def _phi_neg(z) -> np.ndarray:
    return 0.5 * torch.erfc(torch.from_numpy(np.asarray(z, dtype=np.float64) / math.sqrt(2.0))).numpy()


def gelu_delta(x) -> np.ndarray:
    """|gelu_exact(x) evaluated in fp32 - gelu64(x)|: the module docstring's delta(x)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    z = np.minimum(x, 6.0)
    P = np.zeros_like(z)
    for c in GELU_COEF:
        P = P * z + abs(c)
    t = _phi_neg(z)
    return (GELU_FIT + x * t * (math.log(2.0) * 16 * U32 * P + 2 * U32) + 3 * U32 * np.abs(gelu64(x)) + np.where(x > 6.0, 1e-9 * x, 0.0))


def gelu_fp32(x32: np.ndarray) -> np.ndarray:
    """gelu_exact operation for operation in numpy float32 (products and adds rounded separately instead of fused, exp2 from
    libm instead of the hardware's): a correct fp32 evaluation that the bound must let pass."""
    x32 = np.asarray(x32, dtype=np.float32)
    z = np.minimum(np.abs(x32), np.float32(6.0))
    p = np.full_like(z, np.float32(GELU_COEF[0]))
    for c in GELU_COEF[1:]:
        p = (p * z).astype(np.float32) + np.float32(c)
    t = np.exp2(p).astype(np.float32)
    return (x32 * np.where(x32 > 0, np.float32(1.0) - t, t)).astype(np.float32)


# ---- GEMM data --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=6)
def linear_data(regime: str, M: int, N: int, K: int) -> Dict[str, np.ndarray]:
    """a [M, K], w [N, K], resid [M, N]: float64 arrays of bf16-exact values; bias [N] float64 of fp32-exact values;
    c = a w^T and (random regime) absc = |a| |w|^T in float64."""
    assert regime in REGIMES
    seed = (0 if regime == "exact" else 1) * 1_000_003 + M * 7919 + N * 104729 + K
    rng = np.random.default_rng(seed)
    if regime == "exact":
        assert K <= 4096
        a = rng.integers(-8, 9, size=(M, K)).astype(np.float64)
        w = rng.integers(-8, 9, size=(N, K)).astype(np.float64) / 64.0
        bias = rng.integers(-8, 9, size=N).astype(np.float64) / 64.0
        resid = rng.integers(-8, 9, size=(M, N)).astype(np.float64)
    else:
        rb = lambda x: bf16_values(bf16_bits(x))
        a = rb(rng.standard_normal((M, K)) * 0.5)
        w = rb(rng.standard_normal((N, K)) * 0.03)
        bias = (rng.standard_normal(N) * 0.1).astype(np.float32).astype(np.float64)
        resid = rb(rng.standard_normal((M, N)))
    d = dict(a=a, w=w, bias=bias, resid=resid, c=a @ w.T, regime=regime, M=M, N=N, K=K)
    if regime == "exact":
        exactness_precondition(d)
    else:
        d["absc"] = np.abs(a) @ np.abs(w).T
    return d


def exactness_precondition(d) -> int:
    """The exact regime's claim, checked on the data: every operand is an integer number of its unit, bf16-exact, and the
    largest possible |sum| (all K products, the bias and the residual, in units of 2^-6) is below 2^24.  -> that maximum."""
    a, w, bias, resid = d["a"], d["w"], d["bias"], d["resid"]
    for arr, unit in ((a, 1.0), (w, 2.0 ** -6), (bias, 2.0 ** -6), (resid, 1.0)):
        q = arr / unit
        assert np.array_equal(q, np.round(q)) and np.abs(q).max() <= 8
    for arr in (a, w, resid):
        assert np.array_equal(bf16_values(bf16_bits(arr)), arr)
    worst = int(d["K"] * (np.abs(a).max() * np.abs(w * 64).max()) + np.abs(bias * 64).max() + np.abs(resid).max() * 64)
    assert worst < 2 ** 24, worst
    # q carries 1/8: still a multiple of 2^-9 with the same number of significant bits
    assert np.array_equal(f32_values(f32_bits(d["c"])), d["c"])
    return worst


def as_torch(d, dev=None):
    """The case's operands as the tensors the entry takes: a, w, resid bf16; bias f32."""
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt)
    out = dict(a=t(d["a"], torch.bfloat16), w=t(d["w"], torch.bfloat16), resid=t(d["resid"], torch.bfloat16),
               bias=t(d["bias"], torch.float32))
    return {k: (v.to(dev) if dev is not None else v) for k, v in out.items()}


# ---- GEMM reference, with mutants -------------------------------------------------------------------------------------------
MUTANTS = ("drop_kstep", "neighbour_chunk", "no_bias_group", "double_split", "missing_split", "wrong_last_range", "k_scaled",
           "v_untransposed", "v_shifted", "mask_last_row")
# which epilogues a mutant can be seen in
MUTANT_EPIS = {"drop_kstep": (0, 1, 2, 3, 4), "neighbour_chunk": (0, 1, 2, 3, 4), "no_bias_group": (0, 1, 2, 3),
               "double_split": ("partsum",), "missing_split": ("partsum",), "wrong_last_range": (4, "partsum"),
               "k_scaled": (0,), "v_untransposed": (0,), "v_shifted": (0,), "mask_last_row": (0, 1, 2, 4)}


def _qkv_scatter(y: np.ndarray, S: int, heads: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """[M, 3H] -> q, k [nseq, heads, S, 64] and vt [nseq, heads, 64, S]."""
    M = y.shape[0]
    H = heads * 64
    nseq = M // S
    q = y[:, :H].reshape(nseq, S, heads, 64).transpose(0, 2, 1, 3)
    k = y[:, H:2 * H].reshape(nseq, S, heads, 64).transpose(0, 2, 1, 3)
    vt = y[:, 2 * H:].reshape(nseq, S, heads, 64).transpose(0, 2, 3, 1)
    return np.ascontiguousarray(q), np.ascontiguousarray(k), np.ascontiguousarray(vt)


def linear_expected(d, epi, m_valid: Optional[int] = None, S: int = 64, heads: int = 0, ksplit: int = 1,
                    mutant: Optional[str] = None) -> Dict[str, Dict[str, object]]:
    """What hipenc_linear_ex must leave in each output buffer: name -> dict(kind 'f32' | 'bf16', ref float64 (the value BEFORE
    the one bf16 rounding, for bf16 outputs), bound (None = compare bits), written (bool mask; False = still the fill)).
    epi is an EPI_* code or "partsum": the partials of `ksplit` K ranges summed in split order, + bias + residual.
    `mutant` (one of MUTANTS) injects that defect into the computation."""
    assert mutant is None or (mutant in MUTANTS and epi in MUTANT_EPIS[mutant]), (mutant, epi)
    M, N, K, regime = d["M"], d["N"], d["K"], d["regime"]
    a, w, resid = d["a"], d["w"], d["resid"]
    bias = d["bias"].copy()
    m_valid = M if m_valid is None else m_valid
    exact = regime == "exact"
    nsp = ksplit if epi in (EPI_PART, "partsum") else 1
    kr = K // nsp
    ranges = [(s * kr, (s + 1) * kr) for s in range(nsp)]
    if mutant == "wrong_last_range" :
        lo, hi = ranges[-1]
        ranges[-1] = (lo - 64, hi - 64) if nsp > 1 else (lo, hi - 64)          # one k-tile early / short
    if nsp == 1 and mutant is None:
        parts, absparts = [d["c"]], [d.get("absc")]
    else:
        parts = [a[:, lo:hi] @ w[:, lo:hi].T for lo, hi in ranges]
        absparts = [None if exact else np.abs(a[:, lo:hi]) @ np.abs(w[:, lo:hi]).T for lo, hi in ranges]
    parts = [p.copy() for p in parts]
    if mutant == "drop_kstep":
        # the last 32-deep step of the last wave quarter of the last split, in one 16-column tile
        hi = ranges[-1][1]
        n0 = 16 * ((N // 16) // 2)
        parts[-1][:, n0:n0 + 16] -= a[:, hi - 32:hi] @ w[n0:n0 + 16, hi - 32:hi].T
    if mutant == "neighbour_chunk":
        # one 8-element chunk of one row's A fragment comes from the row below
        m, k0 = min(m_valid, M) - 2, ranges[0][0] + 8 * ((kr // 8) // 2)
        parts[0][m, :] += (a[m + 1, k0:k0 + 8] - a[m, k0:k0 + 8]) @ w[:, k0:k0 + 8].T
    if mutant == "no_bias_group":
        g0 = next(g for g in range(N // 4) if np.any(bias[4 * g:4 * g + 4] != 0))
        bias[4 * g0:4 * g0 + 4] = 0.0
    rowmask = np.arange(M) < m_valid
    if mutant == "mask_last_row":
        rowmask[m_valid - 1] = False
    acc = [None if exact else (hi - lo) * U32 * ap for (lo, hi), ap in zip(ranges, absparts)]

    if epi == EPI_PART:
        ref = np.stack([p[:m_valid] for p in parts])                             # [ksplit][m_valid][N]
        bound = None if exact else np.stack([x[:m_valid] for x in acc]) * SLACK + 1e-30
        wr = np.broadcast_to(rowmask[:m_valid, None], ref.shape).copy()
        return {"out": dict(kind="f32", ref=ref, bound=bound, written=wr)}
    if epi == "partsum":
        use = list(range(nsp))
        if mutant == "double_split":
            use = use + [nsp - 1]
        if mutant == "missing_split":
            use = use[:-1]
        ref = sum(parts[s] for s in use) + bias + resid
        bound = None
        if not exact:
            mag = sum(np.abs(p) for p in parts) + np.abs(bias) + np.abs(resid)
            bound = (sum(acc) + (nsp + 1) * U32 * mag) * SLACK
        return {"out": dict(kind="f32", ref=ref, bound=bound, written=np.broadcast_to(rowmask[:, None], ref.shape).copy())}

    c = parts[0]
    x = c + bias
    wr2 = np.broadcast_to(rowmask[:, None], x.shape).copy()
    if epi in (EPI_RESID, EPI_RESID16):
        y = x + resid
        e = None if exact else (acc[0] + 2 * U32 * (np.abs(c) + np.abs(bias) + np.abs(resid))) * SLACK
        if epi == EPI_RESID:
            return {"out": dict(kind="f32", ref=y, bound=e, written=wr2)}
        return {"out": dict(kind="bf16", ref=y, bound=None if exact else round_bound(y, e), written=wr2)}
    if epi == EPI_GELU:
        ex = 0.0 if exact else acc[0] + U32 * (np.abs(c) + np.abs(bias))
        y = gelu64(x)
        e = (GELU_LIPSCHITZ * ex + gelu_delta(x)) * SLACK
        return {"out": dict(kind="bf16", ref=y, bound=round_bound(y, e), written=wr2)}
    assert epi == EPI_QKV and N == 3 * heads * 64 and M % S == 0
    H = heads * 64
    scale = np.ones(N)
    scale[:H] = 0.125
    if mutant == "k_scaled":
        scale[H:2 * H] = 0.125
    y = x * scale
    outs = dict(zip(("q", "k", "vt"), _qkv_scatter(y, S, heads)))
    if mutant == "v_untransposed":
        nseq = M // S
        outs["vt"] = np.ascontiguousarray(outs["vt"].transpose(0, 1, 3, 2)).reshape(nseq, heads, 64, S)
    if mutant == "v_shifted":
        outs["vt"] = np.roll(outs["vt"], 8, axis=-1)
    wrs = dict(zip(("q", "k", "vt"), _qkv_scatter(wr2, S, heads)))
    if exact:
        bounds = dict(q=None, k=None, vt=None)
    else:
        e = (acc[0] + U32 * (np.abs(c) + np.abs(bias))) * scale * SLACK
        # the bound belongs to the TRUE layout: a mutant that moves values is measured against the bound of the place it hits
        ytrue = (c + d["bias"]) * np.where(np.arange(N) < H, 0.125, 1.0)
        bounds = dict(zip(("q", "k", "vt"), _qkv_scatter(round_bound(ytrue, e), S, heads)))
    return {n: dict(kind="bf16", ref=outs[n], bound=bounds[n], written=wrs[n]) for n in ("q", "k", "vt")}


def image_bits(exp: Dict[str, object]) -> np.ndarray:
    """The bit image of an expected output: its one rounding where written, the fill elsewhere (what a kernel computing
    exactly `ref` leaves behind) -- this is how a mutant's output is fed to `worst_ratio`."""
    if exp["kind"] == "f32":
        bits = f32_bits(exp["ref"])
        bits[~exp["written"]] = FILL32
    else:
        bits = bf16_bits(exp["ref"])
        bits[~exp["written"]] = FILL16
    return bits


def worst_ratio(exp: Dict[str, object], got_bits: np.ndarray) -> float:
    """How far `got_bits` (uint32 for f32 outputs, uint16 for bf16) is from what `exp` demands: inf if the set of elements
    that still hold the fill is not exactly the unwritten set (or a written value is not finite); with a bound the worst
    |got - ref| / bound; without one 0.0 for identical bits and inf otherwise."""
    f32 = exp["kind"] == "f32"
    got_bits = np.asarray(got_bits).reshape(exp["ref"].shape)
    assert got_bits.dtype == (np.uint32 if f32 else np.uint16)
    wr = exp["written"]
    if not np.array_equal(got_bits == (FILL32 if f32 else FILL16), ~wr):
        return math.inf
    if not wr.any():
        return 0.0
    if exp["bound"] is None:
        want = f32_bits(exp["ref"]) if f32 else bf16_bits(exp["ref"])
        return 0.0 if np.array_equal(got_bits[wr], want[wr]) else math.inf
    got = f32_values(got_bits) if f32 else bf16_values(got_bits)
    if not np.all(np.isfinite(got[wr])):
        return math.inf
    return float((np.abs(got[wr] - exp["ref"][wr]) / exp["bound"][wr]).max())


def shuffled_fp32_outputs(d, epi, S: int = 64, heads: int = 0, ksplit: int = 1, seed: int = 0) -> Dict[str, np.ndarray]:
    """A CORRECT evaluation in fp32: K in a shuffled order, accumulated 32 products at a time in float32, the epilogue in
    float32 -- the bit images it produces must pass `worst_ratio` against linear_expected."""
    M, N, K = d["M"], d["N"], d["K"]
    a32, w32 = d["a"].astype(np.float32), d["w"].astype(np.float32)
    b32, r32 = d["bias"].astype(np.float32), d["resid"].astype(np.float32)
    rng = np.random.default_rng(seed)
    nsp = ksplit if epi in (EPI_PART, "partsum") else 1
    kr = K // nsp
    parts = []
    for s in range(nsp):
        perm = s * kr + rng.permutation(kr)
        acc = np.zeros((M, N), dtype=np.float32)
        for i in range(0, kr, 32):
            kk = perm[i:i + 32]
            acc = (acc + a32[:, kk] @ w32[:, kk].T).astype(np.float32)
        parts.append(acc)
    if epi == EPI_PART:
        return {"out": np.stack(parts).view(np.uint32)}
    if epi == "partsum":
        t = parts[0]
        for p in parts[1:]:
            t = t + p
        return {"out": np.ascontiguousarray((t + b32) + r32).view(np.uint32)}
    x = parts[0] + b32
    if epi == EPI_RESID:
        return {"out": np.ascontiguousarray(x + r32).view(np.uint32)}
    if epi == EPI_RESID16:
        return {"out": bf16_bits(x + r32)}
    if epi == EPI_GELU:
        return {"out": bf16_bits(gelu_fp32(x))}
    sc = np.ones(N, dtype=np.float32)
    sc[:heads * 64] = 0.125
    return {n: bf16_bits(v) for n, v in zip(("q", "k", "vt"), _qkv_scatter(x * sc, S, heads))}


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------
LN_MUTANTS = ("var_over_padded_lanes", "ln16_partner_stats")


@functools.lru_cache(maxsize=8)
def layernorm_data(regime: str, form: int, M: int, H: int, nsplit: int = 1) -> Dict[str, np.ndarray]:
    """form 0: x f32 [M, H].  form 1: parts f32 [nsplit, M, H], bias f32 [H], resid bf16 [M, H], all multiples of 2^-10 (the
    residual of 2^-3) whose sum is exact in fp32 in any order.  form 2: x bf16 [M, H].  Everything as float64 arrays holding
    exactly representable values; v [M, H] is the exact row the kernel normalises; gamma, beta f32."""
    assert regime in LN_REGIMES and form in (0, 1, 2)
    rng = np.random.default_rng(17 + LN_REGIMES.index(regime) * 1000 + form * 100 + M * 31 + H * 7 + nsplit)
    gamma = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32).astype(np.float64)
    beta = (0.1 * rng.standard_normal(H)).astype(np.float32).astype(np.float64)
    d = dict(regime=regime, form=form, M=M, H=H, nsplit=nsplit, gamma=gamma, beta=beta)
    if regime == "constant":
        const = rng.integers(-24, 25, size=(M, 1)).astype(np.float64) / 8.0          # c * H exact in fp32
        base = np.broadcast_to(const, (M, H)).copy()
    elif regime == "offset":
        base = 100.0 + rng.standard_normal((M, H))
    else:
        base = rng.standard_normal((M, H))
    if form == 0:
        d["x"] = base.astype(np.float32).astype(np.float64)
        d["v"] = d["x"]
    elif form == 2:
        d["x"] = bf16_values(bf16_bits(base))
        d["v"] = d["x"]
    else:
        qz = lambda x, u: np.round(x / u) * u
        if regime == "constant":
            parts = [np.full((M, H), 0.25 * (s + 1)) for s in range(nsplit - 1)]
            bias = np.full(H, -0.5)
            resid = np.full((M, H), 1.5)
            parts.insert(0, base - sum(parts) - bias - resid if parts else base - bias - resid)
        else:
            parts = [qz(rng.standard_normal((M, H)) * 0.5, 2.0 ** -10) for _ in range(nsplit - 1)]
            bias = qz(rng.standard_normal(H) * 0.1, 2.0 ** -10)
            resid = qz(np.clip(rng.standard_normal((M, H)), -4, 4), 2.0 ** -3)
            parts.insert(0, qz(base, 2.0 ** -10) - sum(parts) - bias - resid if parts else qz(base, 2.0 ** -10) - bias - resid)
        d["parts"], d["bias"], d["resid"] = np.stack(parts), bias, resid
        d["v"] = sum(parts) + bias + resid
        terms = list(parts) + [np.broadcast_to(bias, (M, H)), resid]
        units = sum(np.abs(t) for t in terms) * 2.0 ** 10
        assert all(np.array_equal(t * 2.0 ** 10, np.round(t * 2.0 ** 10)) for t in terms) and units.max() < 2 ** 24
        assert np.array_equal(bf16_values(bf16_bits(resid)), resid)
        assert all(np.array_equal(f32_values(f32_bits(t)), t) for t in terms)
    if regime == "constant":
        c = d["v"][:, :1]
        assert np.array_equal(d["v"], np.broadcast_to(c, (M, H)))
        assert np.all(np.abs(c * 8) == np.round(np.abs(c * 8))) and np.abs(c * 8).max() * H < 2 ** 24     # every partial sum exact
    return d


def layernorm_expected(d, mutant: Optional[str] = None, eps: float = LN_EPS) -> Dict[str, object]:
    v, gamma, beta, H, M = d["v"], d["gamma"], d["beta"], d["H"], d["M"]
    mean = v.mean(axis=1, keepdims=True)
    dev = v - mean
    var = (dev * dev).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    y = dev * rstd * gamma + beta
    if d["regime"] == "constant":
        ref, bound = np.broadcast_to(beta, (M, H)).copy(), None
        assert np.array_equal(y, ref)
    else:
        D = LN_SUM_DEPTH
        dm = (D + 1) * U32 * np.abs(v).mean(axis=1, keepdims=True)
        theta = (D + 7) * U32 + dm * dm / (var + eps)
        rho = theta / 2 + 2 * U32
        e = (np.abs(gamma) * rstd * (dm + U32 * np.abs(dev)) + np.abs(dev * rstd * gamma) * (rho + 2 * U32) + U32 * np.abs(y)) * SLACK
        ref, bound = y, round_bound(y, e)
    if mutant == "var_over_padded_lanes":
        # the variance divided by the lanes' padded width (whole 256-float passes) instead of H
        padded = -(-H // 256) * 256
        ref = dev / np.sqrt((dev * dev).sum(axis=1, keepdims=True) / padded + eps) * gamma + beta
    elif mutant == "ln16_partner_stats":
        # the last real row normalised with the statistics of its neighbour in the wave's group of four
        assert M >= 2
        ref = ref.copy()
        ref[M - 1] = (v[M - 1] - mean[M - 2]) * rstd[M - 2] * gamma + beta
    else:
        assert mutant is None
    return dict(kind="bf16", ref=ref, bound=bound, written=np.ones((M, H), dtype=bool))


def layernorm_fp32_shuffled(d, seed: int = 0, eps: float = LN_EPS) -> np.ndarray:
    """A correct fp32 LayerNorm with the row in a shuffled order, summed as 64 lane-local chains and a butterfly (depth <=
    LN_SUM_DEPTH) -> bf16 bits in the original order."""
    v32 = d["v"].astype(np.float32)
    M, H = v32.shape
    perm = np.random.default_rng(seed).permutation(H)

    def tree(x):                                   # [M, H] in permuted order -> [M, 1] float32
        lanes = np.zeros((M, 64), dtype=np.float32)
        for chunk in x.reshape(M, -1, 64).transpose(1, 0, 2):
            lanes = (lanes + chunk).astype(np.float32)
        while lanes.shape[1] > 1:
            half = lanes.shape[1] // 2
            lanes = (lanes[:, :half] + lanes[:, half:]).astype(np.float32)
        return lanes
    pad = (-H) % 64
    xs = np.pad(v32[:, perm], ((0, 0), (0, pad)))
    mean = (tree(xs) / np.float32(H)).astype(np.float32)
    dev = (v32 - mean).astype(np.float32)
    var = (tree(np.pad((dev * dev).astype(np.float32)[:, perm], ((0, 0), (0, pad)))) / np.float32(H)).astype(np.float32)
    rstd = (np.float32(1.0) / np.sqrt(var + np.float32(eps))).astype(np.float32)
    y = ((dev * rstd).astype(np.float32) * d["gamma"].astype(np.float32)).astype(np.float32) + d["beta"].astype(np.float32)
    return bf16_bits(y)


# ---- the cases of tests/test_encoder_linear_gpu.py --------------------------------------------------------------------------
# Every case names the branch it is there for in `reach`: a subset of the plan (tiled_plan / g256_plan / skinny_plan) that
# both test files assert, so a change of the dispatch cannot silently move a case off its branch.
TILED_SHAPES = {
    # (M, N, K): what the shape is for
    (128, 128, 64): dict(tiles=1, nk=1, groups=[1]),                   # one tile, one k-tile: no prefetch at all
    (128, 128, 128): dict(tiles=1, nk=2),
    (128, 384, 64): dict(tiles=3, nk=1),                               # the smallest qkv shape: one head-pair per third
    (256, 1152, 192): dict(tiles=18, xcd_rem=2, groups=[8, 1], nk=3),  # last group of ONE column tile, XCD remainder
    (384, 1536, 256): dict(tiles=36, xcd_rem=4, groups=[8, 4]),
}
TILED_CASES: List[Dict[str, object]] = []
for (M_, N_, K_), reach_ in TILED_SHAPES.items():
    for epi_ in (EPI_QKV, EPI_GELU, EPI_RESID):
        if epi_ == EPI_QKV and N_ % 192 != 0:
            continue
        if epi_ != EPI_QKV and (M_, N_, K_) == (128, 384, 64):
            continue
        TILED_CASES.append(dict(M=M_, N=N_, K=K_, epi=epi_, heads=N_ // 192, S_list=tuple(s for s in (64, 128, 192) if M_ % s == 0),
                                m_valids=(M_, M_ - 64), reach=reach_))
TILED_PART_CASES = [
    dict(M=128, N=128, K=128, ksplit=2, m_valids=(128, 64), reach=dict(nk=1, grid=2)),          # one k-tile per split
    dict(M=128, N=256, K=512, ksplit=2, m_valids=(128, 64), reach=dict(nk=4, grid=4)),
    dict(M=256, N=256, K=1024, ksplit=4, m_valids=(256, 192), reach=dict(nk=4, grid=16)),
]
G256_CAPS = (0, 1, 5, 8, 16)
G256_SHAPES = {
    (256, 256, 128): dict(tiles=1, nk=2),                              # one tile at the smallest even nk
    (768, 768, 128): dict(tiles=9, nk=2),                              # nine tiles: the staging stream crosses tiles every 2 k-tiles
    (768, 768, 1024): dict(tiles=9, nk=16),
    (1536, 1024, 256): dict(tiles=24, nk=4),
}
G256_CASES: List[Dict[str, object]] = []
for (M_, N_, K_), reach_ in G256_SHAPES.items():
    for epi_ in (EPI_QKV, EPI_GELU, EPI_RESID, EPI_RESID16):
        if epi_ == EPI_QKV and N_ != 768:
            continue
        masks = (M_, M_ - 64, M_ - 192) if epi_ in (EPI_QKV, EPI_GELU) else (M_,)     # the residual epilogues never mask
        G256_CASES.append(dict(M=M_, N=N_, K=K_, epi=epi_, heads=4, S_list=(64, 128, 192), m_valids=masks, reach=reach_))
# what the caps make of 9 and of 24 tiles on a device with >= 24 CUs: (grid, xcd_order, max_owned, min_owned)
G256_WALKS = {9: {0: (9, 0, 1, 1), 1: (1, 0, 9, 9), 5: (5, 0, 2, 1), 8: (8, 1, 2, 1), 16: (9, 0, 1, 1)},
              24: {0: (24, 1, 1, 1), 1: (1, 0, 24, 24), 5: (5, 0, 5, 4), 8: (8, 1, 3, 3), 16: (16, 1, 2, 1)},
              1: {c: (1, 0, 1, 1) for c in G256_CAPS}}
SKINNY_CASES = [
    # NT = 1 (<= 64 rows: the single query), each K form
    dict(M=64, N=384, K=128, epi=EPI_QKV, heads=2, S=64, reach=dict(NT=1, steps=1, FULL=0, split=1)),
    dict(M=64, N=80, K=384, epi=EPI_GELU, reach=dict(NT=1, steps=3, FULL=0, split=1)),
    dict(M=64, N=768, K=1024, epi=EPI_QKV, heads=4, S=64, reach=dict(NT=1, FULL=1, split=1)),
    dict(M=64, N=1024, K=4096, epi=EPI_PART, reach=dict(NT=1, FULL=1, split=4)),                # one query's F -> H product
    dict(M=64, N=48, K=1536, epi=EPI_PART, reach=dict(NT=1, FULL=0, split=2, steps=6)),
    # NT = 2 from 128 rows; N = 16 * odd keeps NT = 1 there
    dict(M=128, N=768, K=384, epi=EPI_QKV, heads=4, S=128, reach=dict(NT=2, steps=3, FULL=0)),
    dict(M=128, N=384, K=1024, epi=EPI_QKV, heads=2, S=64, reach=dict(NT=2, FULL=1)),
    dict(M=128, N=80, K=1536, epi=EPI_PART, reach=dict(NT=1, FULL=0, split=2)),
    dict(M=128, N=1024, K=1024, epi=EPI_GELU, reach=dict(NT=2, FULL=1, split=1)),
    dict(M=128, N=1024, K=2048, epi=EPI_PART, reach=dict(NT=2, FULL=1, split=2)),
    dict(M=128, N=768, K=1536, epi=EPI_PART, reach=dict(NT=2, FULL=0, split=2)),
    dict(M=192, N=768, K=128, epi=EPI_QKV, heads=4, S=192, reach=dict(NT=2, steps=1)),
    dict(M=192, N=768, K=4096, epi=EPI_PART, reach=dict(NT=2, FULL=1, split=4)),
    dict(M=192, N=1024, K=384, epi=EPI_GELU, reach=dict(NT=2, steps=3)),
    # more than 1024 workgroup-row-blocks: two row blocks per workgroup, the last workgroup row has one
    dict(M=2624, N=1024, K=1024, epi=EPI_GELU, reach=dict(NT=2, FULL=1, mb_per_wg=2, gy=21, last_group=1)),
    dict(M=2624, N=1024, K=1024, epi=EPI_PART, reach=dict(NT=2, FULL=1, mb_per_wg=2, gy=21, last_group=1, split=1)),
]
LN_CASES = ([dict(form=f, H=H, M=M, nsplit=ns) for f in (0, 1) for H in (128, 256, 384, 1024, 2048) for M in (1, 5, 64)
             for ns in ((1,) if f == 0 else (1, 2, 3, 4))]
            + [dict(form=2, H=H, M=M, nsplit=1) for H in (128, 512, 640, 1024) for M in (1, 4, 5, 18)])
# the exact-regime chain: partials then LayerNorm form 1 == fp32 residual epilogue then form 0, bit for bit
CHAIN_CASES = [dict(M=128, N=256, K=512, ksplit=2, impl=1), dict(M=256, N=256, K=1024, ksplit=4, impl=1),
               dict(M=128, N=384, K=768, ksplit=3, impl=1), dict(M=128, N=1024, K=2048, ksplit=2, impl=3),
               dict(M=128, N=256, K=4096, ksplit=4, impl=3)]


def assert_reach(plan: Dict[str, object], reach: Dict[str, object], what) -> None:
    for k, v in reach.items():
        assert plan[k] == v, (what, k, plan[k], v)
