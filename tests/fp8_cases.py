"""
tests/fp8_cases.py -- cases, an independent restatement and mutants for the fp8 format of the multi-vector store
(csrc/multivec.h; hiprag.colbert.fp8_quantize_reference is the specification), shared by the CPU test (which proves that the
cases can fail) and the GPU tests.  Nothing here is fitted to what the GPU gives.

`quantize` restates the format in integer numpy, without torch's cast: the CPU test holds it equal to the reference on every
case, so the rounding has two independent statements.  Its mutants are the mistakes a kernel can make:
    truncate      the three mantissa bits cut, not rounded to nearest even
    e_plus_one    e one too large (amax * 2^e in [256, 512): codes above 256, one bit of range wasted the other way)
    e_minus_one   e one too small (amax * 2^e in [64, 128): a bit of precision lost)
    amax_first_64 amax over the first 64 components only (a wave that forgets the other lanes)
    amax_first_128 amax over the first 128 components only (a reduction that stops short of the lanes 8 and up; at 128-d it
                  is the format itself, so it is not in MUTANTS, whose members every 128-d case set must catch)
    keep_neg_zero a -0 code stays 0x80
    scale_is_2e   the scale stored as 2^e, not 2^-e

THE ERROR BOUND: a code has 3 mantissa bits, so RNE moves a normal value by at most 2^-4 of itself; below the smallest normal
code the codes are multiples of 2^-9, half a step is 2^-10, times the scale:  |v - deq| <= max(2^-4 |v|, 2^-10 scale).

MAXSIM over an fp8 store is, bit for bit, MaxSim over a bf16 store of the dequantised vectors; against the float64 reference
of the ORIGINAL vectors the score is then within colbert_cases' accumulation bound on the dequantised vectors plus what the
quantisation moves a dot product by, mean_i max_j sum_k |q_ik| max(2^-4 |d_jk|, 2^-10 scale_j)  (|max_j a - max_j b| <=
max_j |a - b|, and the mean of maxima moves by at most the mean of those).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from colbert_cases import csr_of, maxsim_vectors
from oracle.linear_cases import bf16_bits, bf16_values

AMAX_LO, AMAX_HI = 67 << 7, 187 << 7        # bf16 magnitude bits of 2^-60 and 2^60
MUTANTS = ("truncate", "e_plus_one", "e_minus_one", "amax_first_64", "keep_neg_zero", "scale_is_2e")
WIDE_MUTANTS = ("amax_first_128",)           # slips that only a vector wider than 128 can show


def _e4m3(x: np.ndarray, truncate: bool = False) -> np.ndarray:
    """fp32 values, |x| < 512 -> e4m3fn codes in integer arithmetic (RNE, or the mantissa cut).  Values above 448 cannot
    arise from the format (only from the mutant e_plus_one, where they saturate to 0x7E)."""
    f = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    sign, a = (f >> 24) & 0x80, f & 0x7FFFFFFF
    keep, rem = (a >> 20) - (120 << 3), a & 0xFFFFF
    up = np.zeros_like(keep) if truncate else ((rem > 0x80000) | ((rem == 0x80000) & ((keep & 1) == 1))).astype(np.int64)
    normal = np.minimum(keep + up, 0x7E)
    units = np.abs(np.ascontiguousarray(x, dtype=np.float64)) * 512.0          # multiples of 2^-9 below the smallest normal code
    sub = (np.floor(units) if truncate else np.rint(units)).astype(np.int64)   # np.rint rounds half to even
    code = np.where(a >= 0x3C800000, normal, np.minimum(sub, 8))
    return (sign | code).astype(np.uint8)


def quantize(bits, mutant: Optional[str] = None):
    """bf16 bits uint16 [n, dim] -> (codes uint8 [n, dim], scales float32 [n]): the format, or one of MUTANTS."""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    n, dim = b.shape
    mag = (b & 0x7FFF).astype(np.int64)
    seen = {"amax_first_64": 64, "amax_first_128": 128}.get(mutant, dim)
    amax = mag[:, :seen].max(axis=1) if n else np.zeros(0, np.int64)
    ok = (amax >= AMAX_LO) & (amax <= AMAX_HI) & (mag.max(axis=1) < 0x7F80 if n else True)
    codes, scales = np.zeros((n, dim), np.uint8), np.ones(n, np.float32)
    e = 134 - (amax[ok] >> 7) + {"e_plus_one": 1, "e_minus_one": -1}.get(mutant, 0)
    scaled = (bf16_values(b[ok]).astype(np.float64) * np.ldexp(1.0, e)[:, None]).astype(np.float32)      # exact
    c = _e4m3(np.clip(scaled, -511.0, 511.0), truncate=mutant == "truncate")
    if mutant != "keep_neg_zero":
        c[c == 0x80] = 0
    codes[ok] = c
    scales[ok] = np.ldexp(1.0, e if mutant == "scale_is_2e" else -e).astype(np.float32)
    return codes, scales


def code_values(codes) -> np.ndarray:
    """e4m3fn codes -> float64 values, from the bit fields (no torch): NaN patterns give nan."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    ex, man = (c >> 3) & 15, c & 7
    v = np.where(ex > 0, np.ldexp(1.0 + man / 8.0, ex - 7), man * 2.0 ** -9)
    v = np.where((c & 0x7F) == 0x7F, np.nan, v)
    return np.where(c & 0x80, -v, v)


def dequantized(codes, scales) -> np.ndarray:
    """float64 code * scale."""
    return code_values(codes) * np.asarray(scales, dtype=np.float64).reshape(-1, 1)


def error_ratio(bits, codes, scales) -> float:
    """worst |v - deq| / max(2^-4 |v|, 2^-10 scale) over the vectors the domain guard lets through (0.0 = exact)."""
    v = bf16_values(np.asarray(bits, dtype=np.uint16)).astype(np.float64)
    s = np.asarray(scales, dtype=np.float64).reshape(-1, 1)
    bound = np.maximum(np.abs(v) / 16.0, s / 1024.0)
    return float((np.abs(v - dequantized(codes, scales)) / bound).max()) if v.size else 0.0


# ---- cases ---------------------------------------------------------------------------------------------------------------
def sweep_vectors(amax_bits: int, dim: int = 128) -> np.ndarray:
    """Vectors whose first component is amax (it fixes e) and whose other components sweep EVERY bf16 bit pattern of magnitude
    <= amax, both signs, -0 included; the last vector is filled up with +0."""
    mags = np.arange(amax_bits + 1, dtype=np.uint16)
    pats = np.concatenate([mags, mags | 0x8000])
    per = dim - 1
    n = -(-len(pats) // per)
    body = np.zeros(n * per, dtype=np.uint16)
    body[:len(pats)] = pats
    out = np.empty((n, dim), dtype=np.uint16)
    out[:, 0] = amax_bits
    out[:, 1:] = body.reshape(n, per)
    return out


# 1.0 (257 vectors of dim 128 hold every pattern up to it; no amax inside the domain fills 512), and more amax values on
# binade edges: the bf16 just below 1.0, which is 255/256 (ONE value in bf16: it scales to 255, the top of [128, 256)), 0.5,
# and the largest bf16 of the domain's lowest binade, just below 2^-59.  About 910 vectors in all.
SWEEP_AMAX = (0x3F80, 0x3F7F, 0x3F00, (68 << 7) - 1)


def exhaustive_vectors(dim: int = 128) -> np.ndarray:
    return np.concatenate([sweep_vectors(a, dim) for a in SWEEP_AMAX])


def special_vectors(dim: int = 128) -> np.ndarray:
    """Zero, -0, values that round to -0, ties, non-finite components and both edges of the domain, one vector each."""
    f = lambda *vals: bf16_bits(np.asarray(list(vals) + [0.0] * (dim - len(vals)), dtype=np.float32))
    rows = [
        f(),                                                    # the zero vector: codes 0x00, scale 1.0
        np.full(dim, 0x8000, np.uint16),                        # all -0: amax == 0 too
        f(1.0, -0.0, -2.0 ** -20, 2.0 ** -20),                  # -0 and values that round to -0 / +0 beside amax = 1
        f(1.0, 17 / 128, 19 / 128, -17 / 128, 21 / 128, 23 / 128),        # ties between normal codes (16|18, 18|20, 20|24 ..)
        f(1.0, 2.0 ** -17, 3 * 2.0 ** -17, 5 * 2.0 ** -17, -3 * 2.0 ** -17, 15 * 2.0 ** -17, 2.0 ** -18),   # ties between subnormal codes
        f(255 / 256, 1 / 256, -1 / 512),                        # amax scales to 255: RNE takes it to 256 = 0x78
        f(1.0, float("inf")), f(0.5, float("-inf")), f(0.25, float("nan")),   # non-finite: the zero vector, counted
        f(2.0 ** 60, 2.0 ** 57, -2.0 ** 53), f(2.0 ** -60, -2.0 ** -63),      # the edges of the domain: inside
        f(2.0 ** 60 * 1.0078125), f(2.0 ** 61), f(2.0 ** -61), f(2.0 ** -60 * 0.99609375),   # just outside: the zero vector, counted
        np.asarray([0x0001] + [0] * (dim - 1), np.uint16),      # a bf16 subnormal: outside
        f(*([0.0] * 64 + [1.0])) | f(2.0 ** -8),                # amax behind the first 64 components
    ]
    return np.stack([np.asarray(r, dtype=np.uint16) for r in rows])


N_GUARDED_SPECIAL = 8       # of special_vectors: 3 non-finite + 4 just outside + the subnormal


def unit_vectors(n: int, dim: int, seed: int) -> np.ndarray:
    return bf16_bits(maxsim_vectors("random", n, dim, seed))


def integer_vectors(n: int, dim: int, seed: int) -> np.ndarray:
    return bf16_bits(maxsim_vectors("exact", n, dim, seed))


def mixed_docs(lens: Sequence[int], dim: int, seed: int) -> List[np.ndarray]:
    """Documents of bf16 bits for the store tests: Gaussian vectors, every one at its own power-of-two magnitude in 2^-20 ..
    2^20 (so the scales differ), a zero vector and a guarded one now and then."""
    rng = np.random.default_rng(seed)
    docs = []
    for n in lens:
        v = rng.standard_normal((n, dim)) * np.ldexp(1.0, rng.integers(-20, 21, size=(n, 1)))
        b = bf16_bits(v.astype(np.float32))
        kind = rng.integers(0, 12, size=n)
        b[kind == 0] = 0
        b[kind == 1, 3] = 0x7F80                                 # +inf: guarded
        docs.append(b)
    return docs


def fp8_csr_of(docs, dim: int, cap: int):
    """What an fp8 store holds: (offsets, codes, scales) of the reference quantisation of csr_of's vectors."""
    from hiprag import fp8_quantize_reference
    off, vecs = csr_of(docs, dim, cap)
    codes, scales = fp8_quantize_reference(vecs)
    return off, codes, scales


def guarded_count(vecs) -> int:
    """Vectors the domain guard stores as zero: amax != 0 and (non-finite or outside the domain)."""
    v = np.asarray(vecs, dtype=np.uint16)
    if v.size == 0:
        return 0
    amax = (v.reshape(-1, v.shape[-1]) & 0x7FFF).max(axis=1)
    return int(((amax != 0) & ((amax < AMAX_LO) | (amax > AMAX_HI))).sum())
