"""
tests/mxfp4_cases.py -- cases, an independent restatement and mutants for the MXFP4 format of the multi-vector store
(csrc/multivec.h; hiprag.colbert.mxfp4_quantize_reference is the specification), shared by the CPU test (which proves that the
cases can fail) and the GPU tests.  Nothing here is fitted to what the GPU gives.

`quantize` restates the format in integer numpy on the bf16 bit fields.  The reference counts the midpoints a scaled magnitude
has passed; this one rounds to the nearest EVEN multiple of the step of the value's binade (0.5 below 2, 1 in [2, 4), 2 in
[4, 8)) and then saturates -- two statements of the rounding that the CPU test holds equal on every case.  Its mutants are the
mistakes a kernel can make:
    truncate        the mantissa bit cut, not rounded
    e_plus_one      E one too large (the scaled block maximum in [2, 4): a bit of precision lost)
    e_minus_one     E one too small (the scaled block maximum in [8, 16): everything above 7 saturates)
    no_saturation   a scaled value in [7, 8) rounds up to 8, magnitude index 8: the nibble 0x8, the sign bit
    bmax_first_16   the block maximum over the first 16 components of a block only (half its lanes forgotten)
    vector_scale    one scale for the whole vector, from amax
    nibbles_swapped component 2i in the high nibble
    keep_neg_zero   a -0 code stays 0x8
    scale_unbiased  the scale byte is E, not E + 127
    no_floor        E not clamped at -100

THE ERROR BOUND:  |v - deq| <= max(|v| / 4, 2^(E - 2)).  A normal code has one mantissa bit, so half a step is at most a quarter
of the value; below scaled 1 the codes are multiples of 1/2, half a step is 1/4, times 2^E; a saturated scaled value x in
[7, 8) moves by x - 6 < x / 4.

MAXSIM over an MXFP4 store is, bit for bit, MaxSim over a bf16 store of the dequantised vectors; against the float64 reference
of the ORIGINAL vectors the score is then within colbert_cases' accumulation bound on the dequantised vectors plus what the
quantisation moves a dot product by, mean_i max_j sum_k |q_ik| max(|d_jk| / 4, 2^(E_jb - 2)), b the block of k
(|max_j a - max_j b| <= max_j |a - b|, and the mean of maxima moves by at most the mean of those).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from colbert_cases import csr_of, maxsim_vectors
from fp8_cases import guarded_count, mixed_docs  # noqa: F401  (the guard and the store documents are the fp8 format's)
from oracle.linear_cases import bf16_bits, bf16_values

AMAX_LO, AMAX_HI = 67 << 7, 187 << 7        # bf16 magnitude bits of 2^-60 and 2^60
BLOCK = 32
E_MIN = -100
MUTANTS = ("truncate", "e_plus_one", "e_minus_one", "no_saturation", "bmax_first_16", "vector_scale", "nibbles_swapped",
           "keep_neg_zero", "scale_unbiased", "no_floor")
_CODE_OF_QUARTERS = np.full(33, -1, dtype=np.int64)                                # a code's magnitude in quarters -> its index
_CODE_OF_QUARTERS[[0, 2, 4, 6, 8, 12, 16, 24, 32]] = np.arange(9)                  # (8.0 = index 8 only under no_saturation)


def quantize(bits, mutant: Optional[str] = None):
    """bf16 bits uint16 [n, dim] -> (codes uint8 [n, dim / 2], scales uint8 [n, dim / 32]): the format, or one of MUTANTS."""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    n, dim = b.shape
    nb = dim // BLOCK
    mag = (b & 0x7FFF).astype(np.int64).reshape(n, nb, BLOCK)
    neg = (b >> 15).astype(np.int64).reshape(n, nb, BLOCK)
    amax = mag.max(axis=(1, 2)) if n else np.zeros(0, np.int64)
    ok = (amax >= AMAX_LO) & (amax <= AMAX_HI)
    bmax = mag[:, :, :16].max(axis=2) if mutant == "bmax_first_16" else mag.max(axis=2)
    if mutant == "vector_scale":
        bmax = np.broadcast_to(amax[:, None], (n, nb)).copy()
    some = ok[:, None] & (bmax != 0)
    E = (bmax >> 7) - 129 + {"e_plus_one": 1, "e_minus_one": -1}.get(mutant, 0)
    if mutant != "no_floor":
        E = np.maximum(E, E_MIN)
    scales = np.where(some, (E if mutant == "scale_unbiased" else E + 127) & 0xFF, 127).astype(np.uint8)
    # a bf16 magnitude is m * 2^(ex - 134), m = 128 + mantissa (ex >= 1) or the mantissa alone at ex = 1 (subnormal); scaled
    # by 2^-E and counted in quarters it is m * 2^sh: an integer number of quarters and whether anything lies behind it
    ex = mag >> 7
    m = np.where(ex > 0, 128 + (mag & 0x7F), mag & 0x7F)
    sh = np.clip(np.maximum(ex, 1) - 132 - E[:, :, None], -62, 40)
    up_sh, down_sh = np.maximum(sh, 0), np.maximum(-sh, 0)
    quarters = np.minimum((m << up_sh) >> down_sh, 1 << 20)
    sticky = (m & ((np.int64(1) << down_sh) - 1)) != 0
    step = np.where(quarters < 8, 2, np.where(quarters < 16, 4, 8))
    whole, rest = quarters // step, quarters % step
    if mutant == "truncate":
        up = np.zeros_like(whole)
    else:
        half = step // 2
        up = ((rest > half) | ((rest == half) & (sticky | (whole % 2 == 1)))).astype(np.int64)
    rounded = (whole + up) * step
    rounded = np.minimum(rounded, 32 if mutant == "no_saturation" else 24)
    idx = _CODE_OF_QUARTERS[rounded]
    assert np.all(idx >= 0)
    sign = neg * 8 if mutant == "keep_neg_zero" else np.where(idx != 0, neg * 8, 0)
    code = np.where(some[:, :, None], idx | sign, 0).reshape(n, dim).astype(np.uint8)
    lo, hi = (code[:, 1::2], code[:, 0::2]) if mutant == "nibbles_swapped" else (code[:, 0::2], code[:, 1::2])
    return (lo | (hi << 4)).astype(np.uint8), scales


def nibbles(codes) -> np.ndarray:
    """codes uint8 [n, dim / 2] -> the nibbles uint8 [n, dim] in component order"""
    c = np.asarray(codes, dtype=np.uint8)
    out = np.empty((c.shape[0], 2 * c.shape[1]), dtype=np.uint8)
    out[:, 0::2], out[:, 1::2] = c & 15, c >> 4
    return out


def dequantize(codes, scales) -> np.ndarray:
    """bf16 bits uint16 [n, dim] of code * 2^(scale byte - 127), put together from the bit fields: a code's exponent (0.5 has
    -1) plus the scale byte is the bf16 exponent field, its mantissa bit the top mantissa bit.  A zero code is +0."""
    nib = nibbles(codes).astype(np.int64)
    n, dim = nib.shape
    byte = np.repeat(np.asarray(scales, dtype=np.uint8).astype(np.int64), BLOCK, axis=1)
    idx = nib & 7
    e_code = np.asarray([0, -1, 0, 0, 1, 1, 2, 2])[idx]
    man = np.asarray([0, 0, 0, 1, 0, 1, 0, 1])[idx]
    field = e_code + byte
    assert np.all((idx == 0) | ((field >= 1) & (field <= 254))), "code * 2^E is no normal bf16"
    out = np.where(idx == 0, 0, ((nib >> 3) << 15) | (field << 7) | (man << 6))
    return out.astype(np.uint16)


def block_exponents(scales) -> np.ndarray:
    """E per component, float64 [n, dim]"""
    return np.repeat(np.asarray(scales, dtype=np.uint8).astype(np.float64) - 127.0, BLOCK, axis=1)


def error_bound(bits, scales) -> np.ndarray:
    """max(|v| / 4, 2^(E - 2)) per component, float64 [n, dim]"""
    v = bf16_values(np.asarray(bits, dtype=np.uint16)).astype(np.float64)
    return np.maximum(np.abs(v) / 4.0, np.exp2(block_exponents(scales) - 2.0))


def error_ratio(bits, codes, scales) -> float:
    """worst |v - deq| / max(|v| / 4, 2^(E - 2)) over vectors the domain guard lets through (0.0 = exact)"""
    v = bf16_values(np.asarray(bits, dtype=np.uint16)).astype(np.float64)
    deq = bf16_values(dequantize(codes, scales)).astype(np.float64)
    return float((np.abs(v - deq) / error_bound(bits, scales)).max()) if v.size else 0.0


def maxsim_quant_bound(q, d_bits, scales) -> float:
    """mean_i max_j sum_k |q_ik| max(|d_jk| / 4, 2^(E - 2)): what quantising document d (bits [Ld, dim], its scale bytes) can
    move its MaxSim score with query q float64 [Lq, dim] by"""
    return float((np.abs(np.asarray(q, dtype=np.float64)) @ error_bound(d_bits, scales).T).max(axis=1).mean())


# ---- cases ---------------------------------------------------------------------------------------------------------------
def unit_vectors(n: int, dim: int, seed: int) -> np.ndarray:
    return bf16_bits(maxsim_vectors("random", n, dim, seed))


def integer_vectors(n: int, dim: int, seed: int) -> np.ndarray:
    return bf16_bits(maxsim_vectors("exact", n, dim, seed))


TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)          # scaled midpoints between neighbouring codes
TIES_ROUND_TO = (0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0)     # the neighbour with the even mantissa
SATURATING = (6.5, 7.0, 7.96875)                        # scaled block maxima above 6: 7.96875 is the largest bf16 below 8


def special_rows(dim: int = 128) -> Dict[str, np.ndarray]:
    """name -> vector.  Components are given per block of 32, the rest of a block is +0."""
    nb = dim // BLOCK

    def blocks(*per_block):
        v = np.zeros((nb, BLOCK), dtype=np.float32)
        for i, vals in enumerate(per_block):
            v[i, :len(vals)] = vals
        return bf16_bits(v.reshape(dim))

    def late(maximum, *others):       # a block whose maximum sits at position 20, behind the first 16
        vals = [0.0] * BLOCK
        vals[20] = maximum
        vals[:len(others)] = others
        return vals

    ties = list(TIES) + [-t for t in TIES]
    subnormal = blocks([1.0, -0.3, 0.7], [], [], [2.0 ** -5, 3 * 2.0 ** -7])
    subnormal[BLOCK:2 * BLOCK] = np.arange(1, BLOCK + 1, dtype=np.uint16) * 3 | (np.arange(BLOCK, dtype=np.uint16) % 2) << 15
    return {
        "zero": blocks(),
        "neg_zero": np.full(dim, 0x8000, np.uint16),
        "to_neg_zero": blocks([4.0, -0.0, -0.1, -0.25, 0.1, -0.26]),                   # -0.1 and the tie -0.25 round to -0: stored 0x0
        "ties": blocks([4.0] + ties, [2.0 ** -7 * t for t in [4.0] + ties], [-6.0] + ties),
        "saturation": blocks(late(6.5, 5.5, -6.25, 7.0 - 2.0 ** -5), late(-7.0, 6.75, 5.0, 3.0), late(7.96875, -7.5, 7.25, 0.25),
                             late(2.0 ** 9 * 7.96875, 2.0 ** 9 * 7.0, -2.0 ** 9 * 6.5)),
        "inf": blocks([1.0, float("inf")]),
        "neg_inf": blocks([0.5], [float("-inf")]),
        "nan": blocks([0.25], [], [float("nan")]),
        "amax_2^60": blocks([2.0 ** 60, 2.0 ** 58 * 1.5, -2.0 ** 57], [2.0 ** 20]),     # the edges of the domain: inside
        "amax_2^-60": blocks([2.0 ** -60, -2.0 ** -62 * 1.5], [2.0 ** -61]),
        "above": blocks([2.0 ** 60 * 1.0078125]),                                       # just outside: the zero vector, counted
        "above_2": blocks([1.0], [], [], [2.0 ** 61]),
        "below": blocks([2.0 ** -60 * 0.99609375]),
        "below_2": blocks([2.0 ** -61], [2.0 ** -70]),
        "only_subnormal": np.asarray([0x0001] + [0] * (dim - 1), np.uint16),            # a bf16 subnormal amax: outside
        "subnormal_block": subnormal,                                                   # normal | bf16 subnormals | zero | normal
        "floor": blocks([2.0 ** -50, 2.0 ** -52], [2.0 ** -110, -2.0 ** -112], [1.5 * 2.0 ** -99, 2.0 ** -100, -2.0 ** -101],
                        [1.5 * 2.0 ** -98, -2.0 ** -99]),                               # block maxima below, at and above 2^-98
    }


def special_vectors(dim: int = 128) -> np.ndarray:
    return np.stack([np.asarray(r, dtype=np.uint16) for r in special_rows(dim).values()])


N_GUARDED_SPECIAL = 8       # inf, neg_inf, nan, above, above_2, below, below_2, only_subnormal


def position_vectors(dim: int) -> np.ndarray:
    """dim vectors: vector p is 2^-6 everywhere (alternating signs) but 1.0 at component p.  Block p / 32 then has E = -2
    (scale byte 125) and every other block E = -8 (byte 119), whichever lane holds p."""
    v = np.full((dim, dim), 2.0 ** -6, dtype=np.float32)
    v[:, 1::2] *= -1
    v[np.arange(dim), np.arange(dim)] = 1.0
    return bf16_bits(v)


def mxfp4_csr_of(docs, dim: int, cap: int):
    """What an MXFP4 store holds: (offsets, codes, scales) of the reference quantisation of csr_of's vectors."""
    from hiprag import mxfp4_quantize_reference
    off, vecs = csr_of(docs, dim, cap)
    codes, scales = mxfp4_quantize_reference(vecs)
    return off, codes, scales
