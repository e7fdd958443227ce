"""
tests/colbert_cases.py -- data, float64 references, derived bounds and mutants for the ColBERT head (hipenc_colbert_rows,
hipenc_forward_colbert), the multi-vector store and MaxSim (hipmaxsim_*), shared by the CPU test (which proves that the
checks can fail) and the GPU tests.  oracle/linear_cases.py is the model: nothing here is fitted to what the GPU gives; every
bound comes from the float64 reference and the number formats (U32 = 2^-24, SLACK for the second-order terms).

THE HEAD   v = x W^T + b, y = bf16(v / max(||v||, 1e-12)).
  exact    x integers in [-2, 2], W integers in [-1, 1] * 2^-6, b integers in [-8, 8] * 2^-6 (inside the [-8, 8] ranges of
           linear_cases; narrower so that the squares stay exact too).  In units of 2^-6 every partial sum of a row's products
           and the bias is an integer below 2^24, so v is exact in fp32 in any order and split; v^2 is an integer of units 2^-12
           below 2^24, and so is every partial sum of a row's squares: ss is exact in any order (head_data asserts all three).
           sqrt and the division are correctly rounded, so the output must equal colbert_reference bit for bit.
  random   Gaussian rows (std 0.5), W (0.03), b (0.1).  c accumulated in fp32 in any order is within H * U32 * sum|x_k w_k| of
           the exact value, the bias add rounds once:  e = (H U32 sum|x_k w_k| + U32 (|c| + |b|)) SLACK  on v.  Through the
           normalisation y = v / ||v||:  | d y_n | <= e_n / ||v|| + |y_n| * ||e||_2 / ||v|| (the norm moves by at most ||e||_2),
           and sqrt, the division and the product round once each, 3 U32 |y_n|:
               e_y = e / ||v|| + |y| ||e||_2 / ||v|| + 3 U32 |y|,  then one bf16 rounding: hulp16(|y| + e_y) + e_y.

MAXSIM     score = mean_i max_j q_i . d_j.
  exact    bf16 integers in [-4, 4]: every product is an integer of at most 16, every partial sum over dim <= 1024 an integer
           below 2^14: s_ij is exact in any order; max is exact; the fp64 sum of at most 512 integers is exact; one division in
           fp64 and one rounding to fp32, both of which numpy does identically.  Bit for bit.
  random   unit vectors rounded to bf16.  |s_ij(fp32) - s_ij| <= dim * U32 * sum_k |q_ik d_jk| =: a_ij, and
           |max_j s - max_j s'| <= max_j |s - s'|, so m_i is within max_j a_ij; the fp64 sum and division are exact to 2^-53;
           the final rounding to fp32 adds U32 |score|:  bound = mean_i max_j a_ij * SLACK + U32 |score|.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence

import numpy as np

from oracle.linear_cases import SLACK, U32, bf16_bits, bf16_values, hulp16

FILL16 = 0x7FC5                     # the poison of every bf16 output buffer: a quiet NaN no kernel produces
NEG_MAX = -float(np.finfo(np.float32).max)


# ---- the head --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def head_data(regime: str, M: int, H: int) -> Dict[str, np.ndarray]:
    """x [M, H], w [H, H] float64 arrays of bf16-exact values, b [H] of fp32-exact values."""
    rng = np.random.default_rng((0 if regime == "exact" else 1) * 1_000_003 + M * 7919 + H)
    if regime == "exact":
        x = rng.integers(-2, 3, size=(M, H)).astype(np.float64)
        w = rng.integers(-1, 2, size=(H, H)).astype(np.float64) / 64.0
        b = rng.integers(-8, 9, size=H).astype(np.float64) / 64.0
        # the precondition: v, the squares and their sum are exact in fp32 in any order
        worst_v = (np.abs(x) @ np.abs(w).T + np.abs(b)) * 64.0
        assert worst_v.max() < 2 ** 24
        v = (x @ w.T + b) * 64.0
        assert np.array_equal(v, np.round(v)) and (v * v).max() < 2 ** 24 and (v * v).sum(axis=1).max() < 2 ** 24
    else:
        rb = lambda a: bf16_values(bf16_bits(a))
        x = rb(rng.standard_normal((M, H)) * 0.5)
        w = rb(rng.standard_normal((H, H)) * 0.03)
        b = (rng.standard_normal(H) * 0.1).astype(np.float32).astype(np.float64)
    return dict(x=x, w=w, b=b, regime=regime, M=M, H=H)


def head_expected(d, mutant: Optional[str] = None):
    """float64 y [M, H] BEFORE the bf16 rounding, and its bound (None in the exact regime: compare bits of ONE rounding)."""
    x, w, b, H = d["x"], d["w"], d["b"], d["H"]
    c = x @ w.T
    v = c + b
    norm = np.maximum(np.sqrt((v * v).sum(axis=1, keepdims=True)), 1e-12)
    y = v if mutant == "no_normalisation" else v / norm
    if d["regime"] == "exact":
        return y, None
    e = (H * U32 * (np.abs(x) @ np.abs(w).T) + U32 * (np.abs(c) + np.abs(b))) * SLACK
    ytrue = v / norm
    ey = e / norm + np.abs(ytrue) * np.sqrt((e * e).sum(axis=1, keepdims=True)) / norm + 3 * U32 * np.abs(ytrue)
    return y, hulp16(np.abs(ytrue) + ey) + ey


def head_layout(y_rows: np.ndarray, lens: Sequence[int], S: int, row_stride: int, mutant: Optional[str] = None):
    """Token rows y [nseq * S, H] -> (out [nseq, row_stride, H] float64, counts [nseq]): row p < count of sequence i is token
    position p + 1, every row behind the count is zero."""
    nseq, H = len(lens), y_rows.shape[1]
    out = np.zeros((nseq, row_stride, H))
    counts = np.zeros(nseq, dtype=np.int32)
    for i, n in enumerate(lens):
        first, cnt = 1, max(0, n - 1)
        if mutant == "cls_not_skipped":
            first, cnt = 0, n
        if mutant == "eos_dropped":
            cnt = max(0, n - 2)
        cnt = min(cnt, row_stride)
        counts[i] = cnt
        out[i, :cnt] = y_rows[i * S + first:i * S + first + cnt]
    return out, counts


def head_ratio(got_bits: np.ndarray, want: np.ndarray, bound) -> float:
    """Worst |got - want| / bound (inf for a NaN or, with no bound, for different bits; then 0.0 = identical)."""
    got_bits = np.asarray(got_bits, dtype=np.uint16).reshape(want.shape)
    if bound is None:
        return 0.0 if np.array_equal(got_bits, bf16_bits(want).reshape(want.shape)) else float("inf")
    got = bf16_values(got_bits)
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float((np.abs(got - want) / bound).max())


def layout_bound(bound_rows, lens, S, row_stride):
    """The per-element bound in the output layout; rows behind a count must be exactly zero (bound 0 -> compared as equal)."""
    if bound_rows is None:
        return None
    out, _ = head_layout(bound_rows, lens, S, row_stride)
    return out


def layout_ratio(got_bits, want, bound) -> float:
    """head_ratio over a laid-out block: zero rows must be +0 bits, the others within the bound."""
    got_bits = np.asarray(got_bits, dtype=np.uint16).reshape(want.shape)
    if bound is None:
        return head_ratio(got_bits, want, None)
    zero = bound == 0
    if np.any(got_bits[zero] != 0):
        return float("inf")
    if not (~zero).any():
        return 0.0
    got = bf16_values(got_bits)
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float((np.abs(got - want)[~zero] / bound[~zero]).max())


HEAD_MUTANTS = ("cls_not_skipped", "eos_dropped", "no_normalisation")


# ---- MaxSim -----------------------------------------------------------------------------------------------------------
def maxsim_vectors(regime: str, n: int, dim: int, seed: int) -> np.ndarray:
    """n bf16-exact vectors [n, dim] as float64."""
    rng = np.random.default_rng(seed * 1009 + n * 31 + dim + (0 if regime == "exact" else 500_009))
    if regime == "exact":
        return rng.integers(-4, 5, size=(n, dim)).astype(np.float64)
    v = rng.standard_normal((n, dim))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return bf16_values(bf16_bits(v))


def maxsim_expected(q: np.ndarray, d: np.ndarray, regime: str, mutant: Optional[str] = None, pad_rows: int = 0):
    """(score float64, bound or None).  `pad_rows`: zero rows that lie behind the document in a 32-row tile (what the mutant
    `padding_in_max` lets take part)."""
    s = q @ d.T
    if mutant == "padding_in_max" and pad_rows:
        s = np.concatenate([s, np.zeros((len(q), pad_rows))], axis=1)
    m = s.sum(axis=1) if mutant == "sum_not_max" else s.max(axis=1)
    score = m.sum() / (len(d) if mutant == "divide_by_ld" else len(q))
    if regime == "exact":
        assert (np.abs(q) @ np.abs(d).T).max() < 2 ** 24
        return score, None
    true = (q @ d.T).max(axis=1).sum() / len(q)
    a = q.shape[1] * U32 * (np.abs(q) @ np.abs(d).T)
    return score, float(a.max(axis=1).mean() * SLACK + U32 * abs(true))


MAXSIM_MUTANTS = ("sum_not_max", "divide_by_ld", "padding_in_max")


def score_ratio(got: float, want: float, bound) -> float:
    if bound is None:
        return 0.0 if np.float32(got).tobytes() == np.float32(want).tobytes() else float("inf")
    return abs(float(got) - want) / bound


def select_expected(scores: np.ndarray, cand: np.ndarray, valid: np.ndarray, k: int):
    """hipmaxsim_dev's selection over one query's pair scores: valid candidates by (score descending, position ascending)."""
    order = sorted((j for j in range(len(cand)) if valid[j]), key=lambda j: (-float(scores[j]), j))[:k]
    ids = np.full(k, -1, dtype=np.int64)
    sc = np.full(k, NEG_MAX, dtype=np.float32)
    pos = np.full(k, -1, dtype=np.int32)
    for r, j in enumerate(order):
        ids[r], sc[r], pos[r] = cand[j], scores[j], j
    return sc, ids, pos


# ---- the collection's bookkeeping, restated ---------------------------------------------------------------------------------
def drop_ranges(items: List, ranges) -> List:
    gone = set()
    for lo, hi in ranges:
        gone.update(range(lo, hi))
    return [d for i, d in enumerate(items) if i not in gone]


def csr_of(docs: Sequence[np.ndarray], dim: int, cap: int):
    """uint16 documents [len_i, dim] -> (offsets int64, vecs uint16 [total, dim]) as a store holds them under `cap`."""
    kept = [np.asarray(d, dtype=np.uint16).reshape(-1, dim)[:cap] for d in docs]
    off = np.zeros(len(kept) + 1, dtype=np.int64)
    if kept:
        off[1:] = np.cumsum([len(v) for v in kept])
    vecs = np.concatenate(kept) if kept else np.zeros((0, dim), np.uint16)
    return off, vecs
