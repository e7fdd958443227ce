"""
BGE-M3's combined score (hipm3_score_*): a passage's rank from a weighted sum of its dense, sparse and ColBERT scores --
FlagEmbedding's compute_score "dense + sparse + colbert" -- for candidate ids a first stage found.  The three components
are what HipFlatIndex.score_ids, HipBM25.score_ids and maxsim give the pair; one small kernel combines and ranks.

m3_score_reference restates the combination and the order in numpy float64; the components come from the other references.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native as nat

M3_WEIGHTS = (0.4, 0.2, 0.4)      # dense, sparse, colbert: BGE-M3's published mix
_FLT_MAX = np.finfo(np.float32).max
_DBL_MAX = np.finfo(np.float64).max


def _check_weights(weights) -> Tuple[float, float, float]:
    w = tuple(float(x) for x in weights)
    if len(w) != 3 or not all(np.isfinite(x) and x >= 0 for x in w) or not any(x > 0 for x in w):
        raise ValueError("weights = (dense, sparse, colbert): finite, >= 0, at least one > 0")
    return w


def m3_score_reference(dense64, sparse32, maxsim32, valid, weights, k: int, l2: bool = False):
    """The semantics of hipm3_score as a pure function (no GPU).  dense64 float64 [nq, depth] (hipidx_score_ids' fp64 output;
    with l2 the squared distance, mapped to 1.0 - 0.5 * dist), sparse32 and maxsim32 float32 [nq, depth], valid bool
    [nq, depth]; a leg whose weight is 0 is left out (its array may be None) -- left out, not multiplied.  A MaxSim score of
    -FLT_MAX (a padding pair) counts as 0.0.  combined = (((w_d * s_d) + (w_s * s_s)) + (w_c * s_c)) / ((w_d + w_s) + w_c), every
    operation a float64 numpy operation of its own.  -> (pair scores float64 [nq, depth], -DBL_MAX where invalid; scores
    float64 [nq, k], ids-as-positions int64 [nq, k]): the valid candidates by (combined descending, position ascending),
    -DBL_MAX / -1 past them.  The caller maps positions to ids."""
    w_d, w_s, w_c = (np.float64(x) for x in _check_weights(weights))
    valid = np.asarray(valid, dtype=bool)
    nq, depth = valid.shape
    acc = None
    if w_d > 0:
        s_d = np.asarray(dense64, dtype=np.float64)
        if l2:
            s_d = np.float64(1.0) - np.float64(0.5) * s_d
        acc = w_d * s_d
    if w_s > 0:
        p = w_s * np.asarray(sparse32, dtype=np.float32).astype(np.float64)
        acc = p if acc is None else acc + p
    if w_c > 0:
        ms = np.asarray(maxsim32, dtype=np.float32)
        p = w_c * np.where(ms == -_FLT_MAX, np.float64(0.0), ms.astype(np.float64))
        acc = p if acc is None else acc + p
    total = (w_d + w_s) + w_c
    with np.errstate(over="ignore", invalid="ignore"):
        pairs = np.where(valid, acc / total, -_DBL_MAX)
    scores = np.full((nq, k), -_DBL_MAX, dtype=np.float64)
    pos = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        cand = np.flatnonzero(valid[i])
        order = cand[np.lexsort((cand, -pairs[i, cand]))][:k]
        scores[i, :len(order)] = pairs[i, order]
        pos[i, :len(order)] = order
    return pairs, scores, pos


def _flatten_query_terms(bm25, queries, term_weights):
    if term_weights is None:
        terms, qoff = bm25._flatten(queries)
        return terms, None, qoff
    return bm25._flatten_weighted(queries, term_weights)


def m3_score(index, bm25, store, q, queries, term_weights, q_vecs, q_counts, cand_ids, k: int,
             weights: Sequence[float] = M3_WEIGHTS):
    """hipm3_score_host: every array on the host.  index a HipFlatIndex (always), bm25 a HipBM25 and store a MultiVectorStore
    (each may be None when its weight is 0, with its query arguments); q float32 [nq, d], queries / term_weights as
    HipBM25.search_weighted takes them (term_weights None: plain impacts), q_vecs uint16 [nq, q_stride, dim] bf16 bits, q_counts
    int32 [nq], cand_ids int64 [nq, depth].  -> dict of scores float64 [nq, k], ids int64 [nq, k], pos int32 [nq, k], pairs
    float64 [nq, depth], parts float32 [nq, depth, 3]."""
    w = _check_weights(weights)
    cand = np.ascontiguousarray(cand_ids, dtype=np.int64)
    if cand.ndim != 2:
        raise ValueError("cand_ids must be [nq, depth]")
    nq, depth = cand.shape
    k = int(k)
    qa = np.ascontiguousarray(q, dtype=np.float32) if w[0] > 0 else None
    terms = wts = qoff = None
    if w[1] > 0:
        terms, wts, qoff = _flatten_query_terms(bm25, queries, term_weights)
    qv = qc = None
    if w[2] > 0:
        qv = np.ascontiguousarray(q_vecs, dtype=np.uint16)
        qc = np.ascontiguousarray(q_counts, dtype=np.int32).reshape(-1)
        if qv.ndim != 3 or qv.shape[0] != nq or len(qc) != nq:
            raise ValueError("q_vecs must be [nq, q_stride, dim] and q_counts [nq]")
    kk = max(k, 1)
    out = {"scores": np.zeros((nq, kk), np.float64), "ids": np.zeros((nq, kk), np.int64), "pos": np.zeros((nq, kk), np.int32),
           "pairs": np.zeros((nq, max(depth, 1)), np.float64), "parts": np.zeros((nq, max(depth, 1), 3), np.float32)}
    nat.call("hipm3_score_host", index._h, bm25._h if w[1] > 0 else 0, store._h if w[2] > 0 else 0,
             qa.ctypes.data if qa is not None else None,
             terms.ctypes.data if terms is not None and terms.size else None, wts.ctypes.data if wts is not None else None,
             qoff.ctypes.data if qoff is not None else None, qv.ctypes.data if qv is not None else None,
             qc.ctypes.data if qc is not None else None, int(qv.shape[1]) if qv is not None else 1, nq, cand.ctypes.data, depth, k,
             w[0], w[1], w[2], out["parts"].ctypes.data, out["pairs"].ctypes.data, out["scores"].ctypes.data, out["ids"].ctypes.data,
             out["pos"].ctypes.data)
    return out


def m3_score_device(index, bm25, store, q, queries, term_weights, q_vecs, q_counts, cand_ids, k: int,
                    weights: Sequence[float] = M3_WEIGHTS, want_parts: bool = True):
    """hipm3_score_dev on torch's current stream: q float32 [nq, d], q_vecs bfloat16 [nq, q_stride, dim], q_counts int32 [nq]
    and cand_ids int64 [nq, depth] are CUDA tensors (what the first stage and encode_m3 returned); queries / term_weights
    are host lists.  -> dict of CUDA tensors as m3_score's (parts / pairs None without want_parts); the host waits for nothing
    beyond the staging ring of the postings."""
    import torch
    from .index import _stream_ptr
    w = _check_weights(weights)
    if cand_ids.dtype != torch.int64 or cand_ids.dim() != 2 or not cand_ids.is_cuda:
        raise ValueError("cand_ids must be an int64 CUDA tensor [nq, depth]")
    cand = cand_ids.contiguous()
    nq, depth = cand.shape
    k = int(k)
    dev = cand.device
    qa = None
    if w[0] > 0:
        if q.dtype != torch.float32 or q.dim() != 2 or not q.is_cuda or q.shape[0] != nq:
            raise ValueError("q must be a float32 CUDA tensor [nq, d]")
        qa = q.contiguous()
    terms = wts = qoff = None
    if w[1] > 0:
        terms, wts, qoff = _flatten_query_terms(bm25, queries, term_weights)
    qv = qc = None
    if w[2] > 0:
        if q_vecs.dtype != torch.bfloat16 or q_vecs.dim() != 3 or not q_vecs.is_cuda or q_vecs.shape[0] != nq:
            raise ValueError("q_vecs must be a bfloat16 CUDA tensor [nq, q_stride, dim]")
        if q_counts.dtype != torch.int32 or not q_counts.is_cuda or q_counts.numel() != nq:
            raise ValueError("q_counts must be an int32 CUDA tensor [nq]")
        qv, qc = q_vecs.contiguous(), q_counts.contiguous()
    kk = max(k, 1)
    out = {"scores": torch.empty((nq, kk), dtype=torch.float64, device=dev), "ids": torch.empty((nq, kk), dtype=torch.int64, device=dev),
           "pos": torch.empty((nq, kk), dtype=torch.int32, device=dev),
           "pairs": torch.empty((nq, depth), dtype=torch.float64, device=dev) if want_parts else None,
           "parts": torch.empty((nq, depth, 3), dtype=torch.float32, device=dev) if want_parts else None}
    nat.call("hipm3_score_dev", index._h, bm25._h if w[1] > 0 else 0, store._h if w[2] > 0 else 0,
             qa.data_ptr() if qa is not None else None,
             terms.ctypes.data if terms is not None and terms.size else None, wts.ctypes.data if wts is not None else None,
             qoff.ctypes.data if qoff is not None else None, qv.data_ptr() if qv is not None else None,
             qc.data_ptr() if qc is not None else None, int(qv.shape[1]) if qv is not None else 1, nq, cand.data_ptr(), depth, k,
             w[0], w[1], w[2], out["parts"].data_ptr() if want_parts else None, out["pairs"].data_ptr() if want_parts else None,
             out["scores"].data_ptr(), out["ids"].data_ptr(), out["pos"].data_ptr(), _stream_ptr())
    return out


__all__ = ["M3_WEIGHTS", "m3_score", "m3_score_device", "m3_score_reference"]
