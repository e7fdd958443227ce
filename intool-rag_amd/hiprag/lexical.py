"""
BGE-M3's lexical weights as a sparse retrieval leg: the numpy restatement of the encoder's lexical head
(csrc/encoder.hip lexical_kernel, hipenc_forward_lexical), LexicalIndex -- the per-chunk weights of a collection transposed
into term-major postings and searched with the query's own weights (hipbm25_search_weighted*) -- and the hybrid
composition with the dense index and RRF.

BAAI/bge-m3 (rag/config.py:9 EMBEDDING_MODEL) gives, from the forward that makes the dense CLS vector, a weight per token:
relu(sparse_linear(last_hidden_state)), kept per distinct token id as the maximum over its positions; a query and a passage
match lexically with the sum over shared token ids of qw[t] * dw[t].  The reference names hybrid search
(rag/config.py:43-45) and implements none of it.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .sparse import HipBM25, PostingsCSR

BGE_M3_UNUSED_IDS = (0, 1, 2, 3)    # bos, pad, eos, unk of the XLM-R vocabulary


def lexical_token_weights(hidden: np.ndarray, weight: np.ndarray, bias: float) -> np.ndarray:
    """w_t = max(0, fl32(dot_t + bias)) for every row of `hidden` [len, H] (float32 holding bf16 values) against `weight`
    [H] (float32 holding bf16 values), in the kernel's summation order: lane l adds the products of columns l, l + 64, ..
    in ascending order (each product is exact in float32), then a butterfly over lane distances 32, 16, .., 1."""
    x = np.asarray(hidden, dtype=np.float32).reshape(-1, np.asarray(weight).size)
    w = np.asarray(weight, dtype=np.float32).reshape(-1)
    H = w.size
    if H % 64:
        raise ValueError("hidden must be a multiple of 64")
    prod = (x * w[None, :]).reshape(x.shape[0], H // 64, 64)        # [t][j][lane]: column j * 64 + lane
    s = np.zeros((x.shape[0], 64), dtype=np.float32)
    for j in range(H // 64):
        s = s + prod[:, j, :]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ off]
    return np.maximum(np.float32(0), s[:, 0] + np.float32(bias)).astype(np.float32)


def dedupe_token_weights(token_ids: Sequence[int], token_weights: Sequence[float], unused_ids=()) -> Tuple[np.ndarray, np.ndarray]:
    """The row rule of hipenc_forward_lexical: the distinct ids that are not unused and whose largest weight is > 0, ascending,
    each with the maximum of its positions' weights."""
    ids = np.asarray(token_ids, dtype=np.int64).reshape(-1)
    w = np.asarray(token_weights, dtype=np.float32).reshape(-1)
    best = {}
    for i, v in zip(ids.tolist(), w):
        if i not in best or v > best[i]:
            best[i] = v
    keep = sorted(i for i, v in best.items() if i not in set(int(u) for u in unused_ids) and v > 0)
    return np.asarray(keep, dtype=np.int32), np.asarray([best[i] for i in keep], dtype=np.float32)


def lexical_reference(hidden_rows: Sequence[np.ndarray], token_lists: Sequence[Sequence[int]], weight, bias: float, unused_ids=(),
                      max_len: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """hipenc_forward_lexical's three sparse outputs in numpy: (terms int32 [n, L], weights float32 [n, L], counts int32 [n])
    from the final hidden rows of every sequence (hidden_rows[i] = float32 [len_i, H] holding the bf16 rows, what
    HipEncoder.hidden_tokens returns), padded with -1 / 0."""
    n = len(token_lists)
    L = max_len if max_len is not None else max(1, max((len(t) for t in token_lists), default=1))
    terms = np.full((n, L), -1, dtype=np.int32)
    weights = np.zeros((n, L), dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    for i, toks in enumerate(token_lists):
        if len(toks) == 0:
            continue
        wt = lexical_token_weights(np.asarray(hidden_rows[i])[:len(toks)], weight, bias)
        t, w = dedupe_token_weights(toks, wt, unused_ids)
        counts[i] = len(t)
        terms[i, :len(t)] = t
        weights[i, :len(t)] = w
    return terms, weights, counts


def transpose_doc_weights(terms, weights, counts, n_terms: int) -> PostingsCSR:
    """Document-major lexical rows (hipenc_forward_lexical's outputs for the chunks of a collection, row i = chunk i) ->
    term-major CSR postings: doc ids ascend within a list, the impacts are the weights."""
    terms = np.asarray(terms, dtype=np.int64)
    weights = np.asarray(weights, dtype=np.float32)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    n_docs = counts.shape[0]
    L = terms.shape[1] if terms.ndim == 2 and n_docs else 0
    mask = np.arange(L)[None, :] < counts[:, None] if n_docs else np.zeros((0, 0), dtype=bool)
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), counts)
    term = terms.reshape(n_docs, L)[mask]
    w = weights.reshape(n_docs, L)[mask]
    if term.size and (term.min() < 0 or term.max() >= n_terms):
        raise ValueError("a term id lies outside [0, n_terms)")
    order = np.lexsort((doc, term))
    offsets = np.zeros(n_terms + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(term, minlength=n_terms)).astype(np.uint64)
    return PostingsCSR(n_docs, int(n_terms), offsets, doc[order].astype(np.uint32), np.ascontiguousarray(w[order], dtype=np.float32))


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


class LexicalIndex:
    """Lexical weights of a collection's chunks as impact postings on the device; searched with a weight per query term."""

    def __init__(self, postings: PostingsCSR, device: int = 0, id_base: int = 0):
        self.p = postings
        self.bm = HipBM25(postings, device=device, id_base=id_base)

    @classmethod
    def from_doc_weights(cls, terms, weights, counts, n_terms: int, device: int = 0) -> "LexicalIndex":
        return cls(transpose_doc_weights(_host(terms), _host(weights), _host(counts), n_terms), device=device)

    @property
    def n_docs(self) -> int:
        return self.p.n_docs

    def close(self) -> None:
        self.bm.close()

    def search(self, q_terms, q_weights, k: int):
        return self.bm.search_weighted(q_terms, q_weights, k)

    def search_device(self, q_terms, q_weights, k: int, out=None):
        return self.bm.search_weighted_device(q_terms, q_weights, k, out=out)

    def search_scoped(self, q_terms, q_weights, k: int, scopes, scope_of_query=None):
        return self.bm.search_scoped_weighted(q_terms, q_weights, k, scopes, scope_of_query)

    def save(self, path: str) -> None:
        """One .npz: the three arrays of the postings (n_terms is the offsets' length - 1) and the document count."""
        with open(path, "wb") as f:
            np.savez(f, offsets=self.p.offsets, doc_ids=self.p.doc_ids, impacts=self.p.impacts, n_docs=np.int64(self.p.n_docs))

    @classmethod
    def load(cls, path: str, device: int = 0) -> "LexicalIndex":
        with np.load(path) as z:
            off = z["offsets"].astype(np.uint64)
            p = PostingsCSR(int(z["n_docs"]), int(off.shape[0] - 1), off, z["doc_ids"].astype(np.uint32), z["impacts"].astype(np.float32))
        return cls(p, device=device)


def query_terms_of_row(terms_row, weights_row, count: int) -> Tuple[List[int], np.ndarray]:
    """One row of encode_lexical's output as a weighted query: its first `count` (term, weight) pairs."""
    t, w = _host(terms_row)[:int(count)], _host(weights_row)[:int(count)]
    return [int(x) for x in t], np.asarray(w, dtype=np.float32)


def hybrid_search_lexical_device(dense_index, lexical_index: LexicalIndex, q, q_terms, q_weights, depth: int = 50, k: int = 10,
                                 c: float = 60.0, w_dense: float = 1.0, w_sparse: float = 1.0):
    """Dense top-`depth` (hipidx_search_dev) + lexical top-`depth` (hipbm25_search_weighted_dev) + RRF (hiprrf_fuse_dev), all
    enqueued on torch's current stream, no host synchronisation.  `q`: float32 CUDA tensor [nq, d]; `q_terms` / `q_weights`:
    per query its term ids and weights (host).  Returns ((fused scores float32, ids int64) [nq, k],
    (dense scores float64, float32, ids) [nq, depth], (lexical scores float64, float32, ids) [nq, depth])."""
    from .fusion import rrf_fuse_device
    dense = dense_index.search_device(q, int(depth))
    sparse = lexical_index.search_device(q_terms, q_weights, int(depth))
    fused = rrf_fuse_device(dense[2], sparse[2], int(k), c=c, w_a=w_dense, w_b=w_sparse)
    return fused, dense, sparse
