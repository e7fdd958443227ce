"""
BGE-M3's lexical weights as a sparse retrieval leg: the numpy restatement of the encoder's lexical head
(csrc/encoder.hip lexical_kernel, hipenc_forward_lexical), LexicalIndex -- the per-chunk weights of a collection transposed
into term-major postings and searched with the query's own weights (hipbm25_search_weighted*) --, LexicalIndexUpdatable --
the same postings kept on the device, where document rows are appended (transposed there) and removed
(csrc/bm25_impacts.hip) -- and the hybrid compositions with the dense index and RRF, unscoped and scoped.

BAAI/bge-m3 (rag/config.py:9 EMBEDDING_MODEL) gives, from the forward that makes the dense CLS vector, a weight per token:
relu(sparse_linear(last_hidden_state)), kept per distinct token id as the maximum over its positions; a query and a passage
match lexically with the sum over shared token ids of qw[t] * dw[t].  The reference names hybrid search
(rag/config.py:43-45) and implements none of it.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from .sparse import UPDATE_KINDS, HipBM25, PostingsCSR

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


class _ImpactBM25(HipBM25):
    _CREATE = "hipbm25_create_impacts"


class LexicalIndexUpdatable(LexicalIndex):
    """A LexicalIndex that follows its collection on the device (hipbm25_create_impacts / _append_impacts /
    _append_rows_dev / _remove_ranges, csrc/bm25_impacts.hip).

    Defining property: after any sequence of appends and removals the handle is bit for bit
    LexicalIndex(transpose_doc_weights(rows of the surviving documents in order, n_terms)) -- its export and every search
    result.  Lexical weights do not depend on N, df or avgdl, so nothing is reweighed and a search right after an update
    needs no other call.  The host keeps sizes only: the postings live on the device (export() reads them back).  The
    update entries synchronise, and the caller must have no search in flight on the handle."""

    def __init__(self, postings: Optional[PostingsCSR] = None, device: int = 0, id_base: int = 0, n_terms: int = 1):
        """`postings` from transpose_doc_weights, or None for an empty index of `n_terms` term ids."""
        if postings is None:
            postings = PostingsCSR(0, int(n_terms), np.zeros(int(n_terms) + 1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
        self.bm = _ImpactBM25(postings, device=device, id_base=id_base)
        self.p = self.bm.p = PostingsCSR(int(postings.n_docs), int(postings.n_terms), None, None, None)

    @property
    def n_terms(self) -> int:
        return self.p.n_terms

    # ---- state ----
    def sizes(self) -> dict:
        v = np.zeros(4, dtype=np.int64)
        nat.call("hipbm25_sizes", self.bm._h, v.ctypes.data)
        return {"n_docs": int(v[0]), "n_terms": int(v[1]), "postings": int(v[2]), "has_tf": bool(v[3] & 1), "dirty": bool(v[3] & 2),
                "updatable_impacts": bool(v[3] & 4)}

    def export(self) -> dict:
        """hipbm25_export: offsets, doc_ids and impacts as host arrays."""
        sz = self.sizes()
        out = {"n_docs": sz["n_docs"], "n_terms": sz["n_terms"], "offsets": np.zeros(sz["n_terms"] + 1, np.uint64),
               "doc_ids": np.zeros(sz["postings"], np.uint32), "impacts": np.zeros(sz["postings"], np.float32)}
        nat.call("hipbm25_export", self.bm._h, out["offsets"].ctypes.data, out["doc_ids"].ctypes.data, None, out["impacts"].ctypes.data, None)
        return out

    def postings(self) -> PostingsCSR:
        e = self.export()
        return PostingsCSR(e["n_docs"], e["n_terms"], e["offsets"], e["doc_ids"], e["impacts"])

    def update_info(self) -> dict:
        """hipbm25_update_info: the last create / append / removal."""
        v = np.zeros(8, dtype=np.int64)
        nat.call("hipbm25_update_info", self.bm._h, v.ctypes.data)
        return {"kind": UPDATE_KINDS[int(v[0])], "postings_before": int(v[1]), "postings_after": int(v[2]), "postings_moved": int(v[3]),
                "docs_before": int(v[4]), "docs_after": int(v[5]), "extra_bytes": int(v[6]), "grew": bool(v[7])}

    # ---- updates ----
    def _grown(self, n_new: int, n_terms_after: int) -> Tuple[int, int]:
        lo = self.p.n_docs
        self.p.n_docs += int(n_new)
        self.p.n_terms = int(n_terms_after)
        return lo, self.p.n_docs

    def append_postings(self, n_new_docs: int, n_terms_after: int, offsets, doc_ids, impacts) -> Tuple[int, int]:
        """hipbm25_append_impacts: a term-major batch CSR over n_terms_after terms with doc ids local to the batch."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ids = np.ascontiguousarray(doc_ids, dtype=np.uint32)
        imp = np.ascontiguousarray(impacts, dtype=np.float32)
        if off.shape[0] != n_terms_after + 1 or ids.shape != imp.shape or int(off[-1]) != ids.shape[0]:
            raise ValueError("inconsistent batch CSR")
        nat.call("hipbm25_append_impacts", self.bm._h, int(n_new_docs), int(n_terms_after), off.ctypes.data,
                 ids.ctypes.data if ids.size else None, imp.ctypes.data if imp.size else None)
        return self._grown(n_new_docs, n_terms_after)

    def append_rows(self, terms, weights, counts, n_terms_after: Optional[int] = None) -> Tuple[int, int]:
        """Append one document per row of document-major lexical rows (encode_lexical's outputs): terms int32 [n, L], weights
        float32 [n, L], counts int32 [n].  CUDA tensors are transposed and merged on the device (hipbm25_append_rows_dev,
        ordered behind torch's current stream); host arrays go through transpose_doc_weights and hipbm25_append_impacts.
        Returns the documents' id range [lo, hi)."""
        n_terms_after = self.p.n_terms if n_terms_after is None else int(n_terms_after)
        if hasattr(terms, "is_cuda") and terms.is_cuda:
            import torch
            from .index import _stream_ptr
            n = int(counts.shape[0])
            if terms.dim() != 2 or terms.shape != weights.shape or terms.shape[0] != n or counts.dim() != 1 or not (weights.is_cuda and counts.is_cuda):
                raise ValueError("append_rows expects CUDA tensors terms [n, L], weights [n, L] and counts [n]")
            if terms.dtype != torch.int32 or weights.dtype != torch.float32 or counts.dtype != torch.int32:
                raise ValueError("append_rows expects int32 terms, float32 weights and int32 counts")
            terms, weights, counts = terms.contiguous(), weights.contiguous(), counts.contiguous()
            nat.call("hipbm25_append_rows_dev", self.bm._h, terms.data_ptr() if n else None, weights.data_ptr() if n else None,
                     counts.data_ptr() if n else None, n, max(int(terms.shape[1]), 1), n_terms_after, _stream_ptr())
            return self._grown(n, n_terms_after)
        b = transpose_doc_weights(_host(terms), _host(weights), _host(counts), n_terms_after)
        return self.append_postings(b.n_docs, n_terms_after, b.offsets, b.doc_ids, b.impacts)

    def remove_ranges(self, ranges) -> int:
        """hipbm25_remove_ranges: drop the documents of half-open ranges [(lo, hi)] (ascending, not overlapping); the
        survivors keep their order and are renumbered.  Returns the documents removed."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
        nat.call("hipbm25_remove_ranges", self.bm._h, r.ctypes.data if r.size else None, int(r.shape[0]))
        before = self.p.n_docs
        self.p.n_docs = self.sizes()["n_docs"]
        return before - self.p.n_docs

    # ---- persistence: LexicalIndex's .npz layout, either class reads the other's file ----
    def save(self, path: str) -> None:
        e = self.export()
        with open(path, "wb") as f:
            np.savez(f, offsets=e["offsets"], doc_ids=e["doc_ids"], impacts=e["impacts"], n_docs=np.int64(e["n_docs"]))


def npz_doc_count(path: str) -> int:
    """The document count of a lexical .npz file (LexicalIndex.save / LexicalIndexUpdatable.save)."""
    with np.load(path) as z:
        return int(z["n_docs"])


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


def hybrid_search_scoped_lexical_device(dense_index, lex: LexicalIndex, q, q_terms, q_weights, scopes, scope_of_query=None,
                                        depth: int = 50, k: int = 10, c: float = 60.0, w_dense: float = 1.0, w_sparse: float = 1.0,
                                        return_lists: bool = False):
    """The scoped sibling of hybrid_search_lexical_device: dense top-`depth` of every query's scope
    (hipidx_search_scoped_dev) + lexical top-`depth` of the same scope (hipbm25_search_scoped_weighted_dev) + RRF
    (hiprrf_fuse_dev), all enqueued on torch's current stream, no host synchronisation.  `scopes` / `scope_of_query` as in
    HipFlatIndex.search_scoped: row ranges of the collection, which are document ranges of `lex`.  Returns (fused scores
    float32 [nq, k], ids int64 [nq, k]); return_lists=True adds ((dense scores float64, dense ids), (lexical scores float64,
    lexical ids)), each [nq, depth]."""
    from .fusion import rrf_fuse_device
    dense = dense_index.search_scoped_device(q, int(depth), scopes, scope_of_query)
    sparse = lex.bm.search_scoped_weighted_device(q_terms, q_weights, int(depth), scopes, scope_of_query)
    fused = rrf_fuse_device(dense[2], sparse[2], int(k), c=c, w_a=w_dense, w_b=w_sparse)
    if return_lists:
        return tuple(fused) + (((dense[0], dense[2]), (sparse[0], sparse[2])),)
    return fused
