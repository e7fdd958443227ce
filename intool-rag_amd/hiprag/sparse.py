"""
HipBM25 -- BM25 term-at-a-time scoring on the GPU (csrc/bm25.hip) plus the host-side index builder, and
HipBM25Updatable -- the same index with its term frequencies and document lengths kept on the device, so that documents
are appended and removed there and every impact is recomputed by one kernel pass (csrc/bm25_update.hip).

The reference only names BM25 (README.md:54-58, rag/config.py:43-45); the specification implemented here is in
DESIGN.md ("BM25 spec"): tokens = text.lower().split() (the reference's only tokeniser,
rag/agent/query_processor.py:26); idf = ln(1 + (N - df + 0.5)/(df + 0.5)); impact = idf * tf*(k1+1) /
(tf + k1*(1 - b + b*|d|/avgdl)) with k1=1.5, b=0.75, evaluated in float64 and rounded ONCE to float32.  The GPU
adds impacts in query-term order (fp32), excludes score <= 0 and ranks by (score desc, doc id asc).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat

K1 = 1.5
B = 0.75


def tokenize(text: str) -> List[str]:
    return text.lower().split()


@dataclass
class PostingsCSR:
    n_docs: int
    n_terms: int
    offsets: np.ndarray   # uint64 [V+1]
    doc_ids: np.ndarray   # uint32 [P], ascending inside each term's list
    impacts: np.ndarray   # float32 [P]
    vocab: Optional[Dict[str, int]] = None
    tfs: Optional[np.ndarray] = None       # uint32 [P] term frequencies (build_postings fills them; HipBM25Updatable needs them)
    doc_len: Optional[np.ndarray] = None   # int64 [n_docs] document lengths in tokens

    def shard(self, lo: int, hi: int) -> "PostingsCSR":
        """Postings of documents [lo,hi) with LOCAL doc ids; impacts keep the GLOBAL idf / avgdl."""
        keep = (self.doc_ids >= lo) & (self.doc_ids < hi)
        term_of = np.repeat(np.arange(self.n_terms, dtype=np.int64), np.diff(self.offsets.astype(np.int64)))
        df = np.bincount(term_of[keep], minlength=self.n_terms)
        off = np.zeros(self.n_terms + 1, dtype=np.uint64)
        off[1:] = np.cumsum(df).astype(np.uint64)
        return PostingsCSR(hi - lo, self.n_terms, off, (self.doc_ids[keep] - np.uint32(lo)).astype(np.uint32),
                           self.impacts[keep].copy(), self.vocab)


def build_postings(doc_of_tok: np.ndarray, term_of_tok: np.ndarray, n_docs: int, n_terms: int,
                   doc_len: Optional[np.ndarray] = None, k1: float = K1, b: float = B, *,
                   df_global: Optional[np.ndarray] = None, n_docs_global: Optional[int] = None,
                   avgdl_global: Optional[float] = None) -> PostingsCSR:
    """Token stream -> CSR postings (tf = multiplicity) with precomputed fp32 impacts.

    A document-range SHARD built on its own (one rank of a row-sharded collection) passes the collection-wide document
    frequencies, document count and average length (`df_global`, `n_docs_global`, `avgdl_global`): idf and the length
    normalisation are global constants of BM25, so the shard's impacts then equal those of the unsharded build."""
    doc_of_tok = np.asarray(doc_of_tok, dtype=np.int64)
    term_of_tok = np.asarray(term_of_tok, dtype=np.int64)
    if doc_len is None:
        doc_len = np.bincount(doc_of_tok, minlength=n_docs)
    doc_len = np.asarray(doc_len, dtype=np.float64)
    pair = np.sort(term_of_tok * np.int64(n_docs) + doc_of_tok, kind="stable")
    if pair.size:
        first = np.ones(pair.size, dtype=bool)
        first[1:] = pair[1:] != pair[:-1]
        starts = np.flatnonzero(first)
        uniq = pair[starts]
        tf = np.diff(np.append(starts, pair.size)).astype(np.float64)
    else:
        uniq = pair
        tf = np.zeros(0, dtype=np.float64)
    term = uniq // n_docs if n_docs else uniq
    doc = (uniq - term * n_docs).astype(np.uint32)
    df = np.bincount(term, minlength=n_terms).astype(np.float64)
    offsets = np.zeros(n_terms + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(df).astype(np.uint64)
    avgdl = float(avgdl_global) if avgdl_global is not None else (doc_len.sum() / n_docs if n_docs else 1.0)
    n_all = float(n_docs_global) if n_docs_global is not None else float(n_docs)
    df_all = np.asarray(df_global, dtype=np.float64) if df_global is not None else df
    idf = np.log(1.0 + (n_all - df_all + 0.5) / (df_all + 0.5))
    norm = k1 * (1.0 - b + b * doc_len[doc] / avgdl)
    impacts = (idf[term] * tf * (k1 + 1.0) / (tf + norm)).astype(np.float32)
    return PostingsCSR(n_docs, n_terms, offsets, doc, impacts, None, tf.astype(np.uint32), doc_len.astype(np.int64))


def build_postings_from_texts(texts: Sequence[str]) -> PostingsCSR:
    vocab: Dict[str, int] = {}
    docs: List[int] = []
    terms: List[int] = []
    for i, t in enumerate(texts):
        for tok in tokenize(t or ""):
            terms.append(vocab.setdefault(tok, len(vocab)))
            docs.append(i)
    n = len(texts)
    p = build_postings(np.asarray(docs, np.int64), np.asarray(terms, np.int64), n, max(len(vocab), 1),
                       np.bincount(np.asarray(docs, np.int64), minlength=n) if docs else np.zeros(n))
    p.vocab = vocab
    return p


class HipBM25:
    _CREATE = "hipbm25_create"      # hiprag.lexical's updatable impact handle is made by hipbm25_create_impacts, same arguments

    def __init__(self, postings: PostingsCSR, device: int = 0, id_base: int = 0):
        self.p = postings
        self.device = int(device)
        off = np.ascontiguousarray(postings.offsets, dtype=np.uint64)
        ids = np.ascontiguousarray(postings.doc_ids, dtype=np.uint32)
        imp = np.ascontiguousarray(postings.impacts, dtype=np.float32)
        if off.shape[0] != postings.n_terms + 1 or ids.shape != imp.shape or int(off[-1]) != ids.shape[0]:
            raise ValueError("inconsistent CSR postings")
        h = ctypes.c_uint64()
        nat.call(self._CREATE, int(postings.n_docs), int(postings.n_terms), off.ctypes.data, ids.ctypes.data,
                 imp.ctypes.data, self.device, ctypes.byref(h))
        self._h = h.value
        if id_base:
            nat.call("hipbm25_set_id_base", self._h, int(id_base))

    def set_id_base(self, base: int) -> None:
        """First global document id of this (document-range) shard: returned ids are local id + base."""
        nat.call("hipbm25_set_id_base", self._h, int(base))

    def close(self) -> None:
        if getattr(self, "_h", None):
            try:
                nat.call("hipbm25_destroy", self._h)
            finally:
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _flatten(queries: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
        qoff = np.zeros(len(queries) + 1, dtype=np.int32)
        qoff[1:] = np.cumsum([len(q) for q in queries])
        terms = (np.concatenate([np.asarray(q, dtype=np.uint32) for q in queries]) if qoff[-1]
                 else np.zeros(0, np.uint32))
        return np.ascontiguousarray(terms, dtype=np.uint32), qoff

    def terms_of(self, text: str) -> List[int]:
        """Query text -> term ids in query order; out-of-vocabulary tokens are dropped (they match nothing)."""
        if self.p.vocab is None:
            raise ValueError("index was built from term ids, not texts")
        return [self.p.vocab[t] for t in tokenize(text) if t in self.p.vocab]

    def _flatten_weighted(self, queries: Sequence[Sequence[int]], weights: Sequence[Sequence[float]]):
        """(terms, weights, q_offsets); terms of weight zero are dropped (they add nothing and the library refuses them),
        any other weight goes through to the library's check (finite and > 0)."""
        if len(queries) != len(weights):
            raise ValueError("queries and weights must have one entry per query")
        terms, qoff = self._flatten(queries)
        if any(np.size(w) != qoff[b + 1] - qoff[b] for b, w in enumerate(weights)):
            raise ValueError("a query's weights must run parallel to its terms")
        wts = (np.concatenate([np.asarray(w, dtype=np.float32).reshape(-1) for w in weights]) if qoff[-1] else np.zeros(0, np.float32))
        keep = wts != 0
        if not keep.all():                                   # rare: cut the zero-weight slots out of the flat arrays
            qoff = np.concatenate([[0], np.cumsum(keep)[qoff[1:] - 1] * (qoff[1:] > 0)]).astype(np.int32)
            terms, wts = terms[keep], wts[keep]
        if wts.size == 0:
            wts = np.zeros(1, np.float32)                    # a valid pointer for the library; no slot refers to it
        return np.ascontiguousarray(terms, dtype=np.uint32), np.ascontiguousarray(wts, dtype=np.float32), qoff

    def _search(self, queries, k, weights=None, scopes=None, scope_of_query=None, device=False, out=None):
        """The one body of the eight search methods: hipbm25_search{_scoped}{_weighted}{_dev} by `scopes`, `weights`, `device`.
        Host form: (scores float32, ids int64) arrays [nq, k]; device form: (float64, float32, int64) CUDA tensors [nq, k]
        (`out`, where given, in their place; its first two members may be None).  A scoped call of no queries makes no
        library call (the scoped entries refuse nq == 0, the unscoped ones accept it)."""
        nq, k = len(queries), int(k)
        name = "hipbm25_search" + ("_scoped" if scopes is not None else "") + ("_weighted" if weights is not None else "")
        if weights is None:
            terms, qoff = self._flatten(queries)
            args = [terms.ctypes.data if terms.size else None, qoff.ctypes.data, nq, k]
        else:
            terms, wts, qoff = self._flatten_weighted(queries, weights)
            args = [terms.ctypes.data if terms.size else None, wts.ctypes.data, qoff.ctypes.data, nq, k]
        if scopes is not None:
            from .index import pack_scopes
            ranges, offsets, soq = pack_scopes(scopes, scope_of_query, nq)
            args += [ranges.ctypes.data, offsets.ctypes.data, len(offsets) - 1, soq.ctypes.data]
        if device:
            import torch
            from .index import _stream_ptr
            if out is None:
                dev = torch.device("cuda", self.device)
                out = tuple(torch.empty((nq, k), dtype=t, device=dev) for t in (torch.float64, torch.float32, torch.int64))
            args += [out[0].data_ptr() if out[0] is not None else None, out[1].data_ptr() if out[1] is not None else None,
                     out[2].data_ptr(), _stream_ptr()]
            name += "_dev"
        else:
            out = (np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.int64))
            args += [out[0].ctypes.data, out[1].ctypes.data]
        if nq or scopes is None:
            nat.call(name, self._h, *args)
        return out

    def search(self, queries: Sequence[Sequence[int]], k: int) -> Tuple[np.ndarray, np.ndarray]:
        return self._search(queries, k)

    def search_device(self, queries: Sequence[Sequence[int]], k: int, out=None):
        return self._search(queries, k, device=True, out=out)

    # ---- scoped search: per-query document-range scopes over the collection's postings (hipbm25_search_scoped) ----
    def search_scoped(self, queries: Sequence[Sequence[int]], k: int, scopes, scope_of_query=None) -> Tuple[np.ndarray, np.ndarray]:
        """BM25 top k of the documents in the query's scope: scopes[s] = half-open (lo, hi) ranges of LOCAL document ids,
        ascending, not overlapping; query i searches scopes[scope_of_query[i]] (None: one scope for all, or one per query).
        Scores are the collection's (its idf and avgdl): the in-scope entries of the full ranking, in order.  k <= 64."""
        return self._search(queries, k, scopes=scopes, scope_of_query=scope_of_query)

    def search_scoped_device(self, queries: Sequence[Sequence[int]], k: int, scopes, scope_of_query=None, out=None):
        """hipbm25_search_scoped_dev: (scores float64, scores float32, ids int64) CUDA tensors [nq, k], ordered on torch's
        current stream; no host synchronisation."""
        return self._search(queries, k, scopes=scopes, scope_of_query=scope_of_query, device=True, out=out)

    # ---- weighted search: one weight per query term (hipbm25_search_weighted*), e.g. BGE-M3's lexical query weights ----
    def search_weighted(self, queries: Sequence[Sequence[int]], weights: Sequence[Sequence[float]], k: int) -> Tuple[np.ndarray, np.ndarray]:
        """score(d) = fp32 sum in query-term order of fl32(weights[t] * impact[t, d]); everything else as search()."""
        return self._search(queries, k, weights=weights)

    def search_weighted_device(self, queries: Sequence[Sequence[int]], weights: Sequence[Sequence[float]], k: int, out=None):
        """hipbm25_search_weighted_dev: (float64, float32, int64) CUDA tensors [nq, k] on torch's current stream."""
        return self._search(queries, k, weights=weights, device=True, out=out)

    def search_scoped_weighted(self, queries: Sequence[Sequence[int]], weights: Sequence[Sequence[float]], k: int, scopes,
                               scope_of_query=None) -> Tuple[np.ndarray, np.ndarray]:
        """search_scoped() with a weight per query term (hipbm25_search_scoped_weighted); k <= 64."""
        return self._search(queries, k, weights=weights, scopes=scopes, scope_of_query=scope_of_query)

    def search_scoped_weighted_device(self, queries: Sequence[Sequence[int]], weights: Sequence[Sequence[float]], k: int, scopes,
                                      scope_of_query=None, out=None):
        """hipbm25_search_scoped_weighted_dev: as search_scoped_device, with a weight per query term."""
        return self._search(queries, k, weights=weights, scopes=scopes, scope_of_query=scope_of_query, device=True, out=out)

    # ---- the sparse score of given documents (hipbm25_score_ids*): what score_ids is to the flat index --------------
    def score_ids(self, queries: Sequence[Sequence[int]], ids, weights: Optional[Sequence[Sequence[float]]] = None) -> np.ndarray:
        """float32 [nq, depth]: the score every search method gives document ids[i, j] - id_base for query i (0.0 when no term
        matches), -FLT_MAX where the id names no document.  `weights` None: plain impacts."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if ids.ndim != 2 or ids.shape[0] != len(queries):
            raise ValueError("score_ids expects ids [nq, depth], one row per query")
        if weights is None:
            terms, qoff = self._flatten(queries)
            wptr = None
        else:
            terms, wts, qoff = self._flatten_weighted(queries, weights)
            wptr = wts.ctypes.data
        out = np.empty(ids.shape, dtype=np.float32)
        nat.call("hipbm25_score_ids", self._h, terms.ctypes.data if terms.size else None, wptr, qoff.ctypes.data, len(queries),
                 ids.ctypes.data, ids.shape[1], out.ctypes.data)
        return out

    def score_ids_device(self, queries: Sequence[Sequence[int]], ids, weights: Optional[Sequence[Sequence[float]]] = None, out=None):
        """hipbm25_score_ids_dev for an int64 CUDA tensor [nq, depth]: a float32 CUDA tensor [nq, depth] on torch's current
        stream; no host synchronisation."""
        import torch
        from .index import _stream_ptr
        if ids.dtype != torch.int64 or ids.dim() != 2 or not ids.is_cuda or ids.shape[0] != len(queries):
            raise ValueError("score_ids_device expects an int64 [nq, depth] CUDA tensor of ids, one row per query")
        ids = ids.contiguous()
        if weights is None:
            terms, qoff = self._flatten(queries)
            wptr = None
        else:
            terms, wts, qoff = self._flatten_weighted(queries, weights)
            wptr = wts.ctypes.data
        if out is None:
            out = torch.empty(tuple(ids.shape), dtype=torch.float32, device=ids.device)
        nat.call("hipbm25_score_ids_dev", self._h, terms.ctypes.data if terms.size else None, wptr, qoff.ctypes.data, len(queries),
                 ids.data_ptr(), int(ids.shape[1]), out.data_ptr(), _stream_ptr())
        return out

    def score_info(self) -> dict:
        """hipbm25_score_info (synchronises), of the last score_ids call: valid and padding entries, workgroups launched and
        posting probes (bisections: the sum over valid entries of the query's slots with a non-empty list)."""
        v = np.zeros(4, dtype=np.int64)
        nat.call("hipbm25_score_info", self._h, v.ctypes.data)
        return {"valid": int(v[0]), "padding": int(v[1]), "workgroups": int(v[2]), "probes": int(v[3])}

    def scoped_info(self) -> dict:
        """hipbm25_scoped_info (synchronises): documents per tile and, of the last scoped call, its work items (query x tile
        that holds a document of the query's scope), the tiles of its largest scope and its chunks."""
        v = np.zeros(4, dtype=np.int64)
        nat.call("hipbm25_scoped_info", self._h, v.ctypes.data)
        return {"tile_docs": int(v[0]), "work_items": int(v[1]), "max_scope_tiles": int(v[2]), "chunks": int(v[3])}

    def stats(self) -> dict:
        st = nat.HipBm25Stats()
        nat.call("hipbm25_get_stats", self._h, ctypes.byref(st))
        return {f: getattr(st, f) for f, _ in st._fields_}


def _weighted_accumulators(postings: PostingsCSR, query: Sequence[int], weights) -> np.ndarray:
    """float32 [n_docs]: acc[d] = fl32(acc[d] + fl32(w_t * impact[t, d])) over the query's term slots IN ORDER -- the one
    arithmetic of weighted_search_reference and bm25_score_ids_reference.  Zero weights and term ids outside [0, n_terms) add
    nothing; a repeated term is two slots."""
    off = np.asarray(postings.offsets, dtype=np.int64)
    docs = np.asarray(postings.doc_ids, dtype=np.int64)
    imp = np.asarray(postings.impacts, dtype=np.float32)
    acc = np.zeros(postings.n_docs, dtype=np.float32)
    for t, w in zip(query, np.asarray(weights, dtype=np.float32).reshape(-1)):
        t = int(t)
        if w == 0 or t < 0 or t >= postings.n_terms:
            continue
        d = docs[off[t]:off[t + 1]]
        acc[d] = acc[d] + np.float32(w) * imp[off[t]:off[t + 1]]     # float32 * float32 -> float32, then a float32 add
    return acc


def bm25_score_ids_reference(postings: PostingsCSR, queries: Sequence[Sequence[int]], weights, ids, id_base: int = 0) -> np.ndarray:
    """The semantics of hipbm25_score_ids as a pure function over numpy arrays (no GPU): float32 [nq, depth].  Entry (i, j) = c
    is valid iff c >= 0 and 0 <= c - id_base < n_docs and then holds the accumulator weighted_search_reference forms for that
    document (0.0 when no slot matches); any other entry holds -FLT_MAX.  `weights` None: every weight 1.0."""
    ids = np.asarray(ids, dtype=np.int64)
    out = np.full(ids.shape, -np.finfo(np.float32).max, dtype=np.float32)
    for b in range(len(queries)):
        w = np.ones(len(queries[b]), dtype=np.float32) if weights is None else weights[b]
        acc = _weighted_accumulators(postings, queries[b], w)
        local = ids[b] - int(id_base)
        ok = (ids[b] >= 0) & (local >= 0) & (local < postings.n_docs)
        out[b, ok] = acc[local[ok]]
    return out


def weighted_search_reference(postings: PostingsCSR, queries: Sequence[Sequence[int]], weights: Sequence[Sequence[float]], k: int,
                              ranges=None) -> Tuple[np.ndarray, np.ndarray]:
    """numpy restatement of hipbm25_search_weighted (and, with `ranges`, of the scoped form): per query
    acc[d] = fl32(acc[d] + fl32(w_t * impact[t, d])) over its term slots IN ORDER, all in float32 -- numpy rounds the product
    to float32 before the add, which is the two-rounding rule of the kernels.  A term id outside [0, n_terms) scores nothing;
    a repeated term is two slots.  Documents with score <= 0 are excluded, order (score desc, id asc), padding
    (-FLT_MAX, -1).  `ranges`: ranges[b] = the half-open (lo, hi) document ranges of query b's scope; only documents inside
    them are ranked.  Zero weights are dropped, as the search methods drop them."""
    nq = len(queries)
    out_s = np.full((nq, k), -np.finfo(np.float32).max, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    for b in range(nq):
        acc = _weighted_accumulators(postings, queries[b], weights[b])
        keep = acc > 0
        if ranges is not None:
            inside = np.zeros(postings.n_docs, dtype=bool)
            for lo, hi in ranges[b]:
                inside[int(lo):int(hi)] = True
            keep &= inside
        ids = np.flatnonzero(keep)
        order = np.lexsort((ids, -acc[ids].astype(np.float64)))[:k]
        out_s[b, :len(order)] = acc[ids[order]]
        out_i[b, :len(order)] = ids[order]
    return out_s, out_i


def batch_csr(doc_of_tok: np.ndarray, term_of_tok: np.ndarray, n_docs: int, n_terms: int,
              doc_len: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Token stream of a BATCH of documents (ids 0 .. n_docs - 1, local to the batch) -> (offsets uint64 [n_terms + 1],
    doc_ids uint32, tf uint32, doc_len uint32 [n_docs]): the CSR build_postings forms, without impacts -- what
    hipbm25_create_tf and hipbm25_append take."""
    doc_of_tok = np.asarray(doc_of_tok, dtype=np.int64)
    term_of_tok = np.asarray(term_of_tok, dtype=np.int64)
    if doc_len is None:
        doc_len = np.bincount(doc_of_tok, minlength=n_docs)
    pair = np.sort(term_of_tok * np.int64(max(n_docs, 1)) + doc_of_tok, kind="stable")
    if pair.size:
        first = np.ones(pair.size, dtype=bool)
        first[1:] = pair[1:] != pair[:-1]
        starts = np.flatnonzero(first)
        uniq = pair[starts]
        tf = np.diff(np.append(starts, pair.size))
    else:
        uniq, tf = pair, np.zeros(0, dtype=np.int64)
    term = uniq // max(n_docs, 1)
    offsets = np.zeros(n_terms + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(term, minlength=n_terms)).astype(np.uint64)
    return (offsets, (uniq - term * max(n_docs, 1)).astype(np.uint32), tf.astype(np.uint32),
            np.ascontiguousarray(doc_len, dtype=np.uint32))


def tokens_of_texts(texts: Sequence[str], vocab: Dict[str, int]) -> Tuple[np.ndarray, np.ndarray]:
    """(doc_of_tok, term_of_tok) of `texts`; `vocab` grows in order of first appearance, as in build_postings_from_texts."""
    docs: List[int] = []
    terms: List[int] = []
    for i, t in enumerate(texts):
        for tok in tokenize(t or ""):
            terms.append(vocab.setdefault(tok, len(vocab)))
            docs.append(i)
    return np.asarray(docs, np.int64), np.asarray(terms, np.int64)


UPDATE_KINDS = {0: "none", 1: "create_tf", 2: "append", 3: "remove_ranges", 4: "create_impacts", 5: "append_impacts", 6: "append_rows_dev"}


class HipBM25Updatable(HipBM25):
    """A HipBM25 that follows its collection on the device (hipbm25_create_tf / _append / _remove_ranges / _reweigh).

    Defining property: after any sequence of appends and removals, once committed, the handle is bit for bit
    HipBM25(build_postings(...)) over the surviving documents in order with the same term ids -- its export and every search
    and hybrid result.  append_* and remove_ranges change structure only and leave the handle dirty; commit() computes idf
    with numpy (the very expression of build_postings) from the handle's offsets and has the GPU recompute every impact.
    Every search method (and the hybrid entries, which flatten their queries through this object) commits first when the
    handle is dirty, so a bulk ingest appends many documents and pays for one reweigh.
    Out of scope: a postings file or persisted vocabulary, sharded collections, scope-local idf, asynchronous updates (the
    update entries synchronise, and the caller must have no search in flight on the handle)."""

    def __init__(self, postings: Optional[PostingsCSR] = None, device: int = 0, id_base: int = 0, k1: float = K1, b: float = B):
        """`postings` from build_postings / build_postings_from_texts (their tfs and doc_len; the impacts are not used), or
        None for an empty index of one term id."""
        if postings is None:
            postings = PostingsCSR(0, 1, np.zeros(2, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), {},
                                   np.zeros(0, np.uint32), np.zeros(0, np.int64))
        if postings.tfs is None or postings.doc_len is None:
            raise ValueError("HipBM25Updatable needs postings with tfs and doc_len (build_postings fills them)")
        self.device = int(device)
        self.auto_commit = True
        off = np.ascontiguousarray(postings.offsets, dtype=np.uint64)
        ids = np.ascontiguousarray(postings.doc_ids, dtype=np.uint32)
        tfs = np.ascontiguousarray(postings.tfs, dtype=np.uint32)
        dl = np.ascontiguousarray(postings.doc_len, dtype=np.uint32)
        if off.shape[0] != postings.n_terms + 1 or ids.shape != tfs.shape or int(off[-1]) != ids.shape[0] or dl.shape[0] != postings.n_docs:
            raise ValueError("inconsistent CSR postings")
        h = ctypes.c_uint64()
        nat.call("hipbm25_create_tf", int(postings.n_docs), int(postings.n_terms), off.ctypes.data, ids.ctypes.data, tfs.ctypes.data,
                 dl.ctypes.data, float(k1), float(b), self.device, ctypes.byref(h))
        self._h = h.value
        # the host keeps sizes and the vocabulary only: the postings live on the device (export() reads them back)
        self.p = PostingsCSR(int(postings.n_docs), int(postings.n_terms), None, None, None,
                             dict(postings.vocab) if postings.vocab is not None else None)
        if id_base:
            nat.call("hipbm25_set_id_base", self._h, int(id_base))
        self.commit()       # numpy's idf in place of the library's own

    @classmethod
    def from_texts(cls, texts: Sequence[str], **kw) -> "HipBM25Updatable":
        return cls(build_postings_from_texts(texts), **kw)

    @classmethod
    def from_tokens(cls, doc_of_tok, term_of_tok, n_docs: int, n_terms: int, doc_len=None, **kw) -> "HipBM25Updatable":
        off, ids, tf, dl = batch_csr(doc_of_tok, term_of_tok, n_docs, n_terms, doc_len)
        return cls(PostingsCSR(n_docs, n_terms, off, ids, np.zeros(ids.shape, np.float32), None, tf, dl), **kw)

    # ---- state ----
    def sizes(self) -> dict:
        v = np.zeros(4, dtype=np.int64)
        nat.call("hipbm25_sizes", self._h, v.ctypes.data)
        return {"n_docs": int(v[0]), "n_terms": int(v[1]), "postings": int(v[2]), "has_tf": bool(v[3] & 1), "dirty": bool(v[3] & 2)}

    @property
    def dirty(self) -> bool:
        return self.sizes()["dirty"]

    def export(self) -> dict:
        """hipbm25_export: offsets, doc_ids, tf, impacts and doc_len as host arrays (the impacts of a dirty handle are stale)."""
        sz = self.sizes()
        out = {"n_docs": sz["n_docs"], "n_terms": sz["n_terms"],
               "offsets": np.zeros(sz["n_terms"] + 1, np.uint64), "doc_ids": np.zeros(sz["postings"], np.uint32),
               "tf": np.zeros(sz["postings"], np.uint32), "impacts": np.zeros(sz["postings"], np.float32),
               "doc_len": np.zeros(sz["n_docs"], np.uint32)}
        nat.call("hipbm25_export", self._h, out["offsets"].ctypes.data, out["doc_ids"].ctypes.data, out["tf"].ctypes.data,
                 out["impacts"].ctypes.data, out["doc_len"].ctypes.data)
        return out

    def update_info(self) -> dict:
        """hipbm25_update_info: the last create / append / removal."""
        v = np.zeros(8, dtype=np.int64)
        nat.call("hipbm25_update_info", self._h, v.ctypes.data)
        return {"kind": UPDATE_KINDS[int(v[0])], "postings_before": int(v[1]), "postings_after": int(v[2]), "postings_moved": int(v[3]),
                "docs_before": int(v[4]), "docs_after": int(v[5]), "extra_bytes": int(v[6]), "grew": bool(v[7])}

    # ---- updates ----
    def append_postings(self, n_new_docs: int, n_terms_after: int, offsets, doc_ids, tfs, doc_len) -> None:
        """hipbm25_append: a batch CSR over n_terms_after terms with doc ids local to the batch (batch_csr builds one)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ids = np.ascontiguousarray(doc_ids, dtype=np.uint32)
        tf = np.ascontiguousarray(tfs, dtype=np.uint32)
        dl = np.ascontiguousarray(doc_len, dtype=np.uint32)
        if off.shape[0] != n_terms_after + 1 or ids.shape != tf.shape or int(off[-1]) != ids.shape[0] or dl.shape[0] != n_new_docs:
            raise ValueError("inconsistent batch CSR")
        nat.call("hipbm25_append", self._h, int(n_new_docs), int(n_terms_after), off.ctypes.data, ids.ctypes.data if ids.size else None,
                 tf.ctypes.data if tf.size else None, dl.ctypes.data if dl.size else None)
        self.p.n_docs += int(n_new_docs)
        self.p.n_terms = int(n_terms_after)

    def append_tokens(self, doc_of_tok, term_of_tok, n_new_docs: int, n_terms_after: Optional[int] = None, doc_len=None) -> None:
        n_terms_after = self.p.n_terms if n_terms_after is None else int(n_terms_after)
        self.append_postings(n_new_docs, n_terms_after, *batch_csr(doc_of_tok, term_of_tok, n_new_docs, n_terms_after, doc_len))

    def append_texts(self, texts: Sequence[str]) -> Tuple[int, int]:
        """Append one document per text; the vocabulary grows in order of first appearance, the batch CSR is built on the
        host over these texts only.  Returns the documents' id range [lo, hi).  A refused batch leaves the vocabulary as
        it was."""
        if self.p.vocab is None:
            raise ValueError("index was built from term ids, not texts")
        vocab = dict(self.p.vocab)
        docs, terms = tokens_of_texts(texts, vocab)
        lo = self.p.n_docs
        self.append_tokens(docs, terms, len(texts), max(len(vocab), self.p.n_terms),
                           np.bincount(docs, minlength=len(texts)) if docs.size else np.zeros(len(texts), np.int64))
        self.p.vocab = vocab
        return lo, lo + len(texts)

    def remove_ranges(self, ranges) -> int:
        """hipbm25_remove_ranges: drop the documents of half-open ranges [(lo, hi)] (ascending, not overlapping); the
        survivors keep their order and are renumbered.  Returns the documents removed."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 2))
        nat.call("hipbm25_remove_ranges", self._h, r.ctypes.data if r.size else None, int(r.shape[0]))
        before = self.p.n_docs
        self.p.n_docs = self.sizes()["n_docs"]
        return before - self.p.n_docs

    def idf(self) -> np.ndarray:
        """numpy's idf per term from the handle's offsets: the expression of build_postings, array for array."""
        sz = self.sizes()
        off = np.zeros(sz["n_terms"] + 1, np.uint64)
        nat.call("hipbm25_export", self._h, off.ctypes.data, None, None, None, None)
        df_all = np.diff(off.astype(np.int64)).astype(np.float64)
        n_all = float(sz["n_docs"])
        return np.log(1.0 + (n_all - df_all + 0.5) / (df_all + 0.5))

    def commit(self, library_idf: bool = False) -> None:
        """hipbm25_reweigh: recompute every impact and the skip tables; clears the dirty state.  `library_idf`: let the
        library evaluate idf with the C library's log instead (impacts equal numpy's or are the adjacent fp32 value)."""
        if library_idf:
            nat.call("hipbm25_reweigh", self._h, None)
            return
        idf = np.ascontiguousarray(self.idf(), dtype=np.float64)
        nat.call("hipbm25_reweigh", self._h, idf.ctypes.data if idf.size else None)

    def _flatten(self, queries):   # every search method and hybrid entry passes here first
        if self.auto_commit and self.dirty:
            self.commit()
        return HipBM25._flatten(queries)
