"""
rag/query/retriever.py -- the retriever the north star names; with hybrid search off it is the reference's
PageLevelRetriever (rag/query/page_retriever.py:78-288) step for step:

    embed query (no instruction, :109-110) -> vector search, limit = top_chunks = 50 (:117-121)
    -> RetrievedChunk list in search order (:123-139) -> group by page in first-seen order (:145-164)
    -> page score = mean(chunk scores) + min(0.05 * n, 0.15) in Python floats, stable sort descending (:166-213)
    -> first max_pages pages (:215-236)

With hybrid search on (HYBRID_SEARCH_ENABLED, rag/config.py:43) the chunk list is the reciprocal-rank fusion of the
dense list and a BM25 list over the same chunks (both depth top_chunks) -- the hybrid the reference's README.md:54-58
describes but never implements; spec in DESIGN.md.  Fusion order decides which chunks survive; each chunk keeps its
dense similarity as `score` so page scores stay on the reference's 0..1 scale; a chunk only the sparse leg found has
score 0.0 and metadata["sparse_only"], which keeps it out of its page's mean (it still counts for the chunk boost);
metadata["rrf_score"] / ["bm25_score"] carry the rest.  HIP_HYBRID_SCORE_ALL=true (default false): such a chunk is scored
exactly, by id (HipFlatIndex.score_ids), carries that similarity and metadata["dense_scored"] instead, and no chunk is
sparse-only -- every chunk rank_pages sees has a similarity, as in the reference (page_retriever.py:191).

Dense search, BM25 and RRF run in libhiprag.so; grouping and page ranking are a few dozen Python float operations and
stay on the host exactly as the reference has them -- unless HIP_PAGES=true (with HIP_COLLECTION=true): then
retrieve_and_rank_pages ranks the pages on the device as well (hippage_rank_dev, HybridRetriever._rank_pages_on_device) and
reads back only the selected pages.

HIP_LATE_INTERACTION=true (with HIP_COLLECTION=true): the query is embedded with its per-token vectors from one forward
(embed_single_colbert), the top chunks are reordered by late interaction over the collection's multi-vector store
(hipmaxsim_dev) and the first RERANKER_TOP_K go on; each carries metadata["colbert_score"] and ["rerank_mode"] = "colbert".
It stands where the cross-encoder stands: asking for both raises.

HIP_LATE_SEARCH=true (with HIP_LATE_INTERACTION=true, not on a hybrid retriever): late interaction is the FIRST stage -- ONE
MaxSim search over every chunk of the project (hipmaxsim_search_scoped_dev) gives the top_chunks candidates, the first
RERANKER_TOP_K go on; `score` is each chunk's exact dense similarity (score_ids), metadata["rerank_mode"] = "colbert_search".
Under HIP_PAGES the ids stay on the device: maxsim_search_device -> score_ids_device -> rank_pages_device.

HIP_M3_SCORE=true (with HIP_COLLECTION=true, HIP_COLLECTION_SPARSE=lexical and HIP_LATE_INTERACTION=true): BGE-M3's own ranking.
The query is embedded ONCE for all three outputs (embed_single_m3), the first stage is the one the retriever would run anyway
(the scoped dense search, or with hybrid=True the scoped lexical hybrid), and its top_chunks are reordered by the weighted sum
of their dense, lexical and ColBERT scores (hipm3_score_dev, HIP_M3_WEIGHTS); the first RERANKER_TOP_K go on with
metadata["m3_score"], ["m3_dense"], ["m3_sparse"], ["m3_colbert"] and ["rerank_mode"] = "m3".  It is a second stage: it raises
with HIP_RERANK, HIP_LATE_SEARCH and HIP_PAGES (the device page path is out of scope).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional

from rag.config import config
from rag.llm.embeddings.factory import get_embedding_provider
from rag.logging import logger


@dataclass
class RetrievedChunk:
    """Retrieved chunk with similarity score (page_retriever.py:25-32)."""
    chunk_id: str
    text: str
    score: float
    page: int
    metadata: Dict[str, Any]


@dataclass
class PageRanking:
    """Page with ranking score and its chunks (fields of page_retriever.py:35-41)."""
    page: int
    score: float
    chunks: List[RetrievedChunk]
    metadata: Dict[str, Any]

    # The two formatters the reference's response stage calls on every selected page (page_response.py:73 and :163);
    # their OUTPUT is pinned by tests/golden (page_formatting, produced by running the reference's own methods).
    _HEADING = (("chapter", "Chapter {}"), ("section", "Section {}"), ("title", "{}"))
    _CITED = (("chapter", "chapter"), ("section", "section"), ("subsection", "subsection"), ("title", "title"),
              ("source_file", "source_filename"))

    def get_context_text(self) -> str:
        """Prompt context of this page (same text as page_retriever.py:43-63): an optional `[Chapter c | Section s | title]`
        heading built from the truthy metadata fields, then the chunk texts, blank-line separated, outer whitespace stripped."""
        heading = " | ".join(fmt.format(self.metadata[key]) for key, fmt in self._HEADING if self.metadata.get(key))
        blocks = [f"[{heading}]"] if heading else []
        blocks.extend(chunk.text for chunk in self.chunks)
        return "\n\n".join(blocks).strip()

    def to_citation(self) -> Dict[str, Any]:
        """Citation record of this page (same keys and rounding as page_retriever.py:65-75)."""
        cite: Dict[str, Any] = {"page": self.page}
        for out_key, meta_key in self._CITED:
            cite[out_key] = self.metadata.get(meta_key)
        cite["relevance_score"] = round(self.score, 3)
        return cite


def group_chunks_by_page(chunks: List[RetrievedChunk]) -> Dict[int, List[RetrievedChunk]]:
    grouped: Dict[int, List[RetrievedChunk]] = {}
    for chunk in chunks:
        grouped.setdefault(chunk.page, []).append(chunk)
    return grouped


def rank_pages(chunks_by_page: Dict[int, List[RetrievedChunk]]) -> List[PageRanking]:
    """page score = mean(chunk scores) + min(0.05 n, 0.15), stable sort descending (page_retriever.py:166-213).
    Hybrid mode only: a chunk that ONLY the BM25 leg found has no dense similarity; it counts towards n (extra lexical
    evidence raises the page) but stays out of the mean -- averaging a 0.0 in would make a page rank LOWER for having
    more evidence.  With hybrid off no chunk is sparse-only and this is the reference's arithmetic unchanged."""
    rankings = []
    for page_num, page_chunks in chunks_by_page.items():
        scored = [c.score for c in page_chunks if not c.metadata.get("sparse_only")]
        avg_score = sum(scored) / len(scored) if scored else 0.0
        chunk_boost = min(len(page_chunks) * 0.05, 0.15)
        rankings.append(PageRanking(page=page_num, score=avg_score + chunk_boost, chunks=page_chunks,
                                    metadata=page_chunks[0].metadata))
    rankings.sort(key=lambda r: r.score, reverse=True)       # stable: ties keep first-seen page order
    return rankings


_META_KEYS = ("chapter", "section", "subsection", "title", "source_filename", "doc_id")    # page_retriever.py:129-136
_HYBRID_KEYS = ("rrf_score", "bm25_score", "sparse_only", "dense_scored")
_LEXICAL_KEYS = ("sparse_mode",)      # HIP_SPARSE_MODE / HIP_COLLECTION_SPARSE = lexical only: which sparse leg bm25_score comes from


def _as_chunk(result: dict) -> RetrievedChunk:
    """One enriched search row -> RetrievedChunk with the reference's defaults (page_retriever.py:123-139)."""
    metadata: Dict[str, Any] = {key: result.get(key) for key in _META_KEYS}
    metadata.update((key, result[key]) for key in _HYBRID_KEYS + _LEXICAL_KEYS if key in result)
    return RetrievedChunk(result.get("chunk_id", "unknown"), result.get("text", ""), result.get("score", 0),
                          result.get("page", 0), metadata)


class HybridRetriever:
    """Retrieve and rank at page level; `hybrid=None` follows HYBRID_SEARCH_ENABLED, False = the reference's path.
    `rerank=None` follows HIP_RERANK and RERANKER_ENABLED (both must be true), False = no reranking: when on, the
    top_chunks retrieved chunks are reranked by the cross-encoder and the first RERANKER_TOP_K go on to page grouping."""

    def __init__(self, top_chunks: int = 50, top_pages: int = 5, hybrid: Optional[bool] = False,
                 rrf_c: float = 60.0, weighted: bool = False, rerank: Optional[bool] = False):
        self.top_chunks = top_chunks
        self.top_pages = top_pages
        self.hybrid = config.HYBRID_SEARCH_ENABLED if hybrid is None else hybrid
        self.rrf_c = rrf_c
        # weighted RRF uses the reference's unused knobs VECTOR_WEIGHT / BM25_WEIGHT (config.py:44-45)
        self.w_dense, self.w_sparse = (config.VECTOR_WEIGHT, config.BM25_WEIGHT) if weighted else (1.0, 1.0)
        self.rerank = (config.HIP_RERANK and config.RERANKER_ENABLED) if rerank is None else bool(rerank)

    async def retrieve_chunks(self, query: str, project: Optional[str] = None) -> List[RetrievedChunk]:
        logger.info(f"Retrieving top-{self.top_chunks} chunks for query")
        m3 = self._m3_score()                          # raises on the combinations HIP_M3_SCORE refuses, before anything is embedded
        late_search = self._late_search()              # raises on a hybrid or reranking retriever, before anything is embedded
        embedding_provider = get_embedding_provider()
        lexical_query = None
        if m3:
            # the query's vector, lexical weights and token vectors from ONE forward; the first stage is the one below
            if not hasattr(embedding_provider, "embed_single_m3"):
                raise RuntimeError("HIP_M3_SCORE=true needs an embedding provider with both heads (EMBEDDING_PROVIDER=hip)")
            query_embedding, q_terms, q_weights, q_vecs, q_counts = await embedding_provider.embed_single_m3(query)
            lexical_query = (q_terms, q_weights)
        elif self.hybrid and config.HIP_SPARSE_MODE == "lexical":
            # the query's vector and its lexical weights from one forward; the sparse leg scores with the query's own weights
            if not hasattr(embedding_provider, "embed_single_lexical"):
                raise RuntimeError("HIP_SPARSE_MODE=lexical needs an embedding provider with a lexical head (EMBEDDING_PROVIDER=hip)")
            query_embedding, q_terms, q_weights = await embedding_provider.embed_single_lexical(query)
            lexical_query = (q_terms, q_weights)
        elif self.hybrid and _collection_lexical():
            query_embedding, *lexical_query = await _embed_query_lexical(embedding_provider, query)
        elif self._late_interaction():
            query_embedding, q_vecs, q_counts = await _embed_query_colbert(embedding_provider, query)
        else:
            query_embedding = await embedding_provider.embed_single(query)
        if late_search:
            return self._maxsim_search(query_embedding, q_vecs, q_counts, project)
        if self.hybrid:
            search_results = self._hybrid_search(query, query_embedding, project, lexical_query=lexical_query)
        else:
            from rag.storage.hip_index import search_hip_by_vector
            search_results = await search_hip_by_vector(query_embedding, limit=self.top_chunks, project=project)
        chunks = [_as_chunk(result) for result in search_results]
        logger.info(f"Retrieved {len(chunks)} chunks")
        if m3:
            chunks = self._m3(chunks, query_embedding, lexical_query, q_vecs, q_counts) if chunks else chunks
        elif self.rerank and chunks:
            chunks = await self._rerank(query, chunks)
        elif self._late_interaction() and chunks:
            chunks = self._maxsim(chunks, q_vecs, q_counts)
        return chunks

    def _m3_score(self) -> bool:
        """HIP_M3_SCORE, read at use (it raises on every combination the setting refuses); on a reranking retriever it
        raises: two second stages."""
        on = config.HIP_M3_SCORE
        if on and self.rerank:
            raise ValueError("HIP_M3_SCORE=true on a reranking retriever asks for two second stages: choose the cross-encoder "
                             "or the combined score")
        return on

    def _m3(self, chunks: List[RetrievedChunk], query_embedding, lexical_query, q_vecs, q_counts) -> List[RetrievedChunk]:
        """The retrieved chunks in the order of BGE-M3's combined score, cut to RERANKER_TOP_K: ONE hipm3_score_dev call over
        their collection rows with the HIP_M3_WEIGHTS mix (no scope: the rows are already the project's).  Each keeps its
        dense similarity as `score` (page scores stay on the reference's scale) and gains metadata m3_score, m3_dense,
        m3_sparse, m3_colbert (the three components as their entries give them) and rerank_mode = "m3"."""
        import torch
        from hiprag import METRIC_L2, m3_score_device
        from rag.storage.hip_index.collection import open_collection
        from rag.storage.hip_index.passages import rows_of_chunks
        coll = open_collection()
        store = _multivec_of(coll)
        if coll.lex is None:
            raise RuntimeError("HIP_M3_SCORE=true, but the collection holds no lexical postings: ingest it under HIP_M3_SCORE=true")
        rows = rows_of_chunks(coll, chunks)
        dev = q_vecs.device
        cand = torch.tensor([rows], dtype=torch.int64, device=dev)
        q = torch.tensor([query_embedding], dtype=torch.float32, device=dev)
        out = m3_score_device(coll.index, coll.lex.bm, store, q, [list(lexical_query[0])], [lexical_query[1]], q_vecs, q_counts, cand,
                              min(config.RERANKER_TOP_K, len(rows)), weights=config.HIP_M3_WEIGHTS)
        parts = out["parts"][0].tolist()
        l2 = coll.index.metric == METRIC_L2            # the dense component as the score used it: 1 - dist / 2 on an L2 index
        kept = []
        for p, sc in zip(out["pos"][0].tolist(), out["scores"][0].tolist()):
            if p < 0:
                continue
            meta = chunks[p].metadata
            meta["m3_score"] = sc
            dense, meta["m3_sparse"], meta["m3_colbert"] = parts[p]
            meta["m3_dense"] = 1.0 - 0.5 * dense if l2 else dense
            meta["rerank_mode"] = "m3"
            kept.append(chunks[p])
        logger.info(f"Combined score over {len(chunks)} chunks, kept {len(kept)}")
        return kept

    def _late_interaction(self) -> bool:
        """HIP_LATE_INTERACTION, read at use; with a reranking retriever it raises: two second stages."""
        late = config.HIP_LATE_INTERACTION             # raises without HIP_COLLECTION or with HIP_RERANK
        if late and self.rerank:
            raise ValueError("HIP_LATE_INTERACTION=true on a reranking retriever asks for two second stages: choose the "
                             "cross-encoder or late interaction")
        return late

    def _late_search(self) -> bool:
        """HIP_LATE_SEARCH, read at use (it raises without HIP_LATE_INTERACTION); on a hybrid or a reranking retriever it raises."""
        on = config.HIP_LATE_SEARCH
        config.HIP_LATE_CANDIDATES                     # raises when set without HIP_LATE_SEARCH; the collection search reads it
        if on and self.hybrid:
            raise ValueError("HIP_LATE_SEARCH=true on a retriever with hybrid=True: fusing MaxSim with RRF is not supported; "
                             "choose hybrid search or the late-interaction search")
        if on:
            self._late_interaction()                   # raises on a reranking retriever
        return on

    def _maxsim_search(self, query_embedding, q_vecs, q_counts, project: Optional[str]) -> List[RetrievedChunk]:
        """HIP_LATE_SEARCH: the first stage IS the MaxSim search over every chunk of `project` (ONE
        hipmaxsim_search_scoped_dev call, collection.search_collection_maxsim; under HIP_LATE_CANDIDATES ONE
        hipmaxsim_search_pruned_dev call, whose exact stage sees the best candidates by centroid codes), top_chunks results, of which the first
        RERANKER_TOP_K go on.  `score` is the chunk's exact dense similarity (score_ids, the reader's transform), so page
        ranking keeps the reference's arithmetic; metadata carries colbert_score and rerank_mode = "colbert_search"."""
        from rag.storage.hip_index.collection import search_collection_maxsim
        rows = search_collection_maxsim(q_vecs, q_counts, self.top_chunks, project, query_vector=query_embedding)
        chunks = []
        for row in rows[:config.RERANKER_TOP_K]:
            chunk = _as_chunk(row)
            chunk.metadata["colbert_score"] = row["colbert_score"]
            chunk.metadata["rerank_mode"] = "colbert_search"
            chunks.append(chunk)
        logger.info(f"Late-interaction search found {len(rows)} chunks, kept {len(chunks)}")
        return chunks

    def _maxsim(self, chunks: List[RetrievedChunk], q_vecs, q_counts) -> List[RetrievedChunk]:
        """The retrieved chunks in late-interaction order, cut to RERANKER_TOP_K: ONE hipmaxsim_dev call over their collection
        rows.  Each keeps its dense similarity as `score` and gains metadata["colbert_score"] and ["rerank_mode"]."""
        import torch
        from hiprag import maxsim_device
        from rag.storage.hip_index.collection import open_collection
        from rag.storage.hip_index.passages import rows_of_chunks
        coll = open_collection()
        store = _multivec_of(coll)
        rows = rows_of_chunks(coll, chunks)
        cand = torch.tensor([rows], dtype=torch.int64, device=q_vecs.device)
        scores, _ids, pos, _ = maxsim_device(store, q_vecs, q_counts, cand, min(config.RERANKER_TOP_K, len(rows)), want_pairs=False)
        out = []
        for p, sc in zip(pos[0].tolist(), scores[0].tolist()):
            if p < 0:
                continue
            chunks[p].metadata["colbert_score"] = sc
            chunks[p].metadata["rerank_mode"] = "colbert"
            out.append(chunks[p])
        logger.info(f"Late interaction over {len(chunks)} chunks, kept {len(out)}")
        return out

    async def _rerank(self, query: str, chunks: List[RetrievedChunk]) -> List[RetrievedChunk]:
        """The retrieved chunks in cross-encoder order, cut to RERANKER_TOP_K.  Each keeps its dense similarity as `score`
        (page scores stay on the reference's scale) and gains metadata["rerank_score"].  HIP_COLLECTION=true: the device
        path over collection rows (CrossEncoderReranker.rerank_rows); otherwise the text path (rerank).  Missing model files
        raise RerankerError unless HIP_ALLOW_SYNTHETIC is set, as the reranker's constructor does."""
        reranker = _get_reranker()
        if not config.HIP_COLLECTION:
            return await reranker.rerank(query, chunks, config.RERANKER_TOP_K)
        import asyncio
        from rag.storage.hip_index.collection import open_collection
        from rag.storage.hip_index.passages import rows_of_chunks
        rows = rows_of_chunks(open_collection(), chunks)
        out = []
        for pos, _row, logit in await asyncio.to_thread(reranker.rerank_rows, query, rows, config.RERANKER_TOP_K):
            chunks[pos].metadata["rerank_score"] = logit
            out.append(chunks[pos])
        logger.info(f"Reranked {len(chunks)} chunks, kept {len(out)}")
        return out

    def _hybrid_search(self, query: str, query_embedding: List[float], project: Optional[str] = None, lexical_query=None) -> List[dict]:
        """dense top-K + BM25 top-K over the same chunk rows -> RRF -> enriched dicts in fusion order.
        `lexical_query` (HIP_SPARSE_MODE=lexical on the per-document path, HIP_COLLECTION_SPARSE=lexical on the collection): the
        query's (token ids, weights); the sparse leg is then the lexical postings searched with them (hipbm25_search_weighted /
        _scoped_weighted), dense and RRF unchanged, and every item carries sparse_mode = "lexical" with the lexical score
        under bm25_score.
        HIP_COLLECTION=true: ONE scoped library call over the documents of `project` (None: the whole collection),
        rag.storage.hip_index.collection.search_collection_hybrid.  Otherwise the first document's index and postings,
        `project` ignored, as the reference ignores it (rag/storage/faiss_index.py:150)."""
        if config.HIP_COLLECTION:
            from rag.storage.hip_index.collection import search_collection_hybrid
            return search_collection_hybrid(query, query_embedding, self.top_chunks, project, c=self.rrf_c, w_dense=self.w_dense,
                                            w_sparse=self.w_sparse, lexical_query=lexical_query)
        import numpy as np
        from hiprag import rrf_fuse
        from rag.storage.hip_index import enrich, open_first_index
        from rag.storage.hip_index.sparse import get_sparse_index
        opened = open_first_index()
        if opened is None:
            logger.warning("No HIP indices found")
            return []
        reader, doc_id, chunks_list = opened
        depth = self.top_chunks
        dense = [(rid, sc) for rid, sc in reader.search(query_embedding, top_k=depth) if 0 <= rid < len(chunks_list)]
        dense_ids = np.full((1, depth), -1, dtype=np.int64)
        dense_ids[0, :len(dense)] = [rid for rid, _ in dense]
        dense_score = {rid: sc for rid, sc in dense}
        if lexical_query is not None:
            from rag.storage.hip_index.sparse import get_lexical_index
            lex = get_lexical_index(config.STORAGE_DIR, doc_id, chunks_list)
            s_scores, s_ids = lex.search([list(lexical_query[0])], [lexical_query[1]], depth)
        else:
            bm25 = get_sparse_index(config.STORAGE_DIR, doc_id, chunks_list)
            s_scores, s_ids = bm25.search([bm25.terms_of(query)], depth)
        f_scores, f_ids = rrf_fuse(dense_ids, s_ids, depth, c=self.rrf_c, w_a=self.w_dense, w_b=self.w_sparse)
        bm25_of = {int(i): float(s) for i, s in zip(s_ids[0], s_scores[0]) if i >= 0}
        rescored: Dict[int, float] = {}
        if config.HIP_HYBRID_SCORE_ALL:          # the fused rows the dense list lacks get their exact score, by id
            missing = [int(rid) for rid in f_ids[0] if rid >= 0 and int(rid) not in dense_score]
            rescored = dict(reader.score_ids(query_embedding, missing)) if missing else {}
        fused = []
        for rid, fs in zip(f_ids[0], f_scores[0]):
            if rid < 0:
                continue
            rid = int(rid)
            item = enrich([(rid, dense_score.get(rid, rescored.get(rid, 0.0)))], chunks_list, compat_minus_one=False)[0]
            item["rrf_score"] = float(fs)
            if lexical_query is not None:
                item["sparse_mode"] = "lexical"
            if rid in bm25_of:
                item["bm25_score"] = bm25_of[rid]
            if rid in rescored:
                item["dense_scored"] = True
            elif rid not in dense_score:
                item["sparse_only"] = True       # no dense similarity: rank_pages keeps it out of the page mean
            fused.append(item)
        return fused

    # the three page-level steps keep the reference's method names
    def group_chunks_by_page(self, chunks: List[RetrievedChunk]) -> Dict[int, List[RetrievedChunk]]:
        return group_chunks_by_page(chunks)

    def rank_pages(self, chunks_by_page: Dict[int, List[RetrievedChunk]]) -> List[PageRanking]:
        return rank_pages(chunks_by_page)

    def select_top_pages(self, rankings: List[PageRanking], max_pages: Optional[int] = None) -> List[PageRanking]:
        max_pages = max_pages or self.top_pages
        selected = rankings[:max_pages]
        logger.info(f"Selected {len(selected)} pages from {len(rankings)} candidates")
        return selected

    async def _rank_pages_on_device(self, query: str, project: Optional[str], max_pages: int) -> Optional[List[PageRanking]]:
        """retrieve_and_rank_pages under HIP_PAGES=true and HIP_COLLECTION=true: the search results stay on the device
        (collection.search_collection_device: the library calls of the host path), the device reranker orders them when
        reranking is on (the candidates are then its output rows; the dense list is still the search's), hippage_rank_dev
        groups, scores and orders the pages over the collection's page table, the small outputs are copied once, and only
        the members of the selected pages are enriched from their chunk tables.  The PageRanking objects are the host
        path's: `score` of a chunk is its dense similarity, metadata carries rrf_score / bm25_score / sparse_only /
        rerank_score as there, a page's metadata is its first member's.  HIP_HYBRID_SCORE_ALL=true (hybrid only): the
        candidates are scored by id on the device (score_ids_device, after the rerank) and the candidate list is passed as
        its own dense list; a chunk whose id the search's dense list lacks carries dense_scored, none is sparse_only.

        THE DIFFERENCE FROM THE HOST PATH: pages are keyed by (document, page), the host path keys them by page number
        alone.  The result equals the host path's whenever no two documents among a query's candidates share a page
        number; otherwise it equals the host path run with (doc_id, page) as the chunk's page key -- page 3 of one document
        and page 3 of another are two pages here and one citation there.

        Returns None where the device path cannot answer and the host path must: a chunk page that is no int32 (logged)."""
        from hiprag import rank_pages_device
        from rag.storage.hip_index import collection as col
        from rag.storage.hip_index.pages import PageValueError, get_collection_pages
        if self.top_chunks > 256:
            raise RuntimeError(f"top_chunks={self.top_chunks} is beyond what the device page ranking takes (256): HIP_PAGES is on")
        self._m3_score()                                # HIP_M3_SCORE raises with HIP_PAGES: the device page path is out of scope
        late_search = self._late_search()               # raises on a hybrid or reranking retriever
        embedding_provider = get_embedding_provider()
        late = self._late_interaction()
        hybrid = bool(self.hybrid)
        if hybrid:
            config.HIP_SPARSE_MODE      # "lexical" raises here: it governs the per-document path (HIP_COLLECTION_SPARSE is the collection's)
        lexical_query = None
        if hybrid and _collection_lexical():
            query_embedding, *lexical_query = await _embed_query_lexical(embedding_provider, query)
        elif late:
            query_embedding, q_vecs, q_counts = await _embed_query_colbert(embedding_provider, query)
        else:
            query_embedding = await embedding_provider.embed_single(query)
        if late_search:
            # the first stage is the MaxSim search itself; its ids stay on the device and are scored by id below
            found = col.search_collection_maxsim_device(q_vecs, q_counts, self.top_chunks, project)
        else:
            found = col.search_collection_device(query_embedding, self.top_chunks, project, query_text=query if hybrid else None,
                                                 c=self.rrf_c, w_dense=self.w_dense, w_sparse=self.w_sparse, lexical_query=lexical_query)
        if found is None:
            logger.warning("No chunks retrieved")
            return []
        coll = found["coll"]
        try:
            table = get_collection_pages(coll)
        except PageValueError as e:
            logger.warning(f"The page table cannot hold this collection ({e}); pages are ranked on the host")
            return None
        cand, positions, logits = found["cand_ids"], None, None
        if late_search:
            keep = max(1, min(config.RERANKER_TOP_K, int(cand.shape[1])))
            cand, logits = cand[:, :keep].contiguous(), found["colbert_scores"][:, :keep].contiguous()
        elif self.rerank:
            logits, cand, positions = _get_reranker().rerank_rows_device(query, cand, config.RERANKER_TOP_K)
        elif late:
            # the candidates stay on the device between the search and the page ranking, as for the device rerank
            from hiprag import maxsim_device
            logits, cand, positions, _ = maxsim_device(_multivec_of(coll), q_vecs, q_counts, cand.contiguous(),
                                                       min(config.RERANKER_TOP_K, int(cand.shape[1])), want_pairs=False)
        depth = int(cand.shape[1])
        mp = max(1, min(int(max_pages), depth))
        score_all = hybrid and config.HIP_HYBRID_SCORE_ALL
        if late_search:
            # maxsim_search_device -> score_ids_device -> rank_pages_device: the candidates are their own dense list, as below
            import torch
            q_dev = torch.tensor([query_embedding], dtype=torch.float32, device=cand.device)
            scores64, _ = coll.index.score_ids_device(q_dev, cand)
            out = rank_pages_device(table, cand, cand, scores64, mp, metric=coll.index.metric)
        elif score_all:
            # every candidate is scored by id on the flat index (the bits the dense leg gives the rows it found) and the
            # candidate list is its own dense list, as for a dense-only caller: dense_pos >= 0 for every valid candidate
            scores64, _ = coll.index.score_ids_device(found["query"], cand)
            out = rank_pages_device(table, cand, cand, scores64, mp, metric=coll.index.metric)
        else:
            out = rank_pages_device(table, cand, found["dense_ids"], found["dense_scores"].double(), mp, metric=coll.index.metric)
        # the small outputs come over in two copies (the first synchronises); the candidate rows and what the metadata needs behind them
        n_pages, page_scores, _first, _members, page_no, cand_rank, dense_pos, cand_scores = (a[0].tolist() for a in out.host())
        cand_h = cand[0].tolist()
        pos_h = positions[0].tolist() if positions is not None else list(range(depth))
        logit_h = logits[0].tolist() if logits is not None else None
        fused_h = found["fused_scores"][0].tolist() if hybrid else None
        bm25_of = ({int(i): float(s) for i, s in zip(found["sparse_ids"][0].tolist(), found["sparse_scores"][0].tolist()) if i >= 0}
                   if hybrid else {})
        found_dense = set(found["dense_ids"][0].tolist()) if score_all else None
        logger.info(f"Ranked {n_pages} pages on the device")
        rankings = []
        for r in range(min(n_pages, mp)):
            chunks = []
            for j in range(depth):
                if cand_rank[j] != r:
                    continue
                row = cand_h[j]
                item = col._enrich(coll, [(row, cand_scores[j])])[0]
                if hybrid:
                    item["rrf_score"] = float(fused_h[pos_h[j]])
                    if "sparse_mode" in found:
                        item["sparse_mode"] = found["sparse_mode"]
                    if row in bm25_of:
                        item["bm25_score"] = bm25_of[row]
                    if score_all and row not in found_dense:
                        item["dense_scored"] = True
                    elif dense_pos[j] < 0:
                        item["sparse_only"] = True
                chunk = _as_chunk(item)
                if logit_h is not None and late:
                    chunk.metadata["colbert_score"] = logit_h[j]
                    chunk.metadata["rerank_mode"] = "colbert_search" if late_search else "colbert"
                elif logit_h is not None:
                    chunk.metadata["rerank_score"] = logit_h[j]
                chunks.append(chunk)
            rankings.append(PageRanking(page=page_no[r], score=page_scores[r], chunks=chunks, metadata=chunks[0].metadata))
        logger.info(f"Selected {len(rankings)} pages from {n_pages} candidates")
        return rankings

    async def retrieve_and_rank_pages(self, query: str, project: Optional[str] = None,
                                      max_pages: Optional[int] = None) -> List[PageRanking]:
        """Under HIP_PAGES=true with HIP_COLLECTION=true the pages are ranked on the device (_rank_pages_on_device, which
        states how that differs from this path); otherwise, and where the device path hands back, as ever."""
        if config.HIP_PAGES and config.HIP_COLLECTION:
            ranked = await self._rank_pages_on_device(query, project, max_pages or self.top_pages)
            if ranked is not None:
                return ranked
        chunks = await self.retrieve_chunks(query, project)
        if not chunks:
            logger.warning("No chunks retrieved")
            return []
        return self.select_top_pages(self.rank_pages(self.group_chunks_by_page(chunks)), max_pages)


PageLevelRetriever = HybridRetriever      # the reference's class name (page_retriever.py:78)

_RERANKER = None


async def _embed_query_colbert(provider, query: str):
    if not hasattr(provider, "embed_single_colbert"):
        raise RuntimeError("HIP_LATE_INTERACTION=true needs an embedding provider with a ColBERT head (EMBEDDING_PROVIDER=hip)")
    return await provider.embed_single_colbert(query)


def _collection_lexical() -> bool:
    """HIP_COLLECTION_SPARSE=lexical, read at use (it raises on an unknown value and on the combinations it refuses)"""
    return config.HIP_COLLECTION_SPARSE == "lexical"


async def _embed_query_lexical(provider, query: str):
    """the query's vector and its lexical (token ids, weights) from ONE forward"""
    if not hasattr(provider, "embed_single_lexical"):
        raise RuntimeError("HIP_COLLECTION_SPARSE=lexical needs an embedding provider with a lexical head (EMBEDDING_PROVIDER=hip)")
    return await provider.embed_single_lexical(query)


def _multivec_of(coll):
    if coll is None or coll.mv is None:
        raise RuntimeError("HIP_LATE_INTERACTION=true, but the collection holds no per-token vectors: ingest it under "
                           "HIP_LATE_INTERACTION=true")
    return coll.mv


def _get_reranker():
    """The process's CrossEncoderReranker, made at the first reranked query (it loads a 24-layer model)."""
    global _RERANKER
    if _RERANKER is None:
        from rag.query.reranker import CrossEncoderReranker
        _RERANKER = CrossEncoderReranker()
    return _RERANKER


async def retrieve_and_rank_pages(query: str, project: Optional[str] = None, top_pages: int = 5) -> List[PageRanking]:
    """Convenience function with the reference's signature (page_retriever.py:271-288)."""
    retriever = HybridRetriever(top_pages=top_pages, rerank=None)      # reranks only under HIP_RERANK (default off)
    return await retriever.retrieve_and_rank_pages(query, project, top_pages)
