"""CPU: the pair rule of the device rerank call as a pure function, and how HybridRetriever resolves its rerank switch."""
import asyncio
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TOKENIZER = os.path.join(HERE, "golden", "xlmr_style_unigram_tokenizer.json")

QUERIES = ["what is hybrid search", "", "the reranker scores query and passage together", "a"]
PASSAGES = ["Dense search finds the nearest vectors.", "", "BM25 ranks documents by term frequency and length. " * 3,
            "hybrid search fuses both lists with reciprocal rank fusion", "x"]


def test_pair_rule_equals_file_tokenizer_encode_pair():
    """pair_tokens over the token BODIES equals FileTokenizer.encode_pair over the texts, token for token: pairs that fit,
    pairs cut in the passage, a query longer than room (then nothing of the passage is left)."""
    from hiprag import pair_tokens
    from rag.providers.hip.tokenizer import FileTokenizer
    tk = FileTokenizer(TOKENIZER)
    body = lambda t: tk.encode(t, 10 ** 6)[1:-1]      # noqa: E731
    seen = set()
    for q in QUERIES:
        for p in PASSAGES:
            bq, bp = body(q), body(p)
            total = len(bq) + len(bp)
            for L in sorted({5, 8, 16, len(bq) + 3, len(bq) + 4, len(bq) + 5, total + 3, total + 4, total + 5, 512}):
                if L < 5:
                    continue
                room = L - 4
                seen.add("fits" if total <= room else ("query longer than room" if len(bq) > room else "cut in the passage"))
                got = pair_tokens(bq, bp, L, tk.bos, tk.eos)
                assert got == tk.encode_pair(q, p, L), (q, p, L)
                assert len(got) <= max(L, 4) and got[0] == tk.bos and got[-1] == tk.eos
    assert seen == {"fits", "cut in the passage", "query longer than room"}


def test_pair_rule_equals_hash_tokenizer_where_the_pair_fits():
    from hiprag import pair_tokens
    from rag.providers.hip.tokenizer import HashTokenizer
    tk = HashTokenizer(2000)
    body = lambda t: tk.encode(t, 10 ** 6)[1:-1]      # noqa: E731
    for q in QUERIES:
        for p in PASSAGES:
            bq, bp = body(q), body(p)
            for L in (len(bq) + len(bp) + 4, len(bq) + len(bp) + 9, 512):
                if L >= 5:
                    assert pair_tokens(bq, bp, L, tk.bos, tk.eos) == tk.encode_pair(q, p, L), (q, p, L)


def test_passage_and_query_bodies_are_encode_minus_bos_eos():
    from rag.providers.hip.tokenizer import FileTokenizer
    from rag.storage.hip_index.passages import MAX_DOC_TOKENS, passage_tokens, query_tokens
    tk = FileTokenizer(TOKENIZER)
    text = "line one\nline two " * 200
    flat = text.replace("\n", " ")
    assert passage_tokens(tk, text) == tk.encode(flat, 10 ** 6)[1:-1][:MAX_DOC_TOKENS]
    assert len(passage_tokens(tk, text)) == MAX_DOC_TOKENS
    assert passage_tokens(tk, "") == [] and query_tokens(tk, "a\nb", 512) == tk.encode("a b", 10 ** 6)[1:-1]


@pytest.mark.parametrize("hip_rerank,enabled,want", [(None, True, False), ("false", True, False), ("true", True, True),
                                                     ("true", False, False), ("TRUE", True, True)])
def test_retriever_resolves_rerank_from_the_settings(monkeypatch, hip_rerank, enabled, want):
    import rag.query.retriever as rt
    if hip_rerank is None:
        monkeypatch.delenv("HIP_RERANK", raising=False)
    else:
        monkeypatch.setenv("HIP_RERANK", hip_rerank)
    monkeypatch.setattr(rt.config, "RERANKER_ENABLED", enabled)
    assert rt.HybridRetriever(rerank=None).rerank is want
    assert rt.HybridRetriever().rerank is False             # the default argument never reranks
    assert rt.HybridRetriever(rerank=True).rerank is True and rt.HybridRetriever(rerank=False).rerank is False


def test_retrieve_and_rank_pages_is_unchanged_with_the_setting_off(monkeypatch):
    """HIP_RERANK unset: the module-level function asks the settings, finds the switch off, and no reranker is ever made;
    the pages are those of a retriever built the old way."""
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    monkeypatch.delenv("HIP_RERANK", raising=False)
    monkeypatch.delenv("HIP_COLLECTION", raising=False)
    rows = [{"chunk_id": f"c{i}", "text": f"t{i}", "score": 0.9 - 0.01 * i, "page": 1 + i % 4, "title": "T"} for i in range(12)]

    class _Provider:
        async def embed_single(self, text, instruction=None):
            return [0.0]

    async def _search(vec, limit=50, project=None):
        return [dict(r) for r in rows]

    def _no_reranker():
        raise AssertionError("a reranker was asked for with HIP_RERANK unset")

    monkeypatch.setattr(rt, "get_embedding_provider", lambda: _Provider())
    monkeypatch.setattr(hi, "search_hip_by_vector", _search)
    monkeypatch.setattr(rt, "_get_reranker", _no_reranker)
    got = asyncio.run(rt.retrieve_and_rank_pages("q", None, 3))
    want = asyncio.run(rt.HybridRetriever(top_pages=3).retrieve_and_rank_pages("q", None, 3))
    assert [(p.page, p.score, [c.chunk_id for c in p.chunks]) for p in got] == \
           [(p.page, p.score, [c.chunk_id for c in p.chunks]) for p in want]
    assert len(got) == 3 and all("rerank_score" not in c.metadata for p in got for c in p.chunks)


def test_retriever_reranks_through_the_text_path_without_a_collection(monkeypatch):
    """rerank=True without HIP_COLLECTION: the existing CrossEncoderReranker.rerank over chunk texts, cut to RERANKER_TOP_K;
    each chunk keeps its dense score."""
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    monkeypatch.delenv("HIP_COLLECTION", raising=False)
    monkeypatch.setattr(rt.config, "RERANKER_TOP_K", 4)
    rows = [{"chunk_id": f"c{i}", "text": f"t{i}", "score": 0.9 - 0.01 * i, "page": 1} for i in range(9)]

    class _Provider:
        async def embed_single(self, text, instruction=None):
            return [0.0]

    class _Reranker:
        async def rerank(self, query, chunks, top_k=None):
            order = sorted(range(len(chunks)), key=lambda i: (-(i % 3), i))[:top_k]
            for i in order:
                chunks[i].metadata["rerank_score"] = float(i % 3)
            return [chunks[i] for i in order]

    async def _search(vec, limit=50, project=None):
        return [dict(r) for r in rows]

    monkeypatch.setattr(rt, "get_embedding_provider", lambda: _Provider())
    monkeypatch.setattr(hi, "search_hip_by_vector", _search)
    monkeypatch.setattr(rt, "_get_reranker", lambda: _Reranker())
    chunks = asyncio.run(rt.HybridRetriever(rerank=True).retrieve_chunks("q"))
    assert [c.chunk_id for c in chunks] == ["c2", "c5", "c8", "c1"]
    assert [c.score for c in chunks] == [0.9 - 0.02, 0.9 - 0.05, 0.9 - 0.08, 0.9 - 0.01]
    assert [c.metadata["rerank_score"] for c in chunks] == [2.0, 2.0, 2.0, 1.0]
