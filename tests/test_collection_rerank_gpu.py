"""
Reranking inside the retriever over the collection: with HIP_COLLECTION=true and HIP_RERANK=true
HybridRetriever(rerank=None).retrieve_chunks returns RERANKER_TOP_K chunks in cross-encoder order (the device path over
collection rows), each with its dense score kept and rerank_score attached; the passage token store follows index_chunks,
delete_document and replace_document on the device; with HIP_RERANK unset the query returns what it returned before.
"""
import asyncio
import json

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

D, DEPTH, TOP_K, L = 64, 12, 5, 128
RERANK_ATOL = 1.5e-2            # tests/test_encoder_gpu.py::test_reranker_head_logits
DOCS = [("docA", "red", 9), ("docB", "blue", 6), ("docC", "red", 7)]
WORDS = [f"w{j}" for j in range(30)]


class _TableProvider:
    def __init__(self, x):
        self.x = x

    async def embed_batch(self, texts, instruction=None):
        return [[float(v) for v in self.x[int(t.split()[0][1:])]] for t in texts]


class _QueryProvider:
    def __init__(self):
        self.table = {}

    async def embed_single(self, text, instruction=None):
        return [float(v) for v in self.table[text]]


def _texts(n, seed):
    rng = np.random.default_rng(seed)
    return [f"c{i} " + " ".join(rng.choice(WORDS, size=3 + (i * 7) % 23)) + ("\nsecond line" if i % 3 == 0 else "") for i in range(n)]


def _index_doc(tmp_path, doc, x, texts, project, replace=False):
    from rag.ingest.indexing import index_chunks
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": 1 + i // 4, "metadata": {"title": doc}} for i, t in enumerate(texts)]
    with open(tmp_path / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=tmp_path, provider=_TableProvider(x), with_sparse=True, project=project,
                                    replace=replace))


def test_retriever_reranks_collection_rows_and_the_store_follows(gpu, tmp_path, monkeypatch):
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    from hiprag import EncoderConfig, HipEncoder, random_state
    from rag.providers.hip.tokenizer import HashTokenizer
    from rag.query.reranker import CrossEncoderReranker
    from rag.storage.hip_index import collection as col
    from rag.storage.hip_index import passages
    monkeypatch.setenv("HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "l2")
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    monkeypatch.setattr(hi.config, "HIP_SEARCH_ALL_DOCUMENTS", False)
    monkeypatch.setattr(hi.config, "RERANKER_ENABLED", True)
    monkeypatch.setattr(hi.config, "RERANKER_TOP_K", TOP_K)
    monkeypatch.setenv("STORAGE_DIR", str(tmp_path))
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_RERANK", "true")
    monkeypatch.setenv("HIP_ALLOW_SYNTHETIC", "1")
    qp = _QueryProvider()
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: qp)
    hi.clear_caches()

    # the reranker of the process: the small encoder of tests/test_hybrid_gpu.py and the synthetic tokenizer
    cfg = EncoderConfig(vocab=2000, hidden=256, layers=2, heads=4, ffn=512, max_pos=200, max_seq_len=L)
    enc = HipEncoder(cfg, random_state(cfg, seed=9, with_head=True), with_head=True)
    tok = HashTokenizer(cfg.vocab)
    reranker = CrossEncoderReranker(encoder=enc, tokenizer=tok, top_k=TOP_K)
    monkeypatch.setattr(rt, "_RERANKER", reranker)

    xs = {doc: ho.synthetic_vectors(n, D, seed=700 + j) for j, (doc, _p, n) in enumerate(DOCS)}
    texts = {doc: _texts(n, 800 + j) for j, (doc, _p, n) in enumerate(DOCS)}
    for doc, project, _n in DOCS:
        _index_doc(tmp_path, doc, xs[doc], texts[doc], project)
    query = "w3 w17\nw5"
    qp.table[query] = xs["docC"][4]

    def check_reranked(hybrid, project):
        plain = asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, hybrid=hybrid, rerank=False).retrieve_chunks(query, project))
        assert len(plain) > TOP_K and all("rerank_score" not in c.metadata for c in plain)
        got = asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, hybrid=hybrid, rerank=None).retrieve_chunks(query, project))
        # the logits of host-built pairs, through the existing entry
        pairs = [tok.encode_pair(query.replace("\n", " "), c.text.replace("\n", " "), L) for c in plain]
        host = enc.score_tokens(pairs).cpu().numpy()
        order = sorted(range(len(plain)), key=lambda i: (-host[i], i))[:TOP_K]
        print(f"\n[collection rerank hybrid={hybrid} project={project}] host logits {np.sort(host)[::-1][:TOP_K + 1]}")
        assert len(got) == TOP_K
        assert [c.chunk_id for c in got] == [plain[i].chunk_id for i in order]
        for c, i in zip(got, order):
            assert c.score == plain[i].score and c.text == plain[i].text           # the dense similarity is kept
            assert abs(c.metadata["rerank_score"] - float(host[i])) <= RERANK_ATOL
            if project is not None:
                assert c.metadata["doc_id"] in ("docA", "docC")
        return plain

    plain = check_reranked(False, None)
    check_reranked(False, "red")
    check_reranked(True, "red")

    def check_store(tag):
        coll = col.open_collection(tmp_path)
        live = passages.live_collection_tokens(coll)
        assert live is not None, tag                                               # it followed; it was not dropped
        followed = [a.tobytes() for a in live[0].export()]
        want = [passages.passage_tokens(tok, t) for t in col.collection_texts(coll.manifest, tmp_path)]
        assert len(live[0]) == coll.manifest.rows == len(want), tag
        passages.clear_token_cache()
        rebuilt = passages.get_collection_tokens(coll, tok)
        assert rebuilt is not live[0]
        assert [a.tobytes() for a in rebuilt.export()] == followed, tag
        off, tokens = rebuilt.export()
        assert [tokens[off[i]:off[i + 1]].tolist() for i in range(len(want))] == want, tag

    check_store("built by the first reranked query")
    asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, rerank=None).retrieve_chunks(query))       # live again after the rebuild above
    xs["docD"], texts["docD"] = ho.synthetic_vectors(5, D, seed=710), _texts(5, 810)
    _index_doc(tmp_path, "docD", xs["docD"], texts["docD"], "blue")
    check_store("index_chunks")
    asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, rerank=None).retrieve_chunks(query))
    col.delete_document("docA", tmp_path)
    check_store("delete_document")
    asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, rerank=None).retrieve_chunks(query))
    xs["docB"], texts["docB"] = ho.synthetic_vectors(8, D, seed=720), _texts(8, 820)
    _index_doc(tmp_path, "docB", xs["docB"], texts["docB"], "blue", replace=True)
    check_store("replace_document")
    got = asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, rerank=None).retrieve_chunks(query))
    assert len(got) == TOP_K and all(c.metadata["doc_id"] != "docA" for c in got)

    # the switch unset: what the query returns today, and no reranker is asked for
    monkeypatch.delenv("HIP_RERANK")
    monkeypatch.setattr(rt, "_get_reranker", lambda: pytest.fail("a reranker was asked for with HIP_RERANK unset"))
    off = asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, rerank=None).retrieve_chunks(query))
    today = asyncio.run(rt.HybridRetriever(top_chunks=DEPTH).retrieve_chunks(query))
    assert [(c.chunk_id, c.score, c.metadata) for c in off] == [(c.chunk_id, c.score, c.metadata) for c in today]
    assert len(off) > TOP_K and all("rerank_score" not in c.metadata for c in off)
    assert len(plain) == DEPTH
    hi.clear_caches()
