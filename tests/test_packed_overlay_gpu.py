"""
HIP_ENCODER_PACKED=true in the drop-in: the hip embedding provider encodes through hipenc_forward_packed (input-order batches,
no padding to a batch's longest text), and the retriever's rerank over collection rows goes through the packed rerank entry.
With the setting unset nothing changes (the other overlay tests run that way).
"""
import asyncio
import json

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

D, DEPTH, TOP_K, L = 64, 12, 5, 128
RERANK_ATOL = 1.5e-2            # tests/test_encoder_gpu.py::test_reranker_head_logits
WORDS = [f"w{j}" for j in range(30)]


def test_provider_embeds_through_the_packed_entry(gpu, monkeypatch):
    from rag.providers.hip.embeddings import HipEmbeddingProvider
    monkeypatch.setenv("HIP_ALLOW_SYNTHETIC", "1")
    monkeypatch.setenv("HIP_ENCODER_CONFIG", json.dumps(dict(vocab=2000, hidden=256, layers=2, heads=4, ffn=512, max_pos=200, max_seq_len=128)))
    for name in ("HIP_ENCODER_WEIGHTS", "HIP_TOKENIZER_FILE", "HIP_ENCODER_PACKED", "HIPENC_SMALL_ROWS", "HIPENC_GEMM256"):
        monkeypatch.delenv(name, raising=False)
    prov = HipEmbeddingProvider()
    rng = np.random.default_rng(3)
    texts = [" ".join(rng.choice(WORDS, size=n)) for n in (3, 90, 17, 1, 200, 40, 64, 8)] + ["", "  "]
    before = prov.encoder.packed_info()
    padded = np.asarray(asyncio.run(prov.embed_batch(texts)))
    assert prov.encoder.packed_info() == before                          # the default provider never takes the packed entry
    monkeypatch.setenv("HIP_ENCODER_PACKED", "true")
    packed = np.asarray(asyncio.run(prov.embed_batch(texts)))
    Tp, real, nseq, _path = prov.encoder.packed_info()
    assert nseq == len(texts) and Tp % 64 == 0 and 0 < real <= Tp
    assert packed.shape == padded.shape and np.allclose(packed, padded, atol=2e-3)
    one = np.asarray(asyncio.run(prov.embed_single(texts[1])))
    assert prov.encoder.packed_info()[2] == 1 and np.allclose(one, padded[1], atol=2e-3)
    dev = asyncio.run(prov.embed_batch_device(texts)).cpu().numpy()
    assert np.array_equal(dev, packed.astype(np.float32))


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
    return [f"c{i} " + " ".join(rng.choice(WORDS, size=3 + (i * 7) % 23)) for i in range(n)]


def test_collection_rerank_goes_through_the_packed_entry(gpu, tmp_path, monkeypatch):
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    from hiprag import EncoderConfig, HipEncoder, random_state
    from rag.ingest.indexing import index_chunks
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
    monkeypatch.setenv("HIP_ENCODER_PACKED", "true")
    qp = _QueryProvider()
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: qp)
    hi.clear_caches()
    cfg = EncoderConfig(vocab=2000, hidden=256, layers=2, heads=4, ffn=512, max_pos=200, max_seq_len=L)
    enc = HipEncoder(cfg, random_state(cfg, seed=9, with_head=True), with_head=True)
    tok = HashTokenizer(cfg.vocab)
    monkeypatch.setattr(rt, "_RERANKER", CrossEncoderReranker(encoder=enc, tokenizer=tok, top_k=TOP_K))

    for j, (doc, n) in enumerate((("docA", 9), ("docB", 7))):
        x, texts = ho.synthetic_vectors(n, D, seed=700 + j), _texts(n, 800 + j)
        chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": 1 + i // 4, "metadata": {"title": doc}} for i, t in enumerate(texts)]
        with open(tmp_path / f"{doc}_chunks.json", "w") as f:
            json.dump({"total": len(chunks), "chunks": chunks}, f)
        asyncio.run(index_chunks(doc, chunks, storage_dir=tmp_path, provider=_TableProvider(x), with_sparse=True, project="red"))
        if doc == "docB":
            query_vec = x[4]
    query = "w3 w17 w5"
    qp.table[query] = query_vec
    plain = asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, rerank=False).retrieve_chunks(query))
    got = asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, rerank=None).retrieve_chunks(query))
    live = passages.live_collection_tokens(col.open_collection(tmp_path))
    assert live is not None
    valid, padding, rows, batches = live[0].rerank_packed_info()
    assert rows > 0 and batches >= 1 and valid >= TOP_K                   # the call went through hiprerank_packed_*
    # ... and gives the host path's logits for the same pairs (padded entry, host-built), in their order
    host = enc.score_tokens([tok.encode_pair(query, c.text.replace("\n", " "), L) for c in plain]).cpu().numpy()
    by_id = {c.chunk_id: float(h) for c, h in zip(plain, host)}
    assert len(got) == TOP_K
    scores = [c.metadata["rerank_score"] for c in got]
    assert scores == sorted(scores, reverse=True)
    assert all(abs(s - by_id[c.chunk_id]) <= RERANK_ATOL for s, c in zip(scores, got))
    assert min(scores) >= sorted(host)[-TOP_K] - 2 * RERANK_ATOL
    hi.clear_caches()
