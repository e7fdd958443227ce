"""
HIP_SPARSE_MODE=lexical in the drop-in, end to end on synthetic weights and 30 chunks: index_chunks takes the chunks' lexical
weights from the forward that makes their embeddings, builds the LexicalIndex, caches it and writes {doc_id}_hip.lexical.npz;
a cold cache loads the file; HybridRetriever(hybrid=True) searches it with the query's own weights (dense and RRF
unchanged); HIP_SPARSE_MODE=bm25 (or unset) is the parent's path; the collection combination raises.
"""
import asyncio
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DOC = "docL"
DEPTH = 20
WORDS = [f"w{j}" for j in range(40)]
QUERIES = ("w3 w17 w5 w8", "w1 w2 w30 w31 w32 w33", "W9 w9 w21 unknownword", "w12")
ENCODER = {"vocab": 200, "hidden": 128, "layers": 2, "heads": 2, "ffn": 256, "max_pos": 80, "max_seq_len": 64}


def _snapshot(chunks):
    return [(c.chunk_id, c.score, c.metadata.get("rrf_score"), c.metadata.get("bm25_score"), c.metadata.get("sparse_only"),
             c.metadata.get("sparse_mode")) for c in chunks]


def test_lexical_mode_end_to_end(gpu, tmp_path, monkeypatch):
    import torch
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    from hiprag.lexical import hybrid_search_lexical_device
    from hiprag.sparse import weighted_search_reference
    from rag.ingest.indexing import index_chunks
    from rag.providers.hip.embeddings import HipEmbeddingProvider
    from rag.storage.hip_index import sparse as sp
    for name in ("HIP_COLLECTION", "HIP_INDEX_TYPE", "HIP_SPARSE_MODE", "HIP_SPARSE_LINEAR", "HIP_HYBRID_SCORE_ALL", "HIP_ENCODER_WEIGHTS",
                 "HIP_TOKENIZER_FILE", "HIP_PAGES"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("HIP_ALLOW_SYNTHETIC", "1")
    monkeypatch.setenv("HIP_ENCODER_CONFIG", json.dumps(ENCODER))
    monkeypatch.setenv("HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_SEARCH_ALL_DOCUMENTS", False)
    monkeypatch.setenv("STORAGE_DIR", str(tmp_path))
    holder = {}
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: holder["provider"])
    hi.clear_caches()
    sp.clear_sparse_cache()

    rng = np.random.default_rng(12)
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(6, 13)))) for _ in range(30)]
    chunks = [{"chunk_id": f"{DOC}_{i:04d}", "text": t, "page": 1 + i // 7, "metadata": {"title": DOC}} for i, t in enumerate(texts)]
    with open(tmp_path / f"{DOC}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    retriever = rt.HybridRetriever(top_chunks=DEPTH, hybrid=True)

    # ---- the parent's path, before the variable is set ------------------------------------------------------------------
    holder["provider"] = HipEmbeddingProvider()
    assert not holder["provider"].encoder.has_lexical
    summary = asyncio.run(index_chunks(DOC, chunks, storage_dir=tmp_path, provider=holder["provider"], with_sparse=True))
    assert summary["postings_indexed"] > 0 and not (tmp_path / f"{DOC}{sp.LEXICAL_SUFFIX}").exists()
    base = {q: _snapshot(asyncio.run(retriever.retrieve_chunks(q))) for q in QUERIES}
    assert all(len(v) > 0 and all(row[5] is None for row in v) for v in base.values())
    assert any(row[3] is not None for v in base.values() for row in v)

    # ---- lexical: ingest writes the file, retrieval searches it with the query's weights ---------------------------------------
    monkeypatch.setenv("HIP_SPARSE_MODE", "lexical")
    holder["provider"] = prov = HipEmbeddingProvider()
    assert prov.encoder.has_lexical
    hi.clear_caches()
    sp.clear_sparse_cache()
    summary = asyncio.run(index_chunks(DOC, chunks, storage_dir=tmp_path, provider=prov, with_sparse=True))
    npz = tmp_path / f"{DOC}{sp.LEXICAL_SUFFIX}"
    assert npz.exists() and summary["postings_indexed"] > 0 and summary["vectors_indexed"] == 30
    with np.load(npz) as z:
        assert sorted(z.files) == ["doc_ids", "impacts", "n_docs", "offsets"] and int(z["offsets"][-1]) == summary["postings_indexed"]
    chunk_rows = hi._load_chunk_list(tmp_path, DOC)
    lex = sp.get_lexical_index(tmp_path, DOC, chunk_rows)
    dense_index = hi.HipIndexReader(str(tmp_path / f"{DOC}{hi.INDEX_SUFFIX}")).index
    # the postings ARE the chunks' lexical rows from a forward over the same texts
    rows = asyncio.run(prov.embed_batch_lexical_device(texts))
    from hiprag.lexical import transpose_doc_weights
    want = transpose_doc_weights(*(t.cpu().numpy() for t in rows[1:]), ENCODER["vocab"])
    assert np.array_equal(want.offsets, lex.p.offsets) and np.array_equal(want.doc_ids, lex.p.doc_ids)
    assert np.array_equal(want.impacts.view(np.uint32), lex.p.impacts.view(np.uint32))

    found_sparse = 0
    searches = {}
    for q in QUERIES:
        got = asyncio.run(retriever.retrieve_chunks(q))
        vec, q_terms, q_weights = asyncio.run(prov.embed_single_lexical(q))
        assert np.array_equal(np.asarray(vec, np.float32), np.asarray(asyncio.run(prov.embed_single(q)), np.float32))
        qd = torch.tensor([vec], dtype=torch.float32, device="cuda")
        (f_scores, f_ids), _dense, sparse = hybrid_search_lexical_device(dense_index, lex, qd, [q_terms], [q_weights], depth=DEPTH, k=DEPTH)
        torch.cuda.synchronize()
        f_ids, f_scores = f_ids[0].cpu().numpy(), f_scores[0].cpu().numpy()
        keep = f_ids >= 0
        assert [c.chunk_id for c in got] == [f"{DOC}_{i:04d}" for i in f_ids[keep]], q
        assert [c.metadata["rrf_score"] for c in got] == [float(s) for s in f_scores[keep]], q
        assert all(c.metadata["sparse_mode"] == "lexical" for c in got)
        # the sparse leg is the reference's
        es, ei = weighted_search_reference(lex.p, [q_terms], [q_weights], DEPTH)
        assert np.array_equal(sparse[2].cpu().numpy(), ei) and np.array_equal(sparse[1].cpu().numpy().view(np.uint32), es.view(np.uint32)), q
        ref_score = {int(i): float(s) for i, s in zip(ei[0], es[0]) if i >= 0}
        for c in got:
            assert c.metadata.get("bm25_score") == ref_score.get(int(c.chunk_id.rsplit("_", 1)[1])), (q, c.chunk_id)
        found_sparse += len(ref_score)
        searches[q] = lex.search([q_terms], [q_weights], DEPTH)
    assert found_sparse > 0, "no query matched lexically: the test data does not reach the sparse leg"

    # ---- a cold cache loads the file: the same search bits, another object, nothing encoded -----------------------------------
    sp.clear_sparse_cache()
    forwards = []
    real = prov.encoder.encode_lexical
    monkeypatch.setattr(prov.encoder, "encode_lexical", lambda *a, **k: forwards.append(1) or real(*a, **k))
    loaded = sp.get_lexical_index(tmp_path, DOC, chunk_rows)
    assert loaded is not lex and not forwards
    for q in QUERIES:
        _, q_terms, q_weights = asyncio.run(prov.embed_single_lexical(q))
        s, i = loaded.search([q_terms], [q_weights], DEPTH)
        assert np.array_equal(i, searches[q][1]) and np.array_equal(s.view(np.uint32), searches[q][0].view(np.uint32))

    # ---- bm25 (named or unset) is the parent's path ----------------------------------------------------------------------------
    for mode in ("bm25", None):
        if mode is None:
            monkeypatch.delenv("HIP_SPARSE_MODE")
        else:
            monkeypatch.setenv("HIP_SPARSE_MODE", mode)
        sp.clear_sparse_cache()
        for q in QUERIES:
            assert _snapshot(asyncio.run(retriever.retrieve_chunks(q))) == base[q], (mode, q)

    # ---- refusals ----------------------------------------------------------------------------------------------------------------
    monkeypatch.setenv("HIP_SPARSE_MODE", "splade")
    with pytest.raises(ValueError, match="HIP_SPARSE_MODE"):
        asyncio.run(retriever.retrieve_chunks(QUERIES[0]))
    monkeypatch.setenv("HIP_SPARSE_MODE", "lexical")
    monkeypatch.setenv("HIP_COLLECTION", "true")
    with pytest.raises(ValueError, match="not supported yet"):
        asyncio.run(retriever.retrieve_chunks(QUERIES[0]))
    with pytest.raises(ValueError, match="not supported yet"):
        asyncio.run(index_chunks(DOC, chunks, storage_dir=tmp_path, provider=prov, with_sparse=True))
    monkeypatch.delenv("HIP_COLLECTION")
    # a document that was never ingested in lexical mode has no file to load
    npz.unlink()
    sp.clear_sparse_cache()
    with pytest.raises(RuntimeError, match="lexical"):
        asyncio.run(retriever.retrieve_chunks(QUERIES[0]))


def test_provider_needs_a_head_file_or_the_synthetic_switch(gpu, tmp_path, monkeypatch):
    """HIP_SPARSE_LINEAR (a torch-saved dict with weight / bias, BGE-M3's sparse_linear.pt) is what the provider loads; without
    it and without HIP_ALLOW_SYNTHETIC the constructor raises."""
    import torch
    from hiprag import EncoderConfig, HipEncoder, random_state
    from rag.providers.hip.embeddings import HipEmbeddingProvider
    from rag.providers.hip.tokenizer import HashTokenizer
    monkeypatch.delenv("HIP_COLLECTION", raising=False)
    monkeypatch.delenv("HIP_ALLOW_SYNTHETIC", raising=False)
    monkeypatch.delenv("HIP_SPARSE_LINEAR", raising=False)
    monkeypatch.setenv("HIP_SPARSE_MODE", "lexical")
    cfg = EncoderConfig(**ENCODER)
    sd = random_state(cfg, seed=4, with_lexical=True)
    head = {"weight": sd.pop("sparse_linear.weight"), "bias": sd.pop("sparse_linear.bias")}
    tok = HashTokenizer(cfg.vocab)
    with pytest.raises(RuntimeError, match="HIP_SPARSE_LINEAR"):
        HipEmbeddingProvider(encoder=HipEncoder(cfg, sd), tokenizer=tok)
    torch.save(head, str(tmp_path / "sparse_linear.pt"))
    monkeypatch.setenv("HIP_SPARSE_LINEAR", str(tmp_path / "sparse_linear.pt"))
    prov = HipEmbeddingProvider(encoder=HipEncoder(cfg, sd), tokenizer=tok)
    vec, terms, weights = asyncio.run(prov.embed_single_lexical("w1 w2 w3 w4 w5 w6 w7 w8"))
    toks = tok.encode("w1 w2 w3 w4 w5 w6 w7 w8", cfg.max_seq_len)
    ref = HipEncoder(cfg, dict(sd, **{"sparse_linear.weight": head["weight"], "sparse_linear.bias": head["bias"]}))
    d, t, w, c = (x.cpu().numpy() for x in ref.encode_lexical([toks]))
    assert np.array_equal(np.asarray(vec, np.float32), d[0]) and terms == t[0, :c[0]].tolist()
    assert np.array_equal(weights.view(np.uint32), w[0, :c[0]].view(np.uint32)) and len(terms) > 0
