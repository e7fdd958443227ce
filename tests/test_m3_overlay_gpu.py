"""
HIP_M3_SCORE=true in the drop-in, end to end on synthetic weights: three documents in two projects, 30 chunks (the pattern of
tests/test_collection_lexical_gpu.py).  The ingest runs ONE forward per batch (hipenc_forward_m3) that feeds the flat index,
the lexical postings and the multi-vector store; all three follow index_chunks / delete_document / replace_document; and
HybridRetriever.retrieve_chunks returns the first stage's chunks in the order, and with the metadata, that
hiprag.m3_score_reference gives over the first stage's rows from the three component entries -- for hybrid=False and
hybrid=True.  With HIP_M3_SCORE unset the results are the parent's paths', over either kind of storage.
"""
import asyncio
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEPTH, L = 12, 64
DOCS = [("docA", "red", 11), ("docB", "blue", 9), ("docC", "red", 10)]
WORDS = [f"w{j}" for j in range(40)]
QUERIES = ("w3 w17 w5 w8", "w1 w2 w30 w31 w32 w33", "W9 w9 w21 unknownword", "w12")
PROJECTS = (None, "red", "blue")
ENCODER = {"vocab": 200, "hidden": 128, "layers": 2, "heads": 2, "ffn": 256, "max_pos": 80, "max_seq_len": L}
M3_ENV = {"HIP_COLLECTION_SPARSE": "lexical", "HIP_LATE_INTERACTION": "true", "HIP_M3_SCORE": "true"}
MODES = {"m3": M3_ENV, "lexical": {"HIP_COLLECTION_SPARSE": "lexical"}, "late": {"HIP_LATE_INTERACTION": "true"}}


def _texts(n, seed):
    rng = np.random.default_rng(seed)
    out = [" ".join(rng.choice(WORDS, size=int(rng.integers(4, 13)))) for _ in range(n)]
    out[1] = ""                                          # a blank chunk: no lexical weight, no token vector
    return out


def _index_doc(storage, provider, doc, texts, project, replace=False):
    from rag.ingest.indexing import index_chunks
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": 1 + i // 4, "metadata": {"title": doc}} for i, t in enumerate(texts)]
    with open(storage / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=storage, provider=provider, with_sparse=True, project=project,
                                    replace=replace))


def _snapshot(chunks):
    keys = ("doc_id", "rrf_score", "bm25_score", "sparse_only", "sparse_mode", "colbert_score", "rerank_mode", "m3_score", "m3_dense",
            "m3_sparse", "m3_colbert")
    return [(c.chunk_id, np.float64(c.score).tobytes()) + tuple(c.metadata.get(k) for k in keys) for c in chunks]


def _all_snapshots(retriever):
    return {(q, p): _snapshot(asyncio.run(retriever.retrieve_chunks(q, p))) for q in QUERIES for p in PROJECTS}


@pytest.fixture()
def world(gpu, tmp_path, monkeypatch):
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    from rag.providers.hip.embeddings import HipEmbeddingProvider
    monkeypatch.setattr(hi.config, "HIP_SEARCH_ALL_DOCUMENTS", False)
    monkeypatch.setenv("HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "l2")
    for name in ("HIP_INDEX_TYPE", "HIP_RERANK", "HIP_PAGES", "HIP_LATE_INTERACTION", "HIP_LATE_SEARCH", "HIP_SPARSE_MODE", "HIP_SPARSE_LINEAR",
                 "HIP_COLBERT_LINEAR", "HIP_COLBERT_FORMAT", "HIP_IVF_HYBRID", "HIP_HYBRID_SCORE_ALL", "HIP_COLLECTION_SPARSE", "HIP_ENCODER_WEIGHTS",
                 "HIP_TOKENIZER_FILE", "HIP_M3_SCORE", "HIP_M3_WEIGHTS", "HIP_ENCODER_PACKED"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_ALLOW_SYNTHETIC", "1")
    monkeypatch.setenv("HIP_ENCODER_CONFIG", json.dumps(ENCODER))
    for k, v in M3_ENV.items():
        monkeypatch.setenv(k, v)
    provider = HipEmbeddingProvider()                    # the synthetic encoder, hashing tokenizer and (seeded) heads
    assert provider.encoder.has_lexical
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: provider)
    texts = {doc: _texts(n, 800 + j) for j, (doc, _p, n) in enumerate(DOCS)}

    def use(name, mode="m3"):
        storage = tmp_path / name
        storage.mkdir(exist_ok=True)
        monkeypatch.setenv("STORAGE_DIR", str(storage))
        for k in M3_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in MODES[mode].items():
            monkeypatch.setenv(k, v)
        hi.clear_caches()
        return storage

    return dict(rt=rt, hi=hi, provider=provider, texts=texts, use=use, monkeypatch=monkeypatch)


def _ingest_all(w, storage):
    for doc, project, _n in DOCS:
        _index_doc(storage, w["provider"], doc, w["texts"][doc], project)


def _structures(coll):
    """the exports of the three structures that follow the collection's rows"""
    lex = coll.lex.export()
    off, vecs = coll.mv.export()
    rows = np.stack([coll.index.reconstruct(i) for i in range(coll.index.ntotal)]) if coll.index.ntotal else np.zeros((0, 1), np.float32)
    return dict(rows=rows.tobytes(), lex_off=lex["offsets"].tobytes(), lex_ids=lex["doc_ids"].tobytes(), lex_imp=lex["impacts"].tobytes(),
                mv_off=off.tobytes(), mv_vecs=vecs.tobytes())


def test_ingest_runs_one_forward_per_batch_and_the_structures_follow_the_collection(world):
    w = world
    import hiprag._native as nat
    from rag.storage.hip_index import collection as col
    calls = []
    real_call = nat.call
    w["monkeypatch"].setattr(nat, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    live_dir = w["use"]("live")
    for doc, project, _n in DOCS:
        calls.clear()
        _index_doc(live_dir, w["provider"], doc, w["texts"][doc], project)
        forwards = [c for c in calls if c.startswith("hipenc_forward") or c.startswith("hipenc_score")]
        assert forwards == ["hipenc_forward_m3"], (doc, forwards)          # one batch, one forward, all three outputs
    coll = col.open_collection(live_dir)
    manifest = json.load(open(live_dir / col.COLLECTION_MANIFEST))
    assert "lexical" in manifest and "mv" in manifest and (live_dir / col.COLLECTION_LEXICAL).exists() and (live_dir / col.COLLECTION_MV).exists()
    assert coll.index.ntotal == coll.lex.n_docs == len(coll.mv) == coll.manifest.rows == 30
    # what the one forward wrote is what the two single-head forwards write for the same texts
    for doc in coll.manifest.documents[:1]:
        t = w["texts"][doc["doc_id"]]
        m3 = asyncio.run(w["provider"].embed_batch_m3_device(t))
        lex = asyncio.run(w["provider"].embed_batch_lexical_device(t))
        cb = asyncio.run(w["provider"].embed_batch_colbert_device(t))
        import torch
        assert all(torch.equal(a, b) for a, b in zip(m3[:4], lex)) and torch.equal(m3[0], cb[0])
        assert torch.equal(m3[4].view(torch.int16), cb[1].view(torch.int16)) and torch.equal(m3[5], cb[2])
    # delete and replace: every structure follows, and equals a collection ingested from scratch with the final documents
    col.delete_document("docB", storage_dir=live_dir)
    after = col.open_collection(live_dir)
    assert after.index.ntotal == after.lex.n_docs == len(after.mv) == after.manifest.rows == 21
    new_a = _texts(7, 999)
    calls.clear()
    _index_doc(live_dir, w["provider"], "docA", new_a, "red", replace=True)
    assert [c for c in calls if c.startswith("hipenc_forward")] == ["hipenc_forward_m3"]
    live = col.open_collection(live_dir)
    assert [d["doc_id"] for d in live.manifest.documents] == ["docC", "docA"]
    assert live.index.ntotal == live.lex.n_docs == len(live.mv) == live.manifest.rows == 17
    got = _structures(live)
    fresh_dir = w["use"]("fresh")
    _index_doc(fresh_dir, w["provider"], "docC", w["texts"]["docC"], "red")
    _index_doc(fresh_dir, w["provider"], "docA", new_a, "red")
    assert _structures(col.open_collection(fresh_dir)) == got


@pytest.mark.parametrize("hybrid", (False, True))
def test_retrieval_is_the_reference_over_the_first_stage(world, hybrid):
    w = world
    rt = w["rt"]
    import torch
    from hiprag import m3_score_reference, maxsim_device
    from rag.config import config
    from rag.storage.hip_index import collection as col, search_hip_by_vector
    from rag.storage.hip_index.passages import rows_of_chunks
    storage = w["use"]("m3")
    _ingest_all(w, storage)
    coll = col.open_collection(storage)
    retriever = rt.HybridRetriever(top_chunks=DEPTH, hybrid=hybrid)
    keep = config.RERANKER_TOP_K
    assert keep < DEPTH
    reordered = sparse_hits = 0
    for weights_env in (None, "1,0.5,2"):
        if weights_env:
            w["monkeypatch"].setenv("HIP_M3_WEIGHTS", weights_env)
        mix = config.HIP_M3_WEIGHTS
        assert mix == ((0.4, 0.2, 0.4) if weights_env is None else (1.0, 0.5, 2.0))
        for q in QUERIES:
            vec, q_terms, q_weights, q_vecs, q_counts = asyncio.run(w["provider"].embed_single_m3(q))
            for project in PROJECTS:
                if hybrid:
                    first = retriever._hybrid_search(q, vec, project, lexical_query=(q_terms, q_weights))
                else:
                    first = asyncio.run(search_hip_by_vector(vec, limit=DEPTH, project=project))
                first = [rt._as_chunk(r) for r in first]
                got = asyncio.run(retriever.retrieve_chunks(q, project))
                if not first:
                    assert got == []
                    continue
                rows = rows_of_chunks(coll, first)
                cand = torch.tensor([rows], dtype=torch.int64, device="cuda")
                qd = torch.tensor([vec], dtype=torch.float32, device="cuda")
                d64, d32 = coll.index.score_ids_device(qd, cand)
                sp = coll.lex.bm.score_ids_device([q_terms], cand, [q_weights])
                ms = maxsim_device(coll.mv, q_vecs, q_counts, cand, 1)[3]
                torch.cuda.synchronize()
                k = min(keep, len(rows))
                _pairs, scores, pos = m3_score_reference(d64.cpu().numpy(), sp.cpu().numpy(), ms.cpu().numpy(), np.ones((1, len(rows)), bool),
                                                         mix, k, l2=True)
                order = [int(p) for p in pos[0] if p >= 0]
                assert [c.chunk_id for c in got] == [first[p].chunk_id for p in order], (q, project)
                for c, p, s in zip(got, order, scores[0]):
                    m = c.metadata
                    assert m["m3_score"] == float(s) and m["rerank_mode"] == "m3"
                    assert m["m3_dense"] == 1.0 - 0.5 * float(d32[0, p]) and m["m3_sparse"] == float(sp[0, p]) and m["m3_colbert"] == float(ms[0, p])
                    assert np.float64(c.score).tobytes() == np.float64(first[p].score).tobytes()      # `score` stays the dense similarity
                    if hybrid:
                        assert m["sparse_mode"] == "lexical" and m["rrf_score"] == first[p].metadata["rrf_score"]
                reordered += order != list(range(len(order)))
                sparse_hits += int((sp > 0).sum())
                if project == "red":
                    assert all(c.metadata["doc_id"] in ("docA", "docC") for c in got)
    assert reordered > 0, "the combined score never changed the first stage's order: the test data has no power"
    assert sparse_hits > 0, "no query matched lexically"
    # the refusals of the setting reach the retriever and the ingest
    for name in ("HIP_PAGES", "HIP_LATE_SEARCH", "HIP_RERANK"):
        w["monkeypatch"].setenv(name, "true")
        with pytest.raises(ValueError, match="HIP_M3_SCORE"):
            asyncio.run(retriever.retrieve_chunks(QUERIES[0]))
        with pytest.raises(ValueError, match="HIP_M3_SCORE|HIP_LATE"):
            _index_doc(storage, w["provider"], "docX", w["texts"]["docB"], "blue")
        w["monkeypatch"].delenv(name)
    with pytest.raises(ValueError, match="two second stages"):
        asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, hybrid=hybrid, rerank=True).retrieve_chunks(QUERIES[0]))


def test_unset_is_the_parent_over_either_storage(world):
    """HIP_M3_SCORE unset: the lexical hybrid and the late-interaction rerank give, over a collection the combined forward
    ingested, what they give over one their own single-head forward ingested -- and neither carries any m3 metadata."""
    w = world
    rt = w["rt"]
    m3_dir = w["use"]("m3")
    _ingest_all(w, m3_dir)
    base = {}
    for mode, hybrid in (("lexical", True), ("late", False)):
        own = w["use"]("own_" + mode, mode)
        _ingest_all(w, own)                              # the parent's ingest: one single-head forward per batch
        retriever = rt.HybridRetriever(top_chunks=DEPTH, hybrid=hybrid)
        base[mode] = _all_snapshots(retriever)
        assert any(base[mode].values()) and all(row[-4] is None and row[-5] != "m3" for v in base[mode].values() for row in v)
        w["use"]("m3", mode)
        assert _all_snapshots(retriever) == base[mode], mode
    assert any(row[7] is not None for v in base["late"].values() for row in v)           # colbert_score: the late path ran
    assert any(row[6] == "lexical" for v in base["lexical"].values() for row in v)
    # without the setting the pair of settings is refused as before
    w["use"]("m3", "lexical")
    w["monkeypatch"].setenv("HIP_LATE_INTERACTION", "true")
    with pytest.raises(ValueError, match="one forward gives one extra output today"):
        asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, hybrid=True).retrieve_chunks(QUERIES[0]))
