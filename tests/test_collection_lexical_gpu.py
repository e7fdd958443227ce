"""
HIP_COLLECTION_SPARSE=lexical in the drop-in, end to end on synthetic weights: three documents in two projects, 30 chunks.
The ingest passes the lexical rows of the forward that makes the embeddings to the collection, whose lexical postings
(hiprag.LexicalIndexUpdatable) follow index_chunks, delete_document and replace_document on the device and are saved as
hip_collection.lexical.npz; a cold cache loads the file and never encodes; HybridRetriever(hybrid=True) searches them with the
query's own weights inside the project's row ranges -- against the numpy composition: the scoped dense ranking in fp64,
weighted_search_reference with the project's ranges, and the oracle's rrf_fuse.  With the setting unset nothing changes.
"""
import asyncio
import dataclasses
import json

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

DEPTH, MAX_PAGES, L = 12, 3, 64
DOCS = [("docA", "red", 11), ("docB", "blue", 9), ("docC", "red", 10)]
WORDS = [f"w{j}" for j in range(40)]
QUERIES = ("w3 w17 w5 w8", "w1 w2 w30 w31 w32 w33", "W9 w9 w21 unknownword", "w12")
PROJECTS = (None, "red", "blue")
ENCODER = {"vocab": 200, "hidden": 128, "layers": 2, "heads": 2, "ffn": 256, "max_pos": 80, "max_seq_len": L}
VOCAB = ENCODER["vocab"]


def _texts(n, seed):
    rng = np.random.default_rng(seed)
    out = [" ".join(rng.choice(WORDS, size=int(rng.integers(4, 13)))) for _ in range(n)]
    out[1] = ""                                          # a blank chunk: an empty lexical row
    return out


def _index_doc(storage, provider, doc, texts, project, replace=False):
    from rag.ingest.indexing import index_chunks
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": 1 + i // 4, "metadata": {"title": doc}} for i, t in enumerate(texts)]
    with open(storage / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=storage, provider=provider, with_sparse=True, project=project,
                                    replace=replace))


def _snapshot(chunks):
    return [(c.chunk_id, np.float64(c.score).tobytes(), c.metadata.get("doc_id"), c.metadata.get("rrf_score"), c.metadata.get("bm25_score"),
             c.metadata.get("sparse_only"), c.metadata.get("sparse_mode")) for c in chunks]


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
    for name in ("HIP_INDEX_TYPE", "HIP_RERANK", "HIP_PAGES", "HIP_LATE_INTERACTION", "HIP_SPARSE_MODE", "HIP_SPARSE_LINEAR", "HIP_IVF_HYBRID",
                 "HIP_HYBRID_SCORE_ALL", "HIP_COLLECTION_SPARSE", "HIP_ENCODER_WEIGHTS", "HIP_TOKENIZER_FILE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_ALLOW_SYNTHETIC", "1")
    monkeypatch.setenv("HIP_ENCODER_CONFIG", json.dumps(ENCODER))
    make_provider = HipEmbeddingProvider                 # the synthetic encoder and hashing tokenizer of the configuration above
    plain_provider = make_provider()                     # made with the setting unset: the parent's provider, no lexical head
    assert not plain_provider.encoder.has_lexical
    monkeypatch.setenv("HIP_COLLECTION_SPARSE", "lexical")
    provider = make_provider()                           # the provider sets its (synthetic) lexical head for this setting too
    assert provider.encoder.has_lexical
    holder = {"provider": provider}
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: holder["provider"])
    texts = {doc: _texts(n, 800 + j) for j, (doc, _p, n) in enumerate(DOCS)}

    def use(name, lexical=True):
        storage = tmp_path / name
        storage.mkdir(exist_ok=True)
        monkeypatch.setenv("STORAGE_DIR", str(storage))
        if lexical:
            monkeypatch.setenv("HIP_COLLECTION_SPARSE", "lexical")
        else:
            monkeypatch.delenv("HIP_COLLECTION_SPARSE", raising=False)
        holder["provider"] = provider if lexical else plain_provider
        hi.clear_caches()
        return storage

    return dict(rt=rt, hi=hi, provider=provider, plain_provider=plain_provider, texts=texts, use=use, monkeypatch=monkeypatch, holder=holder)


def _ingest_all(w, storage, provider=None):
    for doc, project, _n in DOCS:
        _index_doc(storage, provider or w["provider"], doc, w["texts"][doc], project)


def _reference_postings(w, coll, texts_of):
    """transpose_doc_weights over the lexical rows of every document of the manifest, in row order, each from a forward over
    that document's texts (the batch the ingest ran)"""
    from hiprag import transpose_doc_weights
    parts = []
    for doc in coll.manifest.documents:
        rows = asyncio.run(w["provider"].embed_batch_lexical_device(texts_of[doc["doc_id"]]))
        parts.append([t.cpu().numpy() for t in rows[1:]])
    width = max(p[0].shape[1] for p in parts)
    terms = np.concatenate([np.pad(p[0], ((0, 0), (0, width - p[0].shape[1])), constant_values=-1) for p in parts])
    weights = np.concatenate([np.pad(p[1], ((0, 0), (0, width - p[1].shape[1]))) for p in parts])
    return transpose_doc_weights(terms, weights, np.concatenate([p[2] for p in parts]), VOCAB)


def _export_equals(lex, p):
    ex = lex.export()
    return (ex["n_docs"], ex["n_terms"]) == (p.n_docs, p.n_terms) and np.array_equal(ex["offsets"], p.offsets) and \
        np.array_equal(ex["doc_ids"], p.doc_ids) and np.array_equal(ex["impacts"].view(np.uint32), p.impacts.view(np.uint32))


def test_retrieval_equals_the_numpy_composition_and_unset_is_the_parent(world):
    w = world
    rt = w["rt"]
    from hiprag import weighted_search_reference
    from rag.storage.hip_index import collection as col
    retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=True)
    # ---- the parent's path, in a storage that never heard of the setting, with a provider made without it ----------------
    plain = w["use"]("plain", lexical=False)
    _ingest_all(w, plain, w["plain_provider"])
    assert not (plain / col.COLLECTION_LEXICAL).exists() and "lexical" not in json.load(open(plain / col.COLLECTION_MANIFEST))
    base = _all_snapshots(retriever)
    assert all(row[6] is None for v in base.values() for row in v) and any(row[4] is not None for v in base.values() for row in v)

    # ---- lexical ----------------------------------------------------------------------------------------------------------
    storage = w["use"]("lex")
    _ingest_all(w, storage)
    manifest = json.load(open(storage / col.COLLECTION_MANIFEST))
    assert (storage / col.COLLECTION_LEXICAL).exists() and manifest["lexical"] == {"n_terms": VOCAB}
    assert all((storage / f"{doc}_chunks.json").exists() for doc, _p, _n in DOCS)
    coll = col.open_collection(storage)
    assert coll.lex.n_docs == coll.manifest.rows == 30 and coll.lex.sizes()["updatable_impacts"] and not coll.lex.sizes()["dirty"]
    p = _reference_postings(w, coll, w["texts"])
    assert _export_equals(coll.lex, p), "the collection's postings are not the rows of the ingest's forwards"
    assert p.doc_ids.size > 0 and np.diff(p.offsets.astype(np.int64))[:4].sum() == 0          # bos, pad, eos, unk carry no weight
    x, _metric = col.read_flat_rows(storage / col.COLLECTION_INDEX)
    found_sparse = sparse_only = 0
    for q in QUERIES:
        vec, q_terms, q_weights = asyncio.run(w["provider"].embed_single_lexical(q))
        dist = ho.all_scores_f64(x, np.asarray(vec, np.float32), ho.METRIC_L2)
        for project in PROJECTS:
            scope = coll.manifest.scope_for(project)
            inside = np.concatenate([np.arange(lo, hi) for lo, hi in scope])
            dense_ids = np.full((1, DEPTH), -1, np.int64)
            top = inside[np.lexsort((inside, dist[inside]))][:DEPTH]
            dense_ids[0, :top.size] = top
            es, ei = weighted_search_reference(p, [q_terms], [q_weights], DEPTH, ranges=[scope])
            fs, fi = ho.rrf_fuse(dense_ids, ei, DEPTH)
            keep = fi[0] >= 0
            got = asyncio.run(retriever.retrieve_chunks(q, project))
            want_ids = ["%s_%04d" % coll.manifest.locate(int(r)) for r in fi[0][keep]]
            assert [c.chunk_id for c in got] == want_ids, (q, project)
            assert [np.float32(c.metadata["rrf_score"]).tobytes() for c in got] == [np.float32(s).tobytes() for s in fs[0][keep]], (q, project)
            ref_score = {int(i): float(s) for i, s in zip(ei[0], es[0]) if i >= 0}
            dense_set = set(int(i) for i in dense_ids[0] if i >= 0)
            for c, row in zip(got, fi[0][keep]):
                assert c.metadata["sparse_mode"] == "lexical", (q, project)
                assert c.metadata.get("bm25_score") == ref_score.get(int(row)), (q, project, c.chunk_id)
                assert bool(c.metadata.get("sparse_only")) == (int(row) not in dense_set)
                sparse_only += int(row) not in dense_set
            if project == "red":
                assert all(c.metadata["doc_id"] in ("docA", "docC") for c in got)
            found_sparse += len(ref_score)
        print(f"query {q!r}: {len(q_terms)} weighted terms, postings {p.doc_ids.size}")
    assert found_sparse > 0, "no query matched lexically: the test data does not reach the sparse leg"
    print(f"collection lexical: {found_sparse} sparse hits, {sparse_only} fused rows found by the sparse leg alone")

    # HIP_HYBRID_SCORE_ALL works as before: the rows only the sparse leg found are scored by id
    lex_rows = _all_snapshots(retriever)
    w["monkeypatch"].setenv("HIP_HYBRID_SCORE_ALL", "true")
    for key, rows in _all_snapshots(retriever).items():
        assert [r[0] for r in rows] == [r[0] for r in lex_rows[key]] and not any(r[5] for r in rows)
    w["monkeypatch"].delenv("HIP_HYBRID_SCORE_ALL")

    # ---- the HIP_PAGES path returns the host path's pages ------------------------------------------------------------------
    w["monkeypatch"].setenv("HIP_PAGES", "true")
    for q in QUERIES[:2]:
        for project in (None, "red"):
            chunks = asyncio.run(retriever.retrieve_chunks(q, project))
            keyed = [dataclasses.replace(c, page=(c.metadata["doc_id"], c.page)) for c in chunks]
            want = rt.rank_pages(rt.group_chunks_by_page(keyed))[:MAX_PAGES]
            got = asyncio.run(retriever.retrieve_and_rank_pages(q, project))
            assert len(got) == len(want) > 0
            for g, x_ in zip(got, want):
                assert (g.metadata["doc_id"], g.page) == x_.page and np.float64(g.score).tobytes() == np.float64(x_.score).tobytes()
                assert [c.chunk_id for c in g.chunks] == [c.chunk_id for c in x_.chunks]
                for a, b in zip(g.chunks, x_.chunks):
                    assert a.metadata == b.metadata and a.metadata["sparse_mode"] == "lexical", (q, project, a.metadata, b.metadata)
    w["monkeypatch"].delenv("HIP_PAGES")

    # ---- unset again: the parent's BM25 results, over the plain storage and over the lexical one -------------------------------
    for name in ("plain", "lex"):
        w["use"](name, lexical=False)
        assert _all_snapshots(retriever) == base, name


def test_postings_follow_delete_and_replace_and_a_cold_cache_loads_the_file(world):
    w = world
    rt = w["rt"]
    from hiprag import LexicalIndexUpdatable
    from rag.storage.hip_index import collection as col
    retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=True)
    live_dir = w["use"]("live")
    _ingest_all(w, live_dir)
    col.delete_document("docB", storage_dir=live_dir)
    after_delete = col.open_collection(live_dir)
    assert after_delete.lex.n_docs == after_delete.manifest.rows == 21
    assert _export_equals(after_delete.lex, _reference_postings(w, after_delete, w["texts"]))
    new_a = _texts(7, 999)
    _index_doc(live_dir, w["provider"], "docA", new_a, "red", replace=True)
    live = col.open_collection(live_dir)
    assert [d["doc_id"] for d in live.manifest.documents] == ["docC", "docA"] and live.lex.n_docs == live.manifest.rows == 17
    final_texts = dict(w["texts"], docA=new_a)
    assert _export_equals(live.lex, _reference_postings(w, live, final_texts))
    got_live = _all_snapshots(retriever)
    # a collection ingested from scratch with the final documents
    fresh_dir = w["use"]("fresh")
    _index_doc(fresh_dir, w["provider"], "docC", w["texts"]["docC"], "red")
    _index_doc(fresh_dir, w["provider"], "docA", new_a, "red")
    assert _all_snapshots(retriever) == got_live
    assert _export_equals(live.lex, col.open_collection(fresh_dir).lex.postings())
    assert any(rows for rows in got_live.values()) and not got_live[(QUERIES[0], "blue")]

    # ---- a cold cache LOADS hip_collection.lexical.npz and encodes no chunk -----------------------------------------------------
    before = live.lex.export()
    w["use"]("live")                                                          # clears every cache
    async def refuse(*a, **k):   # noqa: E306
        raise AssertionError("a chunk batch was encoded")
    for name in ("embed_batch", "embed_batch_device", "embed_batch_lexical_device"):
        w["monkeypatch"].setattr(w["provider"], name, refuse)
    cold = col.open_collection(live_dir)
    assert cold is not live and cold.lex is not live.lex
    ex = cold.lex.export()
    assert all(np.array_equal(ex[k], before[k]) for k in ("offsets", "doc_ids")) and ex["impacts"].tobytes() == before["impacts"].tobytes()
    assert _all_snapshots(retriever) == got_live

    # ---- a file whose document count is not the manifest's raises; so does a missing one ------------------------------------------
    keep = (live_dir / col.COLLECTION_LEXICAL).read_bytes()
    other = LexicalIndexUpdatable(n_terms=VOCAB)
    other.append_rows(np.array([[5]], np.int32), np.array([[1.0]], np.float32), np.array([1], np.int32))
    other.save(str(live_dir / col.COLLECTION_LEXICAL))
    w["hi"].clear_caches()
    with pytest.raises(RuntimeError, match="lexical postings hold 1 documents"):
        col.open_collection(live_dir)
    (live_dir / col.COLLECTION_LEXICAL).unlink()
    with pytest.raises(RuntimeError, match="missing"):
        col.open_collection(live_dir)
    (live_dir / col.COLLECTION_LEXICAL).write_bytes(keep)
    assert col.open_collection(live_dir).lex.export()["impacts"].tobytes() == before["impacts"].tobytes()


def test_refused_combinations(world):
    w = world
    rt, mp = w["rt"], w["monkeypatch"]
    from rag.storage.hip_index import collection as col
    retriever = rt.HybridRetriever(top_chunks=DEPTH, hybrid=True)
    storage = w["use"]("lex")
    _index_doc(storage, w["provider"], "docA", w["texts"]["docA"], "red")
    assert asyncio.run(retriever.retrieve_chunks(QUERIES[0]))
    for name, value, match in (("HIP_COLLECTION_SPARSE", "splade", "HIP_COLLECTION_SPARSE"), ("HIP_LATE_INTERACTION", "true", "HIP_LATE_INTERACTION"),
                               ("HIP_IVF_HYBRID", "true", "HIP_IVF_HYBRID"), ("HIP_COLLECTION", "false", "needs HIP_COLLECTION")):
        mp.setenv(name, value)
        with pytest.raises(ValueError, match=match):
            asyncio.run(retriever.retrieve_chunks(QUERIES[0]))
        with pytest.raises(ValueError, match=match):
            _index_doc(storage, w["provider"], "docB", w["texts"]["docB"], "blue")
        mp.setenv("HIP_COLLECTION", "true")
        mp.setenv("HIP_COLLECTION_SPARSE", "lexical")
        mp.delenv("HIP_LATE_INTERACTION", raising=False)
        mp.delenv("HIP_IVF_HYBRID", raising=False)
    mp.setenv("HIP_SPARSE_MODE", "lexical")                                  # the per-document setting goes on refusing the collection
    with pytest.raises(ValueError, match="not supported yet"):
        asyncio.run(retriever.retrieve_chunks(QUERIES[0]))
    mp.delenv("HIP_SPARSE_MODE")
    # a collection with postings takes no plain append; one without takes no lexical append, and answers no lexical query
    w["use"]("lex", lexical=False)
    with pytest.raises(RuntimeError, match="keeps lexical postings"):
        _index_doc(storage, w["provider"], "docB", w["texts"]["docB"], "blue")
    coll = col.open_collection(storage)
    assert [d["doc_id"] for d in coll.manifest.documents] == ["docA"] and coll.lex.n_docs == coll.manifest.rows
    plain = w["use"]("plain", lexical=False)
    _index_doc(plain, w["plain_provider"], "docA", w["texts"]["docA"], "red")
    w["use"]("plain")
    with pytest.raises(RuntimeError, match="without lexical weights"):
        _index_doc(plain, w["provider"], "docB", w["texts"]["docB"], "blue")
    with pytest.raises(RuntimeError, match="holds no lexical postings"):
        asyncio.run(retriever.retrieve_chunks(QUERIES[0]))
    assert [d["doc_id"] for d in col.open_collection(plain).manifest.documents] == ["docA"]
