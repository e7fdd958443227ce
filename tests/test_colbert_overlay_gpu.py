"""
Late interaction inside the drop-in (HIP_LATE_INTERACTION=true with HIP_COLLECTION=true): the ingest keeps the chunks' per-token
vectors from the forward that makes their embeddings, the collection's multi-vector store follows index_chunks,
delete_document and replace_document and is saved as hip_collection.mv, a cold cache loads it, and the retriever reorders
its top chunks by MaxSim -- against maxsim_reference over the stored vectors, within the bound of tests/colbert_cases.py.
With the flag off nothing changes.  About 30 chunks in two projects, synthetic weights.
"""
import asyncio
import dataclasses
import json

import numpy as np
import pytest

from colbert_cases import maxsim_expected
from oracle.linear_cases import bf16_values

pytestmark = pytest.mark.gpu

DEPTH, TOP_K, MAX_PAGES, L = 12, 5, 3, 128
DOCS = [("docA", "red", 11), ("docB", "blue", 9), ("docC", "red", 10)]
WORDS = [f"w{j}" for j in range(40)]
QUERY = "w3 w17\nw5 w8 w21"


def _texts(n, seed):
    rng = np.random.default_rng(seed)
    out = [f"c{i} " + " ".join(rng.choice(WORDS, size=1 + (i * 7) % 37)) for i in range(n)]
    out[1] = ""                                          # a blank chunk is encoded as "": bos + eos, one vector
    return out


def _index_doc(storage, provider, doc, texts, project, replace=False):
    from rag.ingest.indexing import index_chunks
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": 1 + i // 4, "metadata": {"title": doc}} for i, t in enumerate(texts)]
    with open(storage / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=storage, provider=provider, with_sparse=False, project=project,
                                    replace=replace))


def _flat(pages):
    return [(p.page, np.float64(p.score).tobytes(), p.metadata, [(c.chunk_id, c.text, np.float64(c.score).tobytes(), c.page, c.metadata)
                                                                    for c in p.chunks]) for p in pages]


@pytest.fixture()
def world(gpu, tmp_path, monkeypatch):
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    from hiprag import EncoderConfig, HipEncoder, random_state
    from rag.providers.hip.embeddings import HipEmbeddingProvider
    from rag.providers.hip.tokenizer import HashTokenizer
    monkeypatch.setattr(hi.config, "HIP_SEARCH_ALL_DOCUMENTS", False)
    monkeypatch.setattr(hi.config, "RERANKER_TOP_K", TOP_K)
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    for name in ("HIP_RERANK", "HIP_PAGES", "HIP_LATE_INTERACTION", "HIP_SPARSE_MODE", "HIP_COLBERT_LINEAR"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_ALLOW_SYNTHETIC", "1")
    cfg = EncoderConfig(vocab=2000, hidden=128, layers=2, heads=2, ffn=256, max_pos=200, max_seq_len=L)
    provider = HipEmbeddingProvider(encoder=HipEncoder(cfg, random_state(cfg, seed=9)), tokenizer=HashTokenizer(cfg.vocab))
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: provider)
    texts = {doc: _texts(n, 800 + j) for j, (doc, _p, n) in enumerate(DOCS)}

    def use(name, late):
        storage = tmp_path / name
        storage.mkdir(exist_ok=True)
        monkeypatch.setenv("STORAGE_DIR", str(storage))
        monkeypatch.setenv("HIP_LATE_INTERACTION", "true" if late else "false")
        hi.clear_caches()
        return storage

    return dict(rt=rt, hi=hi, provider=provider, texts=texts, use=use, monkeypatch=monkeypatch)


def _ingest_all(w, storage):
    for doc, project, _n in DOCS:
        _index_doc(storage, w["provider"], doc, w["texts"][doc], project)


def test_flag_off_changes_nothing_and_flag_on_reorders_by_maxsim(world):
    w = world
    rt = w["rt"]
    from rag.storage.hip_index import collection as col
    plain = w["use"]("plain", late=False)
    _ingest_all(w, plain)
    assert not (plain / col.COLLECTION_MV).exists() and "mv" not in json.load(open(plain / col.COLLECTION_MANIFEST))
    retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=False, rerank=False)
    off_plain = {p: _flat(asyncio.run(retriever.retrieve_and_rank_pages(QUERY, p))) for p in (None, "red")}
    cand_chunks = {p: asyncio.run(retriever.retrieve_chunks(QUERY, p)) for p in (None, "red")}
    assert all(len(v) == DEPTH for v in cand_chunks.values())

    late = w["use"]("late", late=True)
    _ingest_all(w, late)
    manifest = json.load(open(late / col.COLLECTION_MANIFEST))
    assert (late / col.COLLECTION_MV).exists() and manifest["mv"] == {"dim": 128}
    # the flag off over the very same storage: the result of a collection that never heard of the flag, field for field
    w["monkeypatch"].setenv("HIP_LATE_INTERACTION", "false")
    for p in (None, "red"):
        assert _flat(asyncio.run(retriever.retrieve_and_rank_pages(QUERY, p))) == off_plain[p]
    w["monkeypatch"].setenv("HIP_LATE_INTERACTION", "true")

    coll = col.open_collection(late)
    off, vecs = coll.mv.export()
    assert len(off) - 1 == coll.manifest.rows == sum(n for _d, _p, n in DOCS)
    for doc in coll.manifest.documents:                                      # every chunk: its tokens minus CLS
        for i, t in enumerate(w["texts"][doc["doc_id"]]):
            row = doc["row0"] + i
            assert off[row + 1] - off[row] == len(w["provider"].tokenizer.encode(t.strip(), L)) - 1
    _vec, q_vecs, q_counts = asyncio.run(w["provider"].embed_single_colbert(QUERY))
    q = bf16_values(q_vecs[0, :int(q_counts[0])].cpu().view(__import__("torch").int16).numpy().view(np.uint16)).astype(np.float64)
    assert len(q) == len(QUERY.split()) + 1                                  # the query's tokens and EOS
    from rag.storage.hip_index.passages import rows_of_chunks
    for p in (None, "red"):
        got = asyncio.run(retriever.retrieve_chunks(QUERY, p))
        assert len(got) == TOP_K and all(c.metadata["rerank_mode"] == "colbert" for c in got)
        cands = cand_chunks[p]
        rows = rows_of_chunks(coll, cands)
        ref = [maxsim_expected(q, bf16_values(vecs[off[r]:off[r + 1]]).astype(np.float64), "random") for r in rows]
        by_id = {c.chunk_id: j for j, c in enumerate(cands)}
        worst = 0.0
        for c in got:
            want, bound = ref[by_id[c.chunk_id]]
            worst = max(worst, abs(c.metadata["colbert_score"] - want) / bound)
            assert c.score == cands[by_id[c.chunk_id]].score                 # the dense similarity stays the chunk's score
        print(f"overlay maxsim project {p}: worst |got - ref| / bound = {worst:.3g}")
        assert worst <= 1.0
        # the order is the reference's wherever the reference separates two chunks by more than both bounds
        order = sorted(range(len(cands)), key=lambda j: (-ref[j][0], j))
        got_pos = [by_id[c.chunk_id] for c in got]
        assert [c.metadata["colbert_score"] for c in got] == sorted((c.metadata["colbert_score"] for c in got), reverse=True)
        for a, b in zip(order[:TOP_K], got_pos):
            assert a == b or abs(ref[a][0] - ref[b][0]) <= ref[a][1] + ref[b][1], (p, order[:TOP_K], got_pos)
        if p == "red":
            assert all(c.metadata["doc_id"] in ("docA", "docC") for c in got)

    # under HIP_PAGES the candidates stay on the device: the pages of the host path keyed by (document, page)
    w["monkeypatch"].setenv("HIP_PAGES", "true")
    for p in (None, "red"):
        chunks = asyncio.run(retriever.retrieve_chunks(QUERY, p))
        keyed = [dataclasses.replace(c, page=(c.metadata["doc_id"], c.page)) for c in chunks]
        want = rt.rank_pages(rt.group_chunks_by_page(keyed))[:MAX_PAGES]
        got = asyncio.run(retriever.retrieve_and_rank_pages(QUERY, p))
        assert len(got) == len(want) > 0
        for g, x in zip(got, want):
            assert (g.metadata["doc_id"], g.page) == x.page and np.float64(g.score).tobytes() == np.float64(x.score).tobytes()
            assert [c.chunk_id for c in g.chunks] == [c.chunk_id for c in x.chunks]
            for a, b in zip(g.chunks, x.chunks):
                assert a.metadata["rerank_mode"] == "colbert"
                assert np.float32(a.metadata["colbert_score"]).tobytes() == np.float32(b.metadata["colbert_score"]).tobytes()


def test_the_store_follows_the_collection_and_a_cold_cache_loads_it(world):
    w = world
    from hiprag import MultiVectorStore
    from rag.storage.hip_index import collection as col
    late = w["use"]("late", late=True)
    _ingest_all(w, late)
    col.delete_document("docB", storage_dir=late)
    new_a = _texts(7, 999)
    _index_doc(late, w["provider"], "docA", new_a, "red", replace=True)
    live = col.open_collection(late)
    assert [d["doc_id"] for d in live.manifest.documents] == ["docC", "docA"] and len(live.mv) == live.manifest.rows == 17
    # a fresh build of the surviving documents in their final order
    fresh_dir = w["use"]("fresh", late=True)
    _index_doc(fresh_dir, w["provider"], "docC", w["texts"]["docC"], "red")
    _index_doc(fresh_dir, w["provider"], "docA", new_a, "red")
    fresh = col.open_collection(fresh_dir)
    for a, b in zip(live.mv.export(), fresh.mv.export()):
        assert a.tobytes() == b.tobytes()
    # a cold cache LOADS hip_collection.mv
    before = [a.tobytes() for a in live.mv.export()]
    w["use"]("late", late=True)                                              # clears every cache
    cold = col.open_collection(late)
    assert cold is not live and cold.mv is not live.mv
    assert [a.tobytes() for a in cold.mv.export()] == before
    assert [a.tobytes() for a in MultiVectorStore.load(str(late / col.COLLECTION_MV)).export()] == before
    # a file whose document count is not the manifest's raises; so does a missing one: nothing is encoded again silently
    other = MultiVectorStore(128, max_doc_vectors=4)
    other.append([np.zeros((1, 128), np.uint16)])
    keep = (late / col.COLLECTION_MV).read_bytes()
    other.save(str(late / col.COLLECTION_MV))
    w["hi"].clear_caches()
    with pytest.raises(RuntimeError, match="multi-vector"):
        col.open_collection(late)
    (late / col.COLLECTION_MV).unlink()
    with pytest.raises(RuntimeError, match="missing"):
        col.open_collection(late)
    (late / col.COLLECTION_MV).write_bytes(keep)
    assert [a.tobytes() for a in col.open_collection(late).mv.export()] == before


def test_refused_combinations(world):
    w = world
    rt, mp = w["rt"], w["monkeypatch"]
    from rag.config import config
    from rag.storage.hip_index import collection as col
    late = w["use"]("late", late=True)
    _index_doc(late, w["provider"], "docA", w["texts"]["docA"], "red")
    retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=False, rerank=False)
    assert asyncio.run(retriever.retrieve_chunks(QUERY))                     # the combination that works
    mp.setenv("HIP_RERANK", "true")                                          # two second stages
    with pytest.raises(ValueError, match="two second stages"):
        config.HIP_LATE_INTERACTION
    with pytest.raises(ValueError, match="two second stages"):
        asyncio.run(retriever.retrieve_chunks(QUERY))
    mp.delenv("HIP_RERANK")
    with pytest.raises(ValueError, match="two second stages"):
        asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, hybrid=False, rerank=True).retrieve_chunks(QUERY))
    mp.setenv("HIP_COLLECTION", "false")                                     # no collection
    with pytest.raises(ValueError, match="HIP_COLLECTION"):
        asyncio.run(retriever.retrieve_chunks(QUERY))
    with pytest.raises(ValueError, match="HIP_COLLECTION"):
        _index_doc(late, w["provider"], "docB", w["texts"]["docB"], "blue")
    mp.setenv("HIP_COLLECTION", "true")

    class NoHead:                                                            # a provider without the head
        async def embed_batch(self, texts, instruction=None):
            return [[0.0] * 128 for _ in texts]
    with pytest.raises(RuntimeError, match="ColBERT head"):
        _index_doc(late, NoHead(), "docB", w["texts"]["docB"], "blue")
    # a collection ingested without the vectors: no late query, no late append; and one with them takes no plain append
    plain = w["use"]("plain", late=False)
    _index_doc(plain, w["provider"], "docA", w["texts"]["docA"], "red")
    mp.setenv("HIP_LATE_INTERACTION", "true")
    with pytest.raises(RuntimeError, match="per-token vectors"):
        asyncio.run(retriever.retrieve_chunks(QUERY))
    with pytest.raises(RuntimeError, match="without per-token vectors"):
        _index_doc(plain, w["provider"], "docB", w["texts"]["docB"], "blue")
    assert [d["doc_id"] for d in col.open_collection(plain).manifest.documents] == ["docA"]
    w["use"]("late", late=False)
    with pytest.raises(RuntimeError, match="keeps per-token vectors"):
        _index_doc(late, w["provider"], "docB", w["texts"]["docB"], "blue")
    coll = col.open_collection(late)
    assert [d["doc_id"] for d in coll.manifest.documents] == ["docA"] and len(coll.mv) == coll.manifest.rows
