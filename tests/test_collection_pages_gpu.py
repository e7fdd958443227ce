"""
Page ranking inside the retriever over the collection: with HIP_COLLECTION=true and HIP_PAGES=true
HybridRetriever.retrieve_and_rank_pages ranks the pages on the device and returns what the host path returns when it keys
pages by (doc_id, page) -- the same pages in order, scores bit for bit, chunk ids in order, metadata; the collection's page
table follows index_chunks, delete_document and replace_document on the device; with HIP_PAGES unset the query returns
what it returned before.
"""
import asyncio
import dataclasses
import json

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

D, DEPTH, TOP_K, L, MAX_PAGES = 64, 12, 7, 128, 3
RERANK_ATOL = 1.5e-2            # tests/test_encoder_gpu.py::test_reranker_head_logits
DOCS = [("docA", "red", 9), ("docB", "blue", 6), ("docC", "red", 7)]       # pages 1 + i // 4: every document has pages 1 and 2
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


def _index_doc(tmp_path, doc, x, texts, project, replace=False, first_page=1):
    from rag.ingest.indexing import index_chunks
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": first_page + i // 4, "metadata": {"title": doc}} for i, t in enumerate(texts)]
    with open(tmp_path / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=tmp_path, provider=_TableProvider(x), with_sparse=True, project=project,
                                    replace=replace))


def _host_keyed(rt, retriever, query, project, max_pages):
    """the host path with (doc_id, page) as the chunk's page key"""
    chunks = asyncio.run(retriever.retrieve_chunks(query, project))
    keyed = [dataclasses.replace(c, page=(c.metadata["doc_id"], c.page)) for c in chunks]
    return chunks, rt.rank_pages(rt.group_chunks_by_page(keyed))[:max_pages]


def _same_pages(got, want, tag):
    assert len(got) == len(want) and len(got) > 0, tag
    for g, w in zip(got, want):
        assert g.page == w.page[1] and g.metadata["doc_id"] == w.page[0], tag
        assert np.float64(g.score).tobytes() == np.float64(w.score).tobytes(), (tag, g.score, w.score)
        assert [c.chunk_id for c in g.chunks] == [c.chunk_id for c in w.chunks], tag
        assert g.metadata == {k: v for k, v in g.chunks[0].metadata.items()}, tag
        for a, b in zip(g.chunks, w.chunks):
            assert (a.text, a.page) == (b.text, b.page[1]), tag
            assert np.float64(a.score).tobytes() == np.float64(b.score).tobytes(), tag
            assert list(a.metadata) == list(b.metadata), (tag, a.metadata, b.metadata)          # the same keys in the same order
            for k, v in b.metadata.items():
                if k == "rerank_score":
                    assert abs(a.metadata[k] - v) <= RERANK_ATOL, tag
                else:
                    assert a.metadata[k] == v, (tag, k)


def test_retriever_ranks_pages_on_the_device_and_the_table_follows(gpu, tmp_path, monkeypatch):
    import hiprag
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    from hiprag import EncoderConfig, HipEncoder, random_state
    from rag.providers.hip.tokenizer import HashTokenizer
    from rag.query.reranker import CrossEncoderReranker
    from rag.storage.hip_index import collection as col
    from rag.storage.hip_index import pages as pg
    monkeypatch.setenv("HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "l2")
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    monkeypatch.setattr(hi.config, "HIP_SEARCH_ALL_DOCUMENTS", False)
    monkeypatch.setattr(hi.config, "RERANKER_ENABLED", True)
    monkeypatch.setattr(hi.config, "RERANKER_TOP_K", TOP_K)
    monkeypatch.setenv("STORAGE_DIR", str(tmp_path))
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_RERANK", "true")
    monkeypatch.setenv("HIP_PAGES", "true")
    monkeypatch.setenv("HIP_ALLOW_SYNTHETIC", "1")
    qp = _QueryProvider()
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: qp)
    hi.clear_caches()

    cfg = EncoderConfig(vocab=2000, hidden=256, layers=2, heads=4, ffn=512, max_pos=200, max_seq_len=L)
    enc = HipEncoder(cfg, random_state(cfg, seed=9, with_head=True), with_head=True)
    reranker = CrossEncoderReranker(encoder=enc, tokenizer=HashTokenizer(cfg.vocab), top_k=TOP_K)
    monkeypatch.setattr(rt, "_RERANKER", reranker)

    xs = {doc: ho.synthetic_vectors(n, D, seed=700 + j) for j, (doc, _p, n) in enumerate(DOCS)}
    texts = {doc: _texts(n, 800 + j) for j, (doc, _p, n) in enumerate(DOCS)}
    for doc, project, _n in DOCS:
        _index_doc(tmp_path, doc, xs[doc], texts[doc], project)
    query = "w3 w17\nw5"
    qp.table[query] = xs["docC"][4]

    seen = {"sparse_only": False, "shared_page": False}

    def check(hybrid, rerank, project):
        tag = f"hybrid={hybrid} rerank={rerank} project={project}"
        retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=hybrid, rerank=rerank)
        chunks, want = _host_keyed(rt, retriever, query, project, MAX_PAGES)
        got = asyncio.run(retriever.retrieve_and_rank_pages(query, project))
        print(f"\n[collection pages {tag}] " + ", ".join(f"{w.page}: {w.score!r} x{len(w.chunks)}" for w in want))
        _same_pages(got, want, tag)
        seen["sparse_only"] |= any(c.metadata.get("sparse_only") for w in want for c in w.chunks)
        seen["shared_page"] |= len({c.page for c in chunks}) < len({(c.metadata["doc_id"], c.page) for c in chunks})
        if project == "red":
            assert all(c.metadata["doc_id"] in ("docA", "docC") for g in got for c in g.chunks), tag
        if rerank:
            assert all("rerank_score" in c.metadata for g in got for c in g.chunks), tag
        # max_pages as an argument, and beyond the pages there are
        _same_pages(asyncio.run(retriever.retrieve_and_rank_pages(query, project, 1)), want[:1], tag)
        every = _host_keyed(rt, retriever, query, project, 10 ** 6)[1]
        _same_pages(asyncio.run(retriever.retrieve_and_rank_pages(query, project, 200)), every, tag)

    for project in (None, "red"):
        check(False, False, project)
        check(True, False, project)
        check(False, True, project)
        check(True, True, project)
    assert seen["sparse_only"], "no selected page held a sparse-only chunk: the hybrid case is not covered"
    assert seen["shared_page"], "no two documents shared a page number among the candidates"

    def check_table(tag):
        coll = col.open_collection(tmp_path)
        live = pg.live_collection_pages(coll)
        assert live is not None, tag                                               # it followed; it was not dropped
        pages, tags = live.export()
        want, offsets = pg.collection_pages(coll.manifest, tmp_path)
        assert len(live) == coll.manifest.rows == len(want), tag
        assert pages.tobytes() == want.tobytes(), tag
        doc_of_row = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
        assert np.array_equal(tags[:, None] == tags[None, :], doc_of_row[:, None] == doc_of_row[None, :]), tag     # the partition
        pg.clear_page_cache()
        rebuilt = pg.get_collection_pages(coll)
        assert rebuilt is not live
        r_pages, r_tags = rebuilt.export()
        assert r_pages.tobytes() == pages.tobytes(), tag
        assert np.array_equal(r_tags[:, None] == r_tags[None, :], tags[:, None] == tags[None, :]), tag

    plain = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES)
    check_table("built by the first query")
    asyncio.run(plain.retrieve_and_rank_pages(query))                                # live again after the rebuild above
    xs["docD"], texts["docD"] = ho.synthetic_vectors(5, D, seed=710), _texts(5, 810)
    _index_doc(tmp_path, "docD", xs["docD"], texts["docD"], "blue", first_page=2)
    check_table("index_chunks")
    asyncio.run(plain.retrieve_and_rank_pages(query))
    col.delete_document("docA", tmp_path)
    check_table("delete_document")
    asyncio.run(plain.retrieve_and_rank_pages(query))
    xs["docB"], texts["docB"] = ho.synthetic_vectors(8, D, seed=720), _texts(8, 820)
    _index_doc(tmp_path, "docB", xs["docB"], texts["docB"], "blue", replace=True, first_page=5)
    check_table("replace_document")
    check(True, False, None)                                                         # and the queries see the change
    check(False, False, "blue")

    # a page the table cannot hold: the device path hands back to the host path
    chunks = [{"chunk_id": f"docE_{i:04d}", "text": t, "page": "iv", "metadata": {}} for i, t in enumerate(_texts(4, 830))]
    with open(tmp_path / "docE_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    from rag.ingest.indexing import index_chunks
    asyncio.run(index_chunks("docE", chunks, storage_dir=tmp_path, provider=_TableProvider(ho.synthetic_vectors(4, D, seed=730)),
                             with_sparse=True, project="blue"))
    coll = col.open_collection(tmp_path)
    assert pg.live_collection_pages(coll) is None                                    # the entry was dropped, not half updated
    with pytest.raises(pg.PageValueError):
        pg.get_collection_pages(coll)
    got = asyncio.run(plain.retrieve_and_rank_pages(query))
    host = plain.select_top_pages(plain.rank_pages(plain.group_chunks_by_page(asyncio.run(plain.retrieve_chunks(query)))))
    assert [(g.page, g.score, [c.chunk_id for c in g.chunks]) for g in got] == [(h.page, h.score, [c.chunk_id for c in h.chunks]) for h in host]
    col.delete_document("docE", tmp_path)

    # the switch unset: what the query returns today, and the device ranking is not asked for
    monkeypatch.delenv("HIP_PAGES")
    monkeypatch.setattr(hiprag, "rank_pages_device", lambda *a, **k: pytest.fail("the device ranking ran with HIP_PAGES unset"))
    for hybrid in (False, True):
        r = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=hybrid)
        off = asyncio.run(r.retrieve_and_rank_pages(query, "blue"))
        today = r.select_top_pages(r.rank_pages(r.group_chunks_by_page(asyncio.run(r.retrieve_chunks(query, "blue")))))
        assert len(off) > 0
        assert [(p.page, p.score, p.metadata, [(c.chunk_id, c.score, c.metadata) for c in p.chunks]) for p in off] == \
               [(p.page, p.score, p.metadata, [(c.chunk_id, c.score, c.metadata) for c in p.chunks]) for p in today]
    hi.clear_caches()
