"""
Hybrid retrieval over the collection: with HIP_COLLECTION=true HybridRetriever(hybrid=True).retrieve_chunks(text, project)
is ONE scoped hybrid call over the documents of that project -- chunks of those documents only, in the oracle's fused order
with the oracle's rrf_score / bm25_score / sparse_only -- and with the switch unset it is the parent's path: the first
document's index and postings, `project` ignored.
"""
import asyncio
import json

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

DOCS = [("docA", "red", 130), ("docB", "blue", 70), ("docC", "red", 33), ("docD", "blue", 257)]
EXTRA = ("docE", "red", 40)
D = 64
DEPTH = 20
WORDS = [f"w{j}" for j in range(40)]


class _TableProvider:
    """Stands for the encoder at ingest: a chunk text "c<i> ..." embeds to row i of x."""

    def __init__(self, x):
        self.x = x

    async def embed_batch(self, texts, instruction=None):
        return [[float(v) for v in self.x[int(t.split()[0][1:])]] for t in texts]


class _QueryProvider:
    """... and at query time: a query text embeds to the vector registered for it."""

    def __init__(self):
        self.table = {}

    async def embed_single(self, text, instruction=None):
        return [float(v) for v in self.table[text]]


def _texts(doc, n, seed):
    rng = np.random.default_rng(seed)
    extra = " zebra" if doc == EXTRA[0] else ""
    return [f"c{i} " + " ".join(rng.choice(WORDS, size=5)) + extra for i in range(n)]


def _chunks(doc, texts):
    return [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": 1 + i // 7, "metadata": {"title": doc}} for i, t in enumerate(texts)]


def _index_doc(tmp_path, doc, x, texts, project):
    from rag.ingest.indexing import index_chunks
    chunks = _chunks(doc, texts)
    with open(tmp_path / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=tmp_path, provider=_TableProvider(x), with_sparse=True, project=project))


def _expected(docs, xs, texts, query_text, qvec, project, depth, c=60.0, wd=1.0, ws=1.0):
    """[(chunk_id, doc, rrf_score, dense score or None, bm25_score or None)] in fused order: the oracle's dense list over the
    rows of the project's documents, its BM25 list over the same rows with the COLLECTION's impacts, ho.rrf_fuse"""
    owner = [(doc, i) for doc, _p, n in docs for i in range(n)]
    in_scope = np.asarray([project is None or p == project for _doc, p, n in docs for _ in range(n)])
    rows = np.nonzero(in_scope)[0]
    if len(rows) == 0:
        return []
    x = np.concatenate([xs[doc] for doc, _p, _n in docs])
    s, i = ho.flat_search(np.ascontiguousarray(x[rows]), qvec[None, :], depth, ho.METRIC_L2)
    di = np.where(i[0] >= 0, rows[np.maximum(i[0], 0)], -1)
    dense = {int(r): float(np.clip(1.0 - float(v) / 2.0, 0.0, 1.0)) for r, v in zip(di, s[0]) if r >= 0}
    p = ho.build_postings_from_texts([t for doc, _p, _n in docs for t in texts[doc]])
    sc = ho.bm25_scores_taat(p, [p.vocab[t] for t in ho.tokenize(query_text) if t in p.vocab])
    sc[~in_scope] = 0
    ss, si = ho.topk_desc_id_asc(sc, depth, exclude_nonpositive=True)
    bm = {int(r): float(v) for r, v in zip(si, ss) if r >= 0}
    fs, fi = ho.rrf_fuse(di[None, :], si[None, :], depth, c=c, w_a=wd, w_b=ws)
    return [(f"{owner[r][0]}_{owner[r][1]:04d}", owner[r][0], float(f), dense.get(int(r)), bm.get(int(r)))
            for r, f in zip(fi[0], fs[0]) if r >= 0]


def _check(chunks, want, tag, with_doc_id=True):
    assert [c.chunk_id for c in chunks] == [w[0] for w in want], tag
    for c, (cid, doc, rrf, dense, bm) in zip(chunks, want):
        assert c.metadata["rrf_score"] == rrf, (tag, cid)
        assert c.metadata.get("bm25_score") == bm, (tag, cid)
        assert bool(c.metadata.get("sparse_only")) == (dense is None), (tag, cid)
        assert abs(c.score - (dense or 0.0)) <= 1e-4, (tag, cid)
        assert c.metadata["title"] == doc and c.text.split()[0] == f"c{int(cid.rsplit('_', 1)[1])}"
        if with_doc_id:
            assert c.metadata["doc_id"] == doc


def test_hybrid_retriever_over_project_scopes(gpu, tmp_path, monkeypatch):
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    from rag.storage.hip_index import collection as col
    monkeypatch.setenv("HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "l2")
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    monkeypatch.setattr(hi.config, "HIP_SEARCH_ALL_DOCUMENTS", False)
    monkeypatch.setenv("STORAGE_DIR", str(tmp_path))
    monkeypatch.setenv("HIP_COLLECTION", "true")
    qp = _QueryProvider()
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: qp)
    hi.clear_caches()
    col.clear_collection_cache()

    docs = list(DOCS)
    xs = {doc: ho.synthetic_vectors(n, D, seed=400 + j) for j, (doc, _p, n) in enumerate(docs + [EXTRA])}
    texts = {doc: _texts(doc, n, 500 + j) for j, (doc, _p, n) in enumerate(docs + [EXTRA])}
    for doc, project, n in docs:
        summary = _index_doc(tmp_path, doc, xs[doc], texts[doc], project)
        assert summary["postings_indexed"] > 0
    rng = np.random.default_rng(3)
    qp.table = {
        "w3 w17 w5": xs["docC"][4],
        "W9 w9 w21 c12 unknownword": xs["docD"][200] + 0.05 * rng.standard_normal(D).astype(np.float32),
        "w30": ho.synthetic_queries(1, D, seed=9)[0],
        "zebra w1": xs[EXTRA[0]][7],
        "nothing matches here": xs["docB"][3],
    }

    def run_all(docs, tag):
        for weighted in (False, True):
            r = rt.HybridRetriever(top_chunks=DEPTH, hybrid=True, weighted=weighted)
            for text, qvec in qp.table.items():
                for project in ("red", "blue", None):
                    chunks = asyncio.run(r.retrieve_chunks(text, project))
                    want = _expected(docs, xs, texts, text, np.asarray(qvec, np.float32), project, DEPTH, 60.0, r.w_dense, r.w_sparse)
                    assert len(want) >= DEPTH
                    _check(chunks, want, (tag, text, project, weighted))
                    allowed = {doc for doc, p, _n in docs if project is None or p == project}
                    assert {c.metadata["doc_id"] for c in chunks} <= allowed
                assert asyncio.run(r.retrieve_chunks(text, "nobody")) == []

    run_all(docs, "four documents")
    r = rt.HybridRetriever(top_chunks=65, hybrid=True)
    with pytest.raises(RuntimeError, match="64"):
        asyncio.run(r.retrieve_chunks("w3 w17 w5", "red"))
    pages = asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, hybrid=True).retrieve_and_rank_pages("w3 w17 w5", "red"))
    assert pages and all(c.metadata["doc_id"] in ("docA", "docC") for pg in pages for c in pg.chunks)

    # a fifth document: the next query sees it -- the collection's postings are rebuilt, N / df / avgdl and all
    r = rt.HybridRetriever(top_chunks=DEPTH, hybrid=True)
    before = asyncio.run(r.retrieve_chunks("zebra w1", "red"))
    assert all(not c.chunk_id.startswith("docE") for c in before)
    _index_doc(tmp_path, EXTRA[0], xs[EXTRA[0]], texts[EXTRA[0]], EXTRA[1])
    docs.append(EXTRA)
    after = asyncio.run(r.retrieve_chunks("zebra w1", "red"))
    hit = [c for c in after if c.chunk_id == "docE_0007"]
    assert hit and "bm25_score" in hit[0].metadata and not hit[0].metadata.get("sparse_only")
    run_all(docs, "five documents")

    # the switch off: the parent's path -- the first document's index and postings, `project` ignored
    monkeypatch.delenv("HIP_COLLECTION")
    hi.clear_caches()
    first = hi.open_first_index()[1]
    n_first = [n for doc, _p, n in docs if doc == first][0]
    r = rt.HybridRetriever(top_chunks=DEPTH, hybrid=True)
    for text, qvec in qp.table.items():
        want = _expected([(first, None, n_first)], xs, texts, text, np.asarray(qvec, np.float32), None, DEPTH)
        for project in ("red", "blue", "nobody", None):
            chunks = asyncio.run(r.retrieve_chunks(text, project))
            _check(chunks, want, ("off", text, project), with_doc_id=False)
            assert all(c.metadata["doc_id"] is None for c in chunks)
    hi.clear_caches()
