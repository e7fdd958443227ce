"""
Late interaction as the FIRST stage inside the drop-in (HIP_LATE_SEARCH=true with HIP_LATE_INTERACTION=true and
HIP_COLLECTION=true): the retriever's chunks are `maxsim_search` over the project's scope -- the same ids in the same order,
the same score bits --, no chunk of another project appears, `score` is the score_ids similarity under the collection's
transform, the HIP_PAGES path (ids left on the device) ranks the host path's pages, the search follows a delete_document,
and with the setting off the result is what it was.  The fixture is tests/test_colbert_overlay_gpu.py's: synthetic weights,
about 30 chunks in two projects.
"""
import asyncio
import dataclasses

import numpy as np
import pytest

from test_colbert_overlay_gpu import DEPTH, DOCS, MAX_PAGES, QUERY, TOP_K, _flat, _ingest_all, world  # noqa: F401  (world: the fixture)

pytestmark = pytest.mark.gpu


def _expected(w, coll, project, depth):
    """(chunk ids, colbert scores, dense scores) of maxsim_search over scope_for(project), and score_ids for those rows"""
    import torch
    from hiprag import maxsim_search
    from rag.storage.hip_index import collection as col
    vec, q_vecs, q_counts = asyncio.run(w["provider"].embed_single_colbert(QUERY))
    qv = q_vecs.cpu().view(torch.int16).numpy().view(np.uint16)
    scores, ids = maxsim_search(coll.mv, qv, q_counts.cpu().numpy(), [coll.manifest.scope_for(project)], None, depth)
    rows = [int(r) for r in ids[0] if r >= 0]
    dense = coll.index.score_ids(np.asarray([vec], np.float32), np.asarray([rows], np.int64), return64=True)
    dense = dict(col._transform(coll, dense[0].tolist(), rows))
    chunk_ids = []
    for r in rows:
        doc_id, local = coll.manifest.locate(r)
        chunk_ids.append(f"{doc_id}_{local:04d}")
    return chunk_ids, [float(s) for s in scores[0][:len(rows)]], [dense[r] for r in rows]


def test_the_first_stage_is_the_maxsim_search_over_the_project(world):  # noqa: F811
    w = world
    rt, mp = w["rt"], w["monkeypatch"]
    from rag.storage.hip_index import collection as col
    mp.delenv("HIP_LATE_SEARCH", raising=False)
    late = w["use"]("late", late=True)
    _ingest_all(w, late)
    retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=False, rerank=False)
    before = {p: _flat(asyncio.run(retriever.retrieve_and_rank_pages(QUERY, p))) for p in (None, "red", "blue")}
    coll = col.open_collection(late)

    mp.setenv("HIP_LATE_SEARCH", "true")
    for p in (None, "red", "blue"):
        want_ids, want_colbert, want_dense = _expected(w, coll, p, DEPTH)
        in_scope = sum(n for _d, proj, n in DOCS if p is None or proj == p)
        assert len(want_ids) == min(DEPTH, in_scope)
        got = asyncio.run(retriever.retrieve_chunks(QUERY, p))
        assert [c.chunk_id for c in got] == want_ids[:TOP_K]                              # the search's order, cut to RERANKER_TOP_K
        for c, cs, ds in zip(got, want_colbert, want_dense):
            assert np.float32(c.metadata["colbert_score"]).tobytes() == np.float32(cs).tobytes()
            assert c.metadata["rerank_mode"] == "colbert_search"
            assert np.float64(c.score).tobytes() == np.float64(ds).tobytes()              # score_ids under the usual transform
        if p is not None:
            docs = {d for d, proj, _n in DOCS if proj == p}
            assert all(c.metadata["doc_id"] in docs for c in got)                         # no chunk of the other project
        # the search can find what the dense first stage never handed to a second stage: it ranks the WHOLE scope
        rows = col.search_collection_maxsim(*asyncio.run(w["provider"].embed_single_colbert(QUERY))[1:], limit=256, project=p)
        assert len(rows) == in_scope and [r["chunk_id"] for r in rows[:DEPTH]] == want_ids
        assert [r["colbert_score"] for r in rows] == sorted((r["colbert_score"] for r in rows), reverse=True)

    # under HIP_PAGES the ids stay on the device: the pages of the host path keyed by (document, page)
    mp.setenv("HIP_PAGES", "true")
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
                assert a.metadata["rerank_mode"] == "colbert_search"
                assert np.float32(a.metadata["colbert_score"]).tobytes() == np.float32(b.metadata["colbert_score"]).tobytes()
                assert np.float64(a.score).tobytes() == np.float64(b.score).tobytes()
    mp.delenv("HIP_PAGES")

    # with the setting off the result is what it was, field for field
    mp.setenv("HIP_LATE_SEARCH", "false")
    for p in (None, "red", "blue"):
        assert _flat(asyncio.run(retriever.retrieve_and_rank_pages(QUERY, p))) == before[p]

    # a delete_document is followed by the search
    mp.setenv("HIP_LATE_SEARCH", "true")
    col.delete_document("docA", storage_dir=late)
    coll = col.open_collection(late)
    want_ids, _cs, _ds = _expected(w, coll, "red", DEPTH)
    got = asyncio.run(retriever.retrieve_chunks(QUERY, "red"))
    assert [c.chunk_id for c in got] == want_ids[:TOP_K] and all(c.metadata["doc_id"] == "docC" for c in got)
    assert asyncio.run(retriever.retrieve_chunks(QUERY, "green")) == []                    # an unknown project


def test_refused_on_a_hybrid_retriever_and_without_the_vectors(world):  # noqa: F811
    w = world
    rt, mp = w["rt"], w["monkeypatch"]
    plain = w["use"]("plain", late=False)
    _ingest_all(w, plain)
    mp.setenv("HIP_LATE_SEARCH", "true")
    retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=False, rerank=False)
    with pytest.raises(ValueError, match="HIP_LATE_INTERACTION"):
        asyncio.run(retriever.retrieve_chunks(QUERY, "red"))
    mp.setenv("HIP_LATE_INTERACTION", "true")
    with pytest.raises(RuntimeError, match="per-token vectors"):                           # a collection ingested without them
        asyncio.run(retriever.retrieve_chunks(QUERY, "red"))
    with pytest.raises(ValueError, match="hybrid"):
        asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, hybrid=True, rerank=False).retrieve_chunks(QUERY, "red"))
    mp.setenv("HIP_PAGES", "true")
    with pytest.raises(ValueError, match="hybrid"):
        asyncio.run(rt.HybridRetriever(top_chunks=DEPTH, hybrid=True, rerank=False).retrieve_and_rank_pages(QUERY, "red"))
