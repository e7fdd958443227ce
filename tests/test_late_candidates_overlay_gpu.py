"""
Candidate generation inside the drop-in (HIP_LATE_CANDIDATES with HIP_LATE_SEARCH=true): train_collection_centroids writes
hip_collection.mvc and the manifest entry, a cold cache attaches the table again with the same codes, the retriever's chunks
with at least as many candidates as the project has chunks are those of the exact HIP_LATE_SEARCH path, delete and replace
keep the codes in step with the vectors, and the setting refuses without HIP_LATE_SEARCH and on a collection without
centroids.  The fixture is tests/test_colbert_overlay_gpu.py's: synthetic weights, 30 chunks in two projects.
"""
import asyncio
import json

import numpy as np
import pytest

from test_colbert_overlay_gpu import DEPTH, DOCS, MAX_PAGES, QUERY, _index_doc, _ingest_all, _texts, world  # noqa: F401  (world: the fixture)

pytestmark = pytest.mark.gpu

N_CHUNKS = sum(n for _d, _p, n in DOCS)


def _chunks(retriever, project):
    got = asyncio.run(retriever.retrieve_chunks(QUERY, project))
    return [(c.chunk_id, np.float64(c.score).tobytes(), np.float32(c.metadata["colbert_score"]).tobytes(), c.metadata["rerank_mode"])
            for c in got]


def test_training_writes_the_table_and_the_pruned_retriever_equals_the_exact_one(world):  # noqa: F811
    w = world
    rt, mp = w["rt"], w["monkeypatch"]
    from rag.storage.hip_index import collection as col
    for name in ("HIP_LATE_SEARCH", "HIP_LATE_CANDIDATES"):
        mp.delenv(name, raising=False)
    late = w["use"]("late", late=True)
    _ingest_all(w, late)
    assert not (late / col.COLLECTION_MVC).exists() and "mvc" not in json.load(open(late / col.COLLECTION_MANIFEST))
    coll = col.train_collection_centroids(late, ncent=32)
    table = np.load(late / col.COLLECTION_MVC)
    assert table.dtype == np.uint16 and table.shape == (32, 128) and np.array_equal(table, coll.mv.centroids())
    assert json.load(open(late / col.COLLECTION_MANIFEST))["mvc"] == {"ncent": 32}
    nv = coll.mv.sizes()[1]
    assert coll.mv.centroid_info() == (32, nv, 4 * nv)
    codes = coll.mv.codes().copy()
    # a cold cache attaches the table again: the same codes
    w["use"]("late", late=True)
    cold = col.open_collection(late)
    assert cold is not coll and np.array_equal(cold.mv.codes(), codes) and np.array_equal(cold.mv.centroids(), table)

    # with at least as many candidates as chunks, the pruned path returns the exact path's chunks, field for field
    mp.setenv("HIP_LATE_SEARCH", "true")
    retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=False, rerank=False)
    exact = {p: _chunks(retriever, p) for p in (None, "red", "blue")}
    assert all(exact.values()) and cold.mv.pruned_info()["chunks"] == 0          # no pruned call so far
    mp.setenv("HIP_LATE_CANDIDATES", str(N_CHUNKS))
    for p in (None, "red", "blue"):
        assert _chunks(retriever, p) == exact[p]
    info = cold.mv.pruned_info()
    assert info["chunks"] == 1 and info["exact_pairs"] > 0                       # the pruned entry ran
    assert _chunks(retriever, "green") == []                                     # an unknown project
    # fewer candidates than the limit: max(limit, HIP_LATE_CANDIDATES) candidates, still the exact path's result here
    mp.setenv("HIP_LATE_CANDIDATES", "1")
    rows = col.search_collection_maxsim(*asyncio.run(w["provider"].embed_single_colbert(QUERY))[1:], limit=N_CHUNKS, project=None)
    mp.setenv("HIP_LATE_CANDIDATES", "0")
    assert rows == col.search_collection_maxsim(*asyncio.run(w["provider"].embed_single_colbert(QUERY))[1:], limit=N_CHUNKS, project=None)

    # delete and replace keep the codes in step: they equal a re-attach of the same table
    mp.setenv("HIP_LATE_CANDIDATES", str(N_CHUNKS))
    col.delete_document("docB", storage_dir=late)
    _index_doc(late, w["provider"], "docA", _texts(7, 999), "red", replace=True)
    live = col.open_collection(late)
    assert [d["doc_id"] for d in live.manifest.documents] == ["docC", "docA"]
    assert live.mv.centroid_info()[:2] == (32, live.mv.sizes()[1]) and json.load(open(late / col.COLLECTION_MANIFEST))["mvc"] == {"ncent": 32}
    kept = live.mv.codes().copy()
    live.mv.attach_centroids(table)
    assert np.array_equal(live.mv.codes(), kept)
    pruned = _chunks(retriever, "red")
    mp.setenv("HIP_LATE_CANDIDATES", "0")
    assert pruned == _chunks(retriever, "red") and pruned

    # a conversion attaches the table to the converted store
    live.convert_multivectors("fp8")
    assert live.mv.format == "fp8" and live.mv.centroid_info()[0] == 32 and np.array_equal(live.mv.centroids(), table)
    w["use"]("late", late=True)
    assert np.array_equal(col.open_collection(late).mv.codes(), live.mv.codes())

    # a manifest that names a missing or mis-shaped table raises and names the training function
    keep = (late / col.COLLECTION_MVC).read_bytes()
    np.save(open(late / col.COLLECTION_MVC, "wb"), table[:, :64])
    w["use"]("late", late=True)
    with pytest.raises(RuntimeError, match="train_collection_centroids"):
        col.open_collection(late)
    (late / col.COLLECTION_MVC).unlink()
    with pytest.raises(RuntimeError, match="train_collection_centroids"):
        col.open_collection(late)
    (late / col.COLLECTION_MVC).write_bytes(keep)
    assert col.open_collection(late).mv.centroid_info()[0] == 32
    # and training again replaces what is there; ncent = 0 chooses by the number of stored vectors
    again = col.train_collection_centroids(late)
    assert again.mv.centroid_info()[0] % 32 == 0 and json.load(open(late / col.COLLECTION_MANIFEST))["mvc"] == {"ncent": again.mv.centroid_info()[0]}


def test_the_setting_refuses_without_the_search_and_without_centroids(world):  # noqa: F811
    w = world
    rt, mp = w["rt"], w["monkeypatch"]
    from rag.storage.hip_index import collection as col
    late = w["use"]("late", late=True)
    _ingest_all(w, late)
    retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=False, rerank=False)
    mp.delenv("HIP_LATE_SEARCH", raising=False)
    mp.setenv("HIP_LATE_CANDIDATES", "16")
    with pytest.raises(ValueError, match="HIP_LATE_SEARCH"):
        asyncio.run(retriever.retrieve_chunks(QUERY, "red"))
    mp.setenv("HIP_LATE_SEARCH", "true")
    with pytest.raises(RuntimeError, match="train_collection_centroids"):          # a collection without centroids
        asyncio.run(retriever.retrieve_chunks(QUERY, "red"))
    for bad in ("257", "-1", "many"):
        mp.setenv("HIP_LATE_CANDIDATES", bad)
        with pytest.raises(ValueError, match="HIP_LATE_CANDIDATES"):
            asyncio.run(retriever.retrieve_chunks(QUERY, "red"))
    mp.setenv("HIP_LATE_CANDIDATES", "0")
    assert asyncio.run(retriever.retrieve_chunks(QUERY, "red"))                   # off: the exact search, as before
    plain = w["use"]("plain", late=False)
    _ingest_all(w, plain)
    with pytest.raises(RuntimeError, match="per-token vectors"):
        col.train_collection_centroids(plain)
