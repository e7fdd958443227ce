"""
The collection's BM25 postings follow ingest, delete and replace on the device: under HIP_COLLECTION=true, once the
collection's sparse index is live, index_chunks / delete_document / index_chunks(replace=True) update it in place
(rag/storage/hip_index/sparse.py follow_collection) and the next hybrid query does NOT rebuild the postings from the chunk
tables -- collection_postings runs once.  Every result equals, bit for bit, the one a forced rebuild gives.
"""
import asyncio
import json

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

D = 64
DEPTH = 20
WORDS = [f"w{j}" for j in range(40)]


class _TableProvider:
    """Stands for the encoder at ingest: a chunk text "c<i> ..." embeds to row i of x."""

    def __init__(self, x):
        self.x = x

    async def embed_batch(self, texts, instruction=None):
        return [[float(v) for v in self.x[int(t.split()[0][1:])]] for t in texts]


def _texts(n, seed, extra=""):
    rng = np.random.default_rng(seed)
    return [f"c{i} " + " ".join(rng.choice(WORDS, size=5)) + extra for i in range(n)]


def _index_doc(tmp_path, doc, x, texts, project, replace=False):
    from rag.ingest.indexing import index_chunks
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": 1 + i // 7, "metadata": {"title": doc}} for i, t in enumerate(texts)]
    with open(tmp_path / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=tmp_path, provider=_TableProvider(x), with_sparse=True, project=project,
                                    replace=replace))


def test_collection_postings_follow_ingest_delete_and_replace(gpu, tmp_path, monkeypatch):
    import torch
    import rag.storage.hip_index as hi
    from hiprag import HipBM25Updatable, hybrid_search_scoped_device
    from rag.storage.hip_index import collection as col, sparse
    monkeypatch.setenv("HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "l2")
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    monkeypatch.setenv("STORAGE_DIR", str(tmp_path))
    monkeypatch.setenv("HIP_COLLECTION", "true")
    hi.clear_caches()
    col.clear_collection_cache()
    sparse.clear_sparse_cache()
    calls = {"live": 0, "forced": 0}
    forced = [False]
    real_postings = col.collection_postings

    def counting(manifest, storage_dir=None):
        calls["forced" if forced[0] else "live"] += 1
        return real_postings(manifest, storage_dir)

    monkeypatch.setattr(col, "collection_postings", counting)

    xs = {"docA": ho.synthetic_vectors(130, D, seed=41), "docB": ho.synthetic_vectors(70, D, seed=42),
          "docC": ho.synthetic_vectors(33, D, seed=43), "docA2": ho.synthetic_vectors(90, D, seed=44),
          "docD": ho.synthetic_vectors(257, D, seed=45)}
    queries = [("w3 w17 w5", xs["docC"][4]), ("W9 w9 w21 c12 unknownword", xs["docA"][100]), ("zebra w1", xs["docD"][7]),
               ("quagga w30 w2", xs["docA2"][11]), ("nothing matches here", xs["docB"][3])]

    def run_all(tag):
        """every query x project through the one library call the retriever makes, as bit patterns; then the retriever's rows"""
        coll = col.open_collection(tmp_path)
        bm25 = sparse.get_collection_sparse(coll)
        assert isinstance(bm25, HipBM25Updatable)
        out = []
        for text, qvec in queries:
            for project in ("red", "blue", None):
                scope = coll.manifest.scope_for(project)
                if not scope:
                    out.append((text, project, None))
                    continue
                q = torch.tensor(np.asarray([qvec], np.float32), device=torch.device("cuda", coll.index.device))
                fs, fi, ((ds, di), (ss, si)) = hybrid_search_scoped_device(coll.index, bm25, q, [bm25.terms_of(text)], [scope], depth=DEPTH,
                                                                         k=DEPTH, return_lists=True)
                bits = [fs.view(torch.int32), fi, ds.view(torch.int64), di, ss.view(torch.int64), si]
                out.append((text, project, [t.cpu().numpy().copy() for t in bits]))
                rows = col.search_collection_hybrid(text, [float(v) for v in qvec], DEPTH, project, storage_dir=tmp_path)
                out.append((text, project, [(r["chunk_id"], r["doc_id"], r["rrf_score"], r.get("bm25_score"), r.get("sparse_only")) for r in rows]))
        assert bm25.sizes()["n_docs"] == coll.manifest.rows and not bm25.dirty, tag
        return out

    def check(tag):
        live = run_all(tag)
        with sparse._LOCK:
            saved = dict(sparse._SPARSE_CACHE)
        forced[0] = True
        sparse.clear_sparse_cache()
        rebuilt = run_all(tag + " (rebuilt)")
        forced[0] = False
        with sparse._LOCK:                      # the live index goes back: the next step updates IT
            sparse._SPARSE_CACHE.clear()
            sparse._SPARSE_CACHE.update(saved)
        assert len(live) == len(rebuilt)
        hits = 0
        for (text, project, a), (_t, _p, b) in zip(live, rebuilt):
            if a is None or a == [] or isinstance(a[0], tuple):
                assert a == b, (tag, text, project)
                continue
            for j, (u, v) in enumerate(zip(a, b)):
                assert np.array_equal(u, v), (tag, text, project, j)
            hits += int((a[5] >= 0).sum())
        assert hits > 0, tag
        assert calls["live"] == 1, f"{tag}: collection_postings ran {calls['live']} times outside the forced rebuilds"

    _index_doc(tmp_path, "docA", xs["docA"], _texts(130, 51), "red")
    _index_doc(tmp_path, "docB", xs["docB"], _texts(70, 52), "blue")
    _index_doc(tmp_path, "docC", xs["docC"], _texts(33, 53), "red")
    assert calls["live"] == 0
    check("three documents")                                   # the one build from the chunk tables
    assert col.delete_document("docB", tmp_path) == 70
    check("docB deleted")
    _index_doc(tmp_path, "docA", xs["docA2"], _texts(90, 54, extra=" quagga"), "red", replace=True)
    check("docA replaced")
    _index_doc(tmp_path, "docD", xs["docD"], _texts(257, 55, extra=" zebra"), "blue")
    check("docD ingested")
    coll = col.open_collection(tmp_path)
    assert [d["doc_id"] for d in coll.manifest.documents] == ["docC", "docA", "docD"] and coll.manifest.rows == 380
    info = sparse.get_collection_sparse(coll).update_info()
    assert info["kind"] == "append" and info["docs_after"] == 380
    hi.clear_caches()
    col.clear_collection_cache()
    sparse.clear_sparse_cache()
