"""
HIP_COLLECTION=true through the drop-in: index_chunks(..., project=...) appends every document to the collection index,
search_hip_by_vector(vec, limit, project) answers from the documents of that project only -- ids and order those of the CPU
oracle over that project's rows, every row enriched from its own document's chunk table -- and with the switch unset the
same calls behave as before (first file only, `project` ignored).
"""
import asyncio
import json

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

DOCS = [("docA", "red", 130), ("docB", "blue", 70), ("docC", "red", 33), ("docD", "green", 257), ("docE", "blue", 5),
        ("docF", "blue", 64)]       # ingest order = row order; red = A + C (a gap between), blue = B, E + F (adjacent)
D = 64


class _TableProvider:
    """Stands for the encoder: chunk text "c<i>" embeds to row i of x."""

    def __init__(self, x):
        self.x = x

    async def embed_batch(self, texts, instruction=None):
        return [[float(v) for v in self.x[int(t[1:])]] for t in texts]


def _chunks(n, doc):
    return [{"chunk_id": f"{doc}_{i:04d}", "text": f"c{i}", "page": 1 + i // 7, "metadata": {"title": doc}} for i in range(n)]


def _index_doc(tmp_path, doc, x, project):
    from rag.ingest.indexing import index_chunks
    chunks = _chunks(len(x), doc)
    with open(tmp_path / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=tmp_path, provider=_TableProvider(x), with_sparse=False, project=project))


def _vectors():
    xs, row0 = {}, 0
    for i, (doc, _p, n) in enumerate(DOCS):
        xs[doc] = ho.synthetic_vectors(n, D, seed=300 + i)
        row0 += n
    return xs


def _expected(xs, q, limit, project):
    """chunk ids the oracle ranks first among the rows of the project's documents, in collection row order"""
    docs = [(doc, n) for doc, p, n in DOCS if project is None or p == project]
    if not docs:
        return [], []
    x = np.concatenate([xs[doc] for doc, _ in docs])
    owner = [(doc, i) for doc, n in docs for i in range(n)]
    s, i = ho.flat_search(x, q[None, :], limit, ho.METRIC_L2)
    keep = i[0] >= 0
    scores = np.clip(1.0 - s[0][keep].astype(np.float64) / 2.0, 0.0, 1.0)
    return [f"{owner[j][0]}_{owner[j][1]:04d}" for j in i[0][keep]], scores


def _check(rows, xs, q, limit, project):
    want_ids, want_scores = _expected(xs, q, limit, project)
    assert [r["chunk_id"] for r in rows] == want_ids, project
    assert np.allclose([r["score"] for r in rows], want_scores, rtol=0, atol=1e-4)
    allowed = {doc for doc, p, _n in DOCS if project is None or p == project}
    for r in rows:                                          # enriched from the right document's chunk table
        doc, local = r["chunk_id"].rsplit("_", 1)
        assert r["doc_id"] == doc and doc in allowed
        assert r["title"] == doc and r["text"] == f"c{int(local)}" and r["page"] == 1 + int(local) // 7


def test_collection_and_project_scopes(gpu, tmp_path, monkeypatch):
    import rag.storage.hip_index as hi
    from rag.storage.hip_index import collection as col
    monkeypatch.setenv("HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "l2")
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    monkeypatch.setattr(hi.config, "HIP_SEARCH_ALL_DOCUMENTS", False)
    monkeypatch.setenv("STORAGE_DIR", str(tmp_path))
    monkeypatch.setenv("HIP_COLLECTION", "true")
    hi.clear_caches()
    xs = _vectors()
    total = 0
    for doc, project, n in DOCS:
        summary = _index_doc(tmp_path, doc, xs[doc], project)
        total += n
        assert summary["collection_rows"] == total and summary["vectors_indexed"] == n
        assert open(tmp_path / f"{doc}_hip.index", "rb").read(8) == b"HIPIDX01"      # the per-document file as before
    assert open(tmp_path / col.COLLECTION_INDEX, "rb").read(8) == b"HIPIDX01"
    manifest = json.loads((tmp_path / col.COLLECTION_MANIFEST).read_text())
    assert [(d["doc_id"], d["project"], d["rows"]) for d in manifest["documents"]] == DOCS
    coll = col.open_collection()
    assert coll.manifest.scope_for("red") == [(0, 130), (200, 233)]
    assert coll.manifest.scope_for("blue") == [(130, 200), (490, 559)]
    with pytest.raises(ValueError, match="already in the collection"):
        _index_doc(tmp_path, "docB", xs["docB"], "blue")
    assert col.open_collection().index.ntotal == total                                # nothing was added by the refused call

    rng = np.random.default_rng(7)
    queries = [xs["docC"][4], xs["docF"][60], xs["docD"][200] + 0.05 * rng.standard_normal(D).astype(np.float32),
               ho.synthetic_queries(1, D, seed=9)[0]]

    def run_all(tag):
        for q in queries:
            for project in ("red", "blue", "green", None):
                for limit in (1, 20):
                    rows = asyncio.run(hi.search_hip_by_vector(q.tolist(), limit, project=project))
                    assert len(rows) == limit, (tag, project)
                    _check(rows, xs, q, limit, project)
            rows = asyncio.run(hi.search_hip_by_vector(q.tolist(), 200, project="blue"))   # blue holds 139 rows: padding dropped
            assert len(rows) == 139
            _check(rows, xs, q, 200, "blue")
            assert asyncio.run(hi.search_hip_by_vector(q.tolist(), 20, project="nobody")) == []

    run_all("ingested")
    with pytest.raises(RuntimeError, match="256"):
        asyncio.run(hi.search_hip_by_vector(queries[0].tolist(), 300, project="red"))
    assert len(asyncio.run(hi.search_hip_by_vector(queries[0].tolist(), 300))) == 300     # no project: the ordinary search

    # the batch form: one scoped call, one scope per distinct project
    projects = ["blue", "red", None, "blue", "nobody", "green", "red"]
    qs = np.stack([queries[i % len(queries)] for i in range(len(projects))])
    batch = col.search_collection_batch(qs, 20, projects)
    for rows, q, project in zip(batch, qs, projects):
        if project == "nobody":
            assert rows == []
        else:
            _check(rows, xs, q, 20, project)

    # the load path, then a rebuild from the per-document files: the same answers
    hi.clear_caches()
    run_all("reloaded")
    (tmp_path / col.COLLECTION_INDEX).unlink()
    (tmp_path / col.COLLECTION_MANIFEST).unlink()
    hi.clear_caches()
    assert asyncio.run(hi.search_hip_by_vector(queries[0].tolist(), 5, project="red")) == []      # no collection yet
    rebuilt = col.rebuild_collection(tmp_path, projects={doc: p for doc, p, _n in DOCS})
    assert [(d["doc_id"], d["project"], d["rows"]) for d in rebuilt.manifest.documents] == DOCS
    run_all("rebuilt")

    # the switch off: the parent's behaviour -- first file only, project ignored
    monkeypatch.delenv("HIP_COLLECTION")
    hi.clear_caches()
    first = hi.open_first_index()[1]
    for project in ("red", "blue", "nobody", None):
        rows = asyncio.run(hi.search_hip_by_vector(queries[0].tolist(), 10, project=project))
        assert len(rows) == 10 and all(r["chunk_id"].startswith(first + "_") for r in rows) and "doc_id" not in rows[0]
    summary = _index_doc(tmp_path, "docG", xs["docA"], "red")
    assert "collection_rows" not in summary
    assert json.loads((tmp_path / col.COLLECTION_MANIFEST).read_text())["documents"][-1]["doc_id"] == "docF"
    hi.clear_caches()
