"""
HIP_INDEX_TYPE=ivf through the drop-in: index_chunks writes a HIPIVF01 file under the usual `{doc_id}_hip.index` name, the
reader chooses the index kind by the file's magic, and with HIP_IVF_NPROBE >= nlist the enriched results are the flat
overlay's (the reference's search_faiss_by_vector, rag/storage/faiss_index.py:137-199).
"""
import asyncio
import json

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu


class _TableProvider:
    """Stands for the encoder: chunk text "c<i>" embeds to row i of x."""

    def __init__(self, x):
        self.x = x

    async def embed_batch(self, texts, instruction=None):
        return [[float(v) for v in self.x[int(t[1:])]] for t in texts]


def _chunks(n, doc):
    return [{"chunk_id": f"{doc}_{i:04d}", "text": f"c{i}", "page": 1 + i // 7, "metadata": {"title": doc}} for i in range(n)]


def _index_doc(tmp_path, doc, x):
    from rag.ingest.indexing import index_chunks
    chunks = _chunks(len(x), doc)
    with open(tmp_path / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=tmp_path, provider=_TableProvider(x), with_sparse=False))


def _same_rows(a, b):
    assert [r["chunk_id"] for r in a] == [r["chunk_id"] for r in b]
    assert np.allclose([r["score"] for r in a], [r["score"] for r in b], rtol=0, atol=1e-6)
    for r, s in zip(a, b):
        assert {k: v for k, v in r.items() if k != "score"} == {k: v for k, v in s.items() if k != "score"}


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ivf_overlay_equals_flat_overlay(gpu, tmp_path, monkeypatch, metric):
    import rag.storage.hip_index as hi
    monkeypatch.setenv("HIP_INDEX_METRIC", metric)
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", metric)
    n, d = 900, 64
    x = ho.synthetic_vectors(n, d, seed=151)
    q = x[[5, 77, 400]] + 0.1 * ho.synthetic_vectors(3, d, seed=152)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    flat_dir, ivf_dir = tmp_path / "flat", tmp_path / "ivf"
    flat_dir.mkdir()
    ivf_dir.mkdir()
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    hi.clear_caches()
    _index_doc(flat_dir, "doc", x)
    assert open(flat_dir / "doc_hip.index", "rb").read(8) == b"HIPIDX01"          # unset: the flat file of today
    monkeypatch.setenv("HIP_INDEX_TYPE", "ivf")
    monkeypatch.setenv("HIP_IVF_NLIST", "12")
    monkeypatch.setenv("HIP_IVF_NPROBE", "12")
    summary = _index_doc(ivf_dir, "doc", x)
    assert summary["vectors_indexed"] == n
    assert open(ivf_dir / "doc_hip.index", "rb").read(8) == b"HIPIVF01"
    for limit in (1, 10, 50):
        for qv in q:
            hi.clear_caches()                                                   # the load path, not the cached index
            monkeypatch.setenv("STORAGE_DIR", str(flat_dir))
            want = asyncio.run(hi.search_hip_by_vector(qv.tolist(), limit=limit))
            monkeypatch.setenv("STORAGE_DIR", str(ivf_dir))
            got = asyncio.run(hi.search_hip_by_vector(qv.tolist(), limit=limit))
            assert len(want) == limit
            _same_rows(got, want)
    reader = hi.HipIndexReader(str(ivf_dir / "doc_hip.index"))
    assert reader.get_dimension() == d and reader.get_size() == n
    with pytest.raises(RuntimeError, match="IVF"):
        reader.search(q[0].tolist(), top_k=300)
    hi.clear_caches()


def test_mixed_directory_searches_all_documents(gpu, tmp_path, monkeypatch):
    import rag.storage.hip_index as hi
    monkeypatch.setattr(hi.config, "HIP_SEARCH_ALL_DOCUMENTS", True)
    d = 48
    xa, xb = ho.synthetic_vectors(300, d, seed=161), ho.synthetic_vectors(500, d, seed=162)
    mixed, flat = tmp_path / "mixed", tmp_path / "flat"
    mixed.mkdir()
    flat.mkdir()
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    hi.clear_caches()
    _index_doc(mixed, "docA", xa)
    _index_doc(flat, "docA", xa)
    _index_doc(flat, "docB", xb)
    monkeypatch.setenv("HIP_INDEX_TYPE", "ivf")
    monkeypatch.setenv("HIP_IVF_NPROBE", "1000")                                # >= nlist: every list probed
    _index_doc(mixed, "docB", xb)
    assert open(mixed / "docA_hip.index", "rb").read(8) == b"HIPIDX01"
    assert open(mixed / "docB_hip.index", "rb").read(8) == b"HIPIVF01"
    q = ho.synthetic_queries(4, d, seed=163)
    for qv in q:
        hi.clear_caches()
        monkeypatch.setenv("STORAGE_DIR", str(flat))
        want = asyncio.run(hi.search_hip_by_vector(qv.tolist(), limit=40))
        monkeypatch.setenv("STORAGE_DIR", str(mixed))
        got = asyncio.run(hi.search_hip_by_vector(qv.tolist(), limit=40))
        assert len(want) == 40 and {r["doc_id"] for r in want} == {"docA", "docB"}
        _same_rows(got, want)
    hi.clear_caches()
