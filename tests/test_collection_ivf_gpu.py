"""
The collection's IVF companion on the GPU (rag/storage/hip_index/collection.py): with HIP_INDEX_TYPE=ivf and a companion
trained by train_collection_ivf, search_collection and search_collection_batch answer through hipivf_search_scoped.  At
nprobe = nlist that is the flat scoped search bit for bit, so every answer must EQUAL the one HIP_INDEX_TYPE=flat gives --
after training, after a replacement and a deletion (the companion follows on the device), and after a reload from the files.
"""
import json

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

D = 128
#        doc     project  rows  seed
DOCS = [("docA", "red", 230, 800), ("docB", "blue", 400, 801), ("docC", "green", 200, 802), ("docD", "red", 333, 803),
        ("docE", "blue", 257, 804), ("docF", "green", 301, 805)]
PROJECTS = (None, "red", "blue", "green", "nobody")


def _chunk_table(storage, doc, n):
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": f"c{i} of {doc}", "page": 1 + i // 7, "metadata": {"title": doc}} for i in range(n)]
    with open(storage / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": n, "chunks": chunks}, f)


def _answers(col, storage, queries, monkeypatch, index_type):
    monkeypatch.setenv("HIP_INDEX_TYPE", index_type)
    return {(j, p): col.search_collection(q.tolist(), 20, project=p, storage_dir=storage) for j, q in enumerate(queries) for p in PROJECTS}


def _assert_ivf_equals_flat(col, storage, queries, monkeypatch, tag):
    flat = _answers(col, storage, queries, monkeypatch, "flat")
    ivf = _answers(col, storage, queries, monkeypatch, "ivf")
    for key in flat:
        assert ivf[key] == flat[key], f"{tag}: query {key[0]}, project {key[1]!r}"
    assert all(len(flat[(j, None)]) == 20 and flat[(j, "nobody")] == [] for j in range(len(queries)))
    return ivf


def test_the_companion_answers_like_the_flat_index_through_updates_and_a_reload(gpu, tmp_path, monkeypatch):
    import rag.storage.hip_index as hi
    from rag.storage.hip_index import collection as col
    storage = tmp_path
    monkeypatch.setenv("HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "l2")
    monkeypatch.setenv("STORAGE_DIR", str(storage))
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_IVF_NPROBE", "8")
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    hi.clear_caches()
    try:
        for doc, project, n, seed in DOCS:
            _chunk_table(storage, doc, n)
            col.append_document(doc, project, ho.synthetic_vectors(n, D, seed=seed), storage_dir=storage)
        before = (storage / col.COLLECTION_MANIFEST).read_text()
        assert "ivf" not in json.loads(before) and not (storage / col.COLLECTION_IVF).exists()
        rng = np.random.default_rng(9)
        queries = [ho.synthetic_vectors(333, D, seed=803)[5], ho.synthetic_vectors(400, D, seed=801)[399],
                   ho.synthetic_queries(1, D, seed=77)[0], rng.standard_normal(D).astype(np.float32)]
        # without a companion HIP_INDEX_TYPE=ivf changes nothing
        assert _answers(col, storage, queries[:1], monkeypatch, "ivf") == _answers(col, storage, queries[:1], monkeypatch, "flat")

        coll = col.train_collection_ivf(storage, nlist=8)
        total = sum(n for _, _, n, _ in DOCS)
        assert coll.ivf.nlist == 8 and coll.ivf.ntotal == coll.index.ntotal == total
        assert json.loads((storage / col.COLLECTION_MANIFEST).read_text())["ivf"] == {"nlist": 8}
        assert (storage / col.COLLECTION_IVF).read_bytes()[:8] == b"HIPIVF01"
        first = _assert_ivf_equals_flat(col, storage, queries, monkeypatch, "trained")
        assert {r["doc_id"] for r in first[(0, "red")]} <= {"docA", "docD"} and first[(0, "red")][0]["doc_id"] == "docD"

        # a replacement (another row count, at the end) and a deletion: the companion follows on the device
        _chunk_table(storage, "docB", 290)
        col.replace_document("docB", "blue", ho.synthetic_vectors(290, D, seed=811), storage_dir=storage)
        col.delete_document("docC", storage_dir=storage)
        coll = col.open_collection(storage)
        assert coll.ivf is not None and coll.ivf.ntotal == coll.index.ntotal == coll.manifest.rows == total - 400 + 290 - 200
        queries[1] = ho.synthetic_vectors(290, D, seed=811)[289]
        updated = _assert_ivf_equals_flat(col, storage, queries, monkeypatch, "after replace and delete")
        assert updated[(1, "blue")][0]["doc_id"] == "docB" and not any(r["doc_id"] == "docC" for r in updated[(2, None)])

        col.clear_collection_cache()                       # a reload from the files
        reloaded = _assert_ivf_equals_flat(col, storage, queries, monkeypatch, "reloaded")
        assert reloaded == updated and col.open_collection(storage) is not coll

        # the batch call over mixed projects: one hipivf_search_scoped call, the one-at-a-time answers
        monkeypatch.setenv("HIP_INDEX_TYPE", "ivf")
        projects = ["blue", None, "red", "nobody", "green", "blue", None]
        vecs = np.stack([queries[i % len(queries)] for i in range(len(projects))])
        batch = col.search_collection_batch(vecs, 20, projects, storage_dir=storage)
        assert batch == [reloaded[(i % len(queries), p)] for i, p in enumerate(projects)]
        none_only = col.search_collection_batch(vecs[:3], 20, [None] * 3, storage_dir=storage)
        assert none_only == [reloaded[(i, None)] for i in range(3)]
    finally:
        hi.clear_caches()
