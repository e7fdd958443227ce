"""
The two opt-in settings of the collection's IVF companion on the GPU (rag/storage/hip_index/collection.py), under
HIP_COLLECTION=true HIP_INDEX_TYPE=ivf: HIP_IVF_PROBE=scope makes a project-scoped search probe the best lists among those
that hold a row of the project (HipIVFIndex.search_scoped(..., probe="scope")), HIP_IVF_HYBRID=true puts the companion under
search_collection_hybrid (hiprag.hybrid_search_ivf_scoped_device).  With neither, both answer as before.  Documents are
clustered (a document's rows lie around a few centres), so a project touches fewer lists than the index has.
"""
import asyncio
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, NLIST, NPROBE, LIMIT = 64, 12, 2, 15
#        doc     project  rows  centres
DOCS = [("docA", "red", 230, (0, 1)), ("docB", "blue", 400, (2, 3, 4)), ("docC", "green", 200, (5,)), ("docD", "red", 333, (6, 1)),
        ("docE", "blue", 257, (7, 8)), ("docF", "green", 301, (9, 10, 11))]
WORDS = ["alpha", "beta", "gamma", "delta", "kappa", "sigma", "omega", "theta"]


def _rows(n, centres, seed):
    rng = np.random.default_rng(seed)
    c = np.random.default_rng(1).standard_normal((12, D))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[np.repeat(np.array(centres), (n + len(centres) - 1) // len(centres))[:n]] + (0.3 / np.sqrt(D)) * rng.standard_normal((n, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _chunk_table(storage, doc, n):
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": f"{WORDS[i % 8]} {WORDS[(i // 8) % 8]} of {doc}", "page": 1 + i // 7,
               "metadata": {"title": doc}} for i in range(n)]
    with open(storage / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": n, "chunks": chunks}, f)


def test_probe_and_hybrid_settings_route_to_the_companion(gpu, tmp_path, monkeypatch):
    import torch
    import rag.storage.hip_index as hi
    from hiprag import hybrid_search_ivf_scoped_device, hybrid_search_scoped_device
    from rag.storage.hip_index import collection as col
    from rag.storage.hip_index.sparse import get_collection_sparse
    storage = tmp_path
    monkeypatch.setenv("HIP_INDEX_METRIC", "ip")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "ip")
    monkeypatch.setenv("STORAGE_DIR", str(storage))
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_INDEX_TYPE", "ivf")
    monkeypatch.setenv("HIP_IVF_NPROBE", str(NPROBE))
    monkeypatch.delenv("HIP_IVF_PROBE", raising=False)
    monkeypatch.delenv("HIP_IVF_HYBRID", raising=False)
    hi.clear_caches()
    try:
        for j, (doc, project, n, centres) in enumerate(DOCS):
            _chunk_table(storage, doc, n)
            col.append_document(doc, project, _rows(n, centres, 800 + j), storage_dir=storage)
        coll = col.train_collection_ivf(storage, nlist=NLIST)
        scope = coll.manifest.scope_for("blue")
        offs, orig = coll.ivf.lists()
        members = sum(1 for l in range(NLIST) if any(((orig[offs[l]:offs[l + 1]] >= lo) & (orig[offs[l]:offs[l + 1]] < hi)).any() for lo, hi in scope))
        assert NPROBE < members < NLIST, f"project blue touches {members} of {NLIST} lists"
        queries = [_rows(400, (2, 3, 4), 801)[7], _rows(333, (6, 1), 803)[100], _rows(200, (5,), 802)[3]]

        def expect_vector(q, probe):
            values, ids = coll.ivf.search_scoped(np.array([q], dtype=np.float32), LIMIT, [scope], nprobe=NPROBE, probe=probe)
            return col._enrich(coll, col._transform(coll, values[0], ids[0]))

        def hybrid_rows(out):
            f_scores, f_ids = out[0][0].tolist(), out[1][0].tolist()
            return [(int(i), float(s)) for i, s in zip(f_ids, f_scores) if i >= 0]

        def row_of(item):
            doc = next(d for d in coll.manifest.documents if d["doc_id"] == item["doc_id"])
            return doc["row0"] + int(item["chunk_id"].rsplit("_", 1)[1])

        bm25 = get_collection_sparse(coll)
        text = "gamma delta of docB"
        differs = 0
        for q in queries:
            qd = torch.tensor([q.tolist()], dtype=torch.float32, device="cuda")
            terms = [bm25.terms_of(text)]
            # neither setting: what the calls return today
            monkeypatch.delenv("HIP_IVF_PROBE", raising=False)
            monkeypatch.delenv("HIP_IVF_HYBRID", raising=False)
            base = asyncio.run(hi.search_hip_by_vector(q.tolist(), LIMIT, "blue"))
            assert base == expect_vector(q, "any")
            hyb = col.search_collection_hybrid(text, q.tolist(), LIMIT, project="blue", storage_dir=storage)
            flat = hybrid_rows(hybrid_search_scoped_device(coll.index, bm25, qd, terms, [scope], depth=LIMIT, k=LIMIT))
            assert [(row_of(i), i["rrf_score"]) for i in hyb] == flat
            # HIP_IVF_PROBE=scope: the scoped branches pass the mode
            monkeypatch.setenv("HIP_IVF_PROBE", "scope")
            got = asyncio.run(hi.search_hip_by_vector(q.tolist(), LIMIT, "blue"))
            assert got == expect_vector(q, "scope")
            differs += got != base
            batch = col.search_collection_batch(np.stack([q, q]), LIMIT, ["blue", None], storage_dir=storage)
            assert batch[0] == got
            assert col.search_collection_hybrid(text, q.tolist(), LIMIT, project="blue", storage_dir=storage) == hyb   # still the flat index
            # HIP_IVF_HYBRID=true as well: the new call on the companion, in the configured probe mode
            monkeypatch.setenv("HIP_IVF_HYBRID", "true")
            for probe in ("scope", "any"):
                monkeypatch.setenv("HIP_IVF_PROBE", probe)
                hyb_ivf = col.search_collection_hybrid(text, q.tolist(), LIMIT, project="blue", storage_dir=storage)
                want = hybrid_rows(hybrid_search_ivf_scoped_device(coll.ivf, bm25, qd, terms, [scope], depth=LIMIT, k=LIMIT, nprobe=NPROBE,
                                                                   probe=probe))
                assert [(row_of(i), i["rrf_score"]) for i in hyb_ivf] == want, probe
            # HIP_IVF_HYBRID without HIP_INDEX_TYPE=ivf: the flat index
            monkeypatch.setenv("HIP_INDEX_TYPE", "flat")
            assert col.search_collection_hybrid(text, q.tolist(), LIMIT, project="blue", storage_dir=storage) == hyb
            monkeypatch.setenv("HIP_INDEX_TYPE", "ivf")
        assert differs > 0, "probe=scope never changed an answer: the project is not selective at this nprobe"
        monkeypatch.setenv("HIP_IVF_PROBE", "project")
        with pytest.raises(ValueError, match="HIP_IVF_PROBE"):
            asyncio.run(hi.search_hip_by_vector(queries[0].tolist(), LIMIT, "blue"))
    finally:
        hi.clear_caches()
