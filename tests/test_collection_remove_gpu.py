"""
Deleting and replacing documents of the collection through the drop-in: delete_document, index_chunks(..., replace=True) with
another chunk count and with the same chunk count but other texts (the stale-postings case) leave the manifest, the index
file and every answer -- dense, batch and hybrid, per project and over everything -- equal to those of a collection built
from scratch from the final documents in their final order.
"""
import asyncio
import json
import os

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

D = 64
WORDS = [f"w{j}" for j in range(40)]
#        doc     project  chunks  vector seed  text seed  extra word
FIRST = [("docA", "red", 130, 600, 700, ""), ("docB", "blue", 70, 601, 701, ""), ("docC", "red", 33, 602, 702, ""),
         ("docD", "blue", 257, 603, 703, ""), ("docE", "blue", 5, 604, 704, "")]
NEW_D = ("docD", "blue", 91, 613, 713, " quagga")        # another chunk count
NEW_A = ("docA", "red", 130, 610, 710, " zebra")         # the same chunk count, other texts and vectors
FINAL = [FIRST[2], FIRST[4], NEW_D, NEW_A]               # B deleted; a replacement goes to the end


class _TableProvider:
    """Stands for the encoder at ingest: a chunk text "c<i> ..." embeds to row i of x."""

    def __init__(self, x):
        self.x = x

    async def embed_batch(self, texts, instruction=None):
        return [[float(v) for v in self.x[int(t.split()[0][1:])]] for t in texts]


def _texts(n, seed, extra):
    rng = np.random.default_rng(seed)
    return [f"c{i} " + " ".join(rng.choice(WORDS, size=5)) + extra for i in range(n)]


def _ingest(storage, spec, **kw):
    from rag.ingest.indexing import index_chunks
    doc, project, n, vseed, tseed, extra = spec
    x = ho.synthetic_vectors(n, D, seed=vseed)
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": 1 + i // 7, "metadata": {"title": doc}}
              for i, t in enumerate(_texts(n, tseed, extra))]
    with open(storage / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)
    return asyncio.run(index_chunks(doc, chunks, storage_dir=storage, provider=_TableProvider(x), with_sparse=True, project=project, **kw))


def _answers(col, storage, queries):
    """every search entry of the collection, for every query and scope"""
    out = {}
    for name, (text, vec) in queries.items():
        for project in (None, "red", "blue", "nobody"):
            out[("dense", name, project)] = col.search_collection(vec.tolist(), 20, project=project, storage_dir=storage)
            out[("hybrid", name, project)] = col.search_collection_hybrid(text, vec.tolist(), 20, project=project, storage_dir=storage)
    projects = ["blue", "red", None, "blue", "nobody", "red"]
    names = list(queries)
    vecs = np.stack([queries[names[i % len(names)]][1] for i in range(len(projects))])
    out["batch"] = col.search_collection_batch(vecs, 20, projects, storage_dir=storage)
    return out


def test_delete_and_replace_equal_a_collection_built_from_scratch(gpu, tmp_path, monkeypatch):
    import rag.storage.hip_index as hi
    from rag.storage.hip_index import collection as col
    live, scratch = tmp_path / "live", tmp_path / "scratch"
    live.mkdir()
    scratch.mkdir()
    monkeypatch.setenv("HIP_ALLOW_SYNTHETIC", "1")
    monkeypatch.setenv("HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "l2")
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    monkeypatch.setenv("STORAGE_DIR", str(live))
    monkeypatch.setenv("HIP_COLLECTION", "true")
    hi.clear_caches()

    total = 0
    for spec in FIRST:
        total += spec[2]
        assert _ingest(live, spec)["collection_rows"] == total
    rng = np.random.default_rng(3)
    queries = {
        "a row of C": ("w3 w17 w5", ho.synthetic_vectors(33, D, seed=602)[4]),
        "a row of the new A": ("zebra w1", ho.synthetic_vectors(130, D, seed=610)[7]),
        "a row of the old A": ("w9 w21", ho.synthetic_vectors(130, D, seed=600)[7]),
        "a row of the new D": ("quagga w30", ho.synthetic_vectors(91, D, seed=613)[90] + 0.05 * rng.standard_normal(D).astype(np.float32)),
        "a row of B": ("w2 w4", ho.synthetic_vectors(70, D, seed=601)[3]),
        "anything": ("w30", ho.synthetic_queries(1, D, seed=9)[0]),
    }
    before = _answers(col, live, queries)                     # fills the collection-postings cache
    assert any(r["doc_id"] == "docB" for r in before[("dense", "a row of B", "blue")])
    assert not any("zebra" in r["text"] for r in before[("hybrid", "a row of the new A", "red")])
    manifest_json = json.loads((live / col.COLLECTION_MANIFEST).read_text())
    assert "generation" not in manifest_json                 # nothing removed yet: the file is what it always was

    # without replace a present document is still refused
    with pytest.raises(ValueError, match="already in the collection"):
        _ingest(live, FIRST[1])
    assert col.open_collection(live).index.ntotal == total

    assert col.delete_document("docB", storage_dir=live) == 70
    assert not (live / "docB_hip.index").exists() and (live / "docB_chunks.json").exists()
    with pytest.raises(KeyError):
        col.delete_document("docB", storage_dir=live)
    assert _ingest(live, NEW_D, replace=True)["collection_rows"] == total - 70 - 257 + 91
    # the stale-postings case: postings cached for this manifest, then a replacement that keeps the document count and the
    # row count, and (forced here, a coarse clock does it by itself) the manifest's mtime -- only `generation` tells them apart
    mpath = live / col.COLLECTION_MANIFEST
    stamp = mpath.stat().st_mtime_ns
    mid = col.search_collection_hybrid("zebra w1", queries["a row of the new A"][1].tolist(), 20, project="red", storage_dir=live)
    assert mid and not any("zebra" in r["text"] for r in mid)
    assert _ingest(live, NEW_A, replace=True)["collection_rows"] == total - 70 - 257 + 91    # 130 out, 130 in
    os.utime(mpath, ns=(stamp, stamp))
    manifest_json = json.loads((live / col.COLLECTION_MANIFEST).read_text())
    assert manifest_json["generation"] == 3 and manifest_json["version"] == 1

    monkeypatch.setenv("STORAGE_DIR", str(scratch))
    for spec in FINAL:
        _ingest(scratch, spec)
    want_manifest = json.loads((scratch / col.COLLECTION_MANIFEST).read_text())
    assert "generation" not in want_manifest
    assert [(d["doc_id"], d["project"], d["rows"]) for d in want_manifest["documents"]] == [s[:3] for s in FINAL]
    assert {k: v for k, v in manifest_json.items() if k != "generation"} == want_manifest
    assert (live / col.COLLECTION_INDEX).read_bytes() == (scratch / col.COLLECTION_INDEX).read_bytes()
    assert sorted(p.name for p in live.glob("*_hip.index")) == sorted(p.name for p in scratch.glob("*_hip.index"))
    for p in scratch.glob("*_hip.index"):
        assert (live / p.name).read_bytes() == p.read_bytes()

    # every answer, field for field -- first from the live process state (caches as the removals left them) ...
    want = _answers(col, scratch, queries)
    got = _answers(col, live, queries)
    assert got.keys() == want.keys()
    for key in want:
        assert got[key] == want[key], key
    # ... the same-count replacement is the stale-postings case: the new texts are found, the old are gone
    assert any("zebra" in r["text"] and "bm25_score" in r for r in got[("hybrid", "a row of the new A", "red")])
    top = got[("dense", "a row of the new A", "red")][0]
    assert top["chunk_id"] == "docA_0007" and "zebra" in top["text"]
    assert not any(r["doc_id"] == "docB" for key, rows in got.items() if key != "batch" for r in rows)
    assert not any(r["doc_id"] == "docB" for rows in got["batch"] for r in rows)
    # ... then from the files alone
    hi.clear_caches()
    got = _answers(col, live, queries)
    for key in want:
        assert got[key] == want[key], ("reloaded", key)

    # the deleted document does not come back with a rebuild (sorted doc_id order: A, C, D, E)
    projects = {s[0]: s[1] for s in FINAL}
    rebuilt = col.rebuild_collection(live, projects=projects)
    assert [d["doc_id"] for d in rebuilt.manifest.documents] == ["docA", "docC", "docD", "docE"]
    assert rebuilt.index.ntotal == total - 70 - 257 + 91
    hi.clear_caches()
