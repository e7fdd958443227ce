"""
Scoped BM25 / scoped hybrid search, the parts that need no GPU: the C-ABI surface, the collection's postings (document id ==
collection row) and the scope checks that run on the host before any native call.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hipbm25_search_scoped_dev", "hipbm25_search_scoped", "hipbm25_scoped_info", "hiphybrid_search_scoped_dev",
         "hiphybrid_search_scoped")


def test_header_library_and_binding_carry_the_five_names():
    from hiprag import _native as nat
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "hiprag.h")).read(), flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, text), f"{name} is not declared in hiprag.h"
        assert hasattr(lib, name), f"{name} is not exported by libhiprag.so"
        assert name in nat.SIGNATURES
    # arguments of the binding = parameters of the declaration
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(nat.SIGNATURES[name]) == len(params.split(",")), name


DOCS = [("alpha", "red", ["the quick brown fox", "jumps over the lazy dog", "Fox and dog"]),
        ("beta", "blue", ["a dog is a dog", "", "brown brown brown bear", "quick quick"]),
        ("gamma", "red", ["the end", "of the fox"])]


def _write(tmp_path, docs=DOCS):
    from rag.storage.hip_index.collection import CollectionManifest
    manifest = CollectionManifest(8, "l2")
    for doc_id, project, texts in docs:
        chunks = [{"chunk_id": f"{doc_id}_{i}", "text": t, "page": 1} for i, t in enumerate(texts)]
        with open(tmp_path / f"{doc_id}_chunks.json", "w") as f:
            json.dump({"total": len(chunks), "chunks": chunks}, f)
        manifest.add_document(doc_id, project, len(texts))
    return manifest


def test_collection_postings_are_those_of_the_concatenated_texts(tmp_path):
    from rag.storage.hip_index.collection import collection_postings
    manifest = _write(tmp_path)
    got = collection_postings(manifest, tmp_path)
    texts = [t for _d, _p, ts in DOCS for t in ts]
    want = ho.build_postings_from_texts(texts)
    assert got.n_docs == want.n_docs == manifest.rows == 9 and got.n_terms == want.n_terms
    assert got.vocab == want.vocab
    assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.doc_ids, want.doc_ids)
    assert np.array_equal(got.impacts.view(np.uint32), want.impacts.view(np.uint32))
    # document id == collection row: "bear" occurs in beta's third chunk only, row 3 + 2
    t = got.vocab["bear"]
    assert got.doc_ids[int(got.offsets[t]):int(got.offsets[t + 1])].tolist() == [manifest.scope_for(doc_ids=["beta"])[0][0] + 2]
    assert manifest.locate(5) == ("beta", 2)
    # the impacts are the collection's: those of beta's rows differ from a build over beta alone
    alone = ho.build_postings_from_texts(DOCS[1][2])
    ta = alone.vocab["bear"]
    assert alone.impacts[int(alone.offsets[ta])] != got.impacts[int(got.offsets[t])]


def test_collection_postings_refuse_a_chunk_table_of_the_wrong_length(tmp_path):
    from rag.storage.hip_index.collection import CollectionManifest, collection_postings
    _write(tmp_path)
    manifest = CollectionManifest(8, "l2")
    manifest.add_document("alpha", "red", 3)
    manifest.add_document("beta", "blue", 5)        # its table holds 4 chunks
    with pytest.raises(ValueError, match="beta.*4 rows.*names 5"):
        collection_postings(manifest, tmp_path)
    manifest = CollectionManifest(8, "l2")
    manifest.add_document("nobody", None, 1)
    with pytest.raises(FileNotFoundError):
        collection_postings(manifest, tmp_path)


class _NoNative:
    """stands for a handle: any native call through it would need a real one"""
    _h = 0
    d = 4
    device = 0

    @staticmethod
    def _flatten(queries):
        from hiprag import HipBM25
        return HipBM25._flatten(queries)


def test_malformed_scopes_are_rejected_before_any_native_call(monkeypatch):
    import hiprag
    from hiprag import HipBM25, _native as nat

    def no_call(name, *args):
        raise AssertionError(f"{name} was called")

    monkeypatch.setattr(nat, "call", no_call)
    bm = HipBM25.__new__(HipBM25)
    bm._h, bm.device = None, 0
    queries = [[1, 2], [3], [4]]
    with pytest.raises(ValueError, match="one scope or one per query"):
        bm.search_scoped(queries, 5, [[(0, 4)], [(4, 8)]])                    # 2 scopes, 3 queries, no scope_of_query
    with pytest.raises(ValueError, match="2 entries for 3 queries"):
        bm.search_scoped(queries, 5, [[(0, 4)]], [0, 0])
    with pytest.raises(ValueError):
        bm.search_scoped(queries, 5, [[(0, 4, 9)]])                           # a range is a pair
    q = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="one scope or one per query"):
        hiprag.hybrid_search_scoped(_NoNative(), _NoNative(), q, queries, [[(0, 4)], [(4, 8)]])
    with pytest.raises(ValueError, match="2 entries for 3 queries"):
        hiprag.hybrid_search_scoped(_NoNative(), _NoNative(), q, queries, [[(0, 4)]], [0, 0])
    with pytest.raises(ValueError, match="one term list per query"):
        hiprag.hybrid_search_scoped(_NoNative(), _NoNative(), q, queries[:2], [[(0, 4)]])


def test_hybrid_limit_beyond_the_scoped_depth_is_refused(tmp_path):
    from rag.storage.hip_index.collection import search_collection_hybrid
    with pytest.raises(RuntimeError, match="64"):
        search_collection_hybrid("fox", [0.0] * 8, limit=65, storage_dir=tmp_path)
