"""
The collection index's bookkeeping (rag/storage/hip_index/collection.py) and the pieces of the scoped search that need no
GPU: the manifest's round trip and atomic write, scopes of projects (adjacent documents coalesced, gaps kept), row ->
(document, local row), the file names the per-document readers must not pick up, the HIP_COLLECTION switch, and the
binding of hipidx_search_scoped (a bogus handle is refused before anything touches a device).
"""
import ctypes
import json
import os

import numpy as np
import pytest


def _manifest():
    from rag.storage.hip_index.collection import CollectionManifest
    m = CollectionManifest(64, "l2")
    for doc_id, project, rows in [("a", "p1", 10), ("b", "p1", 7), ("c", "p2", 5), ("d", "p1", 3), ("e", None, 0), ("f", "p2", 4),
                                  ("g", "p2", 1)]:
        m.add_document(doc_id, project, rows)
    return m


def test_manifest_round_trip_and_atomic_write(tmp_path):
    from rag.storage.hip_index.collection import COLLECTION_MANIFEST, CollectionManifest
    m = _manifest()
    path = tmp_path / COLLECTION_MANIFEST
    path.write_text("not json: a reader must never see a half-written file")
    m.save(path)
    assert os.listdir(tmp_path) == [COLLECTION_MANIFEST]                 # the temp file was renamed over the target
    data = json.loads(path.read_text())
    assert data["version"] == 1 and data["d"] == 64 and data["metric"] == "l2"
    assert [sorted(d) for d in data["documents"]] == [["doc_id", "project", "row0", "rows"]] * 7
    assert [d["row0"] for d in data["documents"]] == [0, 10, 17, 22, 25, 25, 29]
    back = CollectionManifest.load(path)
    assert back.to_json() == m.to_json() and back.rows == 30
    data["documents"][2]["row0"] = 18                                  # rows must follow one another
    path.write_text(json.dumps(data))
    with pytest.raises(ValueError, match="starts at row"):
        CollectionManifest.load(path)
    data["version"] = 2
    path.write_text(json.dumps(data))
    with pytest.raises(ValueError, match="version"):
        CollectionManifest.load(path)


def test_scope_for_coalesces_adjacent_documents_and_keeps_gaps():
    m = _manifest()
    assert m.scope_for("p1") == [(0, 17), (22, 25)]                      # a + b adjacent, c between them and d
    assert m.scope_for("p2") == [(17, 22), (25, 30)]                     # f + g adjacent; the empty e does not split anything
    assert m.scope_for() == [(0, 30)]
    assert m.scope_for("nobody") == []
    assert m.scope_for(doc_ids=["b", "c", "g"]) == [(10, 22), (29, 30)]
    assert m.scope_for("p1", doc_ids=["b", "c", "g"]) == [(10, 17)]
    assert m.scope_for(doc_ids=["e"]) == []
    assert m.projects() == ["p1", "p2", None]


def test_locate_at_every_boundary():
    m = _manifest()
    want = {0: ("a", 0), 9: ("a", 9), 10: ("b", 0), 16: ("b", 6), 17: ("c", 0), 21: ("c", 4), 22: ("d", 0), 24: ("d", 2),
            25: ("f", 0), 28: ("f", 3), 29: ("g", 0)}
    for row, where in want.items():
        assert m.locate(row) == where, row
    for row in range(m.rows):                                           # every row lands inside its document's range
        doc_id, local = m.locate(row)
        doc = m.documents[m._by_id[doc_id]]
        assert 0 <= local < doc["rows"] and doc["row0"] + local == row
    for row in (-1, 30):
        with pytest.raises(IndexError):
            m.locate(row)


def test_duplicate_doc_id_raises():
    m = _manifest()
    with pytest.raises(ValueError, match="already in the collection"):
        m.add_document("c", "p9", 4)
    assert m.rows == 30 and len(m.documents) == 7


def test_collection_files_are_invisible_to_the_per_document_globs(tmp_path):
    from rag.storage.hip_index import FAISS_SUFFIX, INDEX_SUFFIX
    from rag.storage.hip_index.collection import COLLECTION_INDEX, COLLECTION_MANIFEST
    for name in (COLLECTION_INDEX, COLLECTION_MANIFEST, "doc" + INDEX_SUFFIX):
        (tmp_path / name).write_bytes(b"")
    assert [f.name for f in tmp_path.glob(f"*{INDEX_SUFFIX}")] == ["doc" + INDEX_SUFFIX]
    assert list(tmp_path.glob(f"*{FAISS_SUFFIX}")) == []
    assert not COLLECTION_MANIFEST.endswith("_chunks.json")


def test_hip_collection_switch(monkeypatch):
    from rag.config import Config, config
    monkeypatch.delenv("HIP_COLLECTION", raising=False)
    assert Config().HIP_COLLECTION is False and config.HIP_COLLECTION is False
    for text, want in [("true", True), (" TRUE ", True), ("false", False), ("1", False), ("", False)]:
        monkeypatch.setenv("HIP_COLLECTION", text)
        assert config.HIP_COLLECTION is want, text                      # read at use, not at import


def test_read_flat_rows(tmp_path):
    import struct
    from rag.storage.hip_index.collection import read_flat_rows
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    path = tmp_path / "doc_hip.index"
    path.write_bytes(b"HIPIDX01" + struct.pack("<iiq", 4, 1, 3) + x.tobytes())
    rows, metric = read_flat_rows(path)
    assert metric == 1 and np.array_equal(rows, x)
    path.write_bytes(b"HIPIVF01" + bytes(40))
    with pytest.raises(ValueError, match="HIPIDX01"):
        read_flat_rows(path)


def test_scoped_search_on_a_bogus_handle_is_refused_without_a_gpu():
    from hiprag import HipRagError
    from hiprag import _native as nat
    ranges = np.array([[0, 1]], dtype=np.int64)
    offsets = np.array([0, 1], dtype=np.int32)
    soq = np.zeros(1, dtype=np.int32)
    q = np.zeros((1, 8), dtype=np.float32)
    s64, s32, ids = np.zeros((1, 1)), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int64)
    with pytest.raises(HipRagError) as e:
        nat.call("hipidx_search_scoped", ctypes.c_uint64(0xDEAD), q.ctypes.data, 1, 1, ranges.ctypes.data, offsets.ctypes.data, 1,
                 soq.ctypes.data, s64.ctypes.data, s32.ctypes.data, ids.ctypes.data)
    assert e.value.code == -3                                           # HIPRAG_E_HANDLE
    v = np.zeros(4, dtype=np.int64)
    with pytest.raises(HipRagError) as e:
        nat.call("hipidx_scoped_info", ctypes.c_uint64(0xDEAD), v.ctypes.data)
    assert e.value.code == -3


def test_pack_scopes():
    from hiprag import pack_scopes
    ranges, offsets, soq = pack_scopes([[(0, 5), (9, 12)], [], [(3, 4)]], None, 3)
    assert ranges.dtype == np.int64 and ranges.tolist() == [[0, 5], [9, 12], [3, 4]]
    assert offsets.dtype == np.int32 and offsets.tolist() == [0, 2, 2, 3]
    assert soq.dtype == np.int32 and soq.tolist() == [0, 1, 2]
    assert pack_scopes([[(0, 5)]], None, 4)[2].tolist() == [0, 0, 0, 0]
    assert pack_scopes([[(0, 5)], [(1, 2)]], [1, 1, 0], 3)[2].tolist() == [1, 1, 0]
    with pytest.raises(ValueError):
        pack_scopes([[(0, 5)], [(1, 2)]], None, 3)
    with pytest.raises(ValueError):
        pack_scopes([[(0, 5)]], [0, 0], 3)
