"""
CollectionManifest.remove_documents and the manifest's generation counter: pure bookkeeping, no GPU.  Removing documents
re-bases everything behind them, scopes coalesce across a removed neighbour, an unknown id changes nothing, and a manifest
that never saw a removal is written exactly as before.
"""
import copy
import json

import pytest

DOCS = [("docA", "red", 130), ("docB", "blue", 70), ("docC", "red", 33), ("docD", "green", 0), ("docE", "blue", 5),
        ("docF", "blue", 64), ("docG", "red", 9)]


def _manifest():
    from rag.storage.hip_index.collection import CollectionManifest      # inside: collecting this file loads no library
    m = CollectionManifest(64, "l2")
    for doc, project, n in DOCS:
        m.add_document(doc, project, n)
    return m


def _state(m):
    return copy.deepcopy((m.to_json(), m._row0, m._by_id, m.generation, m.rows))


def test_remove_rebases_what_lies_behind():
    m = _manifest()
    assert m.scope_for("red") == [(0, 130), (200, 233), (302, 311)]
    assert m.remove_documents(["docB"]) == [(130, 200)]
    assert [(d["doc_id"], d["row0"], d["rows"]) for d in m.documents] == [
        ("docA", 0, 130), ("docC", 130, 33), ("docD", 163, 0), ("docE", 163, 5), ("docF", 168, 64), ("docG", 232, 9)]
    assert m.rows == 241 and "docB" not in m and "docC" in m
    assert m.scope_for("red") == [(0, 163), (232, 241)]            # A and C now touch: one range
    assert m.scope_for("blue") == [(163, 232)]
    assert m.locate(129) == ("docA", 129) and m.locate(130) == ("docC", 0) and m.locate(163) == ("docE", 0)
    assert m.locate(240) == ("docG", 8)
    with pytest.raises(IndexError):
        m.locate(241)
    assert m.projects() == ["red", "green", "blue"]
    # the rebuilt lookup tables serve a later append and a later removal
    assert m.add_document("docB", "blue", 7) == (241, 248)
    assert m.locate(247) == ("docB", 6)
    with pytest.raises(ValueError, match="already in the collection"):
        m.add_document("docB", "blue", 1)


def test_remove_several_coalesces_and_skips_empty_documents():
    m = _manifest()
    # E and F are adjacent (D, empty, lies between C and E and adds no range); A stands alone; order of the ids is free
    assert m.remove_documents(["docF", "docA", "docE", "docD"]) == [(0, 130), (233, 302)]
    assert [(d["doc_id"], d["row0"]) for d in m.documents] == [("docB", 0), ("docC", 70), ("docG", 103)]
    assert m.rows == 112 and m.generation == 1
    assert m.projects() == ["blue", "red"]
    assert m.scope_for() == [(0, 112)]
    assert m.remove_documents(["docB", "docC", "docG"]) == [(0, 112)]
    assert m.rows == 0 and m.documents == [] and m.scope_for() == [] and m.projects() == []
    assert m.add_document("docZ", None, 3) == (0, 3)


def test_removing_an_empty_document_yields_no_range():
    m = _manifest()
    assert m.remove_documents(["docD"]) == []
    assert "docD" not in m and m.rows == 311 and m.generation == 1


def test_unknown_id_raises_and_changes_nothing():
    m = _manifest()
    before = _state(m)
    with pytest.raises(KeyError):
        m.remove_documents(["docB", "nobody"])
    assert _state(m) == before
    with pytest.raises(KeyError):
        m.remove_documents(["nobody"])
    assert _state(m) == before
    assert m.remove_documents([]) == [] and _state(m) == before


def test_generation_is_absent_until_the_first_removal_and_round_trips(tmp_path):
    from rag.storage.hip_index.collection import CollectionManifest
    m = _manifest()
    path = tmp_path / "hip_collection.json"
    m.save(path)
    # exactly what the code before this change wrote: no new key
    assert path.read_text() == json.dumps({"version": 1, "d": 64, "metric": "l2", "documents": [
        {"doc_id": doc, "project": p, "row0": sum(n for _d, _p, n in DOCS[:i]), "rows": n} for i, (doc, p, n) in enumerate(DOCS)]})
    assert "generation" not in m.to_json() and m.generation == 0
    assert CollectionManifest.load(path).generation == 0
    m.remove_documents(["docC"])
    assert m.to_json()["generation"] == 1
    m.remove_documents(["docA"])
    m.save(path)
    back = CollectionManifest.load(path)
    assert back.generation == 2 and back.to_json() == m.to_json() and back.rows == m.rows
    assert json.loads(path.read_text())["version"] == 1
