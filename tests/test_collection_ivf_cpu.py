"""
The IVF companion of the collection (rag/storage/hip_index/collection.py), as far as it needs no GPU: the manifest key, the
updates forwarded to both indexes, the errors that name train_collection_ivf, rebuild_collection dropping a stale
companion, and which index answers under HIP_INDEX_TYPE x companion present x project given.  The indexes are fakes that
record their calls and read and write files of their own.
"""
import json
import struct

import numpy as np
import pytest


class FakeFlat:
    """what Collection asks of HipFlatIndex; save / load use the HIPIDX01 layout read_flat_rows reads"""
    metric = 1

    def __init__(self, d, metric="l2", device=0):
        self.d, self.rows, self.calls = int(d), np.zeros((0, int(d)), np.float32), []

    @property
    def ntotal(self):
        return len(self.rows)

    def add(self, x):
        self.calls.append(("add", len(x)))
        self.rows = np.concatenate([self.rows, np.asarray(x, np.float32)])

    def remove_ranges(self, ranges):
        self.calls.append(("remove_ranges", [tuple(r) for r in ranges]))
        keep = np.ones(len(self.rows), bool)
        for lo, hi in ranges:
            keep[lo:hi] = False
        self.rows = self.rows[keep]
        return int((~keep).sum())

    def save(self, path):
        with open(path, "wb") as f:
            f.write(b"HIPIDX01" + struct.pack("<iiq", self.d, 1, len(self.rows)) + self.rows.tobytes())

    @classmethod
    def load(cls, path, device=0):
        from rag.storage.hip_index.collection import read_flat_rows
        rows, _ = read_flat_rows(path)
        ix = cls(rows.shape[1])
        ix.rows = rows
        return ix

    def _answer(self, name, q, k, *rest):
        self.calls.append((name, len(q), k) + rest)
        return np.full((len(q), k), 0.5, np.float32), np.tile(np.arange(k, dtype=np.int64), (len(q), 1))

    def search(self, q, k):
        return self._answer("search", q, k)

    def search_scoped(self, q, k, scopes, soq=None):
        return self._answer("search_scoped", q, k, [list(s) for s in scopes], None if soq is None else list(soq))


class FakeIVF(FakeFlat):
    """what Collection asks of HipIVFIndex; the file is the magic and a line of JSON"""

    def __init__(self, d, nlist=8, metric="l2", device=0, nprobe=None):
        super().__init__(d)
        self.nlist = nlist

    def build(self, x, iters=0, seed=0, max_train_rows=0):
        self.calls.append(("build", len(x), iters, max_train_rows))
        self.rows = np.asarray(x, np.float32)

    def save(self, path):
        with open(path, "wb") as f:
            f.write(b"HIPIVF01" + json.dumps({"d": self.d, "nlist": self.nlist, "n": len(self.rows)}).encode())

    @classmethod
    def load(cls, path, device=0, nprobe=None):
        data = json.loads(open(path, "rb").read()[8:])
        ix = cls(data["d"], data["nlist"])
        ix.rows = np.zeros((data["n"], data["d"]), np.float32)
        return ix

    def search(self, q, k, nprobe=None):
        return self._answer("search", q, k, nprobe)

    def search_batch(self, q, k, nprobe=None):
        return self._answer("search_batch", q, k, nprobe)

    def search_scoped(self, q, k, scopes, soq=None, nprobe=None):
        return self._answer("search_scoped", q, k, [list(s) for s in scopes], None if soq is None else list(soq), nprobe)


D = 4


def rows_of(n, seed):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)


@pytest.fixture
def fakes(monkeypatch):
    import rag.storage.hip_index as hi
    from rag.storage.hip_index import collection
    monkeypatch.setattr(hi, "HAS_HIP", True)
    monkeypatch.setattr(hi, "HipFlatIndex", FakeFlat, raising=False)
    monkeypatch.setattr(hi, "HipIVFIndex", FakeIVF, raising=False)
    collection.clear_collection_cache()
    yield collection
    collection.clear_collection_cache()


def make_collection(collection, tmp_path, with_ivf):
    from rag.storage.hip_index.collection import Collection, CollectionManifest
    coll = Collection(tmp_path, CollectionManifest(D, "l2"), FakeFlat(D), FakeIVF(D, nlist=8) if with_ivf else None)
    for doc_id, project, n in [("a", "p1", 10), ("b", "p2", 7), ("c", "p1", 5), ("d", "p2", 3)]:
        coll.append(doc_id, project, rows_of(n, len(doc_id) + n))
    return coll


def test_manifest_key_only_once_a_companion_exists(tmp_path):
    from rag.storage.hip_index.collection import CollectionManifest
    m = CollectionManifest(64, "l2")
    m.add_document("a", "p1", 10)
    m.add_document("b", None, 7)
    today = ('{"version": 1, "d": 64, "metric": "l2", "documents": [{"doc_id": "a", "project": "p1", "row0": 0, "rows": 10}, '
             '{"doc_id": "b", "project": null, "row0": 10, "rows": 7}]}')
    m.save(tmp_path / "m.json")
    assert (tmp_path / "m.json").read_text() == today                    # untrained: byte for byte what it was
    assert CollectionManifest.load(tmp_path / "m.json").ivf is None
    m.ivf = {"nlist": 8}
    m.save(tmp_path / "m.json")
    assert (tmp_path / "m.json").read_text() == today[:-1] + ', "ivf": {"nlist": 8}}'
    back = CollectionManifest.load(tmp_path / "m.json")
    assert back.ivf == {"nlist": 8} and back.to_json() == m.to_json()
    m.remove_documents(["a"])                                            # generation first, then the companion
    assert list(m.to_json()) == ["version", "d", "metric", "documents", "generation", "ivf"]


def test_append_and_remove_reach_both_indexes_with_the_same_ranges(fakes, tmp_path):
    from rag.storage.hip_index.collection import COLLECTION_IVF, COLLECTION_INDEX, COLLECTION_MANIFEST
    coll = make_collection(fakes, tmp_path, with_ivf=True)
    assert coll.index.calls == coll.ivf.calls == [("add", 10), ("add", 7), ("add", 5), ("add", 3)]
    assert np.array_equal(coll.index.rows, coll.ivf.rows)
    assert coll.remove(["b", "c"]) == 12
    assert coll.index.calls[-1] == coll.ivf.calls[-1] == ("remove_ranges", [(10, 22)])      # adjacent documents coalesced
    assert coll.remove(["a", "d"]) == 13 and coll.index.calls[-1] == coll.ivf.calls[-1] == ("remove_ranges", [(0, 13)])
    coll.append("e", "p3", rows_of(4, 9))
    assert coll.index.ntotal == coll.ivf.ntotal == coll.manifest.rows == 4
    coll.save()
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted([COLLECTION_INDEX, COLLECTION_IVF, COLLECTION_MANIFEST])
    assert not COLLECTION_IVF.endswith("_hip.index")
    assert json.loads((tmp_path / COLLECTION_MANIFEST).read_text())["ivf"] == {"nlist": 8}
    plain = make_collection(fakes, tmp_path / "plain", with_ivf=False)       # no companion: nothing but the flat index
    (tmp_path / "plain").mkdir()
    plain.remove(["b"])
    plain.save()
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == sorted([COLLECTION_INDEX, COLLECTION_MANIFEST])
    assert "ivf" not in json.loads((tmp_path / "plain" / COLLECTION_MANIFEST).read_text())
    coll.ivf.rows = coll.ivf.rows[:-1]                                   # a companion out of step refuses updates
    with pytest.raises(RuntimeError, match="train_collection_ivf"):
        coll.append("f", "p3", rows_of(2, 1))
    with pytest.raises(RuntimeError, match="train_collection_ivf"):
        coll.remove(["e"])
    assert "f" not in coll.manifest and "e" in coll.manifest


def test_open_loads_the_companion_and_names_train_collection_ivf_when_it_cannot(fakes, tmp_path):
    from rag.storage.hip_index.collection import COLLECTION_IVF
    coll = make_collection(fakes, tmp_path, with_ivf=True)
    coll.save()
    fakes.clear_collection_cache()
    back = fakes.open_collection(tmp_path)
    assert isinstance(back.ivf, FakeIVF) and back.ivf.ntotal == back.index.ntotal == 25 and back.ivf.nlist == 8
    stale = FakeIVF(D, nlist=8)
    stale.rows = np.zeros((24, D), np.float32)
    stale.save(tmp_path / COLLECTION_IVF)
    fakes.clear_collection_cache()
    with pytest.raises(RuntimeError, match="train_collection_ivf") as e:
        fakes.open_collection(tmp_path)
    assert "24" in str(e.value) and "25" in str(e.value)
    (tmp_path / COLLECTION_IVF).unlink()
    with pytest.raises(RuntimeError, match="train_collection_ivf"):
        fakes.open_collection(tmp_path)
    trained = fakes.train_collection_ivf(tmp_path, nlist=5, iters=3)     # and train_collection_ivf repairs the pair
    assert trained.ivf.nlist == 5 and trained.ivf.calls == [("build", 25, 3, 256 * 5)]
    assert np.array_equal(trained.ivf.rows, coll.index.rows)
    fakes.clear_collection_cache()
    assert fakes.open_collection(tmp_path).manifest.ivf == {"nlist": 5}
    from rag.config import ivf_auto_nlist
    assert fakes.train_collection_ivf(tmp_path).ivf.nlist == min(ivf_auto_nlist(25), 25)


def test_rebuild_collection_drops_the_companion_and_the_key(fakes, tmp_path):
    from rag.storage.hip_index.collection import COLLECTION_IVF, COLLECTION_MANIFEST
    coll = make_collection(fakes, tmp_path, with_ivf=True)
    coll.save()
    for doc_id, n in (("a", 10), ("z", 6)):
        doc = FakeFlat(D)
        doc.add(rows_of(n, n))
        doc.save(tmp_path / f"{doc_id}_hip.index")
    rebuilt = fakes.rebuild_collection(tmp_path, {"a": "p1"})
    assert rebuilt.ivf is None and rebuilt.manifest.rows == 16
    assert "ivf" not in json.loads((tmp_path / COLLECTION_MANIFEST).read_text())
    assert not (tmp_path / COLLECTION_IVF).exists()
    fakes.clear_collection_cache()
    assert fakes.open_collection(tmp_path).ivf is None


@pytest.mark.parametrize("index_type", ["flat", "ivf"])
@pytest.mark.parametrize("with_ivf", [False, True])
def test_search_dispatch(fakes, tmp_path, monkeypatch, index_type, with_ivf):
    coll = make_collection(fakes, tmp_path, with_ivf)
    monkeypatch.setenv("HIP_INDEX_TYPE", index_type)
    monkeypatch.setenv("HIP_IVF_NPROBE", "3")
    monkeypatch.setattr(fakes, "open_collection", lambda storage_dir=None: coll)
    monkeypatch.setattr(fakes, "_enrich", lambda c, results: results)
    use_ivf = index_type == "ivf" and with_ivf
    answering, silent = (coll.ivf, coll.index) if use_ivf else (coll.index, coll.ivf)
    tail = (3,) if use_ivf else ()                                       # nprobe = max(1, min(HIP_IVF_NPROBE, nlist))
    q = [0.0] * D

    def last_call():
        for ix in (answering, silent):
            if ix is not None:
                ix.calls_before = len(ix.calls)

    def only_answering_was_called():
        return silent is None or len(silent.calls) == silent.calls_before

    last_call()
    assert len(fakes.search_collection(q, 6, None)) == 6
    assert answering.calls[-1] == ("search", 1, 6) + tail and only_answering_was_called()
    fakes.search_collection(q, 6, "p1")
    assert answering.calls[-1] == ("search_scoped", 1, 6, [[(0, 10), (17, 22)]], None) + tail and only_answering_was_called()
    assert fakes.search_collection(q, 6, "nobody") == []
    with pytest.raises(RuntimeError, match="256"):
        fakes.search_collection(q, 257, "p1")                            # the limit check is unchanged
    vec = np.zeros((3, D), np.float32)
    fakes.search_collection_batch(vec, 4, ["p2", None, "p2"])
    assert answering.calls[-1] == ("search_scoped", 3, 4, [[(10, 17), (22, 25)], [(0, 25)]], [0, 1, 0]) + tail
    fakes.search_collection_batch(vec, 4, [None, None, None])
    if use_ivf:
        assert answering.calls[-1] == ("search_batch", 3, 4, 3)
    else:
        assert answering.calls[-1] == ("search_scoped", 3, 4, [[(0, 25)]], [0, 0, 0])
    assert only_answering_was_called()
    if use_ivf:                                                          # nprobe is clamped to the companion's lists
        monkeypatch.setenv("HIP_IVF_NPROBE", "100")
        fakes.search_collection(q, 6, "p1")
        assert answering.calls[-1][-1] == 8
