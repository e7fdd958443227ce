"""
Updatable lexical postings, the parts that need no GPU: the HIP_COLLECTION_SPARSE setting and its refusals, the .npz layout
LexicalIndex and LexicalIndexUpdatable share, and the numpy model of a sequence of appends and removals over document-major
rows that the GPU tests compare the device against (transpose_doc_weights of the surviving rows).
"""
import numpy as np
import pytest

from hiprag.lexical import LexicalIndex, LexicalIndexUpdatable, npz_doc_count, transpose_doc_weights
from hiprag.sparse import PostingsCSR

SETTINGS = ("HIP_COLLECTION", "HIP_COLLECTION_SPARSE", "HIP_SPARSE_MODE", "HIP_LATE_INTERACTION", "HIP_IVF_HYBRID", "HIP_RERANK")


@pytest.fixture
def cfg(monkeypatch):
    from rag.config import Config
    for name in SETTINGS:
        monkeypatch.delenv(name, raising=False)
    return Config()


# ---- the setting ---------------------------------------------------------------------------------------------------------
def test_collection_sparse_defaults_to_bm25_and_is_read_at_use(cfg, monkeypatch):
    assert cfg.HIP_COLLECTION_SPARSE == "bm25"
    monkeypatch.setenv("HIP_COLLECTION_SPARSE", "BM25 ")
    assert cfg.HIP_COLLECTION_SPARSE == "bm25"                   # and bm25 needs no collection
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_COLLECTION_SPARSE", " Lexical")
    assert cfg.HIP_COLLECTION_SPARSE == "lexical"
    assert cfg.HIP_SPARSE_MODE == "bm25"                         # the per-document setting is another one


def test_collection_sparse_refuses_its_four_cases(cfg, monkeypatch):
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_COLLECTION_SPARSE", "splade")
    with pytest.raises(ValueError, match="HIP_COLLECTION_SPARSE='splade'"):
        cfg.HIP_COLLECTION_SPARSE
    monkeypatch.setenv("HIP_COLLECTION_SPARSE", "lexical")
    monkeypatch.delenv("HIP_COLLECTION")
    with pytest.raises(ValueError, match="needs HIP_COLLECTION=true"):
        cfg.HIP_COLLECTION_SPARSE
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_LATE_INTERACTION", "true")
    with pytest.raises(ValueError, match="HIP_LATE_INTERACTION"):
        cfg.HIP_COLLECTION_SPARSE
    monkeypatch.delenv("HIP_LATE_INTERACTION")
    monkeypatch.setenv("HIP_IVF_HYBRID", "true")
    with pytest.raises(ValueError, match="HIP_IVF_HYBRID"):
        cfg.HIP_COLLECTION_SPARSE
    monkeypatch.delenv("HIP_IVF_HYBRID")
    assert cfg.HIP_COLLECTION_SPARSE == "lexical"


def test_sparse_mode_still_refuses_the_collection_and_names_the_new_setting(cfg, monkeypatch):
    monkeypatch.setenv("HIP_SPARSE_MODE", "lexical")
    assert cfg.HIP_SPARSE_MODE == "lexical"
    monkeypatch.setenv("HIP_COLLECTION", "true")
    with pytest.raises(ValueError, match="not supported yet") as e:
        cfg.HIP_SPARSE_MODE
    assert "HIP_COLLECTION_SPARSE" in str(e.value)
    monkeypatch.setenv("HIP_COLLECTION_SPARSE", "lexical")      # the new setting does not lift the old refusal
    with pytest.raises(ValueError, match="not supported yet"):
        cfg.HIP_SPARSE_MODE


# ---- the file ------------------------------------------------------------------------------------------------------------
def _tiny():
    terms = np.array([[2, 5, -1], [0, 2, 6], [-1, -1, -1], [5, -1, -1]], np.int32)
    weights = np.array([[0.5, 1.5, 0], [0.25, 2.0, 0.125], [0, 0, 0], [3.0, 0, 0]], np.float32)
    return terms, weights, np.array([2, 3, 0, 1], np.int32)


def test_npz_layout_is_shared_by_both_classes(tmp_path):
    """at the file level: what either class writes, the other reads into the same postings (no handle is made: the
    constructors, which need a GPU, are replaced by one that keeps the postings)"""
    p = transpose_doc_weights(*_tiny(), 8)
    plain, upd = object.__new__(LexicalIndex), object.__new__(LexicalIndexUpdatable)
    plain.p = p
    upd.export = lambda: {"n_docs": p.n_docs, "n_terms": p.n_terms, "offsets": p.offsets, "doc_ids": p.doc_ids, "impacts": p.impacts}
    plain.save(str(tmp_path / "plain.npz"))
    upd.save(str(tmp_path / "upd.npz"))

    def keep(self, postings, device=0, id_base=0):
        self.p = postings
    readers = [type("R", (cls,), {"__init__": keep}) for cls in (LexicalIndex, LexicalIndexUpdatable)]
    for name in ("plain.npz", "upd.npz"):
        with np.load(tmp_path / name) as z:
            assert sorted(z.files) == ["doc_ids", "impacts", "n_docs", "offsets"]
            assert z["offsets"].dtype == np.uint64 and z["doc_ids"].dtype == np.uint32 and z["impacts"].dtype == np.float32
        assert npz_doc_count(str(tmp_path / name)) == 4
        for reader in readers:
            got = reader.load(str(tmp_path / name)).p
            assert (got.n_docs, got.n_terms) == (4, 8)
            assert np.array_equal(got.offsets, p.offsets) and np.array_equal(got.doc_ids, p.doc_ids)
            assert np.array_equal(got.impacts.view(np.uint32), p.impacts.view(np.uint32))
    assert (tmp_path / "plain.npz").read_bytes() == (tmp_path / "upd.npz").read_bytes()


# ---- the model of a sequence of updates ------------------------------------------------------------------------------------
class RowsModel:
    """document-major rows under appends and removals: what survives, in order"""

    def __init__(self, stride: int):
        self.terms = np.zeros((0, stride), np.int32)
        self.weights = np.zeros((0, stride), np.float32)
        self.counts = np.zeros(0, np.int32)

    def append(self, terms, weights, counts):
        terms, weights = np.asarray(terms, np.int32), np.asarray(weights, np.float32)
        pad = self.terms.shape[1] - terms.shape[1]
        assert pad >= 0
        self.terms = np.concatenate([self.terms, np.pad(terms, ((0, 0), (0, pad)), constant_values=-1)])
        self.weights = np.concatenate([self.weights, np.pad(weights, ((0, 0), (0, pad)))])
        self.counts = np.concatenate([self.counts, np.asarray(counts, np.int32)])
        return self

    def remove_ranges(self, ranges):
        keep = np.ones(self.counts.size, bool)
        for lo, hi in ranges:
            assert 0 <= lo <= hi <= self.counts.size
            keep[lo:hi] = False
        self.terms, self.weights, self.counts = self.terms[keep], self.weights[keep], self.counts[keep]
        return self

    def postings(self, n_terms: int) -> PostingsCSR:
        return transpose_doc_weights(self.terms, self.weights, self.counts, n_terms)


def _csr(p):
    off = p.offsets.astype(np.int64)
    return {t: list(zip(p.doc_ids[off[t]:off[t + 1]].tolist(), p.impacts[off[t]:off[t + 1]].tolist()))
            for t in range(p.n_terms) if off[t + 1] > off[t]}


def test_rows_model_against_hand_written_postings():
    m = RowsModel(3).append(*_tiny())
    p = m.postings(8)
    assert p.n_docs == 4 and p.offsets.tolist() == [0, 1, 1, 3, 3, 3, 5, 6, 6]
    assert _csr(p) == {0: [(1, 0.25)], 2: [(0, 0.5), (1, 2.0)], 5: [(0, 1.5), (3, 3.0)], 6: [(1, 0.125)]}
    # an append of narrower rows: new documents 4 and 5, a term behind the old vocabulary; junk behind a count is ignored
    m.append([[7, 9], [2, 99]], [[1.0, 4.0], [0.75, np.nan]], [2, 1])
    assert _csr(m.postings(10)) == {0: [(1, 0.25)], 2: [(0, 0.5), (1, 2.0), (5, 0.75)], 5: [(0, 1.5), (3, 3.0)], 6: [(1, 0.125)],
                                    7: [(4, 1.0)], 9: [(4, 4.0)]}
    # a removal renumbers the survivors in order: documents 1 and 2 leave (touching ranges), an empty range changes nothing
    m.remove_ranges([(1, 2), (2, 3), (6, 6)])
    p = m.postings(10)
    assert p.n_docs == 4 and _csr(p) == {2: [(0, 0.5), (3, 0.75)], 5: [(0, 1.5), (1, 3.0)], 7: [(2, 1.0)], 9: [(2, 4.0)]}
    assert p.offsets.tolist() == [0, 0, 0, 2, 2, 2, 4, 4, 5, 5, 6]                  # emptied terms keep their ids
    # append behind a removal, then everything leaves, then an append to the empty rows
    m.append([[0]], [[8.0]], [1])
    assert _csr(m.postings(10))[0] == [(4, 8.0)]
    m.remove_ranges([(0, 5)])
    p = m.postings(10)
    assert p.n_docs == 0 and p.doc_ids.size == 0 and p.offsets.tolist() == [0] * 11
    m.append([[3, 4, 5]], [[1.0, 2.0, 3.0]], [3]).append(np.zeros((0, 3)), np.zeros((0, 3)), [])
    assert _csr(m.postings(10)) == {3: [(0, 1.0)], 4: [(0, 2.0)], 5: [(0, 3.0)]}
    with pytest.raises(ValueError):
        m.postings(5)                                                               # a term id at n_terms
