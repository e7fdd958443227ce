"""
One removal table, the six structures that take one (csrc/range_table.h behind hipidx_, hipivf_, hipbm25_, hiptok_, hippage_
and hipmv_remove_ranges), 40 rows or documents each: a table with empty and touching ranges leaves a structure byte for
byte what its joined form leaves; every bad table is refused with HIPRAG_E_INVALID and the rule's message, the first with
the structure's own name and value of its count; and the refused calls leave the structure's bytes as they were.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 40
GOOD = [(0, 0), (2, 5), (5, 6), (9, 9), (12, 20), (39, 40)]
JOINED = [(2, 6), (12, 20), (39, 40)]
NULL_TABLE, NEGATIVE_COUNT = "null table with n_ranges = 2", "n_ranges = -1"
REFUSED = [([(3, 2)], "is not within"), ([(-1, 2)], "is not within"), ([(0, 41)], "is not within"),
           ([(4, 6), (5, 7)], "ascend and do not overlap"), ([(6, 8), (1, 2)], "ascend and do not overlap"),
           (NULL_TABLE, "ranges is null"), (NEGATIVE_COUNT, "must not be negative")]


def file_bytes(ix, path):
    ix.save(str(path))
    with open(path, "rb") as f:
        return f.read()


def arrays_bytes(arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def rows_1d():
    """40 rows at d = 1, ten around each of the centroids 0, 10, 20, 30 in turn"""
    rng = np.random.default_rng(3)
    return ((np.arange(N) % 4) * 10 + rng.uniform(-1, 1, N)).astype(np.float32).reshape(N, 1)


def make_dense(tmp_path):
    from hiprag import HipFlatIndex
    ix = HipFlatIndex(1, "l2")
    ix.add(rows_1d())
    return ix, "hipidx_remove_ranges", "ntotal", lambda: file_bytes(ix, tmp_path / "dense.idx")


def make_ivf(tmp_path):
    from hiprag import HipIVFIndex
    ix = HipIVFIndex.from_centroids(np.asarray([[0.0], [10.0], [20.0], [30.0]], np.float32), "l2")
    ix.add(rows_1d())
    return ix, "hipivf_remove_ranges", "n", lambda: file_bytes(ix, tmp_path / "lists.ivf")


def make_bm25(tmp_path):
    from hiprag.sparse import HipBM25Updatable, build_postings
    rng = np.random.default_rng(4)
    docs = np.repeat(np.arange(N), 1 + np.arange(N) % 5)
    ix = HipBM25Updatable(build_postings(docs, rng.integers(0, 13, docs.size), N, 13))

    def state():
        ix.commit()
        e = ix.export()
        return arrays_bytes([np.asarray([e["n_docs"], e["n_terms"]]), e["offsets"], e["doc_ids"], e["tf"], e["impacts"], e["doc_len"]])
    return ix, "hipbm25_remove_ranges", "n_docs", state


def make_tokens(tmp_path):
    from hiprag import TokenStore
    rng = np.random.default_rng(5)
    s = TokenStore(100, max_doc_tokens=6)
    s.append([rng.integers(3, 100, n).tolist() for n in np.arange(N) % 4])      # lengths 0, 1, 2, 3 in turn
    return s, "hiptok_remove_ranges", "n_docs", lambda: arrays_bytes(s.export())


def make_pages(tmp_path):
    from hiprag import PageTable
    t = PageTable()
    t.append(np.arange(N) // 3, np.asarray([0, 7, 7, 19, 30, 40], np.int64))      # five documents, one of them empty
    return t, "hippage_remove_ranges", "rows", lambda: arrays_bytes(t.export())


def make_multivec(tmp_path):
    from hiprag.colbert import MultiVectorStore
    rng = np.random.default_rng(6)
    s = MultiVectorStore(64, max_doc_vectors=5)
    s.append([rng.integers(0, 0x4000, (n, 64)).astype(np.uint16) for n in np.arange(N) % 4])
    return s, "hipmv_remove_ranges", "n_docs", lambda: arrays_bytes(s.export())


MAKERS = [make_dense, make_ivf, make_bm25, make_tokens, make_pages, make_multivec]


def remove(entry, h, table):
    from hiprag import _native as nat
    if table == NULL_TABLE:
        return nat.call(entry, h, None, 2)
    r = np.ascontiguousarray([(1, 2)] if table == NEGATIVE_COUNT else table, np.int64).reshape(-1, 2)
    nat.call(entry, h, r.ctypes.data if len(r) else None, -1 if table == NEGATIVE_COUNT else len(r))


@pytest.mark.parametrize("make", MAKERS, ids=[m.__name__[5:] for m in MAKERS])
def test_one_table_on_every_structure(gpu, tmp_path, make):
    from hiprag import _native as nat
    a, entry, count_name, state_a = make(tmp_path)
    b, _, _, state_b = make(tmp_path)
    before = state_a()
    assert before == state_b(), "the twins differ before anything was removed"
    for table, text in REFUSED:
        with pytest.raises(nat.HipRagError) as e:
            remove(entry, a._h, table)
        assert e.value.code == -1 and text in str(e.value), (table, str(e.value))
        if table == [(3, 2)]:
            assert f"{count_name} = {N}" in str(e.value), str(e.value)
    assert state_a() == before, "a refused table changed the structure"
    remove(entry, a._h, GOOD)
    remove(entry, b._h, JOINED)
    after = state_a()
    assert after == state_b(), "empty and touching ranges do not leave what the joined table leaves"
    assert after != before
