"""
The multi-vector store (hipmv_*): after any sequence of appends (from the device layout and from the host) and removals its
export equals that of a fresh store of the surviving documents, bit for bit; the cap is applied; a saved store loads back
equal; bad files and refused calls change nothing.
"""
import os

import numpy as np
import pytest

from colbert_cases import csr_of, drop_ranges

pytestmark = pytest.mark.gpu

DIM = 128
CAP = 40
LENS = [0, 1, 31, 32, 33, CAP - 1, CAP, CAP + 1, CAP + 25, 0, 3, 17, 64, 7, 0, 12] * 2     # 32 documents


def _docs(seed=11, dim=DIM):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 0x7F80, size=(n, dim)).astype(np.uint16) for n in LENS]     # finite positive bf16 bit patterns


def _fresh(docs, cap=CAP, dim=DIM):
    from hiprag import MultiVectorStore
    st = MultiVectorStore(dim, max_doc_vectors=cap)
    st.append(docs)
    return st


def _same(store, docs, cap=CAP, dim=DIM):
    off, vecs = store.export()
    eoff, evecs = csr_of(docs, dim, cap)
    assert off.dtype == np.int64 and vecs.dtype == np.uint16
    assert np.array_equal(off, eoff) and np.array_equal(vecs, evecs)
    n, nv, d, longest = store.sizes()
    assert (n, nv, d) == (len(docs), int(eoff[-1]), dim)
    assert longest == max([min(len(v), cap) for v in docs], default=0)


def _device_block(docs, stride, dim=DIM):
    """The layout hipenc_forward_colbert writes: [n, stride, dim] with poison behind every count."""
    import torch
    block = np.full((len(docs), stride, dim), 0x7FC5, dtype=np.uint16)
    for i, v in enumerate(docs):
        block[i, :len(v)] = v
    t = torch.from_numpy(block.view(np.int16)).cuda().view(torch.bfloat16)
    return t, np.asarray([len(v) for v in docs], dtype=np.int32)


def test_append_remove_append_equals_a_fresh_store(gpu):
    from hiprag import MultiVectorStore
    docs = _docs()
    st = MultiVectorStore(DIM, max_doc_vectors=CAP)
    _same(st, [])
    st.append(docs[:9])
    _same(st, docs[:9])
    st.append_device(*_device_block(docs[9:21], 70))    # from the device layout; grows past the first allocation
    _same(st, docs[:21])
    front = st.export()[1][:1].copy()
    ranges = [(0, 0), (2, 5), (5, 6), (9, 9), (12, 17), (20, 21)]      # empty, touching, a middle one, the last document
    st.remove_ranges(ranges)
    live = drop_ranges(docs[:21], ranges)
    _same(st, live)
    assert np.array_equal(st.export()[1][:1], front)    # in front of the first removed document nothing changed
    st.append_device(*_device_block(docs[21:], 65))
    live += docs[21:]
    _same(st, live)
    fresh = _fresh(live)
    for a, b in zip(st.export(), fresh.export()):
        assert a.tobytes() == b.tobytes()
    # nothing to remove: a no-op; an empty batch and empty documents: valid in both forms
    st.remove_ranges([])
    st.remove_ranges([(3, 3), (len(live), len(live))])
    st.append([])
    extra = [np.zeros((0, DIM), np.uint16), np.zeros((0, DIM), np.uint16), docs[2][:1]]
    st.append(extra[:2])
    st.append_device(*_device_block(extra[2:] + extra[:1], 1))
    live += extra[:2] + extra[2:] + extra[:1]
    _same(st, live)
    # the first document alone, then everything
    st.remove_ranges([(0, 1)])
    live = live[1:]
    _same(st, live)
    st.remove_ranges([(0, len(live))])
    _same(st, [])
    st.append(docs[3:9])                                # and it is usable again
    _same(st, docs[3:9])


def test_the_cap_is_applied_in_both_forms(gpu):
    from hiprag import MultiVectorStore
    docs = _docs(5)
    for cap in (1, 32, CAP):
        _same(_fresh(docs, cap), docs, cap)
        st = MultiVectorStore(DIM, max_doc_vectors=cap)
        st.append_device(*_device_block(docs, max(LENS)))
        _same(st, docs, cap)


def test_wide_vectors_and_many_small_appends_across_reallocations(gpu):
    from hiprag import MultiVectorStore
    rng = np.random.default_rng(3)
    docs = [rng.integers(0, 0x7F80, size=(n, 1024)).astype(np.uint16) for n in (5, 0, 33, 2, 64, 1, 9, 40)]
    st = MultiVectorStore(1024, max_doc_vectors=48)
    for i, v in enumerate(docs):
        if i % 2:
            st.append([v])
        else:
            st.append_device(*_device_block([v], 64, 1024))
        _same(st, docs[:i + 1], 48, 1024)
    st.remove_ranges([(1, 3), (6, 7)])
    _same(st, drop_ranges(docs, [(1, 3), (6, 7)]), 48, 1024)


def test_save_load_round_trip_and_bad_files(gpu, tmp_path):
    from hiprag import HipRagError, MultiVectorStore
    docs = _docs(9)
    st = _fresh(docs)
    path = str(tmp_path / "store.mv")
    st.save(path)
    eoff, evecs = csr_of(docs, DIM, CAP)
    assert os.path.getsize(path) == 36 + 8 * len(eoff) + 2 * evecs.size
    raw = open(path, "rb").read()
    assert raw[:8] == b"HIPMV001" and np.frombuffer(raw[8:20], np.int32).tolist() == [1, DIM, CAP]
    assert np.frombuffer(raw[20:36], np.int64).tolist() == [len(docs), int(eoff[-1])]
    xoff, xvecs = st.export()                           # the whole file, as the comment above hipmv_save lays it out
    assert raw == (b"HIPMV001" + np.asarray([1, DIM, CAP], np.int32).tobytes() + np.asarray([len(docs), len(xvecs)], np.int64).tobytes()
                   + xoff.tobytes() + xvecs.tobytes())
    back = MultiVectorStore.load(path)
    assert back.max_doc_vectors == CAP
    for a, b in zip(st.export(), back.export()):
        assert a.tobytes() == b.tobytes()
    _same(back, docs)
    back.append(docs[:3])                               # a loaded store is an ordinary store
    _same(back, docs + docs[:3])
    # an empty store round-trips too
    empty = str(tmp_path / "empty.mv")
    MultiVectorStore(DIM, max_doc_vectors=CAP).save(empty)
    _same(MultiVectorStore.load(empty), [])

    def refused(data, name):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        with pytest.raises(HipRagError) as e:
            MultiVectorStore.load(p)
        assert e.value.code == -4, name

    refused(raw[:-2], "truncated.mv")
    refused(raw[:30], "short_header.mv")
    refused(raw + b"\0\0", "too_long.mv")
    refused(b"HIPMV002" + raw[8:], "magic.mv")
    off = np.frombuffer(raw[36:36 + 8 * len(eoff)], np.int64).copy()
    off[3], off[4] = off[4], off[3]                     # descending offsets (documents 2..4 differ in length)
    assert off[3] > off[4]
    refused(raw[:36] + off.tobytes() + raw[36 + 8 * len(eoff):], "descending.mv")
    off = np.frombuffer(raw[36:36 + 8 * len(eoff)], np.int64).copy()
    off[0] = 1
    refused(raw[:36] + off.tobytes() + raw[36 + 8 * len(eoff):], "start.mv")
    bad_dim = raw[:12] + np.asarray([DIM + 1], np.int32).tobytes() + raw[16:]
    refused(bad_dim, "dim.mv")
    with pytest.raises(HipRagError):
        MultiVectorStore.load(str(tmp_path / "absent.mv"))


def test_refused_calls_leave_the_store_as_it_was(gpu):
    import torch
    from hiprag import HipRagError, MultiVectorStore
    from hiprag import _native as nat
    docs = _docs(7)[:12]
    st = _fresh(docs)
    before = [a.tobytes() for a in st.export()]
    ok = np.zeros((4, DIM), np.uint16)
    for offsets in (np.asarray([1, 2, 4], np.int64), np.asarray([0, 3, 2, 4], np.int64)):       # start, descent
        with pytest.raises(HipRagError) as e:
            st.append(ok, offsets)
        assert e.value.code == -1
    with pytest.raises(HipRagError):
        nat.call("hipmv_append", st._h, None, np.asarray([0, 2], np.int64).ctypes.data, 1)      # null vectors
    with pytest.raises(HipRagError):
        nat.call("hipmv_append", st._h, ok.ctypes.data, None, 1)                                 # null offsets
    block = torch.zeros((2, 8, DIM), dtype=torch.bfloat16, device="cuda")
    for counts in ([3, 9], [-1, 2]):                                                             # count outside [0, row_stride]
        with pytest.raises(HipRagError) as e:
            st.append_device(block, counts)
        assert e.value.code == -1
    cnt = np.asarray([1, 1], np.int32)
    with pytest.raises(HipRagError):
        nat.call("hipmv_append_dev", st._h, None, 8, cnt.ctypes.data, 2, None)                   # null vectors
    with pytest.raises(HipRagError):
        nat.call("hipmv_append_dev", st._h, block.data_ptr(), 8, None, 2, None)                  # null counts
    with pytest.raises(HipRagError):
        nat.call("hipmv_append_dev", st._h, block.data_ptr(), 0, cnt.ctypes.data, 2, None)       # row_stride 0
    for ranges in ([(3, 2)], [(-1, 2)], [(0, 13)], [(4, 6), (5, 7)], [(6, 8), (1, 2)]):          # the range table rules
        with pytest.raises(HipRagError) as e:
            st.remove_ranges(ranges)
        assert e.value.code == -1
    with pytest.raises(HipRagError):
        nat.call("hipmv_remove_ranges", st._h, None, 2)
    assert [a.tobytes() for a in st.export()] == before
    _same(st, docs)
    for dim, cap in ((0, 8), (96, 8), (1088, 8), (DIM, 0)):                                      # dim, cap
        with pytest.raises(HipRagError):
            MultiVectorStore(dim, max_doc_vectors=cap)
    with pytest.raises(HipRagError) as e:
        nat.call("hipmv_sizes", 123456789, np.zeros(4, np.int64).ctypes.data)
    assert e.value.code == -3
