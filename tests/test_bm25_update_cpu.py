"""
Updatable BM25 postings, the parts that need no GPU: the impact formula's operation order (hipbm25_impacts_host against
build_postings, as uint32 bits), the batch builder and vocabulary growth of HipBM25Updatable.append_texts against
build_postings_from_texts of the concatenation, every check hipbm25_create_tf makes before it touches a device, and the
overlay's bookkeeping around a live collection index with the library calls stubbed out.
"""
import threading
import types

import numpy as np
import pytest

E_INVALID, E_HANDLE = -1, -3   # include/hiprag.h


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the impact formula --------------------------------------------------------------------------------------------------
def test_impacts_host_equals_build_postings_bit_for_bit():
    from hiprag import _native as nat, build_postings
    from hiprag.sparse import B, K1
    rng = np.random.default_rng(11)
    n_docs, n_terms = 6000, 1500
    doc_len = rng.integers(1, 60, n_docs)
    doc_len[0], doc_len[1], doc_len[2] = 1, 7000, 4500            # doc_len 1 and several thousand
    doc = np.repeat(np.arange(n_docs), doc_len)
    w = 1.0 / np.arange(1, n_terms - 1)
    term = 2 + np.minimum(np.searchsorted(np.cumsum(w) / w.sum(), rng.random(doc.size)), n_terms - 3)
    start = np.cumsum(doc_len) - doc_len
    term[start] = 0                                                 # term 0 in every document: df = N
    term[start[0]] = 0                                              # the one-token document: tf 1, dl 1
    term[start[1] + 1: start[1] + 6001] = 1                         # term 1 in one document only, 6000 times: df = 1, large tf
    p = build_postings(doc, term, n_docs, n_terms)
    df = np.diff(p.offsets.astype(np.int64))
    P = p.doc_ids.size
    assert P >= 100_000 and df[0] == n_docs and df[1] == 1 and p.tfs.max() == 6000 and p.tfs.min() == 1
    assert p.doc_len.min() == 1 and p.doc_len.max() == 7000
    idf = np.log(1.0 + (float(n_docs) - df.astype(np.float64) + 0.5) / (df.astype(np.float64) + 0.5))
    idf_p = np.ascontiguousarray(np.repeat(idf, df))
    dl_p = np.ascontiguousarray(p.doc_len[p.doc_ids].astype(np.uint32))
    tf_p = np.ascontiguousarray(p.tfs, dtype=np.uint32)
    out = np.zeros(P, np.float32)
    nat.call("hipbm25_impacts_host", idf_p.ctypes.data, tf_p.ctypes.data, dl_p.ctypes.data, P, float(p.doc_len.sum()) / n_docs, K1, B,
             out.ctypes.data)
    differ = int(np.sum(bits(out) != bits(p.impacts)))
    print(f"{P} postings, {differ} impacts differ")
    assert differ == 0


def test_impacts_host_equals_build_postings_on_a_large_collection():
    """~10^5 postings of a Zipf collection, other k1 / b too"""
    from hiprag import _native as nat, build_postings
    rng = np.random.default_rng(12)
    n_docs, n_terms = 2500, 3000
    doc_len = rng.integers(1, 120, n_docs)
    doc = np.repeat(np.arange(n_docs), doc_len)
    w = 1.0 / np.arange(1, n_terms + 1)
    term = np.minimum(np.searchsorted(np.cumsum(w) / w.sum(), rng.random(doc.size)), n_terms - 1)
    for k1, b in ((1.5, 0.75), (0.9, 0.4), (2.0, 1.0), (1.2, 0.0)):
        p = build_postings(doc, term, n_docs, n_terms, k1=k1, b=b)
        df = np.diff(p.offsets.astype(np.int64)).astype(np.float64)
        P = p.doc_ids.size
        assert P >= 100_000
        idf_p = np.ascontiguousarray(np.repeat(np.log(1.0 + (float(n_docs) - df + 0.5) / (df + 0.5)), df.astype(np.int64)))
        dl_p = np.ascontiguousarray(p.doc_len[p.doc_ids].astype(np.uint32))
        out = np.zeros(P, np.float32)
        nat.call("hipbm25_impacts_host", idf_p.ctypes.data, p.tfs.ctypes.data, dl_p.ctypes.data, P, float(p.doc_len.sum()) / n_docs, k1, b,
                 out.ctypes.data)
        assert np.array_equal(bits(out), bits(p.impacts)), (k1, b)


def test_build_postings_keeps_tf_and_doc_len():
    from hiprag import build_postings_from_texts
    p = build_postings_from_texts(["a b a", "", "b c c c"])
    assert p.vocab == {"a": 0, "b": 1, "c": 2}
    assert p.doc_ids.tolist() == [0, 0, 2, 2] and p.tfs.tolist() == [2, 1, 1, 3] and p.doc_len.tolist() == [3, 0, 4]
    assert p.tfs.dtype == np.uint32


# ---- the batch builder and the vocabulary --------------------------------------------------------------------------------
class _Recorder:
    """stands for the library under HipBM25Updatable: keeps the CSR a hipbm25_append would form, on the host"""

    def __init__(self, p):
        self.n_docs, self.n_terms = p.n_docs, p.n_terms
        off = p.offsets.astype(np.int64)
        self.lists = [(p.doc_ids[off[t]:off[t + 1]].astype(np.int64), p.tfs[off[t]:off[t + 1]].astype(np.int64)) for t in range(p.n_terms)]
        self.doc_len = list(p.doc_len)

    def append(self, n_new, n_terms_after, off, ids, tf, dl):
        assert n_terms_after >= self.n_terms and off.shape[0] == n_terms_after + 1 and off[0] == 0
        self.lists += [(np.zeros(0, np.int64), np.zeros(0, np.int64)) for _ in range(n_terms_after - self.n_terms)]
        for t in range(n_terms_after):
            lo, hi = int(off[t]), int(off[t + 1])
            b = ids[lo:hi].astype(np.int64)
            assert np.all(np.diff(b) > 0) and (b.size == 0 or b[-1] < n_new) and np.all(tf[lo:hi] >= 1)
            self.lists[t] = (np.append(self.lists[t][0], b + self.n_docs), np.append(self.lists[t][1], tf[lo:hi]))
        self.doc_len += list(dl)
        self.n_docs += n_new
        self.n_terms = n_terms_after


def _stubbed_updatable(p, rec, monkeypatch):
    from hiprag import HipBM25Updatable, PostingsCSR
    import hiprag.sparse as sp

    def call(name, h, *args):
        assert name == "hipbm25_append", name
        n_new, n_terms_after, off_p, ids_p, tf_p, dl_p = args
        rec.append(n_new, n_terms_after, *call.arrays)

    upd = HipBM25Updatable.__new__(HipBM25Updatable)
    upd._h = None
    upd.device = 0
    upd.auto_commit = True
    upd.p = PostingsCSR(p.n_docs, p.n_terms, None, None, None, dict(p.vocab))
    real = upd.append_postings

    def append_postings(n_new, n_terms_after, offsets, doc_ids, tfs, doc_len):
        call.arrays = (np.asarray(offsets), np.asarray(doc_ids), np.asarray(tfs), np.asarray(doc_len))
        real(n_new, n_terms_after, offsets, doc_ids, tfs, doc_len)

    upd.append_postings = append_postings
    monkeypatch.setattr(sp.nat, "call", call)
    return upd


def test_append_texts_builds_the_postings_of_the_concatenation(monkeypatch):
    from hiprag import build_postings_from_texts
    rng = np.random.default_rng(3)
    words = [f"w{j}" for j in range(60)]

    def texts(n, lo, hi):
        return [" ".join(rng.choice(words[lo:hi], size=int(rng.integers(0, 12)))) for _ in range(n)]

    first, batches = texts(40, 0, 20), [texts(1, 10, 30), texts(25, 0, 45), ["", "  "], ["W1 w1 brandnew"], texts(30, 30, 60)]
    p0 = build_postings_from_texts(first)
    rec = _Recorder(p0)
    upd = _stubbed_updatable(p0, rec, monkeypatch)
    every = list(first)
    for batch in batches:
        lo, hi = upd.append_texts(batch)
        assert (lo, hi) == (len(every), len(every) + len(batch))
        every += batch
        want = build_postings_from_texts(every)
        assert upd.p.vocab == want.vocab and list(upd.p.vocab) == list(want.vocab), "vocabulary grows in order of first appearance"
        assert (rec.n_docs, rec.n_terms) == (want.n_docs, want.n_terms) == (upd.p.n_docs, upd.p.n_terms)
        assert np.array_equal(np.cumsum([0] + [len(ids) for ids, _ in rec.lists]), want.offsets.astype(np.int64))
        assert np.array_equal(np.concatenate([ids for ids, _ in rec.lists]), want.doc_ids)
        assert np.array_equal(np.concatenate([tf for _, tf in rec.lists]), want.tfs)
        assert np.array_equal(np.asarray(rec.doc_len), want.doc_len)


def test_batch_csr_is_build_postings_without_impacts():
    from hiprag import batch_csr, build_postings
    rng = np.random.default_rng(4)
    doc, term = rng.integers(0, 50, 4000), rng.integers(0, 97, 4000)
    p = build_postings(doc, term, 50, 100)
    off, ids, tf, dl = batch_csr(doc, term, 50, 100)
    assert np.array_equal(off, p.offsets) and np.array_equal(ids, p.doc_ids) and np.array_equal(tf, p.tfs) and np.array_equal(dl, p.doc_len)
    off, ids, tf, dl = batch_csr(np.zeros(0), np.zeros(0), 0, 5)
    assert off.tolist() == [0] * 6 and ids.size == tf.size == dl.size == 0


# ---- checks made before a device is touched ------------------------------------------------------------------------------
def test_create_tf_refuses_bad_arguments_without_a_gpu():
    import ctypes
    from hiprag import _native as nat
    u32, u64 = np.uint32, np.uint64
    good = dict(n_docs=3, n_terms=2, off=np.asarray([0, 2, 3], u64), ids=np.asarray([0, 2, 1], u32), tf=np.asarray([1, 2, 1], u32),
                dl=np.asarray([1, 1, 2], u32), k1=1.5, b=0.75)

    def create(**kw):
        a = dict(good, **kw)
        h = ctypes.c_uint64()
        ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        nat.call("hipbm25_create_tf", a["n_docs"], a["n_terms"], ptr(a["off"]), ptr(a["ids"]), ptr(a["tf"]), ptr(a["dl"]), a["k1"], a["b"],
                 0, ctypes.byref(h) if a.get("out", True) else None)

    bad = [dict(off=None), dict(ids=None), dict(tf=None), dict(dl=None), dict(out=False),
           dict(n_docs=-1), dict(n_terms=-1), dict(n_docs=2 ** 32),
           dict(off=np.asarray([1, 2, 3], u64)),                  # offsets do not start at 0
           dict(off=np.asarray([0, 3, 2], u64)),                  # offsets descend
           dict(ids=np.asarray([2, 0, 1], u32)),                  # a list that is not ascending
           dict(ids=np.asarray([0, 0, 1], u32)),                  # ... not strictly
           dict(ids=np.asarray([0, 3, 1], u32)),                  # doc id >= n_docs
           dict(tf=np.asarray([1, 0, 1], u32)),                   # tf 0
           dict(k1=-0.1), dict(k1=float("nan")), dict(b=-0.01), dict(b=1.01), dict(b=float("nan"))]
    for kw in bad:
        with pytest.raises(nat.HipRagError) as e:
            create(**kw)
        assert e.value.code == E_INVALID, kw


def test_update_entries_on_an_unknown_handle_and_impacts_host_arguments():
    from hiprag import _native as nat
    v = np.zeros(8, np.int64)
    for name, args in (("hipbm25_append", (0, 1, v.ctypes.data, None, None, None)), ("hipbm25_remove_ranges", (None, 0)),
                       ("hipbm25_reweigh", (None,)), ("hipbm25_export", (None, None, None, None, None)),
                       ("hipbm25_update_info", (v.ctypes.data,)), ("hipbm25_sizes", (v.ctypes.data,))):
        with pytest.raises(nat.HipRagError) as e:
            nat.call(name, 987654321, *args)
        assert e.value.code == E_HANDLE, name
    one = np.ones(1, np.float64)
    u = np.ones(1, np.uint32)
    o = np.zeros(1, np.float32)
    ok = [one.ctypes.data, u.ctypes.data, u.ctypes.data, 1, 1.0, 1.5, 0.75, o.ctypes.data]
    nat.call("hipbm25_impacts_host", *ok)
    for j, val in ((0, None), (1, None), (2, None), (7, None), (3, -1), (4, 0.0), (5, -1.0), (6, 1.5)):
        args = list(ok)
        args[j] = val
        with pytest.raises(nat.HipRagError) as e:
            nat.call("hipbm25_impacts_host", *args)
        assert e.value.code == E_INVALID, j


# ---- the overlay around a live collection index, library stubbed out -----------------------------------------------------
class _FakeIndex:
    def __init__(self, d, metric="l2", device=0):
        self.d, self.metric, self.device, self.ntotal = int(d), 1, 0, 0

    def add(self, x):
        self.ntotal += len(x)

    def remove_ranges(self, ranges):
        n = sum(hi - lo for lo, hi in ranges)
        self.ntotal -= n
        return n

    def save(self, path):
        with open(path, "wb") as f:
            f.write(b"fake")


class _FakeLive:
    def __init__(self, n, fail=False):
        self.n, self.calls, self.fail = n, [], fail

    def append_texts(self, texts):
        if self.fail:
            raise RuntimeError("no memory")
        self.calls.append(("append", list(texts)))
        self.n += len(texts)

    def remove_ranges(self, ranges):
        self.calls.append(("remove", [tuple(r) for r in ranges]))
        self.n -= sum(hi - lo for lo, hi in ranges)

    def sizes(self):
        return {"n_docs": self.n}


@pytest.fixture
def overlay(tmp_path, monkeypatch):
    from rag.storage.hip_index import collection as col, sparse
    tables = {}
    shim = types.SimpleNamespace(HipFlatIndex=_FakeIndex, INDEX_SUFFIX="_hip.index", _INDEX_CACHE={}, _LOCK=threading.Lock(),
                                 _load_chunk_list=lambda storage, doc_id: [{"text": t} for t in tables[doc_id]])
    monkeypatch.setattr(col, "_hip", lambda: shim)
    col.clear_collection_cache()
    sparse.clear_sparse_cache()
    yield types.SimpleNamespace(col=col, sparse=sparse, dir=tmp_path, tables=tables)
    col.clear_collection_cache()
    sparse.clear_sparse_cache()


def _install(o, live):
    coll = o.col.open_collection(o.dir)
    with o.sparse._LOCK:
        o.sparse._SPARSE_CACHE[o.sparse._collection_key(coll)] = (o.sparse._collection_version(coll), live)
    return coll


def _cached(o):
    coll = o.col.open_collection(o.dir)
    hit = o.sparse._SPARSE_CACHE.get(o.sparse._collection_key(coll))
    return None if hit is None or hit[0] != o.sparse._collection_version(coll) else hit[1]


def test_a_live_collection_index_follows_append_delete_and_replace(overlay):
    o = overlay
    x = lambda n: np.zeros((n, 4), np.float32)   # noqa: E731
    o.col.append_document("a", "red", x(3), o.dir, texts=["a0", "a1", "a2"])     # cold cache: nothing to follow
    assert not o.sparse._SPARSE_CACHE
    live = _FakeLive(3)
    _install(o, live)
    o.col.append_document("b", "blue", x(2), o.dir, texts=["b0", "b1"])
    assert live.calls == [("append", ["b0", "b1"])] and _cached(o) is live, "re-keyed to the new manifest version"
    o.tables["c"] = ["c0", "c1", "c2", "c3"]
    o.col.append_document("c", "red", x(4), o.dir)                                # no texts: the chunk table is read
    assert live.calls[-1] == ("append", ["c0", "c1", "c2", "c3"]) and _cached(o) is live
    assert o.col.delete_document("b", o.dir) == 2
    assert live.calls[-1] == ("remove", [(3, 5)]) and _cached(o) is live
    o.col.replace_document("a", "red", x(5), o.dir, texts=["A0", "A1", "A2", "A3", "A4"])
    assert live.calls[-2:] == [("remove", [(0, 3)]), ("append", ["A0", "A1", "A2", "A3", "A4"])] and _cached(o) is live
    assert live.n == o.col.open_collection(o.dir).manifest.rows == 9
    o.col.replace_document("d", "blue", x(1), o.dir, texts=["d0"])               # a replacement that finds nothing to remove
    assert live.calls[-1] == ("append", ["d0"]) and _cached(o) is live


def test_a_failed_or_inconsistent_update_drops_the_entry(overlay):
    o = overlay
    x = lambda n: np.zeros((n, 4), np.float32)   # noqa: E731
    o.col.append_document("a", None, x(3), o.dir, texts=["a0", "a1", "a2"])
    _install(o, _FakeLive(3, fail=True))
    o.col.append_document("b", None, x(2), o.dir, texts=["b0", "b1"])            # the library call fails
    assert not o.sparse._SPARSE_CACHE
    _install(o, _FakeLive(5))
    o.col.append_document("c", None, x(2), o.dir, texts=["only one"])            # texts disagree with the rows
    assert not o.sparse._SPARSE_CACHE
    _install(o, _FakeLive(7))
    o.col.append_document("d", None, x(2), o.dir)                                 # no texts and no chunk table
    assert not o.sparse._SPARSE_CACHE
    live = _FakeLive(9)
    coll = _install(o, live)
    with o.sparse._LOCK:                                                           # an entry of another manifest version
        o.sparse._SPARSE_CACHE[o.sparse._collection_key(coll)] = (("collection", 0.0, 0, 0, 0), live)
    assert o.sparse.live_collection_sparse(coll) is None and not o.sparse._SPARSE_CACHE
    o.col.append_document("e", None, x(1), o.dir, texts=["e0"])
    assert live.calls == [] and not o.sparse._SPARSE_CACHE
