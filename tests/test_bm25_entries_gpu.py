"""
The eight BM25 search entries (libhiprag hipbm25_search{,_scoped}{,_weighted}{,_dev}) share one host driver, and these are
the places where they differ ON PURPOSE: what each one answers to an empty batch, the words of its null-output refusal,
the k it takes, and what it adds to hipbm25_get_stats.  Every case is an argument the library is documented to accept or
to refuse; a refused call must leave the prefilled outputs as they were, on the device too.

The collection: 12 documents, 3 terms (one tile, no skip table).
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_INVALID = -1   # include/hiprag.h
N_DOCS = 12
LISTS = ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [1, 4, 7], [2, 3])
ENTRIES = tuple(f"hipbm25_search{s}{w}{d}" for s in ("", "_scoped") for w in ("", "_weighted") for d in ("", "_dev"))
UNSCOPED = tuple(e for e in ENTRIES if "_scoped" not in e)
SCOPED = tuple(e for e in ENTRIES if "_scoped" in e)


@functools.lru_cache(maxsize=None)
def bm25():
    from hiprag import HipBM25, PostingsCSR
    off = np.concatenate([[0], np.cumsum([len(l) for l in LISTS])]).astype(np.uint64)
    ids = np.concatenate(LISTS).astype(np.uint32)
    imp = (np.arange(1, ids.size + 1) / 8.0).astype(np.float32)
    return HipBM25(PostingsCSR(N_DOCS, len(LISTS), off, ids, imp))


class Call:
    """one query [0, 1, 2] (or none) with sentinel outputs; args(entry) lays the arguments out as the entry takes them"""

    def __init__(self, nq=1, k=4, null_weights=False):
        import torch
        self.nq, self.k = nq, k
        self.terms = np.asarray([0, 1, 2], np.uint32)
        self.w = None if null_weights else np.asarray([1.0, 0.5, 2.0], np.float32)
        self.qoff = np.asarray([0, 3] if nq else [0], np.int32)
        self.scope = (np.asarray([0, N_DOCS], np.int64), np.asarray([0, 1], np.int32), np.asarray([0], np.int32))
        self.d64 = torch.full((1, k), -77.0, dtype=torch.float64, device="cuda")
        self.d32 = torch.full((1, k), -77.0, dtype=torch.float32, device="cuda")
        self.did = torch.full((1, k), -77, dtype=torch.int64, device="cuda")
        self.hs, self.hi = np.full((1, k), -77.0, np.float32), np.full((1, k), -77, np.int64)

    def args(self, entry, null_outputs=False, null_ids=False):
        from hiprag.index import _stream_ptr
        a = [self.terms.ctypes.data]
        if "_weighted" in entry:
            a.append(None if self.w is None else self.w.ctypes.data)
        a += [self.qoff.ctypes.data, self.nq, self.k]
        if "_scoped" in entry:
            a += [self.scope[0].ctypes.data, self.scope[1].ctypes.data, 1, self.scope[2].ctypes.data]
        if entry.endswith("_dev"):
            out = [self.d64.data_ptr(), self.d32.data_ptr(), self.did.data_ptr()]
        else:
            out = [self.hs.ctypes.data, self.hi.ctypes.data]
        if null_outputs:
            out = [None] * len(out)
        if null_ids:
            out[-1] = None
        return a + out + ([_stream_ptr()] if entry.endswith("_dev") else [])

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool(torch.all(self.d64 == -77.0) and torch.all(self.d32 == -77.0) and torch.all(self.did == -77)
                    and np.all(self.hs == -77.0) and np.all(self.hi == -77))


def refused(entry, args):
    from hiprag import _native as nat
    with pytest.raises(nat.HipRagError) as e:
        nat.call(entry, bm25()._h, *args)
    assert e.value.code == E_INVALID, entry
    return str(e.value)


def test_an_empty_batch(gpu):
    """nq == 0 and null outputs: the unscoped entries return OK before they look at weights or outputs, the scoped refuse"""
    from hiprag import _native as nat
    c = Call(nq=0, null_weights=True)
    for entry in UNSCOPED:
        nat.call(entry, bm25()._h, *c.args(entry, null_outputs=True))
    for entry in SCOPED:
        assert "nq must be at least 1" in refused(entry, c.args(entry, null_outputs=True)), entry
    assert c.untouched()


def test_a_null_ids_output_is_refused_in_the_entry_s_own_words(gpu):
    c = Call()
    for entry in ENTRIES:
        msg = refused(entry, c.args(entry, null_ids=True))
        assert ("out_ids is null" if entry in SCOPED else "null output") in msg, (entry, msg)
        assert ("out_ids is null" in msg) == (entry in SCOPED), (entry, msg)
    assert c.untouched()


def test_k_65_is_for_the_unscoped_entries_only(gpu):
    import torch
    from hiprag import _native as nat
    c = Call(k=65)
    for entry in SCOPED:
        assert "1..64" in refused(entry, c.args(entry)), entry
    assert c.untouched()
    for entry in UNSCOPED:
        c = Call(k=65)
        nat.call(entry, bm25()._h, *c.args(entry))
        torch.cuda.synchronize()
        ids = c.did.cpu().numpy() if entry.endswith("_dev") else c.hi
        assert sorted(ids[0, :N_DOCS].tolist()) == list(range(N_DOCS)) and np.all(ids[0, N_DOCS:] == -1), entry   # term 0 holds every document


def stats():
    from hiprag import _native as nat
    st = nat.HipBm25Stats()
    nat.call("hipbm25_get_stats", bm25()._h, ctypes.byref(st))
    return np.asarray([st.queries, st.postings_touched, st.bytes_algorithmic], np.int64)


def test_stats_of_one_unscoped_and_one_scoped_call(gpu):
    """both count the query and its postings; the unscoped form alone counts bytes: 8 per posting + 8 per document and query"""
    import torch
    from hiprag import _native as nat
    postings = sum(len(l) for l in LISTS)
    c = Call()
    s0 = stats()
    nat.call("hipbm25_search_dev", bm25()._h, *c.args("hipbm25_search_dev"))
    s1 = stats()
    nat.call("hipbm25_search_scoped_dev", bm25()._h, *c.args("hipbm25_search_scoped_dev"))
    s2 = stats()
    torch.cuda.synchronize()
    assert (s1 - s0).tolist() == [1, postings, postings * 8 + N_DOCS * 8]
    assert (s2 - s1).tolist() == [1, postings, 0]
