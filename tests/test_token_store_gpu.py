"""
The passage token store (hiptok_*): after any sequence of appends and removals its export equals that of a fresh store of
the surviving documents, bit for bit; the cap is applied; refused calls change nothing.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOCAB = 2000
CAP = 130
LENS = [0, 1, 59, 60, 61, 119, 120, 121, 124, 125, CAP, CAP + 1, CAP + 70, 0, 3, 64, 200, 7, 0, 33] * 2     # 40 passages


def _docs(seed=11):
    rng = np.random.default_rng(seed)
    return [rng.integers(3, VOCAB, size=n).astype(np.int32).tolist() for n in LENS]


def _fresh(docs, cap=CAP):
    from hiprag import TokenStore
    st = TokenStore(VOCAB, max_doc_tokens=cap)
    st.append(docs)
    return st


def _expect(docs, cap=CAP):
    from hiprag.rerank import csr
    tokens, offsets = csr([d[:cap] for d in docs])
    return offsets, tokens


def _same(store, docs, cap=CAP):
    off, tok = store.export()
    eoff, etok = _expect(docs, cap)
    assert off.dtype == np.int64 and tok.dtype == np.int32
    assert np.array_equal(off, eoff) and np.array_equal(tok, etok)
    n, nt, c, longest = store.sizes()
    assert (n, nt, c) == (len(docs), int(eoff[-1]), cap)
    assert longest == max([min(len(d), cap) for d in docs], default=0)


def _drop(docs, ranges):
    gone = set()
    for lo, hi in ranges:
        gone.update(range(lo, hi))
    return [d for i, d in enumerate(docs) if i not in gone]


def test_append_remove_append_equals_a_fresh_store(gpu):
    from hiprag import TokenStore
    docs = _docs()
    st = TokenStore(VOCAB, max_doc_tokens=CAP)
    _same(st, [])
    st.append(docs[:17])
    _same(st, docs[:17])
    st.append(docs[17:29])                              # grows past the first allocation
    _same(st, docs[:29])
    ranges = [(0, 0), (2, 5), (5, 6), (9, 9), (12, 20), (28, 29)]      # empty, touching, the last document
    st.remove_ranges(ranges)
    live = _drop(docs[:29], ranges)
    _same(st, live)
    st.append(docs[29:])
    live += docs[29:]
    _same(st, live)
    fresh = _fresh(live)
    for a, b in zip(st.export(), fresh.export()):
        assert a.tobytes() == b.tobytes()
    # nothing to remove: a no-op; an empty batch and empty documents: valid
    st.remove_ranges([])
    st.remove_ranges([(3, 3), (len(live), len(live))])
    st.append([])
    st.append([[], [], [5]])
    live += [[], [], [5]]
    _same(st, live)
    # the first document alone, then everything
    st.remove_ranges([(0, 1)])
    live = live[1:]
    _same(st, live)
    st.remove_ranges([(0, len(live))])
    _same(st, [])
    st.append(docs[3:9])                                # and it is usable again
    _same(st, docs[3:9])


def test_the_cap_is_applied(gpu):
    docs = _docs(5)
    for cap in (1, 60, CAP):
        _same(_fresh(docs, cap), docs, cap)


def test_refused_calls_leave_the_store_as_it_was(gpu):
    from hiprag import HipRagError, TokenStore
    from hiprag import _native as nat
    docs = _docs(7)[:12]
    st = _fresh(docs)
    before = [a.tobytes() for a in st.export()]
    ok_tokens = np.asarray([5, 6, 7, 8], dtype=np.int32)
    bad = [
        (ok_tokens, np.asarray([1, 2, 4], np.int64)),               # offsets do not start at 0
        (ok_tokens, np.asarray([0, 3, 2, 4], np.int64)),            # offsets descend
        (np.asarray([5, VOCAB, 7, 8], np.int32), np.asarray([0, 2, 4], np.int64)),     # id = vocab
        (np.asarray([5, -1, 7, 8], np.int32), np.asarray([0, 2, 4], np.int64)),        # negative id
    ]
    for tokens, offsets in bad:
        with pytest.raises(HipRagError) as e:
            st.append(tokens, offsets)
        assert e.value.code == -1
    with pytest.raises(HipRagError):
        nat.call("hiptok_append", st._h, None, np.asarray([0, 2], np.int64).ctypes.data, 1)      # null tokens
    with pytest.raises(HipRagError):
        nat.call("hiptok_append", st._h, ok_tokens.ctypes.data, None, 1)                          # null offsets
    for ranges in ([(3, 2)], [(-1, 2)], [(0, 13)], [(4, 6), (5, 7)], [(6, 8), (1, 2)]):           # the range table rules
        with pytest.raises(HipRagError) as e:
            st.remove_ranges(ranges)
        assert e.value.code == -1
    with pytest.raises(HipRagError):
        nat.call("hiptok_remove_ranges", st._h, None, 2)
    assert [a.tobytes() for a in st.export()] == before
    _same(st, docs)
    for args in ((0, 0, 2, 1, 8), (VOCAB, 0, 2, 1, 0), (VOCAB, 0, VOCAB, 1, 8)):                  # vocab, cap, eos
        with pytest.raises(HipRagError):
            TokenStore(args[0], bos=args[1], eos=args[2], pad=args[3], max_doc_tokens=args[4])
