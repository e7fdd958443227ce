"""
Updatable BM25 postings (hipbm25_create_tf / _append / _remove_ranges / _reweigh, hiprag.HipBM25Updatable).

Defining property: after any sequence of updates, once committed, the handle cannot be told apart from its TWIN --
HipBM25(build_postings(...)) over the surviving documents in order with the same term ids and n_terms: the export (offsets,
doc ids, tf, impacts as uint32 bits, doc lengths) and every search output, padding included, are equal bit for bit.  The
twin's results are checked once against the CPU oracle (oracle.hybrid_oracle.bm25_search).

The collection is the smallest at which every kernel form can go wrong: 20 000 documents (three 9216-document tiles), 3 000
terms drawn Zipf, doc_len 1..300; term 0 in every document (a long list with a skip table across all tiles), term 1 in
exactly 2047 documents (one below kSkipMinDf), term 2 in a single document, term 3 in none.
"""
import functools

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -6   # include/hiprag.h
N_DOCS = 20000
N_TERMS = 3000
TILE = 9216
SKIP_MIN_DF = 2048
T_ALL, T_2047, T_ONE, T_NONE = 0, 1, 2, 3
ONE_DOC = 9100            # the only document of T_ONE: inside the range the removal test takes out across the tile boundary
EXTRA_DOC = N_DOCS        # one document past the collection that holds T_2047: the 2048th posting of the append test


class Corpus:
    """token streams of N_DOCS + 1 documents as a CSR (tok_off, tok_term)"""

    def __init__(self):
        n = N_DOCS + 1
        rng = np.random.default_rng(20)
        self.doc_len = 1 + (np.arange(n, dtype=np.int64) * 7919 + 150) % 300
        self.doc_len[EXTRA_DOC] = 40
        self.tok_off = np.zeros(n + 1, np.int64)
        self.tok_off[1:] = np.cumsum(self.doc_len)
        # Zipf over the terms 4 .. V(doc) - 1, V growing with the document: later batches bring new terms
        vocab = np.minimum(600 + np.arange(n, dtype=np.int64) // 9, N_TERMS)
        vocab[EXTRA_DOC] = N_TERMS
        cdf = np.cumsum(1.0 / np.arange(1, N_TERMS - 3, dtype=np.float64))
        top = np.repeat(cdf[vocab - 5], self.doc_len)
        term = 4 + np.minimum(np.searchsorted(cdf, rng.random(int(self.tok_off[-1])) * top), np.repeat(vocab, self.doc_len) - 5)
        term[self.tok_off[:-1]] = T_ALL                          # first token of every document
        roomy = np.flatnonzero(self.doc_len[:18000] >= 3)
        for d in np.sort(rng.choice(roomy[roomy != ONE_DOC], size=SKIP_MIN_DF - 1, replace=False)):
            term[self.tok_off[d] + 1] = T_2047
        term[self.tok_off[EXTRA_DOC] + 1] = T_2047
        assert self.doc_len[ONE_DOC] >= 3
        term[self.tok_off[ONE_DOC] + 2] = T_ONE
        self.tok_term = term

    def tokens(self, docs):
        """(doc_of_tok, term_of_tok, doc_len) of the documents `docs` (indices into the corpus), renumbered 0.."""
        docs = np.asarray(docs, dtype=np.int64)
        ln = self.doc_len[docs]
        start = np.repeat(self.tok_off[docs], ln)
        within = np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
        return np.repeat(np.arange(docs.size, dtype=np.int64), ln), self.tok_term[start + within], ln


@functools.lru_cache(maxsize=1)
def corpus():
    return Corpus()


def n_terms_of(docs):
    """vocabulary size after the documents `docs`: new terms extend it at the end"""
    return int(corpus().tokens(docs)[1].max()) + 1 if len(docs) else 1


def twin_postings(docs, n_terms):
    from hiprag import build_postings
    d, t, ln = corpus().tokens(docs)
    return build_postings(d, t, len(docs), n_terms, ln)


def queries_for(n_terms, seed=5):
    """32 queries: the edge cases, then random ones over the planted and the Zipf terms"""
    rng = np.random.default_rng(seed)
    qs = [[], [n_terms + 5], [T_ALL, T_ALL, 7], [T_NONE], [T_ALL], [T_2047], [T_ONE, T_2047], [T_2047, T_ALL, n_terms + 1, 9]]
    while len(qs) < 32:
        m = int(rng.integers(1, 7))
        q = [int(min(n_terms - 1, 4 + int(rng.zipf(1.3)))) for _ in range(m)]
        if rng.random() < 0.4:
            q.insert(int(rng.integers(0, m + 1)), int(rng.choice([T_ALL, T_2047, T_ONE])))
        qs.append(q)
    return [np.asarray(q, dtype=np.uint32) for q in qs]


def scopes_for(n):
    c = lambda v: int(min(v, n))   # noqa: E731
    return [[(c(TILE - 216), c(TILE + 284))], [(c(100), c(200)), (c(TILE - 5), c(TILE + 700)), (c(TILE + 700), c(2 * TILE + 3))]]


def all_searches(bm, n_docs, n_terms):
    import torch
    qs = queries_for(n_terms)
    out = []
    soq = np.arange(len(qs), dtype=np.int32) % 2
    for k in (10, 64):
        out.extend(bm.search(qs, k))
        out.extend(bm.search_scoped(qs, k, scopes_for(n_docs), soq))
        out.extend(t.cpu().numpy() for t in bm.search_device(qs, k))
        out.extend(t.cpu().numpy() for t in bm.search_scoped_device(qs, k, scopes_for(n_docs), soq))
    torch.cuda.synchronize()
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_equals_twin(upd, docs, n_terms, tag, oracle=False):
    """export and every search output of `upd` against a fresh HipBM25 over build_postings of `docs`"""
    from hiprag import HipBM25
    assert not upd.dirty, f"{tag}: compare a committed handle"
    p = twin_postings(docs, n_terms)
    ex = upd.export()
    assert (ex["n_docs"], ex["n_terms"]) == (len(docs), n_terms), tag
    assert np.array_equal(ex["offsets"], p.offsets), f"{tag}: offsets"
    assert np.array_equal(ex["doc_ids"], p.doc_ids), f"{tag}: doc ids"
    assert np.array_equal(ex["tf"], p.tfs), f"{tag}: tf"
    assert np.array_equal(ex["doc_len"].astype(np.int64), p.doc_len), f"{tag}: doc_len"
    diff = int(np.sum(bits(ex["impacts"]) != bits(p.impacts)))
    print(f"{tag}: {len(docs)} documents, {p.doc_ids.size} postings, {diff} impacts differ from build_postings")
    assert diff == 0, f"{tag}: {diff} impacts differ in their bits"
    twin = HipBM25(p)
    got, want = all_searches(upd, len(docs), n_terms), all_searches(twin, len(docs), n_terms)
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(bits(g), bits(w)), f"{tag}: search output {j} differs from the twin's"
    if oracle:
        qs = queries_for(n_terms)
        es, ei = ho.bm25_search(ho.Postings(p.n_docs, p.n_terms, p.offsets, p.doc_ids, p.impacts), qs, 64)
        assert np.array_equal(got[11], ei) and np.array_equal(bits(got[10]), bits(es)), f"{tag}: differs from the oracle"
    twin.close()
    return ex


def updatable(docs, n_terms):
    from hiprag import HipBM25Updatable
    d, t, ln = corpus().tokens(docs)
    return HipBM25Updatable.from_tokens(d, t, len(docs), n_terms, ln)


def append_docs(upd, docs, n_terms_after):
    d, t, ln = corpus().tokens(docs)
    upd.append_tokens(d, t, len(docs), n_terms_after, ln)


def same_export(a, b):
    return all(np.array_equal(bits(a[key]), bits(b[key])) for key in ("offsets", "doc_ids", "tf", "impacts", "doc_len"))


# ---- create ------------------------------------------------------------------------------------------------------------
def test_create_tf_equals_the_twin(gpu):
    docs = np.arange(N_DOCS)
    p = twin_postings(docs, N_TERMS)
    df = np.diff(p.offsets.astype(np.int64))
    assert df[T_ALL] == N_DOCS and df[T_2047] == SKIP_MIN_DF - 1 and df[T_ONE] == 1 and df[T_NONE] == 0
    assert p.doc_len.min() == 1 and p.doc_len.max() == 300
    upd = updatable(docs, N_TERMS)
    assert upd.update_info()["kind"] == "create_tf" and not upd.dirty
    assert_equals_twin(upd, docs, N_TERMS, "create", oracle=True)
    upd.close()


# ---- append ------------------------------------------------------------------------------------------------------------
# the issue's batches, then a second run whose n_docs lands on 9215, 9216, 9217, 18432 (the second tile boundary), 18433
BATCHES = ((1, 31, 9215, 1, 9217, 1500), (9215, 1, 1, 9215, 1))


@pytest.mark.parametrize("sizes", BATCHES)
def test_append_from_an_empty_handle(gpu, sizes):
    from hiprag import HipBM25Updatable
    each, once = HipBM25Updatable(), HipBM25Updatable()     # commit after every batch / only after the last
    assert each.sizes() == {"n_docs": 0, "n_terms": 1, "postings": 0, "has_tf": True, "dirty": False}
    docs = np.zeros(0, np.int64)
    n_terms = 1
    for j, size in enumerate(sizes):
        batch = np.arange(docs.size, docs.size + size)
        if size == 1500:
            batch = np.append(batch, EXTRA_DOC)      # brings the 2048th posting of T_2047
        docs = np.append(docs, batch)
        n_terms = max(n_terms_of(docs), n_terms + 1)      # every batch brings new terms, one (still empty) at the least
        for h in (each, once):
            append_docs(h, batch, n_terms)
            assert h.dirty and h.update_info()["kind"] == "append" and h.update_info()["docs_after"] == docs.size
        each.commit()
        assert_equals_twin(each, docs, n_terms, f"append {j} (+{size})")
    if 1500 in sizes:
        df = np.diff(each.export()["offsets"].astype(np.int64))
        assert df[T_2047] == SKIP_MIN_DF, "T_2047 crossed kSkipMinDf with the last batch"
    assert once.dirty
    once.commit()
    assert_equals_twin(once, docs, n_terms, "one commit behind all batches")
    assert same_export(each.export(), once.export())
    each.close()
    once.close()


# ---- remove ------------------------------------------------------------------------------------------------------------
def test_remove_ranges_step_by_step(gpu):
    docs = np.arange(N_DOCS)
    upd = updatable(docs, N_TERMS)
    steps = [("first document", lambda n: [(0, 1)]),
             ("last document", lambda n: [(n - 1, n)]),
             ("across the tile boundary", lambda n: [(TILE - 216, TILE + 284)]),          # holds ONE_DOC: T_ONE loses its only posting
             ("one whole tile", lambda n: [(TILE, 2 * TILE)]),
             ("touching and empty ranges", lambda n: [(10, 20), (20, 30), (40, 40), (50, 60), (n, n)]),
             ("down to 1500 documents", lambda n: [(1000, n - 500)]),                       # T_ALL falls below kSkipMinDf
             ("every document", lambda n: [(0, n)])]
    for tag, make in steps:
        ranges = make(len(docs))
        before = upd.export()
        gone = np.zeros(len(docs), bool)
        for lo, hi in ranges:
            gone[lo:hi] = True
        removed = upd.remove_ranges(ranges)
        assert removed == int(gone.sum()) and upd.dirty
        info = upd.update_info()
        dead = np.flatnonzero(gone[before["doc_ids"]])
        survivors_behind = int(np.sum(~gone[before["doc_ids"][dead[0]:]])) if dead.size else 0
        assert info["kind"] == "remove_ranges" and info["postings_moved"] == survivors_behind, (tag, info, survivors_behind)
        assert info["postings_before"] - info["postings_after"] == dead.size and info["docs_after"] == len(docs) - removed
        docs = docs[~gone]
        upd.commit()
        ex = assert_equals_twin(upd, docs, N_TERMS, f"remove {tag}")
        df = np.diff(ex["offsets"].astype(np.int64))
        if tag == "across the tile boundary":
            assert df[T_ONE] == 0 and ex["n_terms"] == N_TERMS, "an emptied term keeps its id"
        if tag == "down to 1500 documents":
            assert df[T_ALL] == 1500 < SKIP_MIN_DF
    # a removal that removes nothing is a no-op and leaves the handle clean
    assert upd.remove_ranges([]) == 0 and not upd.dirty
    assert upd.remove_ranges([(0, 0)]) == 0 and not upd.dirty
    # and the emptied handle takes documents again
    docs = np.arange(300)
    append_docs(upd, docs, N_TERMS)
    upd.commit()
    assert_equals_twin(upd, docs, N_TERMS, "append into the emptied handle")
    upd.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def small_handle():
    docs = np.arange(600)
    return updatable(docs, N_TERMS), docs


def test_a_dirty_handle_refuses_every_search_entry(gpu):
    import torch
    from hiprag import HipFlatIndex, HipRagError, hybrid_search, hybrid_search_device, hybrid_search_scoped, hybrid_search_scoped_device
    upd, docs = small_handle()
    upd.auto_commit = False
    append_docs(upd, np.arange(600, 610), N_TERMS)
    assert upd.dirty
    n = 610
    ix = HipFlatIndex(64, "ip")
    x = ho.synthetic_vectors(n, 64, seed=3)
    ix.add(x)
    qs, q = [np.asarray([T_ALL], np.uint32)], x[:1]
    qd = torch.from_numpy(q).cuda()
    scope = [[(0, n)]]
    entries = [lambda: upd.search(qs, 5), lambda: upd.search_device(qs, 5), lambda: upd.search_scoped(qs, 5, scope),
               lambda: upd.search_scoped_device(qs, 5, scope), lambda: hybrid_search(ix, upd, q, qs, depth=5, k=5),
               lambda: hybrid_search_device(ix, upd, qd, qs, depth=5, k=5),
               lambda: hybrid_search_scoped(ix, upd, q, qs, scope, depth=5, k=5),
               lambda: hybrid_search_scoped_device(ix, upd, qd, qs, scope, depth=5, k=5)]
    for j, f in enumerate(entries):
        with pytest.raises(HipRagError, match="hipbm25_reweigh") as e:
            f()
        assert e.value.code == E_INVALID, j
    torch.cuda.synchronize()
    upd.commit()
    assert upd.search(qs, 5)[1][0, 0] >= 0                                    # searches run again
    upd.auto_commit = True
    append_docs(upd, np.arange(610, 612), N_TERMS)
    upd.search(qs, 5)                        # commits by itself
    assert not upd.dirty
    upd.close()
    ix.close()


def test_a_plain_handle_refuses_every_update_entry(gpu):
    from hiprag import HipBM25, HipRagError, _native as nat
    p = twin_postings(np.arange(50), N_TERMS)
    bm = HipBM25(p)
    off = np.zeros(N_TERMS + 1, np.uint64)
    r = np.asarray([[0, 1]], np.int64)
    for name, args in (("hipbm25_append", (0, N_TERMS, off.ctypes.data, None, None, None)),
                       ("hipbm25_remove_ranges", (r.ctypes.data, 1)), ("hipbm25_reweigh", (None,))):
        with pytest.raises(HipRagError) as e:
            nat.call(name, bm._h, *args)
        assert e.value.code == E_UNSUPPORTED and "hipbm25_create_tf" in str(e.value), name
    s, i = bm.search([np.asarray([T_ALL], np.uint32)], 5)
    assert i[0, 0] >= 0
    bm.close()


def test_bad_tables_and_batches_leave_the_handle_as_it_was(gpu):
    from hiprag import HipRagError, _native as nat
    upd, docs = small_handle()
    before = upd.export()
    n = len(docs)
    for ranges in ([(-1, 2)], [(5, 3)], [(0, n + 1)], [(10, 20), (15, 30)], [(30, 40), (10, 20)]):
        with pytest.raises(HipRagError) as e:
            upd.remove_ranges(ranges)
        assert e.value.code == E_INVALID, ranges
    with pytest.raises(HipRagError) as e:
        nat.call("hipbm25_remove_ranges", upd._h, None, 1)
    assert e.value.code == E_INVALID
    u32, u64 = np.uint32, np.uint64

    def batch(n_new, n_terms_after, off, ids, tf, dl):
        upd.append_postings(n_new, n_terms_after, np.asarray(off, u64), np.asarray(ids, u32), np.asarray(tf, u32), np.asarray(dl, u32))

    V = N_TERMS
    tail = [2] * V                                     # [0] + tail: offsets of a batch with two postings in term 0
    bad = [lambda: batch(2, V - 1, [0] + tail[:-1], [0, 1], [1, 1], [1, 1]),         # n_terms_after below n_terms
           lambda: batch(2, V, [1, 2] + tail[1:], [0, 1], [1, 1], [1, 1]),             # offsets do not start at 0
           lambda: batch(2, V, [0, 2, 1] + tail[2:], [0, 1], [1, 1], [1, 1]),          # offsets descend
           lambda: batch(2, V, [0] + tail, [1, 0], [1, 1], [1, 1]),                    # list not ascending
           lambda: batch(2, V, [0] + tail, [0, 0], [1, 1], [1, 1]),                    # ... not strictly
           lambda: batch(2, V, [0] + tail, [0, 2], [1, 1], [1, 1]),                    # doc id >= n_new_docs
           lambda: batch(2, V, [0] + tail, [0, 1], [1, 0], [1, 1])]                    # tf 0
    for j, f in enumerate(bad):
        with pytest.raises(HipRagError) as e:
            f()
        assert e.value.code == E_INVALID, j
    zeros = np.zeros(V + 1, u64)
    one = np.zeros(1, u32)
    with pytest.raises(HipRagError) as e:              # 2^32 documents: refused on the count alone, nothing is read
        nat.call("hipbm25_append", upd._h, 2 ** 32 - n, V, zeros.ctypes.data, None, None, one.ctypes.data)
    assert e.value.code == E_INVALID
    for args in ((2, V, None, None, None, one.ctypes.data), (2, V, zeros.ctypes.data, None, None, None)):
        with pytest.raises(HipRagError) as e:          # null offsets, null doc_len
            nat.call("hipbm25_append", upd._h, *args)
        assert e.value.code == E_INVALID
    assert not upd.dirty
    assert same_export(before, upd.export())
    assert_equals_twin(upd, docs, N_TERMS, "after the refused calls")
    upd.close()


# ---- determinism, NULL idf ---------------------------------------------------------------------------------------------
def test_the_same_updates_twice_give_identical_bytes(gpu):
    def run():
        upd = updatable(np.arange(12000), N_TERMS)
        append_docs(upd, np.arange(12000, 15000), N_TERMS)
        upd.remove_ranges([(5, 700), (TILE - 3, TILE + 9), (11000, 13000)])
        append_docs(upd, np.arange(15000, 15100), N_TERMS)
        upd.commit()
        ex = upd.export()
        upd.close()
        return ex
    assert same_export(run(), run())


def test_null_idf_gives_numpy_impacts_or_their_fp32_neighbours(gpu):
    docs = np.arange(N_DOCS)
    upd = updatable(docs, N_TERMS)
    want = upd.export()["impacts"]
    upd.commit(library_idf=True)
    got = upd.export()["impacts"]
    differ = got != want
    print(f"NULL idf: {int(differ.sum())} of {got.size} impacts differ from numpy's")
    up, down = np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))
    assert np.all((got == want) | (got == up) | (got == down))
    upd.close()


# ---- hybrid ------------------------------------------------------------------------------------------------------------
def test_scoped_hybrid_over_an_updated_pair_equals_the_twins(gpu):
    from hiprag import HipBM25, HipFlatIndex, hybrid_search_scoped
    d = 64
    x = ho.synthetic_vectors(N_DOCS, d, seed=77)
    docs = np.arange(N_DOCS)
    upd = updatable(docs, N_TERMS)
    ix = HipFlatIndex(d, "ip")
    ix.add(x)
    ranges = [(3, 40), (TILE - 100, TILE + 50), (15000, 15700)]
    gone = np.zeros(N_DOCS, bool)
    for lo, hi in ranges:
        gone[lo:hi] = True
    upd.remove_ranges(ranges)          # left dirty: the first hybrid call below commits by itself
    ix.remove_ranges(ranges)
    docs = docs[~gone]
    twin_bm = HipBM25(twin_postings(docs, N_TERMS))
    twin_ix = HipFlatIndex(d, "ip")
    twin_ix.add(np.ascontiguousarray(x[~gone]))
    qs = queries_for(N_TERMS)
    q = ho.synthetic_queries(len(qs), d, seed=78)
    soq = np.arange(len(qs), dtype=np.int32) % 2
    for depth, k in ((10, 10), (64, 20)):
        got = hybrid_search_scoped(ix, upd, q, qs, scopes_for(len(docs)), soq, depth=depth, k=k, return_lists=True)
        want = hybrid_search_scoped(twin_ix, twin_bm, q, qs, scopes_for(len(docs)), soq, depth=depth, k=k, return_lists=True)
        flat = lambda r: [r[0], r[1], r[2][0][0], r[2][0][1], r[2][1][0], r[2][1][1]]   # noqa: E731
        for j, (g, w) in enumerate(zip(flat(got), flat(want))):
            assert np.array_equal(bits(g), bits(w)), (depth, k, j)
    for h in (upd, ix, twin_bm, twin_ix):
        h.close()
