"""
The sparse score of given documents (libhiprag hipbm25_score_ids*, HipBM25.score_ids*).  The expected value is
hiprag.sparse.bm25_score_ids_reference (numpy, float32 throughout), and for the documents a search returns it is what
hipbm25_search_weighted returns for them.  Every comparison is exact: bit patterns equal.

The collection: 3000 documents, 150 terms -- lists of 0, 1 and 2 postings, of 2047 / 2048 / 2049 (the skip-table threshold),
one holding every document, the rest of 1 to 400 postings; documents 0 and 2999 are the first and the last entry of lists;
random fp32 impacts and weights, so the order of the adds and the rounding of the product show in the bits
(tests/test_bm25_score_ids_cpu.py asserts that of the recipe).  Two tiny collections of 1 and 7 documents beside it.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_INVALID = -1   # include/hiprag.h
F32_MAX = np.finfo(np.float32).max
N_DOCS = 3000
N_TERMS = 150
T_EMPTY, T_ONE, T_TWO, T_2047, T_2048, T_2049, T_ALL, T_GAP = 0, 1, 2, 3, 4, 5, 6, 7
DEPTHS = (1, 3, 4, 5, 63, 64, 65, 200)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_postings(n_docs, n_terms, lists, rng):
    from hiprag import PostingsCSR
    off = np.zeros(n_terms + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists]).astype(np.uint64)
    ids = np.concatenate(lists).astype(np.uint32) if int(off[-1]) else np.zeros(0, np.uint32)
    imp = np.exp(rng.normal(0.0, 2.0, size=int(off[-1]))).astype(np.float32)
    return PostingsCSR(n_docs, n_terms, off, ids, imp)


@functools.lru_cache(maxsize=None)
def collection():
    rng = np.random.default_rng(4242)
    pick = lambda n: np.sort(rng.choice(N_DOCS, size=n, replace=False))
    lists = [np.zeros(0, np.int64) for _ in range(N_TERMS)]
    lists[T_ONE] = np.array([0])                                   # document 0 is a whole list
    lists[T_TWO] = np.array([0, N_DOCS - 1])                       # first and last document, first and last entry
    lists[T_2047], lists[T_2048], lists[T_2049] = pick(2047), pick(2048), pick(2049)
    lists[T_ALL] = np.arange(N_DOCS)
    lists[T_GAP] = np.array([10, 12, 500, 502, N_DOCS - 1])        # 11 and 501 are absent between two present documents
    for t in range(8, N_TERMS):
        lists[t] = pick(int(rng.integers(1, 401)))
    return make_postings(N_DOCS, N_TERMS, lists, rng)


@functools.lru_cache(maxsize=None)
def queries():
    """0, 1, 63, 64, 65 and 130 slots; the 65-slot query holds term T_2048 twice with two weights; the 130-slot one ends in
    a term id >= n_terms; the special lists are spread over them."""
    rng = np.random.default_rng(99)
    qs = [[], [T_GAP]]
    for n in (63, 64, 65, 130):
        qs.append(rng.integers(0, N_TERMS, size=n).tolist())
    qs[2][:4] = [T_EMPTY, T_ONE, T_TWO, T_2047]
    qs[3][:3] = [T_2049, T_ALL, T_GAP]
    qs[4][0], qs[4][40] = T_2048, T_2048
    qs[5][-1] = N_TERMS + 9
    qs[5][64], qs[5][65], qs[5][129 - 1] = T_2047, T_2048, T_TWO   # special lists in the second and third pass of 64 slots
    ws = [rng.uniform(0.05, 2.0, size=len(q)).astype(np.float32) for q in qs]
    assert ws[4][0] != ws[4][40]
    return qs, ws


def special_ids(base, n_docs):
    """-1, base - 1, base + n_docs, the same id twice, first / last document, ids around the gaps of T_GAP"""
    return [-1, base - 1, base + n_docs, base + 12, base + 12, base, base + n_docs - 1, base + 11, base + 10, base + 501, base + 502]


def ids_for(nq, depth, base, n_docs, seed):
    rng = np.random.default_rng(seed)
    ids = base + rng.integers(0, n_docs, size=(nq, depth)).astype(np.int64)
    sp = special_ids(base, n_docs)
    for b in range(nq):
        n = min(depth, len(sp))
        where = rng.choice(depth, size=n, replace=False)
        ids[b, where] = sp[:n] if b % 2 == 0 else sp[::-1][:n]
    ids[nq - 1] = np.sort(ids[nq - 1])[::-1]                        # descending order
    return ids


@pytest.fixture(scope="module")
def index(gpu):
    from hiprag import HipBM25
    ix = HipBM25(collection())
    yield ix
    ix.close()


@functools.lru_cache(maxsize=None)
def reference_all():
    """the reference score of every document for every query, weighted and unweighted: computed once"""
    from hiprag import bm25_score_ids_reference
    qs, ws = queries()
    every = np.tile(np.arange(N_DOCS, dtype=np.int64), (len(qs), 1))
    return bm25_score_ids_reference(collection(), qs, ws, every), bm25_score_ids_reference(collection(), qs, None, every)


def expected(qsel, ids, base, weighted=True):
    ref = reference_all()[0 if weighted else 1]
    out = np.full(ids.shape, -F32_MAX, dtype=np.float32)
    for b, q in enumerate(qsel):
        local = ids[b] - base
        ok = (ids[b] >= 0) & (local >= 0) & (local < N_DOCS)
        out[b, ok] = ref[q, local[ok]]
    return out


@pytest.mark.parametrize("depth", DEPTHS)
def test_every_depth_matches_the_reference(index, depth):
    import torch
    qs, ws = queries()
    ids = ids_for(len(qs), depth, 0, N_DOCS, seed=depth)
    want = expected(range(len(qs)), ids, 0)
    got = index.score_ids(qs, ids, ws)
    assert np.array_equal(bits(got), bits(want))
    info = index.score_info()
    local_ok = (ids >= 0) & (ids < N_DOCS)
    lens = np.diff(collection().offsets.astype(np.int64))
    nonempty = [sum(1 for t in q if t < N_TERMS and lens[t] > 0) for q in qs]
    chunk = 4
    while chunk < 64 and len(qs) * -(-depth // chunk) > 4096:
        chunk *= 2
    assert info == {"valid": int(local_ok.sum()), "padding": int((~local_ok).sum()), "workgroups": len(qs) * -(-depth // chunk),
                    "probes": int(sum(int(local_ok[b].sum()) * nonempty[b] for b in range(len(qs))))}
    dev = index.score_ids_device(qs, torch.from_numpy(ids).cuda(), ws)
    torch.cuda.synchronize()
    assert np.array_equal(bits(dev.cpu().numpy()), bits(got))       # the host entry agrees with the device entry


@pytest.mark.parametrize("nq", (1, 2, 33))
def test_every_batch_size_and_a_nonzero_id_base(gpu, nq):
    from hiprag import HipBM25
    base = 70000
    qs, ws = queries()
    sel = [(3 + b) % len(qs) for b in range(nq)]
    ix = HipBM25(collection(), id_base=base)
    try:
        ids = ids_for(nq, 65, base, N_DOCS, seed=100 + nq)
        got = ix.score_ids([qs[q] for q in sel], ids, [ws[q] for q in sel])
        assert np.array_equal(bits(got), bits(expected(sel, ids, base)))
        assert (got[ids == base - 1] == -F32_MAX).all() and (got[ids == base + N_DOCS] == -F32_MAX).all()
    finally:
        ix.close()


def test_unweighted_null_and_all_ones(index):
    qs, ws = queries()
    ids = ids_for(len(qs), 64, 0, N_DOCS, seed=5)
    plain = index.score_ids(qs, ids)
    ones = index.score_ids(qs, ids, [np.ones(len(q), np.float32) for q in qs])
    assert np.array_equal(bits(plain), bits(ones))
    assert np.array_equal(bits(plain), bits(expected(range(len(qs)), ids, 0, weighted=False)))


def test_same_bits_as_the_searches(index):
    """every document hipbm25_search_weighted returns (k = 1000: the global-accumulator form; k = 64: the tiled kernel, for
    the queries it takes) has the bits score_ids gives it; the unweighted search likewise"""
    qs, ws = queries()
    for k, sel in ((1000, range(1, len(qs))), (64, range(1, 4))):
        sq, sw = [qs[q] for q in sel], [ws[q] for q in sel]
        s, i = index.search_weighted(sq, sw, k)
        assert (i >= 0).any(axis=1).all()
        got = index.score_ids(sq, np.where(i >= 0, i, -1), sw)
        assert np.array_equal(bits(got), bits(s))                   # padding ranks: -FLT_MAX on both sides
        s, i = index.search(sq, k)
        got = index.score_ids(sq, np.where(i >= 0, i, -1))
        assert np.array_equal(bits(got), bits(s))


@pytest.mark.parametrize("n_docs", (1, 7))
def test_tiny_collections(gpu, n_docs):
    from hiprag import HipBM25, bm25_score_ids_reference
    rng = np.random.default_rng(n_docs)
    lists = [np.zeros(0, np.int64), np.array([0]), np.array([n_docs - 1]), np.arange(n_docs), np.sort(rng.choice(n_docs, size=(n_docs + 1) // 2, replace=False))]
    p = make_postings(n_docs, len(lists), lists, rng)
    qs = [[3, 1, 4, 2, 0, 3], [], [9]]
    ws = [rng.uniform(0.05, 2.0, size=len(q)).astype(np.float32) for q in qs]
    ids = np.array([[0, n_docs - 1, n_docs, -1, 0], [0, n_docs - 1, n_docs, -1, 0], [n_docs - 1, 0, 0, -5, n_docs]], dtype=np.int64)
    ix = HipBM25(p)
    try:
        got = ix.score_ids(qs, ids, ws)
        assert np.array_equal(bits(got), bits(bm25_score_ids_reference(p, qs, ws, ids)))
        assert got[1].tolist() == [0.0, 0.0, -F32_MAX, -F32_MAX, 0.0]
    finally:
        ix.close()


def test_tf_handle_after_append_remove_reweigh_and_dirty_refusal(gpu):
    from hiprag import HipBM25Updatable, HipRagError, PostingsCSR, bm25_score_ids_reference
    rng = np.random.default_rng(11)
    n, v = 600, 30
    docs = rng.integers(0, n, size=9000)
    terms = rng.integers(0, v, size=9000)
    ix = HipBM25Updatable.from_tokens(docs, terms, n, v)
    try:
        ix.auto_commit = False
        ix.append_tokens(rng.integers(0, 200, size=3000), rng.integers(0, v + 4, size=3000), 200, v + 4)
        qs = [rng.integers(0, v + 4, size=8).tolist(), [1, 1, 2]]
        ws = [rng.uniform(0.05, 2.0, size=len(q)).astype(np.float32) for q in qs]
        ids = rng.integers(-2, 700, size=(2, 40)).astype(np.int64)
        with pytest.raises(HipRagError) as e:                       # dirty: changed and not reweighed
            ix.score_ids(qs, ids, ws)
        assert e.value.code == E_INVALID and "hipbm25_reweigh" in str(e.value)
        ix.remove_ranges([(5, 60), (300, 301), (790, 800)])
        ix.commit()
        ex = ix.export()
        p = PostingsCSR(ex["n_docs"], ex["n_terms"], ex["offsets"], ex["doc_ids"], ex["impacts"])
        assert p.n_docs == 800 - 55 - 1 - 10
        ids = rng.integers(-2, p.n_docs + 3, size=(2, 70)).astype(np.int64)
        assert np.array_equal(bits(ix.score_ids(qs, ids, ws)), bits(bm25_score_ids_reference(p, qs, ws, ids)))
    finally:
        ix.close()


def test_impact_handle_after_append_rows_and_remove(gpu):
    import torch
    from hiprag import LexicalIndexUpdatable, bm25_score_ids_reference
    rng = np.random.default_rng(12)
    n, L, v = 300, 24, 90
    terms = np.full((n, L), -1, dtype=np.int32)
    weights = np.zeros((n, L), dtype=np.float32)
    counts = rng.integers(0, L + 1, size=n).astype(np.int32)
    for i in range(n):
        terms[i, :counts[i]] = np.sort(rng.choice(v, size=counts[i], replace=False))
        weights[i, :counts[i]] = rng.uniform(0.01, 1.0, size=counts[i])
    lex = LexicalIndexUpdatable(n_terms=v)
    try:
        for lo in (0, 180):
            hi = 180 if lo == 0 else n
            lex.append_rows(torch.from_numpy(terms[lo:hi]).cuda(), torch.from_numpy(weights[lo:hi]).cuda(), torch.from_numpy(counts[lo:hi]).cuda(), v)
        lex.remove_ranges([(0, 3), (100, 140)])
        p = lex.postings()
        assert p.n_docs == n - 43
        qs = [rng.integers(0, v, size=20).tolist(), [], rng.integers(0, v + 5, size=70).tolist()]
        ws = [rng.uniform(0.05, 2.0, size=len(q)).astype(np.float32) for q in qs]
        ids = rng.integers(-2, p.n_docs + 3, size=(3, 65)).astype(np.int64)
        got = lex.bm.score_ids(qs, ids, ws)
        assert np.array_equal(bits(got), bits(bm25_score_ids_reference(p, qs, ws, ids)))
        assert (got[(ids >= 0) & (ids < p.n_docs)] >= 0).all() and (got > 0).any()
    finally:
        lex.close()


def test_every_invalid_argument_is_refused(index):
    import hiprag._native as nat
    from hiprag import HipRagError
    terms = np.array([1, 2, 3], dtype=np.uint32)
    wts = np.array([1.0, 0.5, 2.0], dtype=np.float32)
    qoff = np.array([0, 3], dtype=np.int32)
    ids = np.array([[0, 1, 2, 3]], dtype=np.int64)
    out = np.zeros((1, 4), dtype=np.float32)
    T, W, Q, I, O = terms.ctypes.data, wts.ctypes.data, qoff.ctypes.data, ids.ctypes.data, out.ctypes.data
    nat.call("hipbm25_score_ids", index._h, T, W, Q, 1, I, 4, O)     # the baseline is accepted
    bad_w = [np.array([1.0, x, 2.0], dtype=np.float32) for x in (0.0, -1.0, np.nan, np.inf)]
    down = np.array([3, 0], dtype=np.int32)
    neg = np.array([-1, 2], dtype=np.int32)
    cases = {"nq 0": (T, W, Q, 0, I, 4, O), "depth 0": (T, W, Q, 1, I, 0, O), "null q_offsets": (T, W, None, 1, I, 4, O),
             "null ids": (T, W, Q, 1, None, 4, O), "null out": (T, W, Q, 1, I, 4, None), "null terms": (None, W, Q, 1, I, 4, O),
             "descending q_offsets": (T, W, down.ctypes.data, 1, I, 4, O), "negative q_offsets": (T, W, neg.ctypes.data, 1, I, 4, O),
             "nq x depth 2^31": (T, W, Q, 1 << 16, I, 1 << 15, O)}
    for j, w in enumerate(bad_w):
        cases[f"weight {j}"] = (T, w.ctypes.data, Q, 1, I, 4, O)
    for name, args in cases.items():
        for fn in ("hipbm25_score_ids", "hipbm25_score_ids_dev"):
            with pytest.raises(HipRagError) as e:
                nat.call(fn, index._h, *args, *(() if fn == "hipbm25_score_ids" else (None,)))
            assert e.value.code == E_INVALID, (name, fn)
    with pytest.raises(HipRagError) as e:
        nat.call("hipbm25_score_info", index._h, None)
    assert e.value.code == E_INVALID
    with pytest.raises(HipRagError) as e:
        nat.call("hipbm25_score_ids", ctypes.c_uint64(987654321), T, W, Q, 1, I, 4, O)
    assert e.value.code == -3                                       # HIPRAG_E_HANDLE
