"""
Scoped BM25 (libhiprag hipbm25_search_scoped*, HipBM25.search_scoped*): the BM25 top k of every query among the documents
of ITS scope -- a few half-open document ranges of one collection's postings -- scored with the collection's impacts.
The expected value is the CPU oracle: ho.bm25_scores_taat, out-of-scope documents set to 0, ho.topk_desc_id_asc(...,
exclude_nonpositive=True).  Every comparison is exact: ids equal, fp32 score bit patterns equal.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

E_INVALID = -1   # include/hiprag.h
F32_MAX = np.finfo(np.float32).max
F64_MAX = np.finfo(np.float64).max
N_TERMS = 8192   # Zipf over 8192 terms: from 9216 documents on the frequent terms have lists beyond 2048 postings (skip tables), the rare ones not
COLLECTIONS = (700, 9216, 9217, 60000, 300000)
KS = (1, 10, 50, 64)
NQS = (1, 17, 1000)


@functools.lru_cache(maxsize=2)
def postings(n_docs, n_terms=N_TERMS, seed=777):
    return ho.synthetic_postings(n_docs, n_terms=n_terms, seed=seed)


def handle(p, id_base=0):
    from hiprag import HipBM25, PostingsCSR
    return HipBM25(PostingsCSR(p.n_docs, p.n_terms, p.offsets, p.doc_ids, p.impacts), id_base=id_base)


def random_scope(rng, n, n_ranges):
    """n_ranges ranges at random (hence unaligned) cut points, ascending"""
    n_ranges = min(n_ranges, (n + 1) // 2)
    cuts = np.sort(rng.choice(n + 1, size=2 * n_ranges, replace=False))
    return [(int(cuts[2 * j]), int(cuts[2 * j + 1])) for j in range(n_ranges)]


def scope_mask(n, scope):
    m = np.zeros(n, dtype=bool)
    for lo, hi in scope:
        m[lo:hi] = True
    return m


def oracle_scoped(p, queries, k, scopes, soq, id_base=0):
    """the oracle's scores with every document outside the query's scope set to 0, then its top k of the positive ones"""
    S = np.empty((len(queries), k), dtype=np.float32)
    I = np.empty((len(queries), k), dtype=np.int64)
    masks = [scope_mask(p.n_docs, s) for s in scopes]
    for b, qt in enumerate(queries):
        sc = ho.bm25_scores_taat(p, qt)
        sc[~masks[int(soq[b])]] = 0
        S[b], I[b] = ho.topk_desc_id_asc(sc, k, exclude_nonpositive=True, id_base=id_base)
    return S, I


def same_bits(s, i, es, ei):
    return np.array_equal(i, ei) and np.array_equal(s.view(np.uint32), es.view(np.uint32))


def bits_equal(a, b):
    """two (scores64, scores32, ids) device triples: equal ids, equal score BIT PATTERNS"""
    import torch
    return (torch.equal(a[2], b[2]) and torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
            and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def tiles_touched(scope, tile_docs):
    t = set()
    for lo, hi in scope:
        if hi > lo:
            t.update(range(lo // tile_docs, (hi - 1) // tile_docs + 1))
    return len(t)


def best_document(p, query):
    sc = ho.bm25_scores_taat(p, query)
    return int(np.lexsort((np.arange(p.n_docs), -sc.astype(np.float64)))[0]), sc


# ---- 1. the oracle, masked --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_docs", COLLECTIONS)
def test_oracle_parity(gpu, n_docs):
    p = postings(n_docs)
    long_lists = int(np.sum(np.diff(p.offsets.astype(np.int64)) >= 2048))
    print(f"n_docs={n_docs}: {long_lists} lists with skip tables, {p.n_terms - long_lists} without")
    if n_docs >= 9216:
        assert 0 < long_lists < p.n_terms
    bm = handle(p)
    rng = np.random.default_rng(n_docs)
    for nq in NQS:
        queries = ho.synthetic_sparse_queries(nq, n_terms=N_TERMS, seed=900 + nq)
        n_scopes = min(nq, 6)
        scopes = [random_scope(rng, n_docs, int(rng.integers(1, 41))) for _ in range(n_scopes)]
        soq = rng.integers(0, n_scopes, size=nq).astype(np.int32)     # several queries name one scope
        es, ei = oracle_scoped(p, queries, max(KS), scopes, soq)
        for k in KS:
            s, i = bm.search_scoped(queries, k, scopes, soq)
            assert same_bits(s, i, es[:, :k], ei[:, :k]), f"n_docs={n_docs} nq={nq} k={k}: differs from the oracle"
        work = sum(tiles_touched(scopes[int(x)], bm.scoped_info()["tile_docs"]) for x in soq)
        assert bm.scoped_info()["work_items"] == work
    bm.close()


# ---- 2. edges of a range ----------------------------------------------------------------------------------------------
def edge_collection():
    return postings(30000)


def test_scope_edges(gpu):
    p = edge_collection()
    n = p.n_docs
    bm = handle(p)
    T = bm.scoped_info()["tile_docs"]
    assert 2 * T < n < 4 * T and n % T != 0
    queries = ho.synthetic_sparse_queries(12, n_terms=N_TERMS, seed=5)
    scopes = [
        [(T + 10, T + 11), (T + 50, T + 700), (T + 701, T + 702), (T + 3000, T + 3001), (2 * T - 40, 2 * T - 1)],   # inside one tile, gaps
        [(T - 1, T + 1)],                     # straddles a tile boundary by one document on each side
        [(2 * T - 1, 2 * T + 1), (n - 1, n)],
        [(777, 778)],                         # one document
        [],                                   # no document
        [(5, 5)],                             # no document either
        [(n - 300, n)],                       # ends at n_docs in the partial last tile
        [(0, 100), (100, 200), (200, 200), (200, 9300), (9300, 9300)],   # touching and empty ranges
        [(0, n)],
    ]
    for k in (1, 10, 64):
        for s, scope in enumerate(scopes):
            es, ei = oracle_scoped(p, queries, k, [scope], np.zeros(len(queries), np.int32))
            gs, gi = bm.search_scoped(queries, k, [scope])
            assert same_bits(gs, gi, es, ei), f"scope {s} k={k}"
            if not any(hi > lo for lo, hi in scope):
                assert np.all(gi == -1) and np.all(gs == -F32_MAX)
                assert bm.scoped_info()["work_items"] == 0
    # all scopes in one call, one per query
    soq = (np.arange(len(queries)) % len(scopes)).astype(np.int32)
    es, ei = oracle_scoped(p, queries, 10, scopes, soq)
    gs, gi = bm.search_scoped(queries, 10, scopes, soq)
    assert same_bits(gs, gi, es, ei)
    bm.close()


def test_best_document_just_outside_never_appears(gpu):
    p = edge_collection()
    bm = handle(p)
    cases = []
    for qseed in range(1, 40):       # queries whose best document leaves room for a range on either side
        query = ho.synthetic_sparse_queries(1, n_terms=N_TERMS, seed=qseed)
        top, _ = best_document(p, query[0])
        if 1000 < top < p.n_docs - 1000:
            cases.append((query, top))
    assert len(cases) >= 3
    for query, top in cases[:3]:
        for k in (1, 10):
            lo, hi = top + 1, top + 900              # the best document of the collection sits at lo - 1
            _, gi = bm.search_scoped(query, k, [[(lo, hi)]])
            assert top not in gi
            _, gi = bm.search_scoped(query, k, [[(lo - 1, hi)]])
            assert gi[0, 0] == top
            lo, hi = top - 900, top                  # ... and at hi
            _, gi = bm.search_scoped(query, k, [[(lo, hi)]])
            assert top not in gi
            _, gi = bm.search_scoped(query, k, [[(lo, hi + 1)]])
            assert gi[0, 0] == top
    bm.close()


# ---- 3. queries ---------------------------------------------------------------------------------------------------------
def test_query_forms(gpu):
    p = edge_collection()
    n = p.n_docs
    bm = handle(p)
    df = np.diff(p.offsets.astype(np.int64))
    long_terms = np.nonzero(df >= 2048)[0]
    short_terms = np.nonzero((df > 0) & (df < 2048))[0]
    assert len(long_terms) >= 6 and len(short_terms) >= 6
    rng = np.random.default_rng(3)
    many = rng.choice(N_TERMS, size=150, replace=False).astype(np.uint32)     # 150 terms: three batches of slots
    queries = [
        np.zeros(0, np.uint32),                                               # empty
        np.asarray([N_TERMS + 5, 4000000000], np.uint32),                     # unknown terms only
        np.asarray([long_terms[0], short_terms[3], long_terms[0]], np.uint32),   # a duplicated term adds again
        long_terms[:6].astype(np.uint32),
        short_terms[-6:].astype(np.uint32),
        many,
        np.concatenate([many[:64], many[:1]]).astype(np.uint32),              # 65 terms: one past a batch
    ]
    scopes = [[(123, 20011)], [(0, n)], [(9000, 9500), (18000, 18600), (29000, n)]]
    for k in (1, 50, 64):
        for scope in scopes:
            es, ei = oracle_scoped(p, queries, k, [scope], np.zeros(len(queries), np.int32))
            gs, gi = bm.search_scoped(queries, k, [scope])
            assert same_bits(gs, gi, es, ei), f"k={k} scope={scope}"
            assert np.all(gi[:2] == -1) and np.all(gs[:2] == -F32_MAX)
        # at full scope the unscoped entry answers the long queries with its global-accumulator form: same result
        us, ui = bm.search(queries, k)
        gs, gi = bm.search_scoped(queries, k, [[(0, n)]])
        assert same_bits(gs, gi, us, ui)
    bm.close()


# ---- 4. the same bits as the unscoped entry and as a shard ----------------------------------------------------------------
@pytest.mark.parametrize("n_docs", (9217, 60000))
def test_full_scope_equals_unscoped_bit_for_bit(gpu, n_docs):
    import torch
    p = postings(n_docs)
    for id_base in (0, 1 << 33):
        bm = handle(p, id_base=id_base)
        for nq, k in ((1, 1), (17, 10), (300, 50), (64, 64)):
            queries = ho.synthetic_sparse_queries(nq, n_terms=N_TERMS, seed=nq)
            a = bm.search_device(queries, k)
            b = bm.search_scoped_device(queries, k, [[(0, n_docs)]])
            torch.cuda.synchronize()
            assert bits_equal(a, b)
            assert id_base == 0 or int(b[2].max()) >= id_base
            pad = b[2] < 0
            assert torch.all(b[0][pad] == -F64_MAX) and torch.all(b[1][pad] == -F32_MAX)
        bm.close()


def test_range_equals_shard_bit_for_bit(gpu):
    import torch
    from hiprag import HipBM25, PostingsCSR
    p = postings(60000)
    csr = PostingsCSR(p.n_docs, p.n_terms, p.offsets, p.doc_ids, p.impacts)
    bm = HipBM25(csr)
    queries = ho.synthetic_sparse_queries(40, n_terms=N_TERMS, seed=77)
    for lo, hi in ((0, 37), (9215, 9218), (12345, 43210), (59000, 60000)):
        shard = HipBM25(csr.shard(lo, hi), id_base=lo)
        for k in (1, 10, 64):
            a = shard.search_device(queries, k)
            b = bm.search_scoped_device(queries, k, [[(lo, hi)]])
            torch.cuda.synchronize()
            assert bits_equal(a, b), f"[{lo}, {hi}) k={k}"
        shard.close()
    bm.close()


def test_two_runs_and_two_streams_identical(gpu):
    import torch
    p = postings(60000)
    bm = handle(p)
    rng = np.random.default_rng(8)
    queries = ho.synthetic_sparse_queries(200, n_terms=N_TERMS, seed=21)
    scopes = [random_scope(rng, p.n_docs, 12) for _ in range(5)]
    soq = rng.integers(0, 5, size=200).astype(np.int32)
    a = bm.search_scoped_device(queries, 50, scopes, soq)
    b = bm.search_scoped_device(queries, 50, scopes, soq)
    torch.cuda.synchronize()
    assert bits_equal(a, b)
    # a call on a second stream right after one on the first: the handle's one workspace is handed over in order
    other = ho.synthetic_sparse_queries(200, n_terms=N_TERMS, seed=22)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        c = bm.search_scoped_device(queries, 50, scopes, soq)
    with torch.cuda.stream(s2):
        d = bm.search_scoped_device(other, 50, scopes[:1])
    torch.cuda.synchronize()
    assert bits_equal(a, c)
    es, ei = oracle_scoped(p, other, 50, scopes[:1], np.zeros(200, np.int32))
    assert same_bits(d[1].cpu().numpy(), d[2].cpu().numpy(), es, ei)
    bm.close()


# ---- 5. cost follows the scope; chunks ---------------------------------------------------------------------------------
def test_work_items_follow_the_scope(gpu):
    p = postings(300000)
    bm = handle(p)
    T = bm.scoped_info()["tile_docs"]
    ntiles = -(-p.n_docs // T)
    queries = ho.synthetic_sparse_queries(64, n_terms=N_TERMS, seed=31)
    scopes = [[(100000, 103000)], [(0, p.n_docs)], [(T - 1, T + 1), (20 * T, 20 * T + 5)], []]
    soq = (np.arange(64) % 4).astype(np.int32)
    es, ei = oracle_scoped(p, queries, 10, scopes, soq)
    gs, gi = bm.search_scoped(queries, 10, scopes, soq)
    assert same_bits(gs, gi, es, ei)
    info = bm.scoped_info()
    per_scope = [tiles_touched(s, T) for s in scopes]
    assert per_scope == [tiles_touched([(100000, 103000)], T), ntiles, 3, 0] and per_scope[0] <= 2
    assert info["work_items"] == sum(per_scope[int(s)] for s in soq)
    assert info["max_scope_tiles"] == ntiles and info["chunks"] == 1
    bm.search_scoped(queries[:8], 10, scopes[:1])
    assert bm.scoped_info()["work_items"] == 8 * per_scope[0]        # 1 % of the collection: its tiles, not the collection's
    bm.close()


def test_chunked_call_gives_the_same_bits(gpu, monkeypatch):
    """a workspace budget of 1 MiB cuts the batch into chunks of queries: same result, a chunk per few queries"""
    p = postings(60000)
    rng = np.random.default_rng(4)
    queries = ho.synthetic_sparse_queries(100, n_terms=N_TERMS, seed=41)
    scopes = [random_scope(rng, p.n_docs, 20), [(0, p.n_docs)], [(100, 140)]]
    soq = rng.integers(0, 3, size=100).astype(np.int32)
    es, ei = oracle_scoped(p, queries, 64, scopes, soq)
    monkeypatch.setenv("HIPBM25_SCOPED_BUDGET_MIB", "1")
    bm = handle(p)
    gs, gi = bm.search_scoped(queries, 64, scopes, soq)
    assert same_bits(gs, gi, es, ei)
    info = bm.scoped_info()
    assert info["chunks"] > 1
    assert info["work_items"] == sum(tiles_touched(scopes[int(s)], info["tile_docs"]) for s in soq)
    bm.close()


# ---- 6. validation --------------------------------------------------------------------------------------------------------
def test_validation_returns_e_invalid(gpu):
    import torch
    from hiprag import HipRagError, _native as nat
    p = postings(9217)
    bm = handle(p)
    n = p.n_docs
    queries = ho.synthetic_sparse_queries(3, n_terms=N_TERMS, seed=1)

    def rejected(fn, needle):
        with pytest.raises(HipRagError) as e:
            fn()
        assert e.value.code == E_INVALID and needle in str(e.value), str(e.value)

    rejected(lambda: bm.search_scoped(queries, 65, [[(0, n)]]), "k must be in 1..64")
    rejected(lambda: bm.search_scoped(queries, 0, [[(0, n)]]), "k must be in 1..64")
    rejected(lambda: bm.search_scoped(queries, 5, [[(10, 5)]]), "is not within")
    rejected(lambda: bm.search_scoped(queries, 5, [[(100, 200), (50, 60)]]), "ascend and do not overlap")
    rejected(lambda: bm.search_scoped(queries, 5, [[(100, 200), (199, 300)]]), "ascend and do not overlap")
    rejected(lambda: bm.search_scoped(queries, 5, [[(0, n + 1)]]), "is not within")
    rejected(lambda: bm.search_scoped(queries, 5, [[(-1, 4)]]), "is not within")
    rejected(lambda: bm.search_scoped(queries, 5, [[(0, 5)]], [0, 1, 0]), "is not a scope")
    rejected(lambda: bm.search_scoped(queries, 5, [[(0, 5)]], [0, -1, 0]), "is not a scope")
    # null tables, straight through the C-ABI
    terms, qoff = bm._flatten(queries)
    ranges = np.asarray([[0, 5]], np.int64)
    offs = np.asarray([0, 1], np.int32)
    soq = np.zeros(3, np.int32)
    out = (torch.empty((3, 5), dtype=torch.float64, device="cuda"), torch.empty((3, 5), dtype=torch.float32, device="cuda"),
           torch.empty((3, 5), dtype=torch.int64, device="cuda"))

    def raw(r, o, s, ids=out[2].data_ptr(), nq=3, n_scopes=1, qo=qoff.ctypes.data):
        nat.call("hipbm25_search_scoped_dev", bm._h, terms.ctypes.data, qo, nq, 5, r, o, n_scopes, s, out[0].data_ptr(),
                 out[1].data_ptr(), ids, None)

    rejected(lambda: raw(None, offs.ctypes.data, soq.ctypes.data), "ranges is null")
    rejected(lambda: raw(ranges.ctypes.data, None, soq.ctypes.data), "scope_offsets is null")
    rejected(lambda: raw(ranges.ctypes.data, offs.ctypes.data, None), "scope_of_query is null")
    rejected(lambda: raw(ranges.ctypes.data, offs.ctypes.data, soq.ctypes.data, ids=None), "out_ids is null")
    rejected(lambda: raw(ranges.ctypes.data, offs.ctypes.data, soq.ctypes.data, nq=0), "nq must be at least 1")
    rejected(lambda: raw(ranges.ctypes.data, offs.ctypes.data, soq.ctypes.data, n_scopes=0), "n_scopes must be at least 1")
    rejected(lambda: raw(ranges.ctypes.data, offs.ctypes.data, soq.ctypes.data, qo=None), "null q_offsets")
    bad = np.asarray([1, 1], np.int32)
    rejected(lambda: raw(ranges.ctypes.data, bad.ctypes.data, soq.ctypes.data), "must start at 0")
    bad2 = np.asarray([0, 1, 0], np.int32)
    rejected(lambda: raw(ranges.ctypes.data, bad2.ctypes.data, soq.ctypes.data, n_scopes=2), "descends")
    v = np.zeros(4, np.int64)
    with pytest.raises(HipRagError):
        nat.call("hipbm25_scoped_info", ctypes.c_uint64(bm._h), None)
    # the handle still works
    es, ei = oracle_scoped(p, queries, 5, [[(0, 5000)]], soq)
    gs, gi = bm.search_scoped(queries, 5, [[(0, 5000)]])
    assert same_bits(gs, gi, es, ei) and v.sum() == 0
    bm.close()
