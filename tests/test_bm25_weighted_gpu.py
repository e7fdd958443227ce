"""
Weighted sparse search (libhiprag hipbm25_search_weighted*, HipBM25.search_weighted*): a weight per query term,
score(d) = fp32 sum in query-term order of fl32(w_t * impact[t, d]).  The expected value is
hiprag.sparse.weighted_search_reference (numpy, float32 throughout).  Every comparison is exact: ids equal, score bit
patterns equal.

The collection: 2 * 9216 + 37 documents (two tile boundaries and a partial tile), 40 terms -- one list holding every
document, lists of about 9000 and 6000 postings (skip tables from 2048 postings on), lists of 1 to 300 postings, one empty
list.  Two value sets: "exact" (impacts n/8, weights from {0.5, 0.75, 1, 1.5, 2}: every sum is exact and ties abound) and
"random" (random fp32 impacts and weights: the order of the adds and the rounding of the product show).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_INVALID = -1   # include/hiprag.h
F32_MAX = np.finfo(np.float32).max
F64_MAX = np.finfo(np.float64).max
N_DOCS = 2 * 9216 + 37
N_TERMS = 40
KS_TILED = (1, 10, 64)
KS_GLOBAL = (65, 200)
SETS = ("exact", "random")


@functools.lru_cache(maxsize=None)
def collection(values):
    from hiprag import PostingsCSR
    rng = np.random.default_rng(20240 + len(values))
    dfs = [N_DOCS, 9003, 6011] + [int(x) for x in rng.integers(1, 301, size=N_TERMS - 4)] + [0]
    dfs[3], dfs[4] = 1, 300
    lists = [np.sort(rng.choice(N_DOCS, size=df, replace=False)).astype(np.uint32) for df in dfs]
    off = np.zeros(N_TERMS + 1, dtype=np.uint64)
    off[1:] = np.cumsum(dfs).astype(np.uint64)
    n_post = int(off[-1])
    if values == "exact":
        imp = (rng.integers(1, 17, size=n_post) / 8.0).astype(np.float32)
    else:
        imp = rng.uniform(0.1, 4.0, size=n_post).astype(np.float32)
    return PostingsCSR(N_DOCS, N_TERMS, off, np.concatenate(lists), imp)


@functools.lru_cache(maxsize=None)
def queries(values):
    """0, 1, 6, 64 and 65 terms; the 6-term query has term 1 twice with two weights; the last names a term id >= n_terms"""
    rng = np.random.default_rng(77 + len(values))
    qs = [[], [0], [1, 5, 2, 9, 1, 17], rng.integers(0, N_TERMS, size=64).tolist(), rng.integers(0, N_TERMS, size=65).tolist(),
          [3, N_TERMS + 5, 0, 4]]
    if values == "exact":
        ws = [rng.choice(np.asarray([0.5, 0.75, 1.0, 1.5, 2.0], np.float32), size=len(q)).astype(np.float32) for q in qs]
    else:
        ws = [rng.uniform(0.1, 3.0, size=len(q)).astype(np.float32) for q in qs]
    if values == "exact":
        ws[2][0], ws[2][4] = np.float32(0.5), np.float32(2.0)
    assert ws[2][0] != ws[2][4]
    return qs, ws


@functools.lru_cache(maxsize=None)
def reference(values, scope_key=None):
    """the reference's top 200 of every query (computed once per value set and scope; tests take prefixes)"""
    from hiprag.sparse import weighted_search_reference
    qs, ws = queries(values)
    ranges = None if scope_key is None else [list(scope_key)] * len(qs)
    return weighted_search_reference(collection(values), qs, ws, max(KS_GLOBAL), ranges)


@functools.lru_cache(maxsize=None)
def bm25(values):
    from hiprag import HipBM25
    return HipBM25(collection(values))


def host(out):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check_triple(got, es, ei, what):
    s64, s32, ids = got
    assert np.array_equal(ids, ei), f"{what}: ids differ from the reference"
    assert np.array_equal(s32.view(np.uint32), es.view(np.uint32)), f"{what}: fp32 score bits differ from the reference"
    e64 = np.where(ei >= 0, es.astype(np.float64), -F64_MAX)
    assert np.array_equal(s64.view(np.uint64), e64.view(np.uint64)), f"{what}: fp64 score bits differ from the reference"
    assert np.all(s32[ids < 0] == -F32_MAX)


def test_the_data_is_what_the_cases_need():
    p = collection("exact")
    df = np.diff(p.offsets.astype(np.int64))
    assert df[0] == N_DOCS == 18469 and 8500 < df[1] < 9500 and 5500 < df[2] < 6500 and df[-1] == 0
    assert df[3:-1].min() == 1 and df[3:-1].max() == 300
    qs, _ = queries("exact")
    assert [len(q) for q in qs[:5]] == [0, 1, 6, 64, 65] and qs[2].count(1) == 2 and max(qs[5]) >= N_TERMS
    # ties: by the reference some query has two equal scores inside its top k
    es, ei = reference("exact")
    assert any(np.any((es[b, :9] == es[b, 1:10]) & (ei[b, 1:10] >= 0)) for b in range(len(qs)))
    es, ei = reference("random")
    assert np.all(ei[0] == -1) and np.all(ei[1, :200] >= 0)


# Which kernel form a call takes: the tiled one needs k <= 64 AND no query of the call beyond 64 terms.  So every k runs twice:
# the queries of at most 64 terms in one call (tiled for k <= 64), and all six (the 65-term query sends the call to the
# global-accumulator form whatever k is).
CALLS = {"upto64": (0, 1, 2, 3, 5), "all": (0, 1, 2, 3, 4, 5)}


@pytest.mark.parametrize("values", SETS)
@pytest.mark.parametrize("call", sorted(CALLS))
@pytest.mark.parametrize("k", KS_TILED + KS_GLOBAL)
def test_unscoped_equals_the_reference(gpu, values, call, k):
    rows = list(CALLS[call])
    qs, ws = ([x[r] for r in rows] for x in queries(values))
    es, ei = (x[rows, :k] for x in reference(values))
    bm = bm25(values)
    got = host(bm.search_weighted_device(qs, ws, k))
    check_triple(got, es, ei, f"{values} {call} k={k}")
    again = host(bm.search_weighted_device(qs, ws, k))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), "two runs differ"
    s, i = bm.search_weighted(qs, ws, k)       # the host-output entry
    assert np.array_equal(i, ei) and np.array_equal(s.view(np.uint32), es.view(np.uint32))


@pytest.mark.parametrize("values", SETS)
@pytest.mark.parametrize("call", sorted(CALLS))
@pytest.mark.parametrize("k", KS_TILED + KS_GLOBAL)
def test_unit_weights_equal_the_unweighted_entry(gpu, values, call, k):
    qs = [queries(values)[0][r] for r in CALLS[call]]
    bm = bm25(values)
    ones = [np.ones(len(q), np.float32) for q in qs]
    got = host(bm.search_weighted_device(qs, ones, k))
    plain = host(bm.search_device(qs, k))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, plain))


SCOPES = {"all": ((0, N_DOCS),), "inside_a_tile_boundary": ((9200, 9300),), "two_ranges": ((100, 5000), (9210, 18000)), "empty": ()}


@pytest.mark.parametrize("values", SETS)
@pytest.mark.parametrize("scope", sorted(SCOPES))
def test_scoped_equals_the_reference(gpu, values, scope):
    qs, ws = queries(values)
    bm = bm25(values)
    es, ei = reference(values, SCOPES[scope])
    if scope == "empty":
        assert np.all(ei == -1)
    for k in KS_TILED:
        got = host(bm.search_scoped_weighted_device(qs, ws, k, [list(SCOPES[scope])]))
        check_triple(got, es[:, :k], ei[:, :k], f"{values} scope={scope} k={k}")
        if scope == "all":
            unscoped = host(bm.search_weighted_device(qs, ws, k))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, unscoped)), "[0, n) differs from the unscoped result"
        s, i = bm.search_scoped_weighted(qs, ws, k, [list(SCOPES[scope])])
        assert np.array_equal(i, ei[:, :k]) and np.array_equal(s.view(np.uint32), es[:, :k].view(np.uint32))


def test_scoped_second_slot_batch(gpu):
    """the 65-term query alone, its scope per query: slot 65 is the first of the second batch of 64"""
    qs, ws = queries("random")
    es, ei = reference("random", SCOPES["two_ranges"])
    got = host(bm25("random").search_scoped_weighted_device(qs[4:5], ws[4:5], 10, [list(SCOPES["two_ranges"])]))
    check_triple(got, es[4:5, :10], ei[4:5, :10], "65 terms")
    # and the last slot counts: without it the reference gives other bits
    from hiprag.sparse import weighted_search_reference
    cut = weighted_search_reference(collection("random"), [qs[4][:64]], [ws[4][:64]], 10, [list(SCOPES["two_ranges"])])
    assert not np.array_equal(cut[0].view(np.uint32), es[4:5, :10].view(np.uint32))


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), None])
def test_refusals_enqueue_nothing(gpu, bad):
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    bm = bm25("exact")
    terms = np.asarray([0, 1, 2], np.uint32)
    qoff = np.asarray([0, 3], np.int32)
    w = None if bad is None else np.asarray([1.0, bad, 2.0], np.float32)
    ids = torch.full((1, 10), -77, dtype=torch.int64, device="cuda")
    sc = torch.full((1, 10), -77.0, dtype=torch.float32, device="cuda")
    scopes = (np.asarray([0, N_DOCS], np.int64), np.asarray([0, 1], np.int32), np.asarray([0], np.int32))
    hs, hi = np.full((1, 10), -77.0, np.float32), np.full((1, 10), -77, np.int64)
    wp = None if w is None else w.ctypes.data
    calls = [
        ("hipbm25_search_weighted_dev", (terms.ctypes.data, wp, qoff.ctypes.data, 1, 10, None, sc.data_ptr(), ids.data_ptr(), _stream_ptr())),
        ("hipbm25_search_weighted", (terms.ctypes.data, wp, qoff.ctypes.data, 1, 10, hs.ctypes.data, hi.ctypes.data)),
        ("hipbm25_search_scoped_weighted_dev", (terms.ctypes.data, wp, qoff.ctypes.data, 1, 10, scopes[0].ctypes.data, scopes[1].ctypes.data, 1,
                                                scopes[2].ctypes.data, None, sc.data_ptr(), ids.data_ptr(), _stream_ptr())),
        ("hipbm25_search_scoped_weighted", (terms.ctypes.data, wp, qoff.ctypes.data, 1, 10, scopes[0].ctypes.data, scopes[1].ctypes.data, 1,
                                            scopes[2].ctypes.data, hs.ctypes.data, hi.ctypes.data)),
    ]
    for name, args in calls:
        with pytest.raises(nat.HipRagError) as e:
            nat.call(name, bm._h, *args)
        assert e.value.code == E_INVALID, name
    torch.cuda.synchronize()
    assert torch.all(ids == -77) and torch.all(sc == -77.0) and np.all(hi == -77) and np.all(hs == -77.0)


def test_a_dirty_updatable_handle_is_refused(gpu):
    from hiprag import HipBM25Updatable, HipRagError
    up = HipBM25Updatable.from_texts(["a b c", "b c d", "c d e"])
    up.auto_commit = False
    up.append_texts(["a e f"])
    assert up.dirty
    q, w = [up.terms_of("a c")], [np.asarray([1.5, 0.5], np.float32)]
    for call in (lambda: up.search_weighted(q, w, 2), lambda: up.search_weighted_device(q, w, 2),
                 lambda: up.search_scoped_weighted(q, w, 2, [[(0, 3)]]), lambda: up.search_scoped_weighted_device(q, w, 2, [[(0, 3)]])):
        with pytest.raises(HipRagError) as e:
            call()
        assert e.value.code == E_INVALID and "hipbm25_reweigh" in str(e.value)
    up.commit()
    s, i = up.search_weighted(q, w, 2)
    assert i[0, 0] >= 0
    up.close()
