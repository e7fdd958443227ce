"""
Scoped dense search (libhiprag hipidx_search_scoped*, HipFlatIndex.search_scoped*): the top k of every query among the rows
of ITS scope -- a few half-open row ranges of one collection index -- under the flat index's own definition.  Checked
against the CPU oracle over the rows of the scope (ids exactly, fp32 scores under the bar tests/test_dense_gpu.py sets for
dense scores), against the flat search bit for bit where include/hiprag.h promises the same bits, and on the edges a range
can have: no alignment, one row, no row, the end of the index, duplicates just outside.
"""
import ctypes
import math

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

E_INVALID = -1   # include/hiprag.h
TOL = 1e-4   # tests/test_dense_gpu.py: fp32 scores vs the fp64 oracle rounded to fp32, absolute
SHAPES = [(30000, 128, 10), (20011, 100, 50), (6000, 1024, 256), (700, 64, 5)]   # n, d, k
NQS = (1, 17, 1000)
F32_MAX = np.finfo(np.float32).max
F64_MAX = np.finfo(np.float64).max


def make_index(x, metric):
    from hiprag import HipFlatIndex
    ix = HipFlatIndex(x.shape[1], metric)
    ix.add(x)
    return ix


def random_scope(rng, n, n_ranges):
    """n_ranges non-empty, non-touching-or-touching ranges at random (hence unaligned) cut points, ascending"""
    cuts = np.sort(rng.choice(n + 1, size=2 * n_ranges, replace=False))
    return [(int(cuts[2 * j]), int(cuts[2 * j + 1])) for j in range(n_ranges)]


def rows_of(scope):
    parts = [np.arange(lo, hi, dtype=np.int64) for lo, hi in scope]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def oracle_scoped(x, q, k, metric, scopes, soq):
    """ho.flat_search over the rows of every scope for the queries that name it, ids mapped back through the row list"""
    pad = -F32_MAX if metric == ho.METRIC_IP else F32_MAX
    es = np.full((q.shape[0], k), pad, dtype=np.float32)
    ei = np.full((q.shape[0], k), -1, dtype=np.int64)
    for s, scope in enumerate(scopes):
        qi = np.nonzero(soq == s)[0]
        rows = rows_of(scope)
        if len(qi) == 0 or len(rows) == 0:
            continue
        s_, i_ = ho.flat_search(np.ascontiguousarray(x[rows]), np.ascontiguousarray(q[qi]), k, metric)
        es[qi] = s_
        ei[qi] = np.where(i_ >= 0, rows[np.maximum(i_, 0)], -1)
    return es, ei


def bits_equal(a, b):
    """two (scores64, scores32, ids) triples: equal ids, equal score BIT PATTERNS"""
    import torch
    return (torch.equal(a[2], b[2]) and torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
            and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def mid(metric):
    return ho.METRIC_IP if metric == "ip" else ho.METRIC_L2


# ---- 1. the oracle over the rows of the scope ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_parity(gpu, metric, shape):
    n, d, k = shape
    x = ho.synthetic_vectors(n, d, seed=11)
    ix = make_index(x, metric)
    rng = np.random.default_rng(n + d)
    for nq in NQS:
        q = ho.synthetic_queries(nq, d, seed=100 + nq)
        n_scopes = min(nq, 6)
        scopes = [random_scope(rng, n, int(rng.integers(1, 41))) for _ in range(n_scopes)]
        soq = rng.integers(0, n_scopes, size=nq).astype(np.int32)
        s, i = ix.search_scoped(q, k, scopes, soq)
        es, ei = oracle_scoped(x, q, k, mid(metric), scopes, soq)
        assert np.array_equal(i, ei), f"ids differ from the oracle: {shape} {metric} nq={nq}"
        err = float(np.max(np.abs(s.astype(np.float64) - es.astype(np.float64))))
        print(f"{shape} {metric} nq={nq}: max |score - oracle| = {err:.3g}")
        assert np.allclose(s, es, rtol=0, atol=TOL), f"scores differ from the oracle: {shape} {metric} nq={nq}"


# ---- 2. the flat search, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("n,d,k,nq", [(20011, 128, 10, 100), (6000, 1024, 50, 1), (3001, 100, 256, 17)])
def test_whole_index_scope_is_the_flat_search(gpu, metric, n, d, k, nq):
    import torch
    x = ho.synthetic_vectors(n, d, seed=21)
    qd = torch.from_numpy(ho.synthetic_queries(nq, d, seed=22)).cuda()
    ix = make_index(x, metric)
    flat = ix.search_device(qd, k)
    scoped = ix.search_scoped_device(qd, k, [[(0, n)]])
    torch.cuda.synchronize()
    assert bits_equal(scoped, flat)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("lo,hi", [(1003, 9001), (37, 20011 - 6), (5125, 5127)])
def test_range_scope_is_the_flat_search_of_those_rows(gpu, metric, lo, hi):
    import torch
    assert lo % 4 and lo % 32 and hi % 4 and hi % 256
    n, d, k, nq = 20011, 128, 10, 33
    x = ho.synthetic_vectors(n, d, seed=23)
    qd = torch.from_numpy(ho.synthetic_queries(nq, d, seed=24)).cuda()
    ix = make_index(x, metric)
    sub = make_index(np.ascontiguousarray(x[lo:hi]), metric)
    s64, s32, ids = sub.search_device(qd, k)
    ids = torch.where(ids >= 0, ids + lo, ids)
    scoped = ix.search_scoped_device(qd, k, [[(lo, hi)]])
    torch.cuda.synchronize()
    assert bits_equal(scoped, (s64, s32, ids))


# ---- 3. edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_one_row_empty_and_tail_ranges(gpu, metric):
    n, d, k = 1000 + 13, 64, 8          # ntotal % 32 != 0
    x = ho.synthetic_vectors(n, d, seed=31)
    q = ho.synthetic_queries(5, d, seed=32)
    ix = make_index(x, metric)
    scopes = [[(3, 4), (4, 4), (9, 10), (255, 256), (256, 257), (700, 700), (n - 1, n)],      # one-row and empty ranges
              [(0, 33), (40, 40), (40, 40), (41, 300), (300, 300), (990, n)],                 # empty ranges between full ones, the tail
              [],                                                                            # no range at all
              [(5, 5), (77, 77)],                                                            # ranges, no rows
              [(n - 3, n)]]                                                                  # fewer rows than k
    soq = np.arange(5, dtype=np.int32)
    s, i = ix.search_scoped(q, k, scopes, soq)
    es, ei = oracle_scoped(x, q, k, mid(metric), scopes, soq)
    assert np.array_equal(i, ei)
    assert np.allclose(s, es, rtol=0, atol=TOL)
    pad32 = -F32_MAX if metric == "ip" else F32_MAX
    for e in (2, 3):
        assert (i[e] == -1).all() and (s[e] == pad32).all()
    assert (i[4, 3:] == -1).all() and (s[4, 3:] == pad32).all() and sorted(i[4, :3]) == [n - 3, n - 2, n - 1]
    assert (i[0, 5:] == -1).all() and sorted(i[0, :5]) == [3, 9, 255, 256, n - 1]
    # the fp64 padding of the device entry
    import torch
    s64, _, ids = ix.search_scoped_device(torch.from_numpy(q[:1]).cuda(), k, [[]])
    torch.cuda.synchronize()
    assert (ids.cpu().numpy() == -1).all() and (s64.cpu().numpy() == (-F64_MAX if metric == "ip" else F64_MAX)).all()


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("lo,hi", [(1003, 1507), (1024, 1280), (1001, 1002)])
def test_duplicates_outside_the_range_never_appear(gpu, metric, lo, hi):
    n, d, k = 4000, 128, 10
    x = ho.synthetic_vectors(n, d, seed=41)
    r = lo + (hi - lo) // 2
    x[lo - 1] = x[r]          # immediately before lo: the same quad as row lo when lo % 4 != 0
    x[hi] = x[r]              # at hi
    ix = make_index(x, metric)
    q = np.ascontiguousarray(x[r:r + 1])
    s, i = ix.search_scoped(q, k, [[(lo, hi)]])
    assert i[0, 0] == r
    assert lo - 1 not in i[0] and hi not in i[0]
    valid = i[0][i[0] >= 0]
    assert ((valid >= lo) & (valid < hi)).all() and len(valid) == min(k, hi - lo)
    fs, fi = ix.search(q, 3)     # the flat search does see all three copies, in id order
    assert list(fi[0]) == [lo - 1, r, hi]


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_duplicates_inside_the_scope_come_in_id_order(gpu, metric):
    n, d, k = 3000, 100, 25
    x = ho.synthetic_vectors(n, d, seed=43)
    x[1490:1510] = x[77]       # 20 equal rows inside one 256-row slice, across quads
    x[1530:1550] = x[78]       # 20 equal rows across the slice boundary at 1536
    ix = make_index(x, metric)
    q = np.ascontiguousarray(x[[77, 78]])
    s, i = ix.search_scoped(q, k, [[(1201, 1999)]])
    assert list(i[0, :20]) == list(range(1490, 1510))
    assert list(i[1, :20]) == list(range(1530, 1550))
    assert (s[0, :20] == s[0, 0]).all() and (s[1, :20] == s[1, 0]).all()


def test_id_base_shifts_ids_and_only_ids(gpu):
    import torch
    n, d, k = 5000, 128, 256
    x = ho.synthetic_vectors(n, d, seed=51)
    qd = torch.from_numpy(ho.synthetic_queries(9, d, seed=52)).cuda()
    ix = make_index(x, "ip")
    scopes = [[(11, 99), (1000, 1100)]]      # 188 rows < k: padded slots keep id -1
    a = ix.search_scoped_device(qd, k, scopes)
    ix.set_id_base(10 ** 9)
    b = ix.search_scoped_device(qd, k, scopes)
    torch.cuda.synchronize()
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(torch.where(a[2] >= 0, a[2] + 10 ** 9, a[2]), b[2])
    assert int((b[2] == -1).sum()) == 9 * (k - 188)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_a_scope_of_300_ranges(gpu, metric):
    n, d, k = 30000, 64, 40
    x = ho.synthetic_vectors(n, d, seed=61)
    q = ho.synthetic_queries(20, d, seed=62)
    ix = make_index(x, metric)
    scope = random_scope(np.random.default_rng(63), n, 300)
    s, i = ix.search_scoped(q, k, [scope])
    es, ei = oracle_scoped(x, q, k, mid(metric), [scope], np.zeros(20, dtype=np.int32))
    assert np.array_equal(i, ei) and np.allclose(s, es, rtol=0, atol=TOL)


def test_shuffled_scopes_equal_one_scope_at_a_time(gpu):
    import torch
    n, d, k, nq, n_scopes = 20011, 128, 10, 1000, 64
    x = ho.synthetic_vectors(n, d, seed=71)
    q = ho.synthetic_queries(nq, d, seed=72)
    ix = make_index(x, "l2")
    rng = np.random.default_rng(73)
    scopes = [random_scope(rng, n, int(rng.integers(1, 8))) for _ in range(n_scopes)]
    soq = rng.integers(0, n_scopes, size=nq).astype(np.int32)
    qd = torch.from_numpy(q).cuda()
    got = ix.search_scoped_device(qd, k, scopes, soq)
    torch.cuda.synchronize()
    for s in range(n_scopes):
        qi = torch.from_numpy(np.nonzero(soq == s)[0]).cuda()
        if len(qi) == 0:
            continue
        one = ix.search_scoped_device(qd[qi].contiguous(), k, [scopes[s]])
        torch.cuda.synchronize()
        assert bits_equal(tuple(t[qi] for t in got), one), f"scope {s}"


# ---- 4. what a call reads -----------------------------------------------------------------------------------------------
def test_rows_read_and_repeatability(gpu):
    import torch
    n, d, k = 5000, 256, 10
    x = ho.synthetic_vectors(n, d, seed=81)
    ix = make_index(x, "ip")
    scopes = [[(5, 1008)], [(2000, 2077)], [(3000, 4000)]]     # 1003 rows, 77 rows, one scope nobody names
    soq = np.array([0] * 40 + [1], dtype=np.int32)
    np.random.default_rng(82).shuffle(soq)
    qd = torch.from_numpy(ho.synthetic_queries(41, d, seed=83)).cuda()
    a = ix.search_scoped_device(qd, k, scopes, soq)
    info = ix.scoped_info()
    G = info["group_queries"]
    assert G >= 8
    assert info["chunks"] == 1 and info["chunk_queries"] == 41
    assert info["rows_read"] == math.ceil(40 / G) * 1003 + math.ceil(1 / G) * 77
    b = ix.search_scoped_device(qd, k, scopes, soq)
    torch.cuda.synchronize()
    assert bits_equal(a, b)
    assert ix.scoped_info()["rows_read"] == info["rows_read"]      # per call, not accumulated


# ---- 5. rows added between calls ----------------------------------------------------------------------------------------
def test_growth(gpu):
    import torch
    d, k = 128, 10
    x = ho.synthetic_vectors(9000, d, seed=91)
    ix = make_index(x[:4001], "l2")
    q = ho.synthetic_queries(7, d, seed=92)
    s, i = ix.search_scoped(q, k, [[(100, 3999)]])
    es, ei = oracle_scoped(x, q, k, ho.METRIC_L2, [[(100, 3999)]], np.zeros(7, dtype=np.int32))
    assert np.array_equal(i, ei)
    ix.add(x[4001:6000])
    ix.add_device(torch.from_numpy(x[6000:]).cuda())
    scope = [(4003, 5997), (6001, 8999)]
    s, i = ix.search_scoped(q, k, [scope])
    es, ei = oracle_scoped(x, q, k, ho.METRIC_L2, [scope], np.zeros(7, dtype=np.int32))
    assert np.array_equal(i, ei) and np.allclose(s, es, rtol=0, atol=TOL)
    assert i.min() >= 4003


# ---- 6. the checks ------------------------------------------------------------------------------------------------------
def test_errors_name_the_argument_and_leave_the_index_usable(gpu):
    import torch
    from hiprag import HipRagError
    from hiprag import _native as nat
    n, d, k, nq = 1000, 64, 5, 3
    x = ho.synthetic_vectors(n, d, seed=95)
    ix = make_index(x, "ip")
    qd = torch.from_numpy(ho.synthetic_queries(nq, d, seed=96)).cuda()
    o64 = torch.empty((nq, k), dtype=torch.float64, device="cuda")
    o32 = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    oid = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(q=qd.data_ptr(), nq_=nq, k_=k, ranges=((0, 10), (20, 30)), offsets=(0, 1, 2), n_scopes=2, soq=(0, 1, 1),
            s64=o64.data_ptr(), ids=oid.data_ptr(), null=()):
        r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
        o = np.asarray(offsets, dtype=np.int32)
        sq = np.asarray(soq, dtype=np.int32)
        nat.call("hipidx_search_scoped_dev", ix._h, q, nq_, k_, None if "ranges" in null else r.ctypes.data,
                 None if "scope_offsets" in null else o.ctypes.data, n_scopes, None if "scope_of_query" in null else sq.ctypes.data,
                 s64, o32.data_ptr(), ids, st)

    bad = [
        (dict(q=None), "q is null"),
        (dict(s64=None), "out_scores64"),
        (dict(ids=None), "out_ids"),
        (dict(null=("ranges",)), "ranges"),
        (dict(null=("scope_offsets",)), "scope_offsets"),
        (dict(null=("scope_of_query",)), "scope_of_query"),
        (dict(nq_=0), "nq"),
        (dict(k_=0), "k must"),
        (dict(k_=257), "k must"),
        (dict(n_scopes=0), "n_scopes"),
        (dict(offsets=(1, 1, 2)), "scope_offsets"),
        (dict(offsets=(0, 2, 1)), "scope_offsets"),
        (dict(ranges=((-1, 10), (20, 30))), "ranges[0]"),
        (dict(ranges=((0, 10), (30, 20))), "ranges[1]"),
        (dict(ranges=((0, 10), (20, n + 1))), "ranges[1]"),
        (dict(ranges=((0, 10), (9, 30)), offsets=(0, 2, 2)), "ranges[1]"),       # overlap inside one scope
        (dict(soq=(0, 2, 1)), "scope_of_query[1]"),
        (dict(soq=(0, 1, -1)), "scope_of_query[2]"),
    ]
    for kwargs, word in bad:
        with pytest.raises(HipRagError) as e:
            raw(**kwargs)
        assert e.value.code == E_INVALID
        assert word in str(e.value), f"{kwargs}: {e.value}"
    # overlapping ranges in DIFFERENT scopes, touching ranges and descending order across scopes are all valid
    raw(ranges=((0, 10), (5, 30)))
    raw(ranges=((0, 10), (10, 30)), offsets=(0, 2, 2))
    raw(ranges=((500, 600), (0, 10)))
    with pytest.raises(ValueError):
        ix.search_scoped(np.zeros((3, d), np.float32), k, [[(0, 1)], [(1, 2)]])        # 2 scopes, 3 queries, no map
    s, i = ix.search_scoped(qd.cpu().numpy(), k, [[(0, n)]])
    es, ei = ho.flat_search(x, qd.cpu().numpy(), k, ho.METRIC_IP)
    assert np.array_equal(i, ei) and np.allclose(s, es, rtol=0, atol=TOL)
