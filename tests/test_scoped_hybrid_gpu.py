"""
Scoped hybrid search (libhiprag hiphybrid_search_scoped*, hiprag.hybrid_search_scoped*): dense top-`depth` and BM25
top-`depth` over the rows / documents of every query's scope, RRF behind them, in one library call.  Expected: ho.flat_search
over the scope's rows + the scoped BM25 oracle (ho.bm25_scores_taat, out-of-scope documents set to 0) + ho.rrf_fuse.  Ids,
BM25 score bits and fused score bits are compared exactly; dense scores inside the lists take the bar tests/test_dense_gpu.py
and tests/test_scoped_gpu.py set (absolute 1e-4 against the fp64 oracle rounded to fp32).
"""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

E_INVALID = -1
TOL = 1e-4
F32_MAX = np.finfo(np.float32).max
F64_MAX = np.finfo(np.float64).max
N, D, N_TERMS = 30000, 64, 8192


@pytest.fixture(scope="module")
def data():
    return ho.synthetic_vectors(N, D, seed=12), ho.synthetic_postings(N, n_terms=N_TERMS, seed=778)


def handles(x, p, metric):
    from hiprag import HipBM25, HipFlatIndex, PostingsCSR
    ix = HipFlatIndex(D, metric)
    ix.add(x)
    return ix, HipBM25(PostingsCSR(p.n_docs, p.n_terms, p.offsets, p.doc_ids, p.impacts))


def random_scope(rng, n, n_ranges):
    cuts = np.sort(rng.choice(n + 1, size=2 * n_ranges, replace=False))
    return [(int(cuts[2 * j]), int(cuts[2 * j + 1])) for j in range(n_ranges)]


def rows_of(scope):
    parts = [np.arange(lo, hi, dtype=np.int64) for lo, hi in scope]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def oracle(x, p, q, sparse, scopes, soq, depth, k, metric, c, wd, ws):
    nq = q.shape[0]
    pad = -F32_MAX if metric == ho.METRIC_IP else F32_MAX
    ds = np.full((nq, depth), pad, dtype=np.float32)
    di = np.full((nq, depth), -1, dtype=np.int64)
    ss = np.empty((nq, depth), dtype=np.float32)
    si = np.empty((nq, depth), dtype=np.int64)
    for b in range(nq):
        rows = rows_of(scopes[int(soq[b])])
        if len(rows):
            s_, i_ = ho.flat_search(np.ascontiguousarray(x[rows]), q[b:b + 1], depth, metric)
            ds[b] = s_[0]
            di[b] = np.where(i_[0] >= 0, rows[np.maximum(i_[0], 0)], -1)
        sc = ho.bm25_scores_taat(p, sparse[b])
        mask = np.zeros(p.n_docs, dtype=bool)
        mask[rows] = True
        sc[~mask] = 0
        ss[b], si[b] = ho.topk_desc_id_asc(sc, depth, exclude_nonpositive=True)
    fs, fi = ho.rrf_fuse(di, si, k, c=c, w_a=wd, w_b=ws)
    return (ds, di), (ss, si), (fs, fi)


def check(got, want, tag):
    (fs, fi, ((gds, gdi), (gss, gsi))) = got
    (ds, di), (ss, si), (efs, efi) = want
    assert np.array_equal(gdi, di), f"{tag}: dense ids"
    pad = di < 0           # past the rows of the scope: -DBL_MAX (IP) / DBL_MAX (L2) in the fp64 list, no fp32 image
    assert np.array_equal(gds[pad], np.where(ds[pad] < 0, -F64_MAX, F64_MAX)), f"{tag}: dense padding"
    assert np.allclose(gds[~pad].astype(np.float32), ds[~pad], rtol=0, atol=TOL), f"{tag}: dense scores"
    assert np.array_equal(gsi, si), f"{tag}: BM25 ids"
    spad = si < 0          # the BM25 list pads its fp64 scores with -DBL_MAX
    assert np.all(gss[spad] == -F64_MAX), f"{tag}: BM25 padding"
    assert np.array_equal(gss[~spad].astype(np.float32).view(np.uint32), ss[~spad].view(np.uint32)), f"{tag}: BM25 score bits"
    assert np.array_equal(fi, efi), f"{tag}: fused ids"
    assert np.array_equal(fs.view(np.uint32), efs.view(np.uint32)), f"{tag}: fused score bits"


def to_host(out):
    fs, fi, ((a, b), (c, d)) = out
    return fs.cpu().numpy(), fi.cpu().numpy(), ((a.cpu().numpy(), b.cpu().numpy()), (c.cpu().numpy(), d.cpu().numpy()))


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.7, 0.3)], ids=["unweighted", "weighted"])
def test_oracle_parity_host_and_device(gpu, data, metric, weights):
    import torch
    from hiprag import hybrid_search_scoped, hybrid_search_scoped_device
    x, p = data
    ix, bm = handles(x, p, metric)
    m = ho.METRIC_IP if metric == "ip" else ho.METRIC_L2
    wd, ws = weights
    rng = np.random.default_rng(5 + int(wd * 10))
    T = bm.scoped_info()["tile_docs"]
    for nq, depth, k in ((1, 50, 10), (17, 64, 64), (120, 10, 5)):
        q = ho.synthetic_queries(nq, D, seed=50 + nq)
        sparse = ho.synthetic_sparse_queries(nq, n_terms=N_TERMS, seed=60 + nq)
        scopes = [random_scope(rng, N, int(rng.integers(1, 41))) for _ in range(min(nq, 4))]
        scopes += [[(T - 1, T + 1)], [(N - 300, N)]] if nq > 1 else []
        soq = rng.integers(0, len(scopes), size=nq).astype(np.int32)
        want = oracle(x, p, q, sparse, scopes, soq, depth, k, m, 60.0, wd, ws)
        got = hybrid_search_scoped(ix, bm, q, sparse, scopes, soq, depth=depth, k=k, w_dense=wd, w_sparse=ws, return_lists=True)
        check(got, want, f"host {metric} nq={nq}")
        plain = hybrid_search_scoped(ix, bm, q, sparse, scopes, soq, depth=depth, k=k, w_dense=wd, w_sparse=ws)
        assert np.array_equal(plain[1], got[1]) and np.array_equal(plain[0].view(np.uint32), got[0].view(np.uint32))
        dev = hybrid_search_scoped_device(ix, bm, torch.from_numpy(q).cuda(), sparse, scopes, soq, depth=depth, k=k, w_dense=wd,
                                          w_sparse=ws, return_lists=True)
        torch.cuda.synchronize()
        check(to_host(dev), want, f"device {metric} nq={nq}")
    bm.close()


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_full_scope_equals_the_unscoped_hybrid_bit_for_bit(gpu, data, metric):
    import torch
    from hiprag import hybrid_search_device, hybrid_search_scoped_device
    x, p = data
    ix, bm = handles(x, p, metric)
    for nq, depth, k in ((1, 50, 10), (70, 64, 20)):
        q = torch.from_numpy(ho.synthetic_queries(nq, D, seed=70 + nq)).cuda()
        sparse = ho.synthetic_sparse_queries(nq, n_terms=N_TERMS, seed=80 + nq)
        a = hybrid_search_device(ix, bm, q, sparse, depth=depth, k=k, w_dense=0.7, w_sparse=0.3, return_lists=True)
        b = hybrid_search_scoped_device(ix, bm, q, sparse, [[(0, N)]], depth=depth, k=k, w_dense=0.7, w_sparse=0.3, return_lists=True)
        torch.cuda.synchronize()
        assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        for leg in (0, 1):
            assert torch.equal(a[2][leg][1], b[2][leg][1])
            assert torch.equal(a[2][leg][0].view(torch.int64), b[2][leg][0].view(torch.int64))
    bm.close()


def test_empty_scope_is_all_padding(gpu, data):
    import torch
    from hiprag import hybrid_search_scoped, hybrid_search_scoped_device
    x, p = data
    ix, bm = handles(x, p, "ip")
    q = ho.synthetic_queries(3, D, seed=1)
    sparse = ho.synthetic_sparse_queries(3, n_terms=N_TERMS, seed=2)
    for scopes in ([[]], [[(7, 7)]]):
        fs, fi, ((ds, di), (ss, si)) = hybrid_search_scoped(ix, bm, q, sparse, scopes, depth=20, k=10, return_lists=True)
        assert np.all(fi == -1) and np.all(di == -1) and np.all(si == -1)
        assert np.all(fs == -F32_MAX) and np.all(ds == -F64_MAX) and np.all(ss == -F64_MAX)
        out = to_host(hybrid_search_scoped_device(ix, bm, torch.from_numpy(q).cuda(), sparse, scopes, depth=20, k=10, return_lists=True))
        assert np.all(out[1] == -1) and np.all(out[2][0][1] == -1) and np.all(out[2][1][1] == -1)
    bm.close()


def test_validation(gpu, data):
    from hiprag import HipBM25, HipRagError, PostingsCSR, hybrid_search_scoped
    x, p = data
    ix, bm = handles(x, p, "ip")
    q = ho.synthetic_queries(2, D, seed=1)
    sparse = ho.synthetic_sparse_queries(2, n_terms=N_TERMS, seed=2)

    def rejected(fn, needle):
        with pytest.raises(HipRagError) as e:
            fn()
        assert e.value.code == E_INVALID and needle in str(e.value), str(e.value)

    small = ho.synthetic_postings(N - 1, n_terms=N_TERMS, seed=3)
    other = HipBM25(PostingsCSR(small.n_docs, small.n_terms, small.offsets, small.doc_ids, small.impacts))
    rejected(lambda: hybrid_search_scoped(ix, other, q, sparse, [[(0, 100)]]), "a row must be a document")
    rejected(lambda: hybrid_search_scoped(ix, bm, q, sparse, [[(0, 100)]], depth=65), "depth must be in 1..64")
    rejected(lambda: hybrid_search_scoped(ix, bm, q, sparse, [[(0, 100)]], depth=0), "bad hybrid shape")
    rejected(lambda: hybrid_search_scoped(ix, bm, q, sparse, [[(0, 100)]], k=0), "bad hybrid shape")
    rejected(lambda: hybrid_search_scoped(ix, bm, q, sparse, [[(0, N + 1)]]), "is not within")
    rejected(lambda: hybrid_search_scoped(ix, bm, q, sparse, [[(50, 100), (99, 200)]]), "ascend and do not overlap")
    rejected(lambda: hybrid_search_scoped(ix, bm, q, sparse, [[(0, 100)]], [0, 1]), "is not a scope")
    s, i = hybrid_search_scoped(ix, bm, q, sparse, [[(0, 100)]], depth=20, k=5)      # the handles still work
    assert np.all((i >= 0) & (i < 100))
    other.close()
    bm.close()
