"""
Scoped hybrid search over the IVF index (libhiprag hiphybrid_search_ivf_scoped*, hiprag.hybrid_search_ivf_scoped*): the one
call must equal the three public calls it is composed of -- HipIVFIndex.search_scoped_device at depth `depth` in the given
probe mode, HipBM25.search_scoped_device, rrf_fuse_device -- on the fused scores, the fused ids and all four per-leg lists,
bit for bit, in both probe modes; with every list probed it must equal hiphybrid_search_scoped on the flat index of the same
rows; and it must refuse what its parts refuse.
"""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

E_INVALID = -1
N, D, NLIST, N_TERMS, BLOCK = 6000, 64, 16, 4096, 60


def coherent(n, d, seed):
    """document-coherent ids: block b of BLOCK consecutive ids = one of 48 unit centres + noise of norm about 0.3"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((48, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[np.repeat(rng.integers(0, 48, size=(n + BLOCK - 1) // BLOCK), BLOCK)[:n]] + (0.3 / np.sqrt(d)) * rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = x[rng.integers(0, n, size=40)] + (0.3 / np.sqrt(d)) * rng.standard_normal((40, d))
    return x.astype(np.float32), (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


_DATA = {}


def handles(metric):
    """built once per metric, shared, never changed"""
    from hiprag import HipBM25, HipFlatIndex, HipIVFIndex, PostingsCSR
    if metric not in _DATA:
        x, q = coherent(N, D, seed=21)
        p = ho.synthetic_postings(N, n_terms=N_TERMS, seed=779)
        ivf = HipIVFIndex(D, NLIST, metric)
        ivf.build(x, iters=6, seed=0)
        flat = HipFlatIndex(D, metric)
        flat.add(x)
        _DATA[metric] = (x, q, p, ivf, flat, HipBM25(PostingsCSR(p.n_docs, p.n_terms, p.offsets, p.doc_ids, p.impacts)))
    return _DATA[metric]


SCOPES = [[(3 * BLOCK, 5 * BLOCK)], [(0, BLOCK), (40 * BLOCK + 7, 41 * BLOCK)], [(3 * BLOCK, 5 * BLOCK), (N - 30, N)], [], [(0, N)]]


def same(a, b):
    import torch
    (fs, fi, ((ds, di), (ss, si))), (gs, gi, ((es, ei), (ts, ti))) = a, b
    return (torch.equal(fi, gi) and torch.equal(fs.view(torch.int32), gs.view(torch.int32)) and torch.equal(di, ei)
            and torch.equal(ds.view(torch.int64), es.view(torch.int64)) and torch.equal(si, ti)
            and torch.equal(ss.view(torch.int64), ts.view(torch.int64)))


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("probe", ["any", "scope"])
def test_one_call_equals_the_three_public_calls(gpu, metric, probe):
    import torch
    from hiprag import hybrid_search_ivf_scoped, hybrid_search_ivf_scoped_device, rrf_fuse_device
    x, q, p, ivf, flat, bm = handles(metric)
    offs, orig = ivf.lists()
    members = [sum(1 for l in range(NLIST) if any(((orig[offs[l]:offs[l + 1]] >= lo) & (orig[offs[l]:offs[l + 1]] < hi)).any() for lo, hi in s))
               for s in SCOPES[:3]]
    assert max(members) < NLIST, f"member lists {members}: the scopes are not selective"
    for nq, depth, k, nprobe, w in ((1, 50, 10, 2, (1.0, 1.0)), (17, 64, 64, 1, (0.7, 0.3)), (40, 10, 5, 3, (1.0, 1.0))):
        qd = torch.from_numpy(q[:nq]).cuda()
        sparse = ho.synthetic_sparse_queries(nq, n_terms=N_TERMS, seed=60 + nq)
        soq = (np.arange(nq) % len(SCOPES)).astype(np.int32)
        got = hybrid_search_ivf_scoped_device(ivf, bm, qd, sparse, SCOPES, soq, depth=depth, k=k, w_dense=w[0], w_sparse=w[1],
                                              nprobe=nprobe, probe=probe, return_lists=True)
        d64, _, dids = ivf.search_scoped_device(qd, depth, SCOPES, soq, nprobe=nprobe, probe=probe)
        s64, _, sids = bm.search_scoped_device(sparse, depth, SCOPES, soq)
        fs, fi = rrf_fuse_device(dids, sids, k, w_a=w[0], w_b=w[1])
        torch.cuda.synchronize()
        assert same(got, (fs, fi, ((d64, dids), (s64, sids)))), f"{metric} {probe} nq {nq}"
        plain = hybrid_search_ivf_scoped_device(ivf, bm, qd, sparse, SCOPES, soq, depth=depth, k=k, w_dense=w[0], w_sparse=w[1],
                                                nprobe=nprobe, probe=probe)
        host = hybrid_search_ivf_scoped(ivf, bm, q[:nq], sparse, SCOPES, soq, depth=depth, k=k, w_dense=w[0], w_sparse=w[1],
                                        nprobe=nprobe, probe=probe, return_lists=True)
        torch.cuda.synchronize()
        assert torch.equal(plain[1], fi) and torch.equal(plain[0].view(torch.int32), fs.view(torch.int32))
        assert np.array_equal(host[1], fi.cpu().numpy()) and np.array_equal(host[0].view(np.int32), fs.cpu().numpy().view(np.int32))
        assert np.array_equal(host[2][0][1], dids.cpu().numpy()) and np.array_equal(host[2][1][1], sids.cpu().numpy())
        assert np.array_equal(host[2][0][0].view(np.int64), d64.cpu().numpy().view(np.int64))


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_every_list_probed_equals_the_flat_scoped_hybrid(gpu, metric):
    import torch
    from hiprag import hybrid_search_ivf_scoped_device, hybrid_search_scoped_device
    x, q, p, ivf, flat, bm = handles(metric)
    nq, depth, k = 33, 64, 20
    qd = torch.from_numpy(q[:nq]).cuda()
    sparse = ho.synthetic_sparse_queries(nq, n_terms=N_TERMS, seed=91)
    soq = (np.arange(nq) % len(SCOPES)).astype(np.int32)
    want = hybrid_search_scoped_device(flat, bm, qd, sparse, SCOPES, soq, depth=depth, k=k, return_lists=True)
    for probe in ("any", "scope"):
        got = hybrid_search_ivf_scoped_device(ivf, bm, qd, sparse, SCOPES, soq, depth=depth, k=k, nprobe=NLIST, probe=probe, return_lists=True)
        torch.cuda.synchronize()
        assert same(got, want), f"{metric} {probe}"


def test_mismatched_rows_and_depth_65_are_refused(gpu):
    import torch
    from hiprag import HipBM25, HipRagError, PostingsCSR, hybrid_search_ivf_scoped, hybrid_search_ivf_scoped_device
    x, q, p, ivf, flat, bm = handles("ip")
    qd = torch.from_numpy(q[:2]).cuda()
    sparse = ho.synthetic_sparse_queries(2, n_terms=N_TERMS, seed=5)
    good = hybrid_search_ivf_scoped_device(ivf, bm, qd, sparse, SCOPES[:1], depth=20, k=5, nprobe=2, probe="scope")
    torch.cuda.synchronize()
    for call, arg in ((hybrid_search_ivf_scoped_device, qd), (hybrid_search_ivf_scoped, q[:2])):
        with pytest.raises(HipRagError, match="depth") as e:
            call(ivf, bm, arg, sparse, SCOPES[:1], depth=65, k=5, nprobe=2, probe="scope")
        assert e.value.code == E_INVALID
        with pytest.raises(HipRagError, match="probe_mode") as e:
            call(ivf, bm, arg, sparse, SCOPES[:1], depth=20, k=5, nprobe=2, probe=7)
        assert e.value.code == E_INVALID
    p2 = ho.synthetic_postings(N - 1, n_terms=N_TERMS, seed=780)
    short = HipBM25(PostingsCSR(p2.n_docs, p2.n_terms, p2.offsets, p2.doc_ids, p2.impacts))
    with pytest.raises(HipRagError, match="documents") as e:
        hybrid_search_ivf_scoped_device(ivf, short, qd, sparse, SCOPES[:1], depth=20, k=5, nprobe=2, probe="any")
    assert e.value.code == E_INVALID
    short.close()
    again = hybrid_search_ivf_scoped_device(ivf, bm, qd, sparse, SCOPES[:1], depth=20, k=5, nprobe=2, probe="scope")
    torch.cuda.synchronize()
    assert torch.equal(good[1], again[1]) and torch.equal(good[0].view(torch.int32), again[0].view(torch.int32))
