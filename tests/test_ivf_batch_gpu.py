"""
List-major batch search of the IVF-Flat index (libhiprag hipivf_search_batch_dev, HipIVFIndex.search_batch*).  Its
specification is one sentence of include/hiprag.h: the result of hipivf_search_dev, bit for bit, for the same index,
queries, k and nprobe.  So most cases compare the complete outputs of the two entries as integer bit patterns; one case
checks the batch entry against a CPU restatement (oracle.hybrid_oracle.flat_search over the centroids, then over the union
of the probed lists) that does not involve the one-query kernel at all.
"""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

SHAPES = [(30000, 128, 64, 10), (20011, 256, 37, 50), (6000, 1024, 16, 256), (700, 64, 7, 5)]   # n, d, nlist, k
NQS = (1, 63, 64, 65, 1000)


def clustered(n, d, n_centres, sigma, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n_centres, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[rng.integers(0, n_centres, size=n)] + sigma * rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), c


def build(x, nlist, metric, iters=4, seed=0):
    from hiprag import HipIVFIndex
    ix = HipIVFIndex(x.shape[1], nlist, metric)
    ix.build(x, iters=iters, seed=seed)
    return ix


def tied_set(n, d, seed):
    """the clustered generator (48 centres, sigma 0.35) with rows 40..59 equal to row 3, and 1000 queries: query 0 IS row 3
    (its best hits tie and are ordered by original id), the rest are noisy rows and noisy centres (skewed list popularity)"""
    x, centres = clustered(n, d, 48, 0.35, seed)
    x[40:60] = x[3]
    rng = np.random.default_rng(seed + 1)
    q = np.concatenate([x[rng.integers(0, n, size=600)] + 0.05 * rng.standard_normal((600, d)),
                        centres[rng.integers(0, 12, size=400)] + 0.35 * rng.standard_normal((400, d))]).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[0] = x[3]
    return x, q


def bits_equal(a, b):
    """two (scores64, scores32, ids) triples: equal ids, equal score BIT PATTERNS"""
    import torch
    return (torch.equal(a[2], b[2]) and torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
            and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def assert_same(ix, qd, k, nprobe, what):
    import torch
    one = ix.search_device(qd, k, nprobe)
    bat = ix.search_batch_device(qd, k, nprobe)
    torch.cuda.synchronize()
    assert bat[0].shape == one[0].shape and bat[2].dtype == one[2].dtype
    assert torch.equal(bat[2], one[2]), f"ids differ: {what}"
    assert torch.equal(bat[0].view(torch.int64), one[0].view(torch.int64)), f"scores64 bits differ: {what}"
    assert torch.equal(bat[1].view(torch.int32), one[1].view(torch.int32)), f"scores32 bits differ: {what}"
    return one, bat


# ---- 1. the one-query path, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_one_query_path_bit_for_bit(gpu, metric, shape):
    import torch
    n, d, nlist, k = shape
    x, q = tied_set(n, d, seed=500 + d)
    ix = build(x, nlist, metric)
    qd = torch.from_numpy(q).cuda()
    for nprobe in (1, 3, nlist - 1, nlist, nlist + 5):
        for nq in NQS:
            one, _ = assert_same(ix, qd[:nq].contiguous(), k, nprobe, f"{shape} {metric} nprobe {nprobe} nq {nq}")
            if nprobe >= nlist and k >= 21:     # the tie block of query 0: row 3 and its 20 copies, ordered by id
                assert one[2][0, :21].tolist() == [3] + list(range(40, 60))
    # k beyond the rows of the probed lists: trailing -1 / +-DBL_MAX must match too
    kk = min(256, int(ix.list_lengths.max()) + 40)
    one, bat = assert_same(ix, qd[:65].contiguous(), kk, 1, f"{shape} {metric} deep k {kk}")
    assert int((bat[2] < 0).sum()) > 0 or kk == 256, "the deep-k case was meant to reach the padding"
    if int((bat[2] < 0).sum()):
        pad = bat[0][bat[2] < 0]
        assert bool((pad == (-np.finfo(np.float64).max if metric == "ip" else np.finfo(np.float64).max)).all())


# ---- 2. the CPU restatement, independent of the one-query kernel -----------------------------------------------------------
def cpu_ivf_search(x, cents, offs, orig, q, k, nprobe, metric):
    """top-nprobe lists by exact score (ties to the lower list), then the exact top-k of their rows"""
    probe = ho.flat_search(cents, q, nprobe, metric)[1]
    ids = np.full((len(q), k), -1, dtype=np.int64)
    for j in range(len(q)):
        rows = np.sort(np.concatenate([orig[offs[l]:offs[l + 1]] for l in probe[j]]))
        rows = rows[rows >= 0]
        local = ho.flat_search(x[rows], q[j:j + 1], k, metric)[1][0]
        ids[j] = np.where(local >= 0, rows[np.maximum(local, 0)], -1)
    return ids


@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
def test_against_the_cpu_ivf_restatement(gpu, metric):
    n, d, nlist, k = 30000, 128, 64, 10
    x, centres = clustered(n, d, 48, 0.35, seed=111)
    rng = np.random.default_rng(112)
    q_rows = x[rng.integers(0, n, size=40)] + 0.05 * rng.standard_normal((40, d))
    q_held = centres[rng.integers(0, len(centres), size=24)] + 0.35 * rng.standard_normal((24, d))
    q = np.concatenate([q_rows, q_held]).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    ix = build(x, nlist, metric, iters=8)
    cents = ix.centroids()
    offs, orig = ix.lists()
    for nprobe in (1, 2, 8, nlist):
        _, i = ix.search_batch(q, k, nprobe=nprobe)
        assert np.array_equal(i, cpu_ivf_search(x, cents, offs, orig, q, k, nprobe, metric)), f"nprobe {nprobe}"
    s, i = ix.search_batch(q, k, nprobe=nlist)
    es, ei = ho.flat_search(x, q, k, metric)
    assert np.array_equal(i, ei) and np.allclose(s, es, rtol=0, atol=1e-4)


# ---- 3. one list for the whole batch; lists nobody probes; empty lists -----------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_all_queries_on_one_list(gpu, metric):
    import torch
    n, d, nlist, k = 30000, 128, 64, 10
    x, _ = clustered(n, d, 48, 0.35, seed=131)
    rng = np.random.default_rng(132)
    q = (x[7] + 0.01 * rng.standard_normal((2000, d))).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    ix = build(x, nlist, metric)
    qd = torch.from_numpy(q).cuda()
    for nprobe in (1, 3):
        assert_same(ix, qd, k, nprobe, f"one list, {metric}, nprobe {nprobe}")


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_empty_lists(gpu, metric):
    import torch
    d, nlist, k = 64, 8, 20
    rng = np.random.default_rng(141)
    vals = rng.standard_normal((5, d)).astype(np.float32)
    vals /= np.linalg.norm(vals, axis=1, keepdims=True)
    x = np.ascontiguousarray(vals[rng.permutation(np.repeat(np.arange(5), [300, 250, 400, 200, 350]))])
    ix = build(x, nlist, metric)
    assert int((ix.list_lengths == 0).sum()) >= 3
    q = np.concatenate([vals, rng.standard_normal((95, d)).astype(np.float32)])
    qd = torch.from_numpy(q).cuda()
    for nprobe in (1, 5, 8):
        one, bat = assert_same(ix, qd, k, nprobe, f"empty lists, {metric}, nprobe {nprobe}")
    ids = bat[2].cpu().numpy()                     # nprobe = nlist: the top 20 of query v are the first 20 copies of value v
    for v in range(5):
        assert np.array_equal(ids[v], np.nonzero((x == vals[v]).all(axis=1))[0][:k])


# ---- 4. chunking --------------------------------------------------------------------------------------------------------
def test_chunked_batch_equals_its_halves(gpu):
    import torch
    n, d, nlist, k, nq = 20000, 64, 16, 10, 40000
    x, _ = clustered(n, d, 48, 0.35, seed=151)
    rng = np.random.default_rng(152)
    q = (x[rng.integers(0, n, size=nq)] + 0.1 * rng.standard_normal((nq, d))).astype(np.float32)
    ix = build(x, nlist, "ip")
    qd = torch.from_numpy(q).cuda()
    whole = ix.search_batch_device(qd, k, nlist)
    info = ix.batch_info()
    assert info["chunks"] > 1 and info["chunk_queries"] * (info["chunks"] - 1) < nq <= info["chunk_queries"] * info["chunks"]
    # every stored row is read once per chunk at nprobe = nlist (lists that hold rows are probed by every query)
    assert info["rows_read"] == info["chunks"] * int(ix.lists()[0][-1])
    a = ix.search_batch_device(qd[:nq // 2].contiguous(), k, nlist)
    b = ix.search_batch_device(qd[nq // 2:].contiguous(), k, nlist)
    torch.cuda.synchronize()
    assert bits_equal(whole, tuple(torch.cat([u, v]) for u, v in zip(a, b)))
    one = ix.search_device(qd[:512].contiguous(), k, nlist)
    torch.cuda.synchronize()
    assert bits_equal(tuple(t[:512] for t in whole), one)


# ---- 5. stream order and repeatability -----------------------------------------------------------------------------------
def test_stream_order_and_repeatability(gpu):
    import torch
    n, d, nlist, k, nprobe = 30000, 128, 64, 10, 4
    x, qall = tied_set(n, d, seed=161)
    ix = build(x, nlist, "l2")
    q1 = torch.from_numpy(qall[:300]).cuda()
    q2 = torch.from_numpy(qall[300:700]).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        r1 = ix.search_batch_device(q1, k, nprobe)
        r2 = ix.search_batch_device(q2, k, nprobe)
    st.synchronize()
    e1 = ix.search_device(q1, k, nprobe)
    e2 = ix.search_device(q2, k, nprobe)
    torch.cuda.synchronize()
    assert bits_equal(r1, e1) and bits_equal(r2, e2)
    again = ix.search_batch_device(q2, k, nprobe)
    torch.cuda.synchronize()
    assert bits_equal(again, r2)


# ---- 6. arguments ---------------------------------------------------------------------------------------------------------
def test_arguments(gpu):
    import torch
    from hiprag import HipIVFIndex, HipRagError
    x = ho.synthetic_vectors(500, 32, seed=5)
    ix = HipIVFIndex(32, 8, "l2")
    with pytest.raises(RuntimeError):
        ix.search_batch(x[:1], 5, 2)                       # not built
    ix.train_add(x)
    qd = torch.from_numpy(x[:2]).cuda()
    with pytest.raises(ValueError):
        ix.search_batch_device(qd, 5)                      # no nprobe and no default, as search_device
    with pytest.raises(HipRagError):
        ix.search_batch_device(qd, 257, 2)
    with pytest.raises(HipRagError):
        ix.search_batch_device(qd, 5, 0)
    null = (torch.empty(0, dtype=torch.float64, device="cuda"), torch.empty(0, dtype=torch.float32, device="cuda"),
            torch.empty(0, dtype=torch.int64, device="cuda"))
    assert null[0].data_ptr() == 0
    for fn in (ix.search_device, ix.search_batch_device):
        with pytest.raises(HipRagError) as e:
            fn(qd, 5, 2, out=null)
        assert "null device pointer" in str(e.value)
    s64, s32, ids = ix.search_batch_device(torch.empty((0, 32), dtype=torch.float32, device="cuda"), 5, 2)
    assert s64.shape == (0, 5) and s32.shape == (0, 5) and ids.shape == (0, 5) and ids.dtype == torch.int64
    s, i = ix.search_batch(x[:3], 5, 8)
    es, ei = ho.flat_search(x, x[:3], 5, ho.METRIC_L2)
    assert np.array_equal(i, ei) and np.allclose(s, es, rtol=0, atol=1e-4)
    ix.nprobe = 8
    assert np.array_equal(ix.search_batch(x[:3], 5)[1], ei)   # the default nprobe
