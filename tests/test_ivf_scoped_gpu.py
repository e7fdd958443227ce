"""
Scoped IVF-Flat search (libhiprag hipivf_search_scoped*, HipIVFIndex.search_scoped*): the top k of the rows that are in a
probed list AND whose id lies in a range of the query's scope.  include/hiprag.h defines the entry by two identities, both
bit for bit on all three outputs: (A) the scope [0, n) gives hipivf_search_batch_dev's result at the same nprobe; (B) at
nprobe >= nlist the result is hipidx_search_scoped_dev's on a flat index of the same rows in id order.  Most cases compare
integer bit patterns against those two entries; one case checks partial nprobe against a CPU restatement that involves
neither; the rest are the edges of the new step (slices, quads, shuffled ids, rows_read, updates, chunks, arguments).
The generators are those of tests/test_ivf_batch_gpu.py and tests/test_scoped_gpu.py.
"""
import ctypes

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

E_INVALID = -1   # include/hiprag.h
SHAPES = [(700, 64, 7, 5), (20011, 256, 37, 50), (6000, 1024, 16, 256)]   # n, d, nlist, k
F64_MAX = np.finfo(np.float64).max
F32_MAX = np.finfo(np.float32).max


def clustered(n, d, n_centres, sigma, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n_centres, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[rng.integers(0, n_centres, size=n)] + sigma * rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), c


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


def random_scope(rng, n, n_ranges):
    """n_ranges non-empty, non-touching-or-touching ranges at random (hence unaligned) cut points, ascending"""
    cuts = np.sort(rng.choice(n + 1, size=2 * n_ranges, replace=False))
    return [(int(cuts[2 * j]), int(cuts[2 * j + 1])) for j in range(n_ranges)]


def mid(metric):
    return ho.METRIC_IP if metric == "ip" else ho.METRIC_L2


def flat_of(x, metric):
    from hiprag import HipFlatIndex
    ix = HipFlatIndex(x.shape[1], metric)
    ix.add(x)
    return ix


def all_padding(out, metric):
    s64, s32, ids = (t.cpu().numpy() for t in out)
    sign = -1.0 if metric == "ip" else 1.0
    return bool((ids == -1).all() and (s64 == sign * F64_MAX).all() and (s32 == sign * F32_MAX).all())


_BUILT = {}


def built(shape, metric):
    """(x, queries on the device, the IVF index) of a shape and metric: built once, shared by the tests, never changed"""
    import torch
    from hiprag import HipIVFIndex
    key = (shape, metric)
    if key not in _BUILT:
        n, d, nlist, _ = shape
        x, q = tied_set(n, d, seed=500 + d)
        ix = HipIVFIndex(d, nlist, metric)
        ix.build(x, iters=4, seed=0)
        _BUILT[key] = (x, torch.from_numpy(q).cuda(), ix)
    return _BUILT[key]


# ---- 1. identity A: the whole scope is the batch search --------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_whole_scope_is_the_batch_search_bit_for_bit(gpu, metric, shape):
    import torch
    n, d, nlist, k = shape
    x, qd, ix = built(shape, metric)
    a = n // 3 + 1
    for nq in (1, 17, 65):
        q = qd[:nq].contiguous()
        for nprobe in (1, 3, nlist, nlist + 5):
            bat = ix.search_batch_device(q, k, nprobe)
            whole = ix.search_scoped_device(q, k, [[(0, n)]], nprobe=nprobe)
            touching = ix.search_scoped_device(q, k, [[(0, a), (a, n)]], nprobe=nprobe)
            torch.cuda.synchronize()
            assert bits_equal(whole, bat), f"[0, n) differs from the batch search: {shape} {metric} nq {nq} nprobe {nprobe}"
            assert bits_equal(touching, bat), f"[0, a) + [a, n) differs from the batch search: {shape} {metric} nq {nq} nprobe {nprobe}"
    s, i = ix.search_scoped(qd[:9].cpu().numpy(), k, [[(0, n)]], nprobe=3)       # the host entry
    want = ix.search_batch_device(qd[:9].contiguous(), k, 3)
    torch.cuda.synchronize()
    assert np.array_equal(i, want[2].cpu().numpy()) and np.array_equal(s.view(np.int32), want[1].cpu().numpy().view(np.int32))


# ---- 2. identity B: every list probed is the flat scoped search -----------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_all_lists_probed_is_the_flat_scoped_search_bit_for_bit(gpu, metric, shape):
    import torch
    n, d, nlist, k = shape
    x, qd, ix = built(shape, metric)
    flat = flat_of(x, metric)
    rng = np.random.default_rng(n + d)
    scopes = [random_scope(rng, n, 5), [(n // 2 + 1, n // 2 + 2)], [], [(n - 1, n)], random_scope(rng, n, 300 if n == 20011 else 40), [(0, n)]]
    q = qd[:40].contiguous()
    soq = (np.arange(40) % len(scopes)).astype(np.int32)      # every list: 40 pairs of mixed scopes = 3 groups per slice
    got = ix.search_scoped_device(q, k, scopes, soq, nprobe=nlist)
    want = flat.search_scoped_device(q, k, scopes, soq)
    torch.cuda.synchronize()
    assert bits_equal(got, want), f"{shape} {metric}"
    assert all_padding(tuple(t[2::6] for t in got), metric), "the empty scope returned a row"
    assert got[2][3].tolist() == [n - 1] + [-1] * (k - 1)
    # the duplicate block of query 0 (row 3 and rows 40..59): in id order inside the scope, absent outside it
    tie = [3] + list(range(40, 60))
    inside = ix.search_scoped_device(q[:1], k, [[(0, 100)]], nprobe=nlist)
    outside = ix.search_scoped_device(q[:1], k, [[(0, 40), (60, n)]], nprobe=nlist)
    w_in = flat.search_scoped_device(q[:1], k, [[(0, 100)]])
    w_out = flat.search_scoped_device(q[:1], k, [[(0, 40), (60, n)]])
    torch.cuda.synchronize()
    assert bits_equal(inside, w_in) and bits_equal(outside, w_out)
    assert inside[2][0, :min(k, 21)].tolist() == tie[:min(k, 21)]
    ids_out = outside[2][0].tolist()
    assert ids_out[0] == 3 and not any(40 <= i < 60 for i in ids_out)


# ---- 3. slice and quad edges over shuffled ids (hipivf_create) -----------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_slice_and_quad_edges_with_shuffled_ids(gpu, metric):
    import torch
    from hiprag import HipIVFIndex
    d, k = 64, 10
    lens = [0, 1, 255, 256, 257, 513]
    nlist, n = len(lens), sum(lens)
    rng = np.random.default_rng(31)
    x = ho.synthetic_vectors(n, d, seed=32)
    perm = rng.permutation(n)                       # ids shuffled across and inside the lists
    offs = np.zeros(nlist + 1, dtype=np.int64)
    for l, m in enumerate(lens):
        offs[l + 1] = offs[l] + (m + 31) // 32 * 32
    orig = np.full(int(offs[-1]), -1, dtype=np.int64)
    at = 0
    for l, m in enumerate(lens):
        orig[offs[l]:offs[l] + m] = perm[at:at + m]
        at += m
    assert not np.all(np.diff(orig[offs[5]:offs[5] + 513]) > 0)
    stored = np.zeros((len(orig), d), dtype=np.float32)
    stored[orig >= 0] = x[orig[orig >= 0]]
    rows, cents = flat_of(stored, metric), flat_of(ho.synthetic_vectors(nlist, d, seed=33), metric)
    ix = HipIVFIndex.from_parts(rows, cents, offs, orig)
    assert ix.ntotal == n
    flat = flat_of(x, metric)
    one_id = int(orig[offs[5] + 256 + 37])          # a row of the second slice of the 513-member list
    scopes = [[(100 + a, 900 + b)] for a in range(4) for b in range(4)] + [[(one_id, one_id + 1)]]
    qd = torch.from_numpy(ho.synthetic_queries(len(scopes), d, seed=34)).cuda()
    got = ix.search_scoped_device(qd, k, scopes, nprobe=nlist)
    want = flat.search_scoped_device(qd, k, scopes)
    torch.cuda.synchronize()
    assert bits_equal(got, want)
    assert got[2][-1].tolist() == [one_id] + [-1] * (k - 1)
    # the whole batch under every scope in turn: groups of 17 members that share each slice
    for s in (0, 5, 15, 16):
        got = ix.search_scoped_device(qd, k, [scopes[s]], nprobe=nlist)
        want = flat.search_scoped_device(qd, k, [scopes[s]])
        torch.cuda.synchronize()
        assert bits_equal(got, want), f"scope {scopes[s]}"
    assert ix.scoped_info()["rows_read"] == 2 * 4   # one quad, 17 members = 2 groups
    ix.close()


# ---- 4. the CPU restatement at partial nprobe ---------------------------------------------------------------------------------
def cpu_ivf_scoped(x, cents, offs, orig, q, k, nprobe, metric, scopes, soq):
    """top-nprobe lists by exact score (ties to the lower list), whatever the scope; then the exact top-k of their rows that
    lie in the query's scope"""
    probe = ho.flat_search(cents, q, nprobe, metric)[1]
    ids = np.full((len(q), k), -1, dtype=np.int64)
    s64 = np.zeros((len(q), k), dtype=np.float64)
    for j in range(len(q)):
        rows = np.sort(np.concatenate([orig[offs[l]:offs[l + 1]] for l in probe[j]]))
        rows = rows[rows >= 0]
        keep = np.zeros(len(rows), dtype=bool)
        for lo, hi in scopes[soq[j]]:
            keep |= (rows >= lo) & (rows < hi)
        rows = rows[keep]
        if len(rows) == 0:
            continue
        _, local, sc = ho.flat_search(x[rows], q[j:j + 1], k, metric, return_f64=True)
        ids[j] = np.where(local[0] >= 0, rows[np.maximum(local[0], 0)], -1)
        s64[j] = sc[0]
    return ids, s64


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_against_the_cpu_restatement_at_partial_nprobe(gpu, metric):
    import torch
    from hiprag import HipIVFIndex
    n, d, nlist, k, nq = 5000, 128, 16, 10, 48
    x, centres = clustered(n, d, 48, 0.35, seed=111)
    rng = np.random.default_rng(112)
    q = np.concatenate([x[rng.integers(0, n, size=30)] + 0.05 * rng.standard_normal((30, d)),
                        centres[rng.integers(0, len(centres), size=18)] + 0.35 * rng.standard_normal((18, d))]).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    ix = HipIVFIndex(d, nlist, metric)
    ix.build(x, iters=8, seed=0)
    cents = ix.centroids()
    offs, orig = ix.lists()
    scopes = [random_scope(rng, n, 3), random_scope(rng, n, 12), random_scope(rng, n, 1)]
    soq = rng.integers(0, 3, size=nq).astype(np.int32)
    qd = torch.from_numpy(q).cuda()
    for nprobe in (1, 2, 8):
        s64, _, ids = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nprobe)
        torch.cuda.synchronize()
        ids, s64 = ids.cpu().numpy(), s64.cpu().numpy()
        e_ids, e_s64 = cpu_ivf_scoped(x, cents, offs, orig, q, k, nprobe, mid(metric), scopes, soq)
        assert np.array_equal(ids, e_ids), f"nprobe {nprobe}"
        err = float(np.max(np.abs(np.where(ids >= 0, s64 - e_s64, 0.0))))
        print(f"{metric} nprobe {nprobe}: max |score64 - oracle| = {err:.3g}")
        assert err <= 1e-4, f"nprobe {nprobe}"


# ---- 5. rows_read and repeatability -------------------------------------------------------------------------------------------
def test_rows_read_counts_the_loaded_quads_and_runs_repeat(gpu):
    import torch
    shape, metric = SHAPES[1], "ip"
    n, d, nlist, k = shape
    x, qd, ix = built(shape, metric)
    nprobe = 3
    q1 = qd[5:6].contiguous()
    offs, orig = ix.lists()
    probe = ho.flat_search(ix.centroids(), q1.cpu().numpy(), nprobe, mid(metric))[1][0]

    def quads(lo, hi):
        total = 0
        for l in probe:
            seg = orig[offs[l]:offs[l + 1]]
            total += int(((seg >= lo) & (seg < hi)).reshape(-1, 4).any(axis=1).sum())
        return total

    lo = int(orig[offs[probe[0]] + min(100, int(ix.list_lengths[probe[0]]) - 1)])   # a member of a probed list: the 40-id range meets it
    got = ix.search_scoped_device(q1, k, [[(lo, lo + 40)]], nprobe=nprobe)
    info = ix.scoped_info()
    assert quads(lo, lo + 40) >= 1 and info["rows_read"] == 4 * quads(lo, lo + 40)
    assert info["group_queries"] == 16 and info["chunks"] == 1 and info["chunk_queries"] == 1
    inside = got[2][0][got[2][0] >= 0].tolist()
    assert inside and all(lo <= i < lo + 40 for i in inside)
    # a scope that meets no probed list: one id of a list the query does not probe
    other = next(l for l in range(nlist) if l not in probe and ix.list_lengths[l] > 0)
    away = int(orig[offs[other]])
    got = ix.search_scoped_device(q1, k, [[(away, away + 1)]], nprobe=nprobe)
    assert ix.scoped_info()["rows_read"] == 0 and all_padding(got, metric)
    # the whole scope: every quad of the probed lists that holds a row, where the batch search reads their stored rows
    ix.search_batch_device(q1, k, nprobe)
    assert ix.batch_info()["rows_read"] == sum(int(offs[l + 1] - offs[l]) for l in probe)
    ix.search_scoped_device(q1, k, [[(0, n)]], nprobe=nprobe)
    assert ix.scoped_info()["rows_read"] == sum((int(ix.list_lengths[l]) + 3) // 4 * 4 for l in probe) == 4 * quads(0, n)
    # two runs on a non-default stream, no host synchronisation in between
    rng = np.random.default_rng(7)
    scopes = [random_scope(rng, n, 7), [(0, n)], random_scope(rng, n, 2)]
    soq = (np.arange(65) % 3).astype(np.int32)
    q65 = qd[:65].contiguous()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        r1 = ix.search_scoped_device(q65, k, scopes, soq, nprobe=nprobe)
        r2 = ix.search_scoped_device(q65, k, scopes, soq, nprobe=nprobe)
    st.synchronize()
    assert bits_equal(r1, r2)
    assert ix.scoped_info()["rows_read"] > 0


# ---- 6. after updates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_after_add_and_remove_ranges(gpu, metric):
    import torch
    from hiprag import HipIVFIndex
    d, nlist, k = 64, 8, 20
    x, _ = clustered(3500, d, 48, 0.35, seed=61)
    trained = HipIVFIndex(d, nlist, metric)
    trained.build(x[:1500], iters=4, seed=0)
    ix = HipIVFIndex.from_centroids(trained.centroids(), metric)
    trained.close()
    rng = np.random.default_rng(62)
    qd = torch.from_numpy(ho.synthetic_queries(33, d, seed=63)).cuda()

    def check(rows, tag):
        m = len(rows)
        assert ix.ntotal == m
        flat = flat_of(rows, metric)
        scopes = [random_scope(rng, m, 5), [(0, m)], [(m - 1, m)]]
        soq = (np.arange(33) % 3).astype(np.int32)
        got = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nlist)
        want = flat.search_scoped_device(qd, k, scopes, soq)
        torch.cuda.synchronize()
        assert bits_equal(got, want), tag

    ix.add(x[:3000])
    check(x[:3000], "after the first add")           # also makes the per-list tables the updates below must invalidate
    ix.remove_ranges([(100, 700), (2000, 2901)])
    keep = np.concatenate([x[:100], x[700:2000], x[2901:3000]])
    check(keep, "after remove_ranges")
    ix.add(torch.from_numpy(x[3000:3500]).cuda())
    check(np.concatenate([keep, x[3000:3500]]), "after the second add")


# ---- 7. chunking ----------------------------------------------------------------------------------------------------------------
def test_chunked_call_equals_its_halves(gpu):
    import torch
    from hiprag import HipIVFIndex
    n, d, nlist, k, nq = 20000, 64, 4, 256, 2400      # long lists and k = 256: about 1600 queries fill the workspace budget
    x, _ = clustered(n, d, 48, 0.35, seed=151)
    rng = np.random.default_rng(152)
    q = (x[rng.integers(0, n, size=nq)] + 0.1 * rng.standard_normal((nq, d))).astype(np.float32)
    ix = HipIVFIndex(d, nlist, "ip")
    ix.build(x, iters=4, seed=0)
    qd = torch.from_numpy(q).cuda()
    scopes = [[(1000, 9000)], random_scope(rng, n, 9)]
    soq = (np.arange(nq) % 2).astype(np.int32)
    whole = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nlist)
    info = ix.scoped_info()
    assert info["chunks"] >= 2 and info["chunk_queries"] * (info["chunks"] - 1) < nq <= info["chunk_queries"] * info["chunks"]
    h = nq // 2
    a = ix.search_scoped_device(qd[:h].contiguous(), k, scopes, soq[:h], nprobe=nlist)
    b =ix.search_scoped_device(qd[h:].contiguous(), k, scopes, soq[h:], nprobe=nlist)
    torch.cuda.synchronize()
    assert bits_equal(whole, tuple(torch.cat([u, v]) for u, v in zip(a, b)))
    want = flat_of(x, "ip").search_scoped_device(qd[:64].contiguous(), k, scopes, soq[:64])
    torch.cuda.synchronize()
    assert bits_equal(tuple(t[:64] for t in whole), want)


# ---- 8. the checks ------------------------------------------------------------------------------------------------------------
def test_errors_name_the_argument_and_leave_the_index_usable(gpu):
    import torch
    from hiprag import HipIVFIndex, HipRagError
    from hiprag import _native as nat
    n, d, nlist, k, nq = 1000, 64, 8, 5, 3
    x = ho.synthetic_vectors(n, d, seed=95)
    ix = HipIVFIndex(d, nlist, "ip")
    ix.build(x, iters=2, seed=0)
    qd = torch.from_numpy(ho.synthetic_queries(nq, d, seed=96)).cuda()
    o64 = torch.empty((nq, k), dtype=torch.float64, device="cuda")
    o32 = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    oid = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(q=qd.data_ptr(), nq_=nq, k_=k, nprobe=2, ranges=((0, 10), (20, 30)), offsets=(0, 1, 2), n_scopes=2, soq=(0, 1, 1),
            s64=o64.data_ptr(), s32=o32.data_ptr(), ids=oid.data_ptr(), null=()):
        r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
        o = np.asarray(offsets, dtype=np.int32)
        sq = np.asarray(soq, dtype=np.int32)
        nat.call("hipivf_search_scoped_dev", ix._h, q, nq_, k_, nprobe, None if "ranges" in null else r.ctypes.data,
                 None if "scope_offsets" in null else o.ctypes.data, n_scopes, None if "scope_of_query" in null else sq.ctypes.data,
                 s64, s32, ids, st)

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
        (dict(nprobe=0), "nprobe"),
        (dict(nprobe=1001), "nprobe"),
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
    with pytest.raises(HipRagError) as e:
        nat.call("hipivf_scoped_info", ix._h, None)
    assert e.value.code == E_INVALID and "out4" in str(e.value)
    # overlapping ranges in DIFFERENT scopes, touching ranges, descending order across scopes, no fp32 output: all valid
    raw(ranges=((0, 10), (5, 30)))
    raw(ranges=((0, 10), (10, 30)), offsets=(0, 2, 2))
    raw(ranges=((500, 600), (0, 10)))
    raw(s32=None)
    with pytest.raises(ValueError):
        ix.search_scoped(np.zeros((3, d), np.float32), k, [[(0, 1)], [(1, 2)]], nprobe=2)      # 2 scopes, 3 queries, no map
    with pytest.raises(ValueError):
        ix.search_scoped_device(qd, k, [[(0, n)]])                                             # no nprobe and no default
    got = ix.search_scoped_device(qd, k, [[(0, n)]], nprobe=2)
    want = ix.search_batch_device(qd, k, 2)
    torch.cuda.synchronize()
    assert bits_equal(got, want)
    ix.nprobe = nlist                                                                          # the default nprobe
    s, i = ix.search_scoped(qd.cpu().numpy(), k, [[(0, n)]])
    es, ei = ho.flat_search(x, qd.cpu().numpy(), k, ho.METRIC_IP)
    assert np.array_equal(i, ei) and np.allclose(s, es, rtol=0, atol=1e-4)
