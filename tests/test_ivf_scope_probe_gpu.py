"""
Scope-aware probing of the scoped IVF-Flat search (libhiprag hipivf_search_scoped_probe*, HipIVFIndex.search_scoped*(...,
probe="scope")): query i probes the first min(nprobe, member lists of its scope) MEMBER lists of its coarse order, a member
list being one that stores a row of the scope.  include/hiprag.h defines the mode by four identities, all bit for bit on the
three outputs: (P0) mode 0 is hipivf_search_scoped_dev; (P1) where every list is a member list the two modes agree; (P2) at
nprobe >= the member lists the result is the flat scoped search's; (P3) row i is hipivf_search_scoped_dev's at nprobe =
p'_i, the depth of the coarse order that holds the probed member lists.  The cases compare integer bit patterns against
those entries; one case restates the selection in numpy; the rest are the edges of the two new kernels (controlled lists from
from_centroids + add), the counters, updates, chunking and the argument checks.
The data is clustered with DOCUMENT-COHERENT ids (consecutive blocks of ids are drawn around one centre), so a scope of a few
blocks has only a few member lists: every test that relies on it asserts it.
"""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -6   # include/hiprag.h
SHAPES = [(700, 64, 7, 5), (20011, 256, 37, 50), (6000, 1024, 16, 256)]   # n, d, nlist, k: tests/test_ivf_scoped_gpu.py
F64_MAX = np.finfo(np.float64).max
F32_MAX = np.finfo(np.float32).max


def block_of(n, nlist):
    return max(20, n // (6 * nlist))


def coherent(n, d, nlist, seed):
    """3 nlist unit centres; block b of block_of(n, nlist) consecutive ids = one centre + noise of norm about 0.3"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((3 * nlist, d))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    blk = block_of(n, nlist)
    centre = np.repeat(rng.integers(0, len(c), size=(n + blk - 1) // blk), blk)[:n]
    x = c[centre] + (0.3 / np.sqrt(d)) * rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = np.concatenate([x[rng.integers(0, n, size=48)] + (0.2 / np.sqrt(d)) * rng.standard_normal((48, d)),
                        c[rng.integers(0, len(c), size=17)] + (0.6 / np.sqrt(d)) * rng.standard_normal((17, d))])
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return x.astype(np.float32), q.astype(np.float32)


def bits_equal(a, b):
    import torch
    return (torch.equal(a[2], b[2]) and torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
            and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def rows_equal(a, b, rows):
    import torch
    r = torch.as_tensor(rows, device=a[0].device)
    return bits_equal(tuple(t[r] for t in a), b)


def all_padding(out, metric):
    s64, s32, ids = (t.cpu().numpy() for t in out)
    sign = -1.0 if metric == "ip" else 1.0
    return bool((ids == -1).all() and (s64 == sign * F64_MAX).all() and (s32 == sign * F32_MAX).all())


def flat_of(x, metric):
    from hiprag import HipFlatIndex
    ix = HipFlatIndex(x.shape[1], metric)
    ix.add(x)
    return ix


def members_of(offs, orig, scope):
    """the member lists of a scope, in numpy: lists with a stored row (padding is -1) whose id lies in a range"""
    out = []
    for l in range(len(offs) - 1):
        seg = orig[offs[l]:offs[l + 1]]
        if any(((seg >= lo) & (seg < hi)).any() for lo, hi in scope):
            out.append(l)
    return out


def depth_of(order, members, nprobe, nlist):
    """p' of include/hiprag.h: the shortest prefix of the coarse order that holds min(nprobe, members) member lists"""
    want = min(nprobe, len(members))
    if want == 0:
        return nlist
    seen = 0
    for p, l in enumerate(order):
        seen += int(l) in members
        if seen == want:
            return p + 1
    raise AssertionError("the coarse order does not hold every list")


def expected_info(member_sets, soq, nprobe, nlist, chunk=None):
    """hipivf_scope_probe_info in numpy: member pairs, probed slots, chunks, 4 x the centroid quads a group of 16 loads"""
    nq = len(soq)
    chunk = chunk or nq
    rows = 0
    for c0 in range(0, nq, chunk):
        for g0 in range(c0, min(nq, c0 + chunk), 16):
            quads = set()
            for i in range(g0, min(g0 + 16, c0 + chunk, nq)):
                quads |= {l // 4 for l in member_sets[soq[i]]}
            rows += 4 * len(quads)
    return {"member_pairs": sum(len(m) for m in member_sets), "probed_slots": sum(min(nprobe, nlist, len(member_sets[s])) for s in soq),
            "chunks": (nq + chunk - 1) // chunk, "centroid_rows_read": rows}


def check_p3(ix, coarse, qd, k, scopes, soq, nprobe, tag):
    """(P3) for every query of the call, grouped by p'; returns the scope-mode result and the member lists of every scope"""
    import torch
    offs, orig = ix.lists()
    msets = [set(members_of(offs, orig, s)) for s in scopes]
    coarse_order = coarse.search(qd.cpu().numpy(), ix.nlist)[1]
    got = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nprobe, probe="scope")
    depth = np.array([depth_of(coarse_order[i], msets[soq[i]], nprobe, ix.nlist) for i in range(len(soq))])
    for p in np.unique(depth):
        rows = np.flatnonzero(depth == p)
        want = ix.search_scoped_device(qd[torch.as_tensor(rows, device=qd.device)].contiguous(), k, scopes, soq[rows], nprobe=int(p))
        torch.cuda.synchronize()
        assert rows_equal(got, want, rows), f"{tag}: the queries of p' = {p} ({rows.tolist()})"
    return got, msets, depth


_BUILT = {}


def built(shape, metric):
    """of a shape and metric, built once, shared, never changed: rows, queries (device), the IVF index, the flat index of the
    rows, the flat index of the centroids (the coarse order), the scopes and the member lists of each"""
    import torch
    from hiprag import HipIVFIndex
    key = (shape, metric)
    if key not in _BUILT:
        n, d, nlist, _ = shape
        x, q = coherent(n, d, nlist, seed=900 + d)
        ix = HipIVFIndex(d, nlist, metric)
        ix.build(x, iters=6, seed=0)
        b = block_of(n, nlist)
        scopes = [[(3 * b, 5 * b)],                                        # two blocks
                  [(0, b), (7 * b + 3, 8 * b - 2), (n - b // 2, n)],       # three pieces far apart
                  [(3 * b, 5 * b), (9 * b, 10 * b)],                       # shares a range with scope 0
                  [(5 * b + 1, 5 * b + 2)],                                # one id
                  [],                                                      # empty
                  [(2 * b, 2 * b), (6 * b, 6 * b + 7)]]                    # an empty range and a short one
        offs, orig = ix.lists()
        msets = [set(members_of(offs, orig, s)) for s in scopes]
        _BUILT[key] = (x, torch.from_numpy(q).cuda(), ix, flat_of(x, metric), flat_of(ix.centroids(), metric), scopes, msets)
    return _BUILT[key]


SHAPE_IDS = dict(ids=lambda s: "x".join(map(str, s)))


# ---- P0: mode 0 is the scoped search -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("shape", SHAPES, **SHAPE_IDS)
def test_p0_probe_any_is_the_scoped_search_bit_for_bit(gpu, metric, shape):
    import torch
    n, d, nlist, k = shape
    x, qd, ix, flat, coarse, scopes, msets = built(shape, metric)
    soq = (np.arange(len(qd)) % len(scopes)).astype(np.int32)
    for nprobe in (1, 3, nlist + 5):
        a = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nprobe)
        b = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nprobe, probe="any")
        c = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nprobe, probe=0)
        torch.cuda.synchronize()
        assert bits_equal(a, b) and bits_equal(a, c), f"{shape} {metric} nprobe {nprobe}"
    from hiprag import _native as nat
    from hiprag.index import pack_scopes
    ranges, offsets, sq = pack_scopes(scopes, soq, len(qd))
    out = (torch.empty((len(qd), k), dtype=torch.float64, device="cuda"), torch.empty((len(qd), k), dtype=torch.float32, device="cuda"),
           torch.empty((len(qd), k), dtype=torch.int64, device="cuda"))
    nat.call("hipivf_search_scoped_probe_dev", ix._h, qd.data_ptr(), len(qd), k, 3, 0, ranges.ctypes.data, offsets.ctypes.data,
             len(offsets) - 1, sq.ctypes.data, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None)
    want = ix.search_scoped_device(qd, k, scopes, soq, nprobe=3)
    torch.cuda.synchronize()
    assert bits_equal(out, want), "the probe entry at mode 0"


# ---- P1: every list a member list ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("shape", SHAPES, **SHAPE_IDS)
def test_p1_where_every_list_is_a_member_the_modes_agree(gpu, metric, shape):
    import torch
    n, d, nlist, k = shape
    from hiprag import HipIVFIndex
    x, qd, built_ix, flat, coarse, scopes, msets = built(shape, metric)
    # (P1) needs an index without an empty list.  A k-means build may leave one; a list that attracts no row can be taken
    # out without moving any other row, so the index under test is the built centroids that have rows, and the rows again
    keep = np.flatnonzero(built_ix.list_lengths > 0)
    ix = HipIVFIndex.from_centroids(built_ix.centroids()[keep], metric)
    ix.add(x)
    nlist = ix.nlist
    offs, orig = ix.lists()
    firsts = sorted(int(orig[offs[l]]) for l in range(nlist) if offs[l + 1] > offs[l] and orig[offs[l]] >= 0)
    touch_all = [(i, i + 1) for i in firsts]             # the first id of every list
    assert len(firsts) == nlist == len(members_of(offs, orig, touch_all)) == len(members_of(offs, orig, [(0, n)]))
    for sc in ([[(0, n)]], [touch_all], [[(0, n)], touch_all]):
        soq = (np.arange(len(qd)) % len(sc)).astype(np.int32)
        for nprobe in (1, 3, nlist):
            a = ix.search_scoped_device(qd, k, sc, soq, nprobe=nprobe, probe="scope")
            b = ix.search_scoped_device(qd, k, sc, soq, nprobe=nprobe, probe="any")
            torch.cuda.synchronize()
            assert bits_equal(a, b), f"{shape} {metric} nprobe {nprobe}"
    ix.close()


# ---- P2: nprobe >= the member lists is the exact scoped search --------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("shape", SHAPES, **SHAPE_IDS)
def test_p2_at_the_member_count_the_result_is_the_flat_scoped_search(gpu, metric, shape):
    import torch
    n, d, nlist, k = shape
    x, qd, ix, flat, coarse, scopes, msets = built(shape, metric)
    counts = [len(m) for m in msets]
    print(f"{shape} {metric}: member lists per scope {counts} of {nlist}")
    assert all(c < nlist for c in counts) and max(counts) >= 2, "the scopes must have fewer member lists than nlist"
    soq = (np.arange(len(qd)) % len(scopes)).astype(np.int32)
    want = flat.search_scoped_device(qd, k, scopes, soq)
    for nprobe in (max(counts), nlist):
        got = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nprobe, probe="scope")
        torch.cuda.synchronize()
        assert bits_equal(got, want), f"{shape} {metric} nprobe {nprobe}"
    # one scope at exactly its own member count, where PROBE_ANY at that nprobe is NOT exact for some query
    s = int(np.argmax(counts))
    got = ix.search_scoped_device(qd, k, [scopes[s]], nprobe=counts[s], probe="scope")
    want1 = flat.search_scoped_device(qd, k, [scopes[s]])
    torch.cuda.synchronize()
    assert bits_equal(got, want1)
    assert all_padding(tuple(t[4::6] for t in ix.search_scoped_device(qd, k, scopes, soq, nprobe=1, probe="scope")), metric)
    s_host, i_host = ix.search_scoped(qd[:9].cpu().numpy(), k, scopes, soq[:9], nprobe=max(counts), probe="scope")   # the host entry
    assert np.array_equal(i_host, want[2][:9].cpu().numpy())
    assert np.array_equal(s_host.view(np.int32), want[1][:9].cpu().numpy().view(np.int32))


# ---- P3: every query against the scoped search at its own depth ------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("shape", SHAPES, **SHAPE_IDS)
def test_p3_every_query_is_the_scoped_search_at_its_own_depth(gpu, metric, shape):
    n, d, nlist, k = shape
    x, qd, ix, flat, coarse, scopes, msets = built(shape, metric)
    rng = np.random.default_rng(n)
    soq = rng.integers(0, len(scopes), size=len(qd)).astype(np.int32)      # mixed scopes inside every group of 16
    deeper = 0
    for nprobe in (1, 2):
        _, _, depth = check_p3(ix, coarse, qd, k, scopes, soq, nprobe, f"{shape} {metric} nprobe {nprobe}")
        deeper += int((depth > nprobe).sum())
    assert deeper > 0, "no query probed past nprobe lists of its coarse order: the scopes are not selective"


# ---- the numpy restatement at partial nprobe ---------------------------------------------------------------------------------
def ranges_of(ids):
    ids = np.sort(np.asarray(ids, dtype=np.int64))
    if len(ids) == 0:
        return []
    cut = np.flatnonzero(np.diff(ids) > 1)
    lo = np.concatenate([[ids[0]], ids[cut + 1]])
    hi = np.concatenate([ids[cut], [ids[-1]]]) + 1
    return [(int(a), int(b)) for a, b in zip(lo, hi)]


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_against_the_numpy_restatement_at_partial_nprobe(gpu, metric):
    """The selection restated on the host: the coarse order from the fp64 oracle over centroids(), the member lists and the
    candidate rows (the in-scope rows of the first min(nprobe, members) member lists) from lists() in numpy.  The exact top k
    of a query's candidate rows is then the flat scoped search over exactly those ids -- the entry that defines a row's score
    bits -- so the ids must be exact and the scores bit-equal."""
    import torch
    shape = SHAPES[1]
    n, d, nlist, k = shape
    x, qd, ix, flat, coarse, scopes, msets = built(shape, metric)
    offs, orig = ix.lists()
    order = ho.flat_search(ix.centroids(), qd.cpu().numpy(), nlist, ho.METRIC_IP if metric == "ip" else ho.METRIC_L2)[1]
    rng = np.random.default_rng(5)
    soq = rng.integers(0, len(scopes), size=len(qd)).astype(np.int32)
    for nprobe in (1, 2, 3):
        cand_scopes = []
        for i in range(len(qd)):
            probes = [int(l) for l in order[i] if int(l) in msets[soq[i]]][:nprobe]
            ids = []
            for l in probes:
                seg = orig[offs[l]:offs[l + 1]]
                for lo, hi in scopes[soq[i]]:
                    ids.extend(seg[(seg >= lo) & (seg < hi)].tolist())
            cand_scopes.append(ranges_of(ids))
        got = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nprobe, probe="scope")
        want = flat.search_scoped_device(qd, k, cand_scopes, np.arange(len(qd), dtype=np.int32))
        torch.cuda.synchronize()
        assert bits_equal(got, want), f"{metric} nprobe {nprobe}"


# ---- edges: controlled lists from from_centroids + add ----------------------------------------------------------------------
EDGE_LENS = {0: 32, 1: 33, 2: 256, 3: 257, 6: 5, 7: 40}      # list -> rows of the first batch; 4 duplicates 3, 5 attracts no row
EDGE_NLIST, EDGE_D = 9, 64


def edge_index(metric):
    """centroid l = the unit vector e_l, centroid 4 = centroid 3 (the lower list wins the tie: list 4 stays empty and ranks
    right behind 3), no row near e_5 or e_8.  Ids: the lists of EDGE_LENS one after the other (0..622), then 20 rows that
    alternate between lists 6 and 7 (623..642)."""
    from hiprag import HipIVFIndex
    rng = np.random.default_rng(77)
    cents = np.eye(EDGE_NLIST, EDGE_D, dtype=np.float32)
    cents[4] = cents[3]
    owner = np.concatenate([np.full(m, l) for l, m in EDGE_LENS.items()] + [np.tile([6, 7], 10)])
    x = cents[owner] + 0.02 * rng.standard_normal((len(owner), EDGE_D)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    ix = HipIVFIndex.from_centroids(cents, metric)
    ix.add(x)
    offs, orig = ix.lists()
    for l in range(EDGE_NLIST):
        seg = orig[offs[l]:offs[l + 1]]
        assert sorted(seg[seg >= 0].tolist()) == np.flatnonzero(owner == l).tolist(), f"list {l} is not what the test controls"
    return ix, x.astype(np.float32), cents, owner


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_edges_of_membership_and_probe_selection(gpu, metric):
    import torch
    ix, x, cents, owner = edge_index(metric)
    n, nlist, k = len(x), EDGE_NLIST, 12
    flat, coarse = flat_of(x, metric), flat_of(cents, metric)
    offs, orig = ix.lists()
    first = {l: int(np.flatnonzero(owner == l)[0]) for l in EDGE_LENS}
    last = {l: int(np.flatnonzero(owner == l)[-1]) for l in EDGE_LENS}
    assert (first[2], last[3], first[6]) == (65, 577, 578)
    scopes = [[(30, 70)],                     # 0: lists 0, 1, 2 -> 3 member lists
              [(60, 70)],                     # 1: lists 1, 2
              [(first[2], first[2] + 5)],     # 2: begins on list 2's first id
              [(last[3] - 7, last[3] + 1)],   # 3: ends on list 3's last id
              [(624, 625)],                   # 4: between the consecutive ids 623 and 625 of list 6 -> list 7 alone
              [(100, 100)],                   # 5: an empty range
              [],                             # 6: an empty scope
              [(0, n)],                       # 7: every non-empty list
              [(31, 33), (320, 322), (640, n)],   # 8: the last id of list 0 / first of 1, last of 2 / first of 3, lists 6 and 7
              [(30, 70), (100, 100)]]         # 9: shares a range with scope 0
    want_members = [{0, 1, 2}, {1, 2}, {2}, {3}, {7}, set(), set(), {0, 1, 2, 3, 6, 7}, {0, 1, 2, 3, 6, 7}, {0, 1, 2}]
    assert [set(members_of(offs, orig, s)) for s in scopes] == want_members
    rng = np.random.default_rng(78)
    q = np.concatenate([cents[[3, 3, 2, 0, 7, 6, 5, 8]], x[rng.integers(0, n, size=9)]]).astype(np.float32)
    q += 0.05 * rng.standard_normal(q.shape).astype(np.float32)
    q[0] = cents[3]                           # lists 3 and 4 tie at the top of its coarse order, 3 first
    assert coarse.search(q[:1], 2)[1][0].tolist() == [3, 4]
    qall = torch.from_numpy(q).cuda()
    for nq in (1, 16, 17):
        qd = qall[:nq].contiguous()
        for soq in (np.full(nq, 7, dtype=np.int32), (np.arange(nq) % len(scopes)).astype(np.int32),
                    ((np.arange(nq) * 7 + 3) % len(scopes)).astype(np.int32)):
            for nprobe in (1, 2, 3, 4, nlist + 5):       # scope 0: member lists = nprobe - 1, nprobe, ... ; nprobe > nlist
                tag = f"{metric} nq {nq} nprobe {nprobe} scopes {soq.tolist()}"
                got, msets, _ = check_p3(ix, coarse, qd, k, scopes, soq, nprobe, tag)
                assert msets == want_members
                info = ix.scope_probe_info()
                assert info == expected_info(msets, soq, nprobe, nlist), tag
                again = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nprobe, probe="scope")
                torch.cuda.synchronize()
                assert bits_equal(got, again) and ix.scope_probe_info() == info, f"{tag}: the second run differs"
                if nprobe >= 6:                           # every member list of every scope: the exact scoped search
                    want = flat.search_scoped_device(qd, k, scopes, soq)
                    torch.cuda.synchronize()
                    assert bits_equal(got, want), tag
                for s in (5, 6):
                    rows = np.flatnonzero(soq == s)
                    if len(rows):
                        r = torch.as_tensor(rows, device="cuda")
                        assert all_padding(tuple(t[r] for t in got), metric), f"{tag}: scope {s} returned a row"
    # nprobe = 3 is exact for the scopes of at most 3 member lists; list 4 (empty, second in query 0's order) is never counted
    small = [s for s in range(len(scopes)) if len(want_members[s]) <= 3]
    soq = np.array(small * 3, dtype=np.int32)[:17]
    got = ix.search_scoped_device(qall, k, scopes, soq, nprobe=3, probe="scope")
    want = flat.search_scoped_device(qall, k, scopes, soq)
    torch.cuda.synchronize()
    assert bits_equal(got, want)
    got = ix.search_scoped_device(qall[:1].contiguous(), k, [scopes[8]], nprobe=6, probe="scope")
    want = flat.search_scoped_device(qall[:1].contiguous(), k, [scopes[8]])
    torch.cuda.synchronize()
    assert bits_equal(got, want)
    assert ix.scope_probe_info() == {"member_pairs": 6, "probed_slots": 6, "chunks": 1, "centroid_rows_read": 8}
    ix.close()


# ---- after updates: the device copy of the list lengths follows them ------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_p2_and_p3_after_add_and_remove_ranges(gpu, metric):
    import torch
    from hiprag import HipIVFIndex
    d, nlist, k = 64, 8, 20
    x, q = coherent(3500, d, nlist, seed=61)
    trained = HipIVFIndex(d, nlist, metric)
    trained.build(x[:1500], iters=4, seed=0)
    ix = HipIVFIndex.from_centroids(trained.centroids(), metric)
    coarse = flat_of(trained.centroids(), metric)
    trained.close()
    qd = torch.from_numpy(q[:33]).cuda()
    soq = (np.arange(33) % 4).astype(np.int32)

    def check(rows, tag):
        m = len(rows)
        assert ix.ntotal == m
        flat = flat_of(rows, metric)
        scopes = [[(m // 2, m // 2 + 60)], [(10, 40), (m - 50, m)], [(m - 1, m)], [(m // 2, m // 2 + 60), (m // 2 + 200, m // 2 + 230)]]
        got, msets, _ = check_p3(ix, coarse, qd, k, scopes, soq, 1, tag)
        counts = [len(s) for s in msets]
        assert max(counts) < nlist, f"{tag}: member lists {counts}"
        got = ix.search_scoped_device(qd, k, scopes, soq, nprobe=max(counts), probe="scope")
        want = flat.search_scoped_device(qd, k, scopes, soq)
        torch.cuda.synchronize()
        assert bits_equal(got, want), f"{tag}: P2"
        assert ix.scope_probe_info()["member_pairs"] == sum(counts)

    ix.search_scoped_device(qd, k, [[]], nprobe=2, probe="scope")        # the empty index: the lengths are known to be zero
    assert ix.scope_probe_info()["member_pairs"] == 0
    ix.add(x[:3000])
    check(x[:3000], "after the first add")
    ix.remove_ranges([(100, 700), (2000, 2901)])
    keep = np.concatenate([x[:100], x[700:2000], x[2901:3000]])
    check(keep, "after remove_ranges")
    ix.add(torch.from_numpy(x[3000:3500]).cuda())
    check(np.concatenate([keep, x[3000:3500]]), "after the second add")
    ix.close()


# ---- chunking ---------------------------------------------------------------------------------------------------------------------
def test_chunked_call_equals_its_halves(gpu):
    import torch
    from hiprag import HipIVFIndex
    n, d, nlist, k, nq = 20000, 64, 4, 256, 2400      # tests/test_ivf_scoped_gpu.py: long lists and k = 256 fill the budget
    x, _ = coherent(n, d, 16, seed=151)
    rng = np.random.default_rng(152)
    q = (x[rng.integers(0, n, size=nq)] + 0.02 * rng.standard_normal((nq, d))).astype(np.float32)
    ix = HipIVFIndex(d, nlist, "ip")
    ix.build(x, iters=4, seed=0)
    qd = torch.from_numpy(q).cuda()
    scopes = [[(1000, 1200)], [(5000, 5100), (15000, 15200)]]
    soq = (np.arange(nq) % 2).astype(np.int32)
    whole = ix.search_scoped_device(qd, k, scopes, soq, nprobe=nlist, probe="scope")   # every slot of the partial lists: the budget
    info, sinfo = ix.scope_probe_info(), ix.scoped_info()
    assert info["chunks"] == sinfo["chunks"] >= 2 and sinfo["chunk_queries"] * (info["chunks"] - 1) < nq
    offs, orig = ix.lists()
    msets = [set(members_of(offs, orig, s)) for s in scopes]
    assert info == expected_info(msets, soq, nlist, nlist, chunk=sinfo["chunk_queries"])
    h = nq // 2
    a = ix.search_scoped_device(qd[:h].contiguous(), k, scopes, soq[:h], nprobe=nlist, probe="scope")
    b = ix.search_scoped_device(qd[h:].contiguous(), k, scopes, soq[h:], nprobe=nlist, probe="scope")
    torch.cuda.synchronize()
    assert bits_equal(whole, tuple(torch.cat([u, v]) for u, v in zip(a, b)))
    want = flat_of(x, "ip").search_scoped_device(qd[:64].contiguous(), k, scopes, soq[:64])
    got = ix.search_scoped_device(qd[:64].contiguous(), k, scopes, soq[:64], nprobe=nlist, probe="scope")
    torch.cuda.synchronize()
    assert bits_equal(got, want)
    ix.close()


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def test_errors_name_the_argument_and_leave_the_index_usable(gpu):
    import torch
    from hiprag import HipIVFIndex, HipRagError
    shape, metric = SHAPES[0], "ip"
    n, d, nlist, k = shape
    x, qd, ix, flat, coarse, scopes, msets = built(shape, metric)
    q = qd[:3].contiguous()
    good = ix.search_scoped_device(q, k, [scopes[0]], nprobe=2, probe="scope")
    torch.cuda.synchronize()
    for bad in (2, -1):
        with pytest.raises(HipRagError, match="probe_mode") as e:
            ix.search_scoped_device(q, k, [scopes[0]], nprobe=2, probe=bad)
        assert e.value.code == E_INVALID
        with pytest.raises(HipRagError, match="probe_mode") as e:
            ix.search_scoped(q.cpu().numpy(), k, [scopes[0]], nprobe=2, probe=bad)
        assert e.value.code == E_INVALID
    with pytest.raises(ValueError, match="probe"):
        ix.search_scoped_device(q, k, [scopes[0]], nprobe=2, probe="project")
    for kwargs, word in ((dict(nprobe=0), "nprobe"), (dict(nprobe=2, k=257), "k must")):
        with pytest.raises(HipRagError, match=word) as e:
            ix.search_scoped_device(q, kwargs.pop("k", k), [scopes[0]], probe="scope", **kwargs)
        assert e.value.code == E_INVALID
    with pytest.raises(HipRagError, match="ranges") as e:
        ix.search_scoped_device(q, k, [[(0, n + 1)]], nprobe=2, probe="scope")
    assert e.value.code == E_INVALID
    again = ix.search_scoped_device(q, k, [scopes[0]], nprobe=2, probe="scope")
    torch.cuda.synchronize()
    assert bits_equal(good, again)
    # a from_parts handle whose ids are shuffled inside the lists: UNSUPPORTED in mode 1, an answer in mode 0
    offs, orig = ix.lists()
    rng = np.random.default_rng(3)
    shuffled = orig.copy()
    for l in range(nlist):
        m = int((orig[offs[l]:offs[l + 1]] >= 0).sum())
        shuffled[offs[l]:offs[l] + m] = rng.permutation(orig[offs[l]:offs[l] + m])
    assert not np.array_equal(shuffled, orig)
    stored = np.zeros((len(shuffled), d), dtype=np.float32)
    stored[shuffled >= 0] = x[shuffled[shuffled >= 0]]
    rows, cents = flat_of(stored, metric), flat_of(ix.centroids(), metric)
    parts = HipIVFIndex.from_parts(rows, cents, offs, shuffled)
    for _ in range(2):
        with pytest.raises(HipRagError, match="HIPIVF_PROBE_SCOPE") as e:
            parts.search_scoped_device(q, k, [scopes[0]], nprobe=2, probe="scope")
        assert e.value.code == E_UNSUPPORTED
        any0 = parts.search_scoped_device(q, k, [scopes[0]], nprobe=2, probe="any")
        want = ix.search_scoped_device(q, k, [scopes[0]], nprobe=2)
        torch.cuda.synchronize()
        assert bits_equal(any0, want)
    parts.close()
    # a from_parts handle in the build's layout is served in mode 1
    stored = np.zeros((len(orig), d), dtype=np.float32)
    stored[orig >= 0] = x[orig[orig >= 0]]
    rows2 = flat_of(stored, metric)
    parts = HipIVFIndex.from_parts(rows2, cents, offs, orig)
    got = parts.search_scoped_device(q, k, [scopes[0]], nprobe=2, probe="scope")
    torch.cuda.synchronize()
    assert bits_equal(got, good)
    parts.close()
