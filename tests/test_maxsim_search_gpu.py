"""
Late-interaction search (hipmaxsim_search_scoped*): the exact MaxSim top k over every document of a scope.  The expected value
of a query is built from what the library already defines: pair scores from `maxsim` (hipmaxsim_host) over the ids in
candidate chunks of at most 256, then `maxsim_search_reference`, the selection restated in numpy; ids and the uint32 images
of the scores must be EQUAL.  The pair scores themselves are held against colbert_cases.maxsim_expected (bits on integer
data, the accumulation bound on unit vectors).  Shapes: the smallest at which the kernel takes each of its paths -- stored
lengths around the 32-vector tile, a query shorter than, equal to and longer than a tile, queries that share a tile, a
query that straddles a pass and, at 1024-d where R is smallest, one longer than R; ranges that start and end off every slice
boundary; k below, at and above the entries a slice keeps.
"""
import ctypes
import functools

import numpy as np
import pytest

from colbert_cases import NEG_MAX, maxsim_expected, maxsim_vectors, score_ratio
from oracle.linear_cases import bf16_bits, bf16_values

pytestmark = pytest.mark.gpu

N_DOCS = 150
LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 100)               # stored lengths, cycled
COUNTS = (0, 1, 5, 8, 8, 31, 32, 33, 64, 65, 70)
Q_STRIDE = 96
SCOPES = ([(0, 150)], [(3, 3)], [(7, 8)], [(15, 17), (17, 40), (100, 131)], [(0, 1), (10, 11), (140, 141)])   # the last: empty documents only
KS = (1, 10, 256)
SETS = [("exact", 128, "bf16"), ("exact", 128, "fp8"), ("random", 128, "bf16"), ("random", 128, "fp8"), ("exact", 1024, "bf16"),
        ("random", 1024, "bf16")]                              # "random" = unit vectors


def _doc_vectors(regime, dim):
    docs = [maxsim_vectors(regime, LENGTHS[i % 10], dim, 300 + i) for i in range(N_DOCS)]
    for i in range(10):
        docs[50 + i] = docs[i].copy()                           # equal scores: they must fall in id order
    return docs


def _pairs_by_maxsim(store, qv, qc, n_docs):
    """hipmaxsim's pair scores of every query against documents 0..n_docs-1, in candidate chunks of at most 256."""
    from hiprag import maxsim
    cols = []
    for lo in range(0, n_docs, 256):
        cand = np.tile(np.arange(lo, min(lo + 256, n_docs), dtype=np.int64), (len(qc), 1))
        cols.append(maxsim(store, qv, qc, cand, k=1)[3])
    return np.concatenate(cols, axis=1)


@functools.lru_cache(maxsize=None)
def _setup(regime, dim, fmt):
    """One store, one query block, hipmaxsim's pair table and the expected rows of every (query, scope, k)."""
    from hiprag import MultiVectorStore, maxsim_search_reference
    from hiprag.index import pack_scopes
    docs = _doc_vectors(regime, dim)
    store = MultiVectorStore(dim, max_doc_vectors=160, format=fmt)
    store.append([bf16_bits(d) for d in docs])
    queries = [maxsim_vectors(regime, n, dim, 700 + i) for i, n in enumerate(COUNTS)]
    qv = np.full((len(COUNTS), Q_STRIDE, dim), 0x7FC5, dtype=np.uint16)   # poison behind every count: it must not be read
    for i, q in enumerate(queries):
        qv[i, :len(q)] = bf16_bits(q)
    qc = np.asarray(COUNTS, np.int32)
    pairs = _pairs_by_maxsim(store, qv, qc, N_DOCS)
    lens = np.asarray([len(d) for d in docs])
    valid = (qc[:, None] > 0) & (lens[None, :] > 0)
    # the batch: every query under every scope
    nq, ns = len(COUNTS), len(SCOPES)
    b_q = np.repeat(np.arange(nq), ns)
    b_s = np.tile(np.arange(ns), nq).astype(np.int32)
    ranges, offsets, _ = pack_scopes(SCOPES, b_s, len(b_s))
    n_ranges = int(offsets[-1])
    want = {k: maxsim_search_reference(pairs[b_q], valid[b_q], ranges[:n_ranges], offsets, b_s, k) for k in KS}
    return dict(store=store, docs=docs, queries=queries, qv=qv, qc=qc, pairs=pairs, valid=valid, lens=lens, b_q=b_q, b_s=b_s, want=want)


def _same(got, want):
    return got[1].tobytes() == want[1].tobytes() and got[0].view(np.uint32).tobytes() == want[0].view(np.uint32).tobytes()


@pytest.mark.parametrize("regime,dim,fmt", SETS)
def test_pair_scores_are_maxsims_and_maxsims_are_right(gpu, regime, dim, fmt):
    """The table the expectation rests on: hipmaxsim's pair scores against the float64 reference over what the store holds."""
    s = _setup(regime, dim, fmt)
    off, vecs = s["store"].export()
    stored = bf16_values(vecs).astype(np.float64)
    worst = 0.0
    for i, q in enumerate(s["queries"]):
        for j in range(N_DOCS):
            if not s["valid"][i, j]:
                assert s["pairs"][i, j] == np.float32(NEG_MAX)
                continue
            want, bound = maxsim_expected(q, stored[off[j]:off[j + 1]], regime)
            r = score_ratio(s["pairs"][i, j], want, bound)
            worst = max(worst, r)
            assert r <= 1.0, (regime, dim, fmt, i, j, float(s["pairs"][i, j]), want, bound)
    print(f"pair scores {regime} {dim} {fmt}: worst |got - ref| / bound = {worst:.3g} (bound None = bits)")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("regime,dim,fmt", SETS)
def test_bits_and_order_of_every_query_under_every_scope(gpu, regime, dim, fmt, k):
    from hiprag import maxsim_search
    s = _setup(regime, dim, fmt)
    got = maxsim_search(s["store"], s["qv"][s["b_q"]], s["qc"][s["b_q"]], SCOPES, s["b_s"], k)
    want = s["want"][k]
    for row in range(len(s["b_q"])):
        assert np.array_equal(got[1][row], want[1][row]), (COUNTS[s["b_q"][row]], SCOPES[s["b_s"][row]], got[1][row][:12], want[1][row][:12])
        assert np.array_equal(got[0][row].view(np.uint32), want[0][row].view(np.uint32)), (COUNTS[s["b_q"][row]], SCOPES[s["b_s"][row]])
    # what the cases are there for: the copies tie and fall in id order; the empty scopes and the empty query are all padding
    full = [r for r in range(len(s["b_q"])) if s["b_s"][r] == 0 and s["qc"][s["b_q"][r]] > 0]
    if regime == "exact" and k == 256:
        for r in full:
            ids = list(got[1][r])
            for d in range(1, 10):
                assert ids.index(d) < ids.index(50 + d) and got[0][r][ids.index(d)] == got[0][r][ids.index(50 + d)], (r, d)
    for r in range(len(s["b_q"])):
        if s["b_s"][r] in (1, 4) or s["qc"][s["b_q"][r]] == 0:
            assert np.all(got[1][r] == -1) and np.all(got[0][r] == np.float32(NEG_MAX))


@pytest.mark.parametrize("regime,dim,fmt", [("exact", 128, "bf16"), ("random", 128, "fp8"), ("random", 1024, "bf16")])
def test_a_row_depends_on_its_query_and_scope_alone(gpu, regime, dim, fmt):
    import torch
    from hiprag import maxsim_search, maxsim_search_device
    s = _setup(regime, dim, fmt)
    k = 10
    want = s["want"][k]
    qv, qc, b_s = s["qv"][s["b_q"]], s["qc"][s["b_q"]], s["b_s"]
    batch = maxsim_search(s["store"], qv, qc, SCOPES, b_s, k)
    assert _same(batch, want)
    assert _same(maxsim_search(s["store"], qv, qc, SCOPES, b_s, k), batch)                     # the same bytes from run to run
    for row in range(len(b_s)):                                                                   # every query alone
        alone = maxsim_search(s["store"], qv[row:row + 1], qc[row:row + 1], [SCOPES[b_s[row]]], None, k)
        assert _same(alone, (want[0][row:row + 1], want[1][row:row + 1])), row
    perm = np.random.default_rng(5).permutation(len(b_s))                                        # a permuted batch: permuted rows
    assert _same(maxsim_search(s["store"], qv[perm], qc[perm], SCOPES, b_s[perm], k), (want[0][perm], want[1][perm]))
    based = maxsim_search(s["store"], qv, qc, SCOPES, b_s, k, id_base=1000)                    # id_base changes ids only
    assert based[0].tobytes() == want[0].tobytes() and np.array_equal(based[1], np.where(want[1] >= 0, want[1] + 1000, -1))
    dq = torch.from_numpy(qv.view(np.int16)).cuda().view(torch.bfloat16)                          # the device entry
    ds, di = maxsim_search_device(s["store"], dq, torch.from_numpy(qc).cuda(), SCOPES, b_s, k)
    torch.cuda.synchronize()
    assert _same((ds.cpu().numpy(), di.cpu().numpy()), want)


def _stored(s, scope):
    return int(sum(s["lens"][lo:hi].sum() for lo, hi in scope))


@pytest.mark.parametrize("dim", (128, 1024))
def test_queries_of_a_scope_share_one_read_of_it(gpu, dim):
    from hiprag import maxsim_search
    s = _setup("exact", dim, "bf16")
    store = s["store"]
    qv, qc = s["qv"][[3, 4, 5, 6]].copy(), np.asarray([8, 8, 8, 8], np.int32)   # four 8-vector queries (two cut from longer ones)
    big, small = SCOPES[3], SCOPES[2]
    maxsim_search(store, qv, qc, [big], None, 5)
    info = store.search_info()
    R, G, S = info["pass_rows"], info["group_queries"], info["slice_docs"]
    assert 4 <= G and 32 <= R and R % 32 == 0 and S >= 1
    assert info["doc_vectors_read"] == _stored(s, big), info                     # once, not four times
    in_scope = sum(hi - lo for lo, hi in big)
    n_valid = sum(int((s["lens"][lo:hi] > 0).sum()) for lo, hi in big)
    assert info["valid_pairs"] == 4 * n_valid and info["padding_pairs"] == 4 * (in_scope - n_valid)
    assert info["work_items"] == sum((hi - 1) // S - lo // S + 1 for lo, hi in big if hi > lo) and info["chunks"] == 1
    total = 0
    for i in range(4):                                                            # the same four in four calls: four reads
        maxsim_search(store, qv[i:i + 1], qc[i:i + 1], [big], None, 5)
        total += store.search_info()["doc_vectors_read"]
    assert total == 4 * _stored(s, big)
    maxsim_search(store, qv, qc, [big, small], [0, 1, 0, 1], 5)                   # two disjoint scopes: the sum of both, nothing else
    assert store.search_info()["doc_vectors_read"] == _stored(s, big) + _stored(s, small)
    maxsim_search(store, s["qv"][10:11], s["qc"][10:11], [big], None, 5)          # the 70-vector query: ceil(70 / R) passes
    assert store.search_info()["doc_vectors_read"] == -(-70 // R) * _stored(s, big)
    if dim == 1024:
        assert R == 64                                                            # two tiles: the query is longer than a pass


@pytest.mark.parametrize("fmt", ("bf16", "fp8"))
def test_the_search_follows_removals_and_appends(gpu, fmt):
    from colbert_cases import drop_ranges
    from hiprag import MultiVectorStore, maxsim_search
    s = _setup("random", 128, fmt)
    docs = [bf16_bits(d) for d in s["docs"]]
    gone = [(5, 12), (60, 61), (120, 150)]
    extra = [bf16_bits(maxsim_vectors("random", n, 128, 900 + n)) for n in (40, 0, 33)]
    store = MultiVectorStore(128, max_doc_vectors=160, format=fmt)
    store.append(docs)
    store.remove_ranges(gone)
    store.append(extra)
    fresh = MultiVectorStore(128, max_doc_vectors=160, format=fmt)
    survivors = drop_ranges(docs, gone) + extra
    fresh.append(survivors)
    n = len(survivors)
    assert len(store) == n
    scopes = [[(0, n)], [(3, 20), (20, 21), (n - 5, n)]]
    soq = [i % 2 for i in range(len(COUNTS))]
    for k in (10, 256):
        assert _same(maxsim_search(store, s["qv"], s["qc"], scopes, soq, k), maxsim_search(fresh, s["qv"], s["qc"], scopes, soq, k))
    # and it is the right answer, not merely the same one
    from hiprag import maxsim_search_reference
    from hiprag.index import pack_scopes
    pairs = _pairs_by_maxsim(fresh, s["qv"], s["qc"], n)
    lens = np.asarray([len(d) for d in survivors])
    ranges, offsets, soq32 = pack_scopes(scopes, soq, len(COUNTS))
    want = maxsim_search_reference(pairs, (s["qc"][:, None] > 0) & (lens[None, :] > 0), ranges, offsets, soq32, 10)
    assert _same(maxsim_search(store, s["qv"], s["qc"], scopes, soq, 10), want)


def test_refusals_leave_the_outputs_untouched(gpu):
    import torch
    from hiprag import _native as nat
    from hiprag.index import pack_scopes
    s = _setup("exact", 128, "bf16")
    store = s["store"]
    nq = 2
    qv = torch.from_numpy(s["qv"][[3, 5]].view(np.int16)).cuda().view(torch.bfloat16).contiguous()
    qc = torch.from_numpy(s["qc"][[3, 5]]).cuda()

    def refused(k=5, scopes=([(0, 10)],), soq=(0, 0), q_stride=Q_STRIDE, q_ptr=None, offsets=None, host=False):
        ranges, off, so = pack_scopes(scopes, np.asarray(soq, np.int32), nq)
        if offsets is not None:
            off = np.asarray(offsets, np.int32)
        kk = 256
        if host:
            sc, ids = np.full((nq, kk), 7.5, np.float32), np.full((nq, kk), 77, np.int64)
            args = (store._h, s["qv"][[3, 5]].ctypes.data, s["qc"][[3, 5]].ctypes.data, q_stride, nq, k, ranges.ctypes.data, off.ctypes.data,
                    len(off) - 1, so.ctypes.data, 0, sc.ctypes.data, ids.ctypes.data)
            name = "hipmaxsim_search_scoped"
        else:
            sc = torch.full((nq, kk), 7.5, dtype=torch.float32, device="cuda")
            ids = torch.full((nq, kk), 77, dtype=torch.int64, device="cuda")
            args = (store._h, q_ptr if q_ptr is not None else qv.data_ptr(), qc.data_ptr(), q_stride, nq, k, ranges.ctypes.data,
                    off.ctypes.data, len(off) - 1, so.ctypes.data, 0, sc.data_ptr(), ids.data_ptr(), None)
            name = "hipmaxsim_search_scoped_dev"
        with pytest.raises(nat.HipRagError) as e:
            nat.call(name, *args)
        assert e.value.code == -1, str(e.value)                                   # HIPRAG_E_INVALID
        if not host:
            torch.cuda.synchronize()
            sc, ids = sc.cpu().numpy(), ids.cpu().numpy()
        assert np.all(sc == np.float32(7.5)) and np.all(ids == 77)

    for host in (False, True):
        refused(k=0, host=host)
        refused(k=257, host=host)
        refused(scopes=([(0, N_DOCS + 1)],), host=host)                          # hi > documents
        refused(scopes=([(0, 10), (9, 12)],), host=host)                         # overlapping ranges
        refused(scopes=([(0, 10)], [(20, 30)]), soq=(0, 1), offsets=[0, 2, 1], host=host)   # descending offsets
        refused(soq=(0, 1), host=host)                                            # scope_of_query out of range
        refused(soq=(-1, 0), host=host)
        refused(q_stride=513, host=host)
    refused(q_ptr=qv.data_ptr() + 2)                                              # a misaligned q_vecs
    with pytest.raises(nat.HipRagError):
        nat.call("hipmaxsim_search_scoped_dev", store._h, qv.data_ptr(), qc.data_ptr(), Q_STRIDE, nq, 5, None, None, 1, None, -1, None, None, None)
    out = np.zeros(8, np.int64)
    nat.call("hipmaxsim_search_info", store._h, out.ctypes.data)                  # the store is still usable
    assert out[4] >= 1 and out[5] >= 1
