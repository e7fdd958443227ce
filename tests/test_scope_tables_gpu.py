"""
The scope tables through every device entry that takes them: the flat scoped search, the scoped IVF search, the scoped BM25
search, the late-interaction search and the two scoped hybrid calls share one copy of the table rules and one upload of
the table image (csrc/scope_plan.h, ScopeUpload::upload).  (a) the refused tables of tests/test_scoped_gpu.py give
HIPRAG_E_INVALID with the same words from every entry, each with its own word for the count, and leave the handle
answering as before; (b) six calls in a row on one stream with six different tables and no host synchronisation between
them -- the pinned ring has four buffers, so calls 5 and 6 rewrite those of calls 1 and 2 -- each equal the same call
made alone.
"""
import ctypes

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

E_INVALID = -1
N, D, NLIST, N_TERMS = 600, 32, 8, 1024
MV_DOCS, MV_DIM, Q_STRIDE = 40, 128, 8
NQ_MAX, K, DEPTH = 7, 5, 10

_ENTRIES = {}


def table(ranges, offsets, soq, null=()):
    """(the arrays, kept alive by the caller; the four table arguments of an entry)"""
    r = np.ascontiguousarray(ranges, np.int64).reshape(-1, 2)
    o = np.ascontiguousarray(offsets, np.int32)
    s = np.ascontiguousarray(soq, np.int32)
    args = (None if "ranges" in null or not len(r) else r.ctypes.data, None if "scope_offsets" in null else o.ctypes.data, len(o) - 1,
            None if "scope_of_query" in null else s.ctypes.data)
    return (r, o, s), args


def entries():
    """name -> (call(table arguments, nq) -> the output tensors, the entry's word for its count, the count); the handles
    are built once, shared, never changed"""
    import torch
    from hiprag import HipBM25, HipFlatIndex, HipIVFIndex, MultiVectorStore, PostingsCSR
    from hiprag import _native as nat
    from hiprag.colbert import bf16_bits
    if _ENTRIES:
        return _ENTRIES
    x = ho.synthetic_vectors(N, D, seed=611)
    qd = torch.from_numpy(ho.synthetic_queries(NQ_MAX, D, seed=612)).cuda()
    flat = HipFlatIndex(D, "ip")
    flat.add(x)
    ivf = HipIVFIndex(D, NLIST, "ip")
    ivf.build(x, iters=4, seed=0)
    p = ho.synthetic_postings(N, n_terms=N_TERMS, seed=613)
    bm = HipBM25(PostingsCSR(p.n_docs, p.n_terms, p.offsets, p.doc_ids, p.impacts))
    sparse = ho.synthetic_sparse_queries(NQ_MAX, n_terms=N_TERMS, seed=614)
    rng = np.random.default_rng(615)
    mv = MultiVectorStore(MV_DIM)
    mv.append([bf16_bits(rng.integers(-4, 5, size=(int(n_), MV_DIM))) for n_ in rng.integers(0, 20, size=MV_DOCS)])
    mq = torch.from_numpy(bf16_bits(rng.integers(-4, 5, size=(NQ_MAX, Q_STRIDE, MV_DIM))).view(np.int16)).view(torch.bfloat16).cuda()
    mc = torch.from_numpy(rng.integers(1, Q_STRIDE + 1, size=NQ_MAX).astype(np.int32)).cuda()

    def stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def outs(nq, k, *dtypes):
        return tuple(torch.empty((nq, k), dtype=t, device="cuda") for t in dtypes)

    def flat_call(tab, nq):
        o = outs(nq, K, torch.float64, torch.float32, torch.int64)
        nat.call("hipidx_search_scoped_dev", flat._h, qd.data_ptr(), nq, K, *tab, *(t.data_ptr() for t in o), stream())
        return o

    def ivf_call(tab, nq):
        o = outs(nq, K, torch.float64, torch.float32, torch.int64)
        nat.call("hipivf_search_scoped_dev", ivf._h, qd.data_ptr(), nq, K, 3, *tab, *(t.data_ptr() for t in o), stream())
        return o

    def bm25_call(tab, nq):
        terms, qoff = bm._flatten(sparse[:nq])
        o = outs(nq, K, torch.float64, torch.float32, torch.int64)
        nat.call("hipbm25_search_scoped_dev", bm._h, terms.ctypes.data if terms.size else None, qoff.ctypes.data, nq, K, *tab,
                 *(t.data_ptr() for t in o), stream())
        return o

    def maxsim_call(tab, nq):
        o = outs(nq, K, torch.float32, torch.int64)
        nat.call("hipmaxsim_search_scoped_dev", mv._h, mq.data_ptr(), mc.data_ptr(), Q_STRIDE, nq, K, *tab, 0, *(t.data_ptr() for t in o),
                 stream())
        return o

    def hybrid_call(tab, nq):
        terms, qoff = bm._flatten(sparse[:nq])
        lists = torch.empty((4, nq, DEPTH), dtype=torch.int64, device="cuda")
        o = outs(nq, K, torch.float32, torch.int64)
        nat.call("hiphybrid_search_scoped_dev", flat._h, bm._h, qd.data_ptr(), terms.ctypes.data if terms.size else None, qoff.ctypes.data,
                 nq, DEPTH, K, 60.0, 1.0, 1.0, *tab, lists.data_ptr(), *(t.data_ptr() for t in o), stream())
        return o + (lists,)

    def ivf_hybrid_call(tab, nq):    # HIPIVF_PROBE_SCOPE: the other coarse step of the scoped IVF driver
        terms, qoff = bm._flatten(sparse[:nq])
        lists = torch.empty((4, nq, DEPTH), dtype=torch.int64, device="cuda")
        o = outs(nq, K, torch.float32, torch.int64)
        nat.call("hiphybrid_search_ivf_scoped_dev", ivf._h, bm._h, qd.data_ptr(), terms.ctypes.data if terms.size else None,
                 qoff.ctypes.data, nq, DEPTH, K, 3, nat.PROBE_SCOPE, 60.0, 1.0, 1.0, *tab, lists.data_ptr(), *(t.data_ptr() for t in o),
                 stream())
        return o + (lists,)

    _ENTRIES.update({
        "hipidx_search_scoped_dev": (flat_call, "ntotal", N),
        "hipivf_search_scoped_dev": (ivf_call, "n", N),
        "hipbm25_search_scoped_dev": (bm25_call, "n_docs", N),
        "hipmaxsim_search_scoped_dev": (maxsim_call, "documents", MV_DOCS),
        "hiphybrid_search_scoped_dev": (hybrid_call, "ntotal", N),
        "hiphybrid_search_ivf_scoped_dev": (ivf_hybrid_call, "n", N),
    })
    _ENTRIES["keep"] = (flat, ivf, bm, mv, qd, mq, mc)
    return _ENTRIES


NAMES = ["hipidx_search_scoped_dev", "hipivf_search_scoped_dev", "hipbm25_search_scoped_dev", "hipmaxsim_search_scoped_dev",
         "hiphybrid_search_scoped_dev", "hiphybrid_search_ivf_scoped_dev"]


def as_bytes(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in tensors]


def refused_tables(n):
    """the refused tables of tests/test_scoped_gpu.py over n entries (two scopes, three queries) and the words of their messages"""
    good = dict(ranges=((0, 10), (20, 30)), offsets=(0, 1, 2), soq=(0, 1, 1))
    bad = [
        (dict(null=("ranges",)), "ranges is null"),
        (dict(null=("scope_offsets",)), "scope_offsets is null"),
        (dict(null=("scope_of_query",)), "scope_of_query is null"),
        (dict(offsets=(1, 1, 2)), "scope_offsets"),
        (dict(offsets=(0, 2, 1)), "scope_offsets"),
        (dict(ranges=((-1, 10), (20, 30))), "ranges[0]"),
        (dict(ranges=((0, 10), (30, 20))), "ranges[1]"),
        (dict(ranges=((0, 10), (20, n + 1))), "ranges[1]"),
        (dict(ranges=((0, 10), (9, 30)), offsets=(0, 2, 2)), "ranges[1]"),       # overlap inside one scope
        (dict(soq=(0, 2, 1)), "scope_of_query[1]"),
        (dict(soq=(0, 1, -1)), "scope_of_query[2]"),
    ]
    return good, [(dict(good, **kw), word) for kw, word in bad]


@pytest.mark.parametrize("name", NAMES)
def test_refused_tables_say_the_same_from_every_entry(gpu, name):
    from hiprag import HipRagError
    call, count_word, n = entries()[name]
    good, bad = refused_tables(n)
    keep, tab = table(**good)
    want = as_bytes(call(tab, 3))
    named = 0
    for kw, word in bad:
        keep_bad, tab_bad = table(**kw)
        with pytest.raises(HipRagError) as e:
            call(tab_bad, 3)
        msg = str(e.value)
        assert e.value.code == E_INVALID and word in msg, f"{kw}: {msg}"
        if "is not within" in msg:
            assert f"<= hi <= {count_word} = {n}" in msg, msg
            named += 1
        assert as_bytes(call(tab, 3)) == want, f"the search behind the refusal of {kw}"
    assert named == 3, "three of the tables break the bounds rule"


def six_tables(n):
    """six valid tables of different sizes over n entries, with what the rules allow: an empty scope, touching and empty
    ranges, scopes that overlap and descend"""
    return [
        ([(0, n)], [0, 1], [0] * 7),
        ([(0, n // 3), (n // 2, n)], [0, 1, 2], [0, 1, 0, 1, 1]),
        ([(n // 4, n // 2), (n // 2, n // 2 + 7), (0, 5)], [0, 2, 2, 3], [0, 1, 2, 2, 0, 1]),
        ([(n - 9, n)], [0, 1], [0]),
        ([(1, n - 1), (0, 1), (n - 1, n - 1), (n - 1, n)], [0, 1, 4], [1, 0, 1]),
        ([(n // 5, 2 * n // 5), (3 * n // 5, 4 * n // 5), (0, n), (3, 3)], [0, 1, 2, 3, 4], [2, 1, 0, 3]),
    ]


@pytest.mark.parametrize("name", NAMES)
def test_six_calls_in_a_row_reuse_the_ring(gpu, name):
    import torch
    call, _, n = entries()[name]
    tabs = [table(*t) for t in six_tables(n)]
    alone = [as_bytes(call(args, len(keep[2]))) for keep, args in tabs]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = [call(args, len(keep[2])) for keep, args in tabs]      # no host synchronisation between the calls
    side.synchronize()
    for i, (g, a) in enumerate(zip(got, alone)):
        assert as_bytes(g) == a, f"call {i + 1} of six"
