"""
Scoring rows by id (libhiprag hipidx_score_ids*, HipFlatIndex.score_ids*): the exact score of any (query, row id) pair, with
the bits every search entry gives that row.  Checked bit for bit against the flat search and the scoped search of the same
index, independently of them against hiprag.score_ids_reference and the textbook summation bound, over the launch shapes
the grid rule produces, across removals and adds, past 4 GiB of rows, and end to end through the collection with
HIP_HYBRID_SCORE_ALL=true, where the host path and the HIP_PAGES path must agree and a chunk outside the probed IVF list
gets the flat index's score.
"""
import asyncio
import ctypes
import dataclasses
import json

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

E_INVALID = -1   # include/hiprag.h
F32_MAX = float(np.finfo(np.float32).max)
F64_MAX = float(np.finfo(np.float64).max)
N = 75           # two full 32-row blocks and a partial one whose last quad holds three rows
WIDTHS = [1, 7, 128, 136, 520, 1000, 1024]      # 520: the first width with more than 64 pieces (the second load half)


def make_index(x, metric, id_base=0):
    from hiprag import HipFlatIndex
    ix = HipFlatIndex(x.shape[1], metric)
    if len(x):
        ix.add(x)
    if id_base:
        ix.set_id_base(id_base)
    return ix


def pads(metric):
    return (-F64_MAX, -F32_MAX) if metric == "ip" else (F64_MAX, F32_MAX)


def valid_mask(ids, n, id_base):
    return (ids >= 0) & (ids - id_base >= 0) & (ids - id_base < n)


def expected_from_lists(found, ids, n, id_base, metric):
    """(scores64, scores32, ids) of a search that returned all n rows -> what score_ids must give for `ids`: the row's
    score looked up by id, the padding values elsewhere.  Torch tensors on the device."""
    import torch
    s64, s32, sid = found
    nq = ids.shape[0]
    p64, p32 = pads(metric)
    t64 = torch.full((nq, n + 1), p64, dtype=torch.float64, device="cuda")
    t32 = torch.full((nq, n + 1), p32, dtype=torch.float32, device="cuda")
    if n:
        assert int(sid.min()) >= id_base and sorted(sid[0].tolist()) == list(range(id_base, id_base + n))    # every row, once
        t64.scatter_(1, sid - id_base, s64)
        t32.scatter_(1, sid - id_base, s32)
    ok = valid_mask(ids, n, id_base)
    col = torch.where(ok, ids - id_base, torch.full_like(ids, n))
    return t64.gather(1, col), t32.gather(1, col)


def same_bits(a, b):
    import torch
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


def lists_of_case_1(id_base, depth=80):
    rng = np.random.default_rng(5)
    ids = np.full((3, depth), -1, dtype=np.int64)
    ids[0, :N] = id_base + np.arange(N)[::-1]                                            # every row, descending
    ids[1] = id_base + rng.integers(0, N, depth)                                         # duplicates ...
    ids[1, [0, 1, 2]] = id_base + N - 1                                                  # ... the last row three times
    ids[1, [5, 40]] = -1
    ids[1, [6, 41]] = id_base - 1
    ids[1, [7, 79]] = id_base + N
    ids[1, 8] = 2 ** 62
    ids[2, depth - N:] = id_base + rng.permutation(N)                                    # a permutation behind padding
    return ids


def grid_of(nq, depth):
    """the grid rule include/hiprag.h states: entries per workgroup = the smallest of 4, 8, .. 64 at which the grid is at
    most 4096 workgroups, else 64"""
    chunk = 4
    while chunk < 64 and nq * -(-depth // chunk) > 4096:
        chunk *= 2
    return nq * -(-depth // chunk)


def check_against_the_searches(ix, x, q, ids, metric, id_base, host=True):
    """score_ids_device and score_ids against hipidx_search_dev and hipidx_search_scoped_dev over all rows, bit for bit, and
    hipidx_score_info against the counts"""
    import torch
    n = len(x)
    qd, idd = torch.from_numpy(q).cuda(), torch.from_numpy(ids).cuda()
    s64, s32 = ix.score_ids_device(qd, idd)
    ok = valid_mask(ids, n, id_base)
    info = ix.score_info()
    assert info == {"valid": int(ok.sum()), "padding": int((~ok).sum()), "workgroups": grid_of(*ids.shape)}
    p64, p32 = pads(metric)
    assert np.all(s64.cpu().numpy()[~ok] == p64) and np.all(s32.cpu().numpy()[~ok] == p32)
    searches = (ix.search_device(qd, n), ix.search_scoped_device(qd, n, [[(0, n)]])) if n else ()     # no rows: all padding, above
    for found in searches:
        e64, e32 = expected_from_lists(found, idd, n, id_base, metric)
        assert same_bits(s64, e64) and same_bits(s32, e32)
    if host:
        h32 = ix.score_ids(q, ids)
        h64 = ix.score_ids(q, ids, return64=True)
        assert h32.dtype == np.float32 and h64.dtype == np.float64
        assert h32.tobytes() == s32.cpu().numpy().tobytes() and h64.tobytes() == s64.cpu().numpy().tobytes()
        if n:
            fs, fi = ix.search(q, n)                                                     # hipidx_search, host entry
            table = np.full((len(q), n + 1), p32, dtype=np.float32)
            np.put_along_axis(table, fi - id_base, fs, axis=1)
            want = np.take_along_axis(table, np.where(ok, ids - id_base, n), axis=1)
            assert h32.tobytes() == want.tobytes()
    return s64, s32


# ---- 1. the bits of the searches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("id_base", [0, 1000])
@pytest.mark.parametrize("d", WIDTHS)
def test_bits_of_the_searches(gpu, metric, id_base, d):
    x = ho.synthetic_vectors(N, d, seed=300 + d)
    q = ho.synthetic_queries(3, d, seed=400 + d)
    ix = make_index(x, metric, id_base)
    check_against_the_searches(ix, x, q, lists_of_case_1(id_base), metric, id_base)


# ---- 2. independent of the searches -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
def test_inner_product_is_the_reference_bit_for_bit(gpu, d):
    """hiprag.score_ids_reference restates rescore4's order in numpy fp64; a product of two fp32 values is exact in fp64, so
    a contracted multiply-add rounds as the separate add does.  Gaussian data as well: no structure to hide behind."""
    from hiprag import score_ids_reference
    rng = np.random.default_rng(d)
    for x, q in ((ho.synthetic_vectors(N, d, seed=310 + d), ho.synthetic_queries(3, d, seed=410 + d)),
                 (rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((3, d)).astype(np.float32))):
        ids = lists_of_case_1(1000)
        got = make_index(x, "ip", 1000).score_ids(q, ids, return64=True)
        assert got.tobytes() == score_ids_reference(x, q, ids, "ip", id_base=1000).tobytes()
        # and the bound form of the L2 check below, for the inner product: |s - x.q| <= (d_pad + 2) 2^-52 sum |x_i q_i|
        ok = valid_mask(ids, N, 1000)
        d_pad = (d + 7) // 8 * 8
        for i in range(3):
            rows = x[ids[i, ok[i]] - 1000].astype(np.float64)
            exact, mag = rows @ q[i].astype(np.float64), np.abs(rows * q[i].astype(np.float64)).sum(axis=1)
            assert np.all(np.abs(got[i, ok[i]] - exact) <= (d_pad + 2) * 2.0 ** -52 * mag)


@pytest.mark.parametrize("d", WIDTHS)
def test_l2_is_within_the_summation_bound(gpu, d):
    """A contracted t * t + acc rounds once where numpy rounds twice, so no bit equality: |s - sum (x - q)^2| <= (d_pad + 2)
    2^-52 sum (x - q)^2, the sum in numpy fp64 -- the bound of any order of d_pad non-negative terms (gamma_{n-1} of
    Higham eq. 4.4, n = d_pad, plus the roundings of the difference and the square of a term)."""
    from hiprag import score_ids_reference
    rng = np.random.default_rng(50 + d)
    x, q = rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((3, d)).astype(np.float32)
    ids = lists_of_case_1(0)
    got = make_index(x, "l2").score_ids(q, ids, return64=True)
    ok = valid_mask(ids, N, 0)
    d_pad = (d + 7) // 8 * 8
    ref = score_ids_reference(x, q, ids, "l2")
    for i in range(3):
        rows = x[ids[i, ok[i]]].astype(np.float64)
        exact = ((rows - q[i].astype(np.float64)) ** 2).sum(axis=1)
        assert np.all(np.abs(got[i, ok[i]] - exact) <= (d_pad + 2) * 2.0 ** -52 * exact)
        assert np.all(np.abs(ref[i, ok[i]] - exact) <= (d_pad + 2) * 2.0 ** -52 * exact)
    assert np.all(got[~ok] == F64_MAX)


# ---- 3. launch shapes ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shape_index(gpu):
    d = 136
    x = ho.synthetic_vectors(N, d, seed=77)
    return x, {m: make_index(x, m, 1000) for m in ("ip", "l2")}


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("nq", [1, 5, 300])
@pytest.mark.parametrize("depth", [1, 50, 256, 257])
def test_launch_shapes(shape_index, metric, nq, depth):
    x, ixs = shape_index
    rng = np.random.default_rng(nq * 1000 + depth)
    q = ho.synthetic_queries(nq, x.shape[1], seed=nq + depth)
    ids = 1000 + rng.integers(-3, N + 3, (nq, depth)).astype(np.int64)
    check_against_the_searches(ixs[metric], x, q, ids, metric, 1000, host=nq <= 5)


def test_the_largest_chunk_and_a_grid_of_single_entries(shape_index):
    """600 x 256: 64 entries per workgroup, all full; 4100 x 1: 64 per workgroup by the rule, one entry each"""
    x, ixs = shape_index
    for nq, depth in ((600, 256), (4100, 1)):
        assert grid_of(nq, depth) == nq * -(-depth // 64)
        rng = np.random.default_rng(nq)
        q = ho.synthetic_queries(nq, x.shape[1], seed=nq)
        ids = 1000 + rng.integers(-1, N + 1, (nq, depth)).astype(np.int64)
        check_against_the_searches(ixs["l2"], x, q, ids, "l2", 1000, host=False)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_an_empty_index_and_a_list_of_padding(gpu, metric, shape_index):
    x, ixs = shape_index
    q = ho.synthetic_queries(2, x.shape[1], seed=3)
    empty = make_index(x[:0], metric, 0)
    ids = np.array([[0, 1, -1, 74, 5], [2 ** 40, 0, 0, -7, 31]], dtype=np.int64)
    s64, s32 = check_against_the_searches(empty, x[:0], q, ids, metric, 0)
    assert empty.score_info() == {"valid": 0, "padding": 10, "workgroups": 4}
    nothing = np.array([[-1, 999, 1075, -1000, 2 ** 62, -2 ** 62, 0]] * 2, dtype=np.int64)       # id_base 1000, 75 rows
    check_against_the_searches(ixs[metric], x, q, nothing, metric, 1000)
    assert ixs[metric].score_info()["valid"] == 0


# ---- 4. state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_after_a_removal_the_scores_are_those_of_the_survivors(gpu, metric):
    import torch
    d, n = 136, 300
    x = ho.synthetic_vectors(n, d, seed=21)
    q = ho.synthetic_queries(4, d, seed=22)
    ix = make_index(x, metric)
    ix.score_ids(q, np.arange(8)[None, :].repeat(4, 0))                # a call before the removal: nothing of it may stay
    assert ix.remove_ranges([(97, 203)]) == 106
    keep = np.concatenate([np.arange(97), np.arange(203, n)])
    fresh = make_index(x[keep], metric)
    rng = np.random.default_rng(23)
    ids = rng.integers(-2, n, (4, 120)).astype(np.int64)               # ids past the survivors are padding now
    a = ix.score_ids_device(torch.from_numpy(q).cuda(), torch.from_numpy(ids).cuda())
    b = fresh.score_ids_device(torch.from_numpy(q).cuda(), torch.from_numpy(ids).cuda())
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    assert ix.score_info() == fresh.score_info()
    assert ix.score_info()["valid"] == int(valid_mask(ids, len(keep), 0).sum())
    check_against_the_searches(ix, x[keep], q, ids, metric, 0)


def test_rows_added_on_one_stream_are_seen_from_another_at_once(gpu):
    """hipidx_add_dev on stream A, hipidx_score_ids_dev on stream B right behind it, no synchronisation in between: the
    library orders the read behind the add (include/hiprag.h)."""
    import torch
    from hiprag import _native as nat
    from hiprag import score_ids_reference
    d, n0, n1 = 128, 1000, 9000
    x = ho.synthetic_vectors(n0 + n1, d, seed=31)
    q = ho.synthetic_queries(3, d, seed=32)
    ix = make_index(x[:n0], "ip")
    ix.reserve_rows(n0 + n1)
    new = torch.from_numpy(x[n0:]).cuda()
    qd = torch.from_numpy(q).cuda()
    ids = np.random.default_rng(33).integers(0, n0 + n1, (3, 50)).astype(np.int64)
    ids[:, :4] = [n0 - 1, n0, n0 + n1 - 1, n0 + n1]
    idd = torch.from_numpy(ids).cuda()
    s64 = torch.empty((3, 50), dtype=torch.float64, device="cuda")
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    nat.call("hipidx_add_dev", ix._h, new.data_ptr(), n1, ctypes.c_void_p(a.cuda_stream))
    with torch.cuda.stream(b):
        ix.score_ids_device(qd, idd, out=(s64, None))
    torch.cuda.synchronize()
    assert s64.cpu().numpy().tobytes() == score_ids_reference(x, q, ids, "ip").tobytes()
    assert ix.score_info() == {"valid": 147, "padding": 3, "workgroups": grid_of(3, 50)}


def test_bad_arguments_are_refused_and_write_nothing(gpu):
    import torch
    from hiprag import HipRagError
    from hiprag import _native as nat
    d, nq, depth = 64, 3, 6
    x = ho.synthetic_vectors(100, d, seed=41)
    q = ho.synthetic_queries(nq, d, seed=42)
    ids = np.arange(nq * depth, dtype=np.int64).reshape(nq, depth)
    ix = make_index(x, "l2")
    good = ix.score_ids(q, ids, return64=True)
    before = ix.score_info()
    qd, idd = torch.from_numpy(q).cuda(), torch.from_numpy(ids).cuda()
    o64 = torch.full((nq, depth), -7.0, dtype=torch.float64, device="cuda")
    o32 = torch.full((nq, depth), -7.0, dtype=torch.float32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    h64, h32 = np.full((nq, depth), -7.0), np.full((nq, depth), -7.0, dtype=np.float32)

    def dev(q_=qd.data_ptr(), nq_=nq, ids_=idd.data_ptr(), depth_=depth, s64=o64.data_ptr()):
        nat.call("hipidx_score_ids_dev", ix._h, q_, nq_, ids_, depth_, s64, o32.data_ptr(), st)

    def host(q_=q.ctypes.data, nq_=nq, ids_=ids.ctypes.data, depth_=depth, s64=h64.ctypes.data):
        nat.call("hipidx_score_ids", ix._h, q_, nq_, ids_, depth_, s64, h32.ctypes.data)

    bad = [(dict(q_=None), "q is null"), (dict(ids_=None), "ids is null"), (dict(s64=None), "out_scores64"), (dict(nq_=0), "nq"),
           (dict(nq_=-1), "nq"), (dict(depth_=0), "depth"), (dict(nq_=65536, depth_=32768), "2^31"),
           (dict(nq_=2 ** 31 - 1, depth_=2 ** 31 - 1), "2^31")]
    for call in (dev, host):
        for kwargs, word in bad:
            with pytest.raises(HipRagError) as e:
                call(**kwargs)
            assert e.value.code == E_INVALID and word in str(e.value), f"{kwargs}: {e.value}"
    with pytest.raises(HipRagError) as e:
        nat.call("hipidx_score_info", ix._h, None)
    assert e.value.code == E_INVALID
    torch.cuda.synchronize()
    assert bool((o64 == -7.0).all()) and bool((o32 == -7.0).all()) and np.all(h64 == -7.0) and np.all(h32 == -7.0)
    assert ix.score_info() == before                                   # nothing was enqueued
    # out_scores may be null in both, and the index is as usable as before
    nat.call("hipidx_score_ids_dev", ix._h, qd.data_ptr(), nq, idd.data_ptr(), depth, o64.data_ptr(), None, st)
    nat.call("hipidx_score_ids", ix._h, q.ctypes.data, nq, ids.ctypes.data, depth, h64.ctypes.data, None)
    assert o64.cpu().numpy().tobytes() == good.tobytes() == h64.tobytes()
    assert bool((o32 == -7.0).all()) and np.all(h32 == -7.0)
    with pytest.raises(ValueError):
        ix.score_ids_device(qd, idd[:2])
    with pytest.raises(ValueError):
        ix.score_ids(q, ids[:2])


# ---- 5. row offsets past 4 GiB ------------------------------------------------------------------------------------------
def test_rows_past_4_gib(gpu):
    """2^20 + 64 rows of 1024 floats: row 2^20 starts at byte 2^32 of the blocked rows.  The rows are made on the device,
    the 64 scored ones are read back (reconstruct) and compared with an fp64 dot product under the bound of case 2."""
    import torch
    from hiprag import HipFlatIndex
    d, n, step = 1024, (1 << 20) + 64, 1 << 16
    ix = HipFlatIndex(d, "ip")
    ix.reserve_rows(n)
    gen = torch.Generator(device="cuda").manual_seed(1234)
    for lo in range(0, n, step):
        ix.add_device(torch.randn((min(step, n - lo), d), generator=gen, dtype=torch.float32, device="cuda"))
    assert ix.ntotal == n
    q = torch.randn((2, d), generator=gen, dtype=torch.float32, device="cuda")
    rows = np.concatenate([np.arange((1 << 20) - 31, (1 << 20) + 32), [n - 1]]).astype(np.int64)
    assert len(rows) == 64
    ids = torch.from_numpy(np.stack([rows, rows[::-1].copy()])).cuda()
    s64, s32 = ix.score_ids_device(q, ids)
    assert ix.score_info() == {"valid": 128, "padding": 0, "workgroups": grid_of(2, 64)}
    xr = torch.from_numpy(np.stack([ix.reconstruct(int(r)) for r in rows])).cuda().double()
    got = s64.cpu().numpy()
    for i in range(2):
        order = torch.from_numpy(rows if i == 0 else rows[::-1].copy()).cuda()
        sel = xr[torch.searchsorted(torch.from_numpy(rows).cuda(), order)]
        exact = (sel @ q[i].double()).cpu().numpy()
        mag = (sel * q[i].double()).abs().sum(dim=1).cpu().numpy()
        assert np.all(np.abs(got[i] - exact) <= (d + 2) * 2.0 ** -52 * mag)
    assert np.array_equal(s32.cpu().numpy(), got.astype(np.float32))
    assert len(np.unique(got[0])) == 64 and len(np.unique(got[1])) == 64     # 64 different rows were read for each query


# ---- 6. the collection, end to end --------------------------------------------------------------------------------------
D, DEPTH, MAX_PAGES = 64, 12, 3
DOCS = [("docA", "red", 9), ("docB", "blue", 6), ("docC", "red", 7)]       # pages 1 + i // 4
WORDS = [f"w{j}" for j in range(30)]


class _QueryProvider:
    def __init__(self):
        self.table = {}

    async def embed_single(self, text, instruction=None):
        return [float(v) for v in self.table[text]]


def _texts(n, seed):
    rng = np.random.default_rng(seed)
    return [f"c{i} " + " ".join(rng.choice(WORDS, size=3 + (i * 7) % 23)) + f" u{i}" for i in range(n)]     # u{i}: chunk i of every document


def _chunk_table(storage, doc, texts, per_page=4):
    chunks = [{"chunk_id": f"{doc}_{i:04d}", "text": t, "page": 1 + i // per_page, "metadata": {"title": doc}} for i, t in enumerate(texts)]
    with open(storage / f"{doc}_chunks.json", "w") as f:
        json.dump({"total": len(chunks), "chunks": chunks}, f)


def _host_keyed(rt, retriever, query, project, max_pages):
    """the host path with (doc_id, page) as the chunk's page key: what the device path keys pages by"""
    chunks = asyncio.run(retriever.retrieve_chunks(query, project))
    keyed = [dataclasses.replace(c, page=(c.metadata["doc_id"], c.page)) for c in chunks]
    return chunks, rt.rank_pages(rt.group_chunks_by_page(keyed))[:max_pages]


def _same_pages(got, want, tag):
    assert len(got) == len(want) and len(got) > 0, tag
    for g, w in zip(got, want):
        assert g.page == w.page[1] and g.metadata["doc_id"] == w.page[0], tag
        assert np.float64(g.score).tobytes() == np.float64(w.score).tobytes(), (tag, g.score, w.score)
        assert [c.chunk_id for c in g.chunks] == [c.chunk_id for c in w.chunks], tag
        for a, b in zip(g.chunks, w.chunks):
            assert np.float64(a.score).tobytes() == np.float64(b.score).tobytes(), (tag, a.chunk_id, a.score, b.score)
            assert list(a.metadata.items()) == list(b.metadata.items()), (tag, a.metadata, b.metadata)


def _exact_similarity(coll, q, row):
    """the flat index's own score of one row -- a scoped search of the one-row scope -- after the reader's transform"""
    from rag.storage.hip_index import collection as col
    import torch
    s64, _s32, ids = coll.index.search_scoped_device(torch.tensor([q], dtype=torch.float32, device="cuda"), 1, [[(row, row + 1)]])
    assert ids.tolist() == [[row]]
    return col._transform(coll, s64[0].tolist(), [row])[0][1]


def _row_of(coll, chunk):
    doc = next(d for d in coll.manifest.documents if d["doc_id"] == chunk.metadata["doc_id"])
    return doc["row0"] + int(chunk.chunk_id.rsplit("_", 1)[1])


def test_collection_scores_every_chunk_on_both_paths(gpu, tmp_path, monkeypatch):
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    from rag.storage.hip_index import collection as col
    monkeypatch.setenv("HIP_INDEX_METRIC", "l2")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "l2")
    monkeypatch.delenv("HIP_INDEX_TYPE", raising=False)
    monkeypatch.delenv("HIP_RERANK", raising=False)
    monkeypatch.setenv("STORAGE_DIR", str(tmp_path))
    monkeypatch.setenv("HIP_COLLECTION", "true")
    qp = _QueryProvider()
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: qp)
    hi.clear_caches()
    try:
        xs = {doc: ho.synthetic_vectors(n, D, seed=700 + j) for j, (doc, _p, n) in enumerate(DOCS)}
        for j, (doc, project, n) in enumerate(DOCS):
            _chunk_table(tmp_path, doc, _texts(n, 800 + j))
            col.append_document(doc, project, xs[doc], storage_dir=tmp_path)
        # the query text names the chunk of a red document that lies FARTHEST from the query vector: at most three chunks
        # carry the word, so the sparse leg finds it and it is fused, and the dense leg (12 of 22 rows, or of the 16 red
        # ones) cannot have found it
        vec = xs["docC"][4]
        far = max(((float(((xs[doc][i] - vec) ** 2).sum()), i) for doc in ("docA", "docC") for i in range(len(xs[doc]))))[1]
        query = f"u{far}"
        qp.table[query] = vec
        q = [float(v) for v in vec]
        retriever = rt.HybridRetriever(top_chunks=DEPTH, top_pages=MAX_PAGES, hybrid=True)
        seen = 0
        for project in (None, "red"):
            # off: sparse-only chunks as ever, on both paths
            monkeypatch.delenv("HIP_HYBRID_SCORE_ALL", raising=False)
            monkeypatch.delenv("HIP_PAGES", raising=False)
            off_chunks, off_pages = _host_keyed(rt, retriever, query, project, 10 ** 6)
            sparse_only = [c.chunk_id for c in off_chunks if c.metadata.get("sparse_only")]
            assert sparse_only and not any("dense_scored" in c.metadata for c in off_chunks)
            monkeypatch.setenv("HIP_PAGES", "true")
            _same_pages(asyncio.run(retriever.retrieve_and_rank_pages(query, project, 200)), off_pages, f"off {project}")
            # on: the host path ...
            monkeypatch.setenv("HIP_HYBRID_SCORE_ALL", "true")
            monkeypatch.delenv("HIP_PAGES")
            on_chunks, on_pages = _host_keyed(rt, retriever, query, project, 10 ** 6)
            assert [c.chunk_id for c in on_chunks] == [c.chunk_id for c in off_chunks]             # the fused list is the same
            assert [c.chunk_id for c in on_chunks if c.metadata.get("dense_scored")] == sparse_only
            assert not any("sparse_only" in c.metadata for c in on_chunks)
            coll = col.open_collection(tmp_path)
            for a, b in zip(on_chunks, off_chunks):
                if a.metadata.get("dense_scored"):
                    assert a.score == _exact_similarity(coll, q, _row_of(coll, a))
                    seen += 1
                else:
                    assert a.score == b.score and a.metadata == b.metadata
            # ... and the device path: the same pages, page scores, chunks, chunk scores and metadata
            monkeypatch.setenv("HIP_PAGES", "true")
            _same_pages(asyncio.run(retriever.retrieve_and_rank_pages(query, project, 200)), on_pages, f"on {project}")
            _same_pages(asyncio.run(retriever.retrieve_and_rank_pages(query, project, MAX_PAGES)), on_pages[:MAX_PAGES], f"on {project} top")
        assert seen > 0
        # the per-document path (HIP_COLLECTION off) scores through the reader's index
        monkeypatch.delenv("HIP_PAGES")
        monkeypatch.setenv("HIP_COLLECTION", "false")
        from rag.ingest.indexing import index_chunks

        class _Rows:
            async def embed_batch(self, texts, instruction=None):
                return [[float(v) for v in xs["docA"][int(t.split()[0][1:])]] for t in texts]

        solo = tmp_path / "solo"
        solo.mkdir()
        monkeypatch.setenv("STORAGE_DIR", str(solo))
        hi.clear_caches()
        texts = _texts(9, 800)
        _chunk_table(solo, "docA", texts)
        chunks = json.load(open(solo / "docA_chunks.json"))["chunks"]
        asyncio.run(index_chunks("docA", chunks, storage_dir=solo, provider=_Rows(), with_sparse=True))
        small = rt.HybridRetriever(top_chunks=4, top_pages=MAX_PAGES, hybrid=True)
        query = f"u{max((float(((xs['docA'][i] - vec) ** 2).sum()), i) for i in range(9))[1]}"      # the farthest of 9, depth 4
        qp.table[query] = vec
        monkeypatch.setenv("HIP_HYBRID_SCORE_ALL", "false")
        off = asyncio.run(small.retrieve_chunks(query))
        monkeypatch.setenv("HIP_HYBRID_SCORE_ALL", "true")
        on = asyncio.run(small.retrieve_chunks(query))
        assert [c.chunk_id for c in on] == [c.chunk_id for c in off] and any(c.metadata.get("sparse_only") for c in off)
        reader = hi.open_first_index()[0]
        every = dict(reader.search(q, top_k=9))
        for a, b in zip(on, off):
            assert "sparse_only" not in a.metadata and bool(a.metadata.get("dense_scored")) == bool(b.metadata.get("sparse_only"))
            assert a.score == every[int(a.chunk_id.rsplit("_", 1)[1])]
    finally:
        hi.clear_caches()


def test_a_chunk_outside_the_probed_list_gets_the_flat_score(gpu, tmp_path, monkeypatch):
    """HIP_INDEX_TYPE=ivf HIP_IVF_HYBRID=true at nprobe = 1: the dense leg sees one list; the fused rows it lacks -- found by
    BM25, in other lists -- are scored on the flat index the collection keeps."""
    import rag.query.retriever as rt
    import rag.storage.hip_index as hi
    from rag.storage.hip_index import collection as col
    nlist, limit = 12, 15
    docs = [("docA", "red", 230, (0, 1)), ("docB", "blue", 400, (2, 3, 4)), ("docC", "green", 200, (5,)), ("docD", "red", 333, (6, 1))]
    names = ["alpha", "beta", "gamma", "delta", "kappa", "sigma", "omega", "theta"]

    def rows(n, centres, seed):
        rng = np.random.default_rng(seed)
        c = np.random.default_rng(1).standard_normal((12, D))
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        x = c[np.repeat(np.array(centres), (n + len(centres) - 1) // len(centres))[:n]] + (0.3 / np.sqrt(D)) * rng.standard_normal((n, D))
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)

    monkeypatch.setenv("HIP_INDEX_METRIC", "ip")
    monkeypatch.setattr(hi.config, "HIP_INDEX_METRIC", "ip")
    monkeypatch.setenv("STORAGE_DIR", str(tmp_path))
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_INDEX_TYPE", "ivf")
    monkeypatch.setenv("HIP_IVF_NPROBE", "1")
    monkeypatch.setenv("HIP_IVF_HYBRID", "true")
    monkeypatch.delenv("HIP_IVF_PROBE", raising=False)
    monkeypatch.delenv("HIP_RERANK", raising=False)
    monkeypatch.setenv("HIP_HYBRID_SCORE_ALL", "true")
    qp = _QueryProvider()
    monkeypatch.setattr(rt, "get_embedding_provider", lambda: qp)
    hi.clear_caches()
    try:
        for j, (doc, project, n, centres) in enumerate(docs):
            _chunk_table(tmp_path, doc, [f"{names[i % 8]} {names[(i // 8) % 8]} of {doc}" for i in range(n)], per_page=7)
            col.append_document(doc, project, rows(n, centres, 800 + j), storage_dir=tmp_path)
        coll = col.train_collection_ivf(tmp_path, nlist=nlist)
        offs, orig = coll.ivf.lists()
        list_of = np.empty(coll.manifest.rows, dtype=np.int64)
        for l in range(nlist):
            list_of[orig[offs[l]:offs[l + 1]]] = l
        text = "gamma delta of docB"
        vec = rows(400, (2, 3, 4), 801)[7]
        q = [float(v) for v in vec]
        qp.table[text] = vec
        got = col.search_collection_hybrid(text, q, limit, project=None, storage_dir=tmp_path)
        assert len(got) == limit and not any("sparse_only" in r for r in got)
        chunks = [rt._as_chunk(r) for r in got]
        found = [c for c in chunks if not c.metadata.get("dense_scored")]
        scored = [c for c in chunks if c.metadata.get("dense_scored")]
        probed = {int(list_of[_row_of(coll, c)]) for c in found}
        assert len(probed) == 1                                                          # nprobe = 1
        outside = [c for c in scored if int(list_of[_row_of(coll, c)]) not in probed]
        assert outside, "no fused chunk lay outside the probed list"
        for c in chunks:                                                                 # found or scored: the flat index's bits
            assert c.score == _exact_similarity(coll, q, _row_of(coll, c)), c.chunk_id
        # and the device path agrees with the host path here too
        retriever = rt.HybridRetriever(top_chunks=limit, top_pages=MAX_PAGES, hybrid=True)
        _chunks, want = _host_keyed(rt, retriever, text, None, MAX_PAGES)
        monkeypatch.setenv("HIP_PAGES", "true")
        _same_pages(asyncio.run(retriever.retrieve_and_rank_pages(text, None)), want, "ivf hybrid")
    finally:
        hi.clear_caches()
