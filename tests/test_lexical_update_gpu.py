"""
Updatable lexical postings (hipbm25_create_impacts / _append_impacts / _append_rows_dev / _remove_ranges on an impact handle,
hiprag.LexicalIndexUpdatable) and the scoped lexical hybrid composition.

Defining property: after any sequence of updates the handle cannot be told apart from
hipbm25_create(transpose_doc_weights(rows of the surviving documents in order, n_terms)): the export (offsets, doc ids,
impacts as uint32 bits) and every weighted search output, padding included, are equal bit for bit -- to the numpy definition
(weighted_search_reference) and to a fresh HipBM25 over the reference postings.

The rows sit at the code's boundaries: row_stride 37 (no multiple of 4), row lengths 0..37 with empty rows, a vocabulary
that grows from 1500 to 1600 terms (the scan of the per-term counts crosses its 1024-thread block, new ids lie behind the
old ones), T_ALL in every document that has an entry at all (an empty row has none), T_GROW with 2040 postings at 9260
documents, 2060 after the next append and under kSkipMinDf = 2048 again after the removal; the large append takes 8955 rows
(two 8192-row slices of the transposition, the 9216-document tile boundary, lists of many 4096-posting items).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -6   # include/hiprag.h
STRIDE = 37
V_OLD, V_NEW = 1500, 1600
TILE = 9216
SKIP_MIN_DF = 2048
T_ALL, T_GROW = 0, 1
N_ROWS = 9400
N_CREATE, N_SMALL, N_BIG, N_TOP = 300, 305, 9260, 9300     # document counts after create and the three device appends


class Rows:
    """N_ROWS document-major lexical rows: terms int32 [n, 37] (-1 behind the count), weights float32, counts int32"""

    def __init__(self):
        rng = np.random.default_rng(37)
        n = N_ROWS
        self.counts = ((np.arange(n) * 7 + 3) % (STRIDE + 1)).astype(np.int32)
        self.terms = np.full((n, STRIDE), -1, np.int32)
        self.weights = np.zeros((n, STRIDE), np.float32)
        roomy = np.flatnonzero(self.counts >= 2)
        grow = np.zeros(n, bool)
        grow[rng.choice(roomy[roomy < N_BIG], size=2040, replace=False)] = True
        grow[rng.choice(roomy[(roomy >= N_BIG) & (roomy < N_TOP)], size=20, replace=False)] = True
        self.grow = grow
        for i in range(n):
            c = int(self.counts[i])
            if c == 0:
                continue
            v = V_OLD if i < N_SMALL else V_NEW
            fixed = [T_ALL] + ([T_GROW] if grow[i] else [])
            if i >= N_SMALL and i % 3 == 0 and c > len(fixed):
                fixed.append(V_OLD + i % (V_NEW - V_OLD))            # new ids, behind the old vocabulary
            pool = 2 + np.unique((rng.random(3 * c) ** 3 * (V_OLD - 2)).astype(np.int64))   # skewed: a few long lists, many short ones
            rest = rng.permutation(pool[~np.isin(pool, fixed)])[:c - len(fixed)]
            t = np.sort(np.concatenate([np.asarray(fixed, np.int64), rest]))
            assert t.size <= c and t.max() < v
            self.counts[i] = t.size
            self.terms[i, :t.size] = t
            self.weights[i, :t.size] = (0.01 + 2.0 * rng.random(t.size)).astype(np.float32)
        # junk behind the counts is ignored by the library
        self.terms[5, self.counts[5]:] = 7
        self.weights[5, self.counts[5]:] = np.nan

    def take(self, docs):
        docs = np.asarray(docs, dtype=np.int64)
        return self.terms[docs], self.weights[docs], self.counts[docs]


@functools.lru_cache(maxsize=1)
def rows():
    return Rows()


def twin_postings(docs, n_terms):
    from hiprag import transpose_doc_weights
    return transpose_doc_weights(*rows().take(docs), n_terms)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_export(a, b):
    return (a["n_docs"], a["n_terms"]) == (b["n_docs"], b["n_terms"]) and \
        all(np.array_equal(bits(a[key]), bits(b[key])) for key in ("offsets", "doc_ids", "impacts"))


def queries_for(n_terms):
    """16 weighted queries of 1..12 terms; one repeats a term, one names an id outside the vocabulary"""
    rng = np.random.default_rng(11)
    qs = [[T_ALL], [T_GROW], [T_ALL, 9, T_ALL], [T_GROW, T_ALL, n_terms + 3, 5], [V_OLD + 7, V_OLD + 30, 2]]
    while len(qs) < 16:
        m = int(rng.integers(1, 13))
        q = (2 + (rng.random(m) ** 3 * (V_OLD - 2)).astype(np.int64)).tolist()
        if len(qs) % 3 == 0:
            q[int(rng.integers(0, m))] = int(rng.choice([T_ALL, T_GROW, V_OLD + 12]))
        qs.append(q)
    ws = [(0.05 + 1.5 * rng.random(len(q))).astype(np.float32) for q in qs]
    return qs, ws


def scopes_for(n, marks=()):
    """two scopes; edges on and beside the 9216 boundary and the places `marks` (the ends of removed ranges), clipped to n"""
    c = lambda v: int(max(0, min(v, n)))   # noqa: E731
    a = [(c(TILE - 216), c(TILE)), (c(TILE + 1), c(TILE + 60))]
    b = [(c(3), c(40))]
    for m in sorted(set(marks)):
        if c(m - 1) >= b[-1][1] and c(m + 9) > c(m - 1):
            b.append((c(m - 1), c(m)))
            b.append((c(m), c(m + 9)))          # touching ranges: an edge ON the mark, one BESIDE it
    b.append((max(b[-1][1], c(TILE - 5)), max(b[-1][1], c(TILE + 700))))
    return [a, b]


def assert_equals_twin(lex, docs, n_terms, tag, marks=()):
    """export and the weighted searches of `lex` against transpose_doc_weights of `docs`, the numpy definition of the search
    and a fresh HipBM25 over the reference postings"""
    from hiprag import HipBM25, weighted_search_reference
    sz = lex.sizes()
    assert sz["updatable_impacts"] and not sz["dirty"] and not sz["has_tf"], f"{tag}: {sz}"
    p = twin_postings(docs, n_terms)
    ex = lex.export()
    assert (ex["n_docs"], ex["n_terms"], lex.n_docs) == (len(docs), n_terms, len(docs)), tag
    assert np.array_equal(ex["offsets"], p.offsets), f"{tag}: offsets"
    assert np.array_equal(ex["doc_ids"], p.doc_ids), f"{tag}: doc ids"
    diff = int(np.sum(bits(ex["impacts"]) != bits(p.impacts)))
    print(f"{tag}: {len(docs)} documents, {p.doc_ids.size} postings, {diff} impacts differ from transpose_doc_weights")
    assert diff == 0, f"{tag}: {diff} impacts differ in their bits"
    qs, ws = queries_for(n_terms)
    scopes = scopes_for(len(docs), marks)
    soq = np.arange(len(qs), dtype=np.int32) % 2
    twin = HipBM25(p)
    for k in (10, 64):
        want = weighted_search_reference(p, qs, ws, k)
        for name, got in (("updated", lex.search(qs, ws, k)), ("fresh", twin.search_weighted(qs, ws, k))):
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), f"{tag}: {name} search_weighted, k = {k}"
        want = weighted_search_reference(p, qs, ws, k, ranges=[scopes[s] for s in soq])
        for name, got in (("updated", lex.search_scoped(qs, ws, k, scopes, soq)), ("fresh", twin.search_scoped_weighted(qs, ws, k, scopes, soq))):
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), f"{tag}: {name} search_scoped_weighted, k = {k}"
    twin.close()
    return ex


def cuda_rows(docs):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in rows().take(docs))


def fresh(docs, n_terms):
    from hiprag import LexicalIndexUpdatable
    return LexicalIndexUpdatable(twin_postings(docs, n_terms))


# ---- the sequence ------------------------------------------------------------------------------------------------------
def test_sequence_of_updates_equals_the_twin_after_every_step(gpu):
    from hiprag import LexicalIndexUpdatable
    docs = np.arange(N_CREATE)
    lex = fresh(docs, V_OLD)
    assert lex.update_info()["kind"] == "create_impacts"
    assert_equals_twin(lex, docs, V_OLD, "create")

    def append(batch, n_terms, tag, marks=()):
        nonlocal docs
        before = lex.export()
        assert lex.append_rows(*cuda_rows(batch), n_terms_after=n_terms) == (len(docs), len(docs) + len(batch))
        docs = np.append(docs, batch)
        info = lex.update_info()
        ex = assert_equals_twin(lex, docs, n_terms, tag, marks)
        assert info["kind"] == "append_rows_dev" and info["docs_after"] == len(docs) and info["postings_after"] == ex["doc_ids"].size
        assert info["postings_before"] == before["doc_ids"].size
        return ex, info

    append(np.arange(N_CREATE, N_SMALL), V_OLD, "device append of 5 rows")
    ex, _ = append(np.arange(N_SMALL, N_BIG), V_NEW, "device append to 9260 documents (two slices, the vocabulary grows)")
    df = np.diff(ex["offsets"].astype(np.int64))
    assert df[T_GROW] == 2040 and df[T_ALL] == int(np.sum(rows().counts[:N_BIG] > 0)) and df[V_OLD:].sum() > 0
    ex, info = append(np.arange(N_BIG, N_TOP), V_NEW, "device append to 9300 documents (across the 9216 tile)")
    assert np.diff(ex["offsets"].astype(np.int64))[T_GROW] == 2060 >= SKIP_MIN_DF
    # one slice: moved = everything at or behind the first inserted posting, which is in T_ALL's list (every batch row that
    # has an entry has T_ALL, the first list)
    assert info["postings_moved"] == ex["doc_ids"].size - int(np.sum(rows().counts[:N_BIG] > 0))

    # front, empty, middle, touching, across the 9216 tile, and 25 single documents of T_GROW (some of them touch)
    singles = np.flatnonzero(rows().grow[docs] & (docs >= 5000))[:25]
    ranges = [(0, 3), (100, 100), (4000, 4010), (4010, 4020)] + [(int(d), int(d) + 1) for d in singles] + [(9210, 9222), (9300, 9300)]
    gone = np.zeros(len(docs), bool)
    for lo, hi in ranges:
        gone[lo:hi] = True
    before = lex.export()
    assert lex.remove_ranges(ranges) == int(gone.sum()) == 60
    info = lex.update_info()
    dead = np.flatnonzero(gone[before["doc_ids"]])
    assert info["kind"] == "remove_ranges" and info["postings_moved"] == int(np.sum(~gone[before["doc_ids"][dead[0]:]]))
    assert info["postings_before"] - info["postings_after"] == dead.size
    marks = [lo - int(gone[:lo].sum()) for lo in (4000, 9210)]      # where removed ranges were, in the new numbering
    docs = docs[~gone]
    assert len(docs) > TILE
    ex = assert_equals_twin(lex, docs, V_NEW, "removal of front, middle, touching and empty ranges", marks)
    assert np.diff(ex["offsets"].astype(np.int64))[T_GROW] < SKIP_MIN_DF, "T_GROW fell back under kSkipMinDf"

    append(np.arange(N_TOP, N_TOP + 60), V_NEW, "append again after the removal", marks)
    assert lex.remove_ranges([(0, len(docs))]) == len(docs)
    docs = docs[:0]
    ex = assert_equals_twin(lex, docs, V_NEW, "everything removed")
    assert ex["doc_ids"].size == 0 and ex["n_terms"] == V_NEW, "emptied terms keep their ids"
    append(np.arange(N_TOP + 60, N_ROWS), V_NEW, "append to the emptied handle")
    before = lex.export()
    append(np.zeros(0, np.int64), V_NEW, "append of zero rows")
    assert same_export(before, lex.export())
    lex.close()
    # an index that was never anything but empty
    lex = LexicalIndexUpdatable(n_terms=V_OLD)
    docs = np.zeros(0, np.int64)
    assert_equals_twin(lex, docs, V_OLD, "empty index")
    append(np.arange(40), V_OLD, "append to an empty index")
    lex.close()


# ---- host and device paths -----------------------------------------------------------------------------------------------
def test_host_and_device_appends_give_the_same_bytes(gpu):
    base, batch = np.arange(N_CREATE), np.arange(N_CREATE, N_CREATE + 700)
    exports = []
    for path in ("device", "device", "host rows", "host csr"):
        lex = fresh(base, V_OLD)
        if path == "device":
            lex.append_rows(*cuda_rows(batch), n_terms_after=V_NEW)
        elif path == "host rows":
            lex.append_rows(*rows().take(batch), n_terms_after=V_NEW)
            assert lex.update_info()["kind"] == "append_impacts"
        else:
            b = twin_postings(batch, V_NEW)
            lex.append_postings(len(batch), V_NEW, b.offsets, b.doc_ids, b.impacts)
        lex.remove_ranges([(5, 9), (650, 800)])
        lex.append_rows(*cuda_rows(batch[:33]))
        exports.append(lex.export())
        info = lex.update_info()
        assert info["kind"] == "append_rows_dev" and info["extra_bytes"] > 0
        lex.close()
    docs = np.append(np.delete(np.append(base, batch), np.r_[5:9, 650:800]), batch[:33])
    p = twin_postings(docs, V_NEW)
    want = {"n_docs": len(docs), "n_terms": V_NEW, "offsets": p.offsets, "doc_ids": p.doc_ids, "impacts": p.impacts}
    for path, ex in zip(("device", "device again", "host rows", "host csr"), exports):
        assert same_export(ex, want), path


# ---- clean handle, cross-refusals -----------------------------------------------------------------------------------------
def _rc(fn, *args):
    from hiprag import HipRagError
    with pytest.raises(HipRagError) as e:
        fn(*args)
    return e.value.code


def test_handle_stays_clean_and_kinds_refuse_each_other(gpu):
    from hiprag import HipBM25, HipBM25Updatable, _native as nat
    docs = np.arange(N_CREATE)
    lex = fresh(docs, V_OLD)
    flags = lambda: (lex.sizes()["updatable_impacts"], lex.sizes()["dirty"], lex.sizes()["has_tf"])   # noqa: E731
    assert flags() == (True, False, False)
    lex.append_rows(*cuda_rows(np.arange(300, 320)), n_terms_after=V_NEW)
    assert flags() == (True, False, False)
    lex.append_rows(*rows().take(np.arange(320, 330)))
    assert flags() == (True, False, False)
    lex.remove_ranges([(3, 30)])
    assert flags() == (True, False, False)
    lex.search([[T_ALL]], [np.ones(1, np.float32)], 5)          # a search right behind an update needs no other call
    before = lex.export()
    off, ids, u32 = np.zeros(V_NEW + 1, np.uint64), np.zeros(1, np.uint32), np.ones(1, np.uint32)
    assert _rc(nat.call, "hipbm25_reweigh", lex.bm._h, None) == E_UNSUPPORTED
    assert _rc(nat.call, "hipbm25_append", lex.bm._h, 0, V_NEW, off.ctypes.data, ids.ctypes.data, u32.ctypes.data, u32.ctypes.data) == E_UNSUPPORTED
    assert same_export(before, lex.export())
    t, w, c = cuda_rows(np.arange(4))
    b = twin_postings(np.arange(4), V_OLD)
    plain = HipBM25(twin_postings(docs, V_OLD))
    tf = HipBM25Updatable()
    for other, n_terms in ((plain, V_OLD), (tf, V_OLD)):
        assert _rc(nat.call, "hipbm25_append_impacts", other._h, 4, n_terms, b.offsets.ctypes.data, b.doc_ids.ctypes.data,
                   b.impacts.ctypes.data) == E_UNSUPPORTED
        assert _rc(nat.call, "hipbm25_append_rows_dev", other._h, t.data_ptr(), w.data_ptr(), c.data_ptr(), 4, STRIDE, n_terms, None) == E_UNSUPPORTED
    assert _rc(nat.call, "hipbm25_remove_ranges", plain._h, None, 0) == E_UNSUPPORTED
    v = np.zeros(4, np.int64)
    nat.call("hipbm25_sizes", plain._h, v.ctypes.data)
    assert v[3] == 0
    assert tf.sizes() == {"n_docs": 0, "n_terms": 1, "postings": 0, "has_tf": True, "dirty": False}
    for h in (lex, plain, tf):
        h.close()


# ---- refusals leave the handle as it was ----------------------------------------------------------------------------------
def _bad_rows():
    base = np.arange(40, 52)
    def make(edit):   # noqa: E306
        t, w, c = (a.copy() for a in rows().take(base))
        edit(t, w, c)
        return t, w, c
    full = int(np.flatnonzero(rows().counts[40:52] >= 3)[0])      # a row with three entries at the least
    def setv(arr, r, j, v):   # noqa: E306
        arr[r, j] = v
    return {
        "a count above row_stride": make(lambda t, w, c: c.__setitem__(3, STRIDE + 1)),
        "a negative count": make(lambda t, w, c: c.__setitem__(11, -1)),
        "an id at n_terms_after": make(lambda t, w, c: setv(t, full, c[full] - 1, V_NEW)),
        "a negative id": make(lambda t, w, c: setv(t, full, 0, -2)),
        "descending ids": make(lambda t, w, c: (setv(t, full, 1, t[full, 2]), setv(t, full, 2, t[full, 1] - 1))),
        "a duplicate id in a row": make(lambda t, w, c: setv(t, full, 2, t[full, 1])),
        "a weight of 0": make(lambda t, w, c: setv(w, full, 1, 0.0)),
        "a negative weight": make(lambda t, w, c: setv(w, full, 0, -0.5)),
        "a NaN weight": make(lambda t, w, c: setv(w, full, 2, np.nan)),
        "an infinite weight": make(lambda t, w, c: setv(w, full, 2, np.inf)),
    }


def test_refused_calls_leave_the_handle_bit_for_bit(gpu):
    import torch
    docs = np.arange(N_CREATE)
    lex = fresh(docs, V_OLD)
    lex.append_rows(*cuda_rows(np.arange(200, 240)), n_terms_after=V_OLD + 10)
    before = lex.export()
    for tag, (t, w, c) in _bad_rows().items():
        dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (t, w, c))
        assert _rc(lambda: lex.append_rows(*dev, n_terms_after=V_NEW)) == E_INVALID, tag
        assert same_export(before, lex.export()), tag
        assert lex.n_docs == before["n_docs"] and lex.n_terms == before["n_terms"], tag
    good = cuda_rows(np.arange(40, 52))
    assert _rc(lambda: lex.append_rows(*good, n_terms_after=V_OLD + 9)) == E_INVALID, "n_terms_after below n_terms"
    b = twin_postings(np.arange(40, 52), V_NEW)
    ids = b.doc_ids.copy()
    lo = int(b.offsets[T_ALL])
    ids[lo], ids[lo + 1] = ids[lo + 1], ids[lo]
    assert _rc(lex.append_postings, 12, V_NEW, b.offsets, ids, b.impacts) == E_INVALID, "a host CSR with a descending list"
    imp = b.impacts.copy()
    imp[3] = np.inf
    assert _rc(lex.append_postings, 12, V_NEW, b.offsets, b.doc_ids, imp) == E_INVALID, "a host CSR with an infinite impact"
    assert _rc(lex.append_postings, 12, V_OLD + 9, b.offsets[:V_OLD + 10], b.doc_ids[:int(b.offsets[V_OLD + 9])],
               b.impacts[:int(b.offsets[V_OLD + 9])]) == E_INVALID, "n_terms_after below n_terms, host"
    assert _rc(lex.remove_ranges, [(5, 3)]) == E_INVALID and _rc(lex.remove_ranges, [(0, before["n_docs"] + 1)]) == E_INVALID
    assert same_export(before, lex.export())
    assert lex.n_docs == before["n_docs"] and lex.n_terms == before["n_terms"]
    from hiprag import LexicalIndexUpdatable, PostingsCSR      # create_impacts checks its impacts too
    p = twin_postings(np.arange(10), V_OLD)
    bad = p.impacts.copy()
    bad[0] = 0.0
    assert _rc(LexicalIndexUpdatable, PostingsCSR(p.n_docs, p.n_terms, p.offsets, p.doc_ids, bad)) == E_INVALID
    lex.append_rows(*good, n_terms_after=V_NEW)       # and the handle goes on working
    assert_equals_twin(lex, np.r_[0:300, 200:240, 40:52], V_NEW, "append behind the refusals")
    lex.close()


# ---- the scoped composition -----------------------------------------------------------------------------------------------
def test_scoped_lexical_hybrid_equals_its_three_calls_and_the_reference(gpu):
    import torch
    from hiprag import HipFlatIndex, hybrid_search_scoped_lexical_device, rrf_fuse_device, weighted_search_reference
    from oracle import hybrid_oracle as ho
    n, d, depth, k = 2500, 64, 20, 10
    docs = np.arange(n)
    lex = fresh(docs[:N_CREATE], V_OLD)
    lex.append_rows(*cuda_rows(docs[N_CREATE:]), n_terms_after=V_NEW)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, d)).astype(np.float32)
    ix = HipFlatIndex(d, "ip")
    ix.add(x)
    qs, ws = queries_for(V_NEW)
    q = rng.standard_normal((len(qs), d)).astype(np.float32)
    qd = torch.from_numpy(q).cuda()
    scopes = [[(0, 40), (100, 1300)], [(2000, 2500)], [(7, 8)]]
    soq = np.arange(len(qs), dtype=np.int32) % 3
    fused, (dense, sparse) = (lambda r: (r[:2], r[2]))(hybrid_search_scoped_lexical_device(
        ix, lex, qd, qs, ws, scopes, soq, depth=depth, k=k, w_dense=1.0, w_sparse=0.7, return_lists=True))
    one = (ix.search_scoped_device(qd, depth, scopes, soq), lex.bm.search_scoped_weighted_device(qs, ws, depth, scopes, soq))
    one_fused = rrf_fuse_device(one[0][2], one[1][2], k, w_a=1.0, w_b=0.7)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()   # noqa: E731
    assert np.array_equal(bits(host(dense[0])), bits(host(one[0][0]))) and np.array_equal(host(dense[1]), host(one[0][2]))
    assert np.array_equal(bits(host(sparse[0])), bits(host(one[1][0]))) and np.array_equal(host(sparse[1]), host(one[1][2]))
    assert np.array_equal(bits(host(fused[0])), bits(host(one_fused[0]))) and np.array_equal(host(fused[1]), host(one_fused[1]))
    # the references: fp64 scores of the scope's rows ranked (score desc, id asc), the numpy definition of the weighted
    # search over the same ranges, and the oracle's RRF of the two
    all64 = np.stack([ho.all_scores_f64(x, q[b], ho.METRIC_IP) for b in range(len(qs))])
    ref_dense = np.full((len(qs), depth), -1, np.int64)
    for b in range(len(qs)):
        inside = np.concatenate([np.arange(lo, hi) for lo, hi in scopes[soq[b]]])
        top = inside[np.lexsort((inside, -all64[b, inside]))][:depth]
        ref_dense[b, :top.size] = top
    ref_sparse = weighted_search_reference(twin_postings(docs, V_NEW), qs, ws, depth, ranges=[scopes[s] for s in soq])
    assert np.array_equal(host(dense[1]), ref_dense)
    assert np.array_equal(host(sparse[1]), ref_sparse[1]) and np.array_equal(bits(host(one[1][1])), bits(ref_sparse[0]))
    want = ho.rrf_fuse(ref_dense, ref_sparse[1], k, w_a=1.0, w_b=0.7)
    assert np.array_equal(bits(host(fused[0])), bits(want[0])) and np.array_equal(host(fused[1]), want[1])
    plain = hybrid_search_scoped_lexical_device(ix, lex, qd, qs, ws, scopes, soq, depth=depth, k=k, w_dense=1.0, w_sparse=0.7)
    torch.cuda.synchronize()
    assert len(plain) == 2 and np.array_equal(host(plain[1]), want[1])
    lex.close()
