"""
The page table (hippage_*) and the ranking call (hippage_rank_dev).  Table: after any sequence of appends and removals its
export equals a fresh table of the survivors in pages, and in tags up to naming (equal exactly where the documents are
equal); refused calls change nothing.  Ranking: all eight outputs equal hiprag.rank_pages_reference bit for bit, at every
depth and query count around the kernel's dispatch constants.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DOC_ROWS = [40, 25, 35]                    # three documents, pages drawn from 1..6: their page numbers overlap
NAMES = ("n_pages", "page_scores", "page_first", "page_members", "page_no", "cand_rank", "cand_dense_pos", "cand_scores")


def _consts():
    from hiprag import pages as pg
    return pg.RANK_WAVE_DEPTH, pg.RANK_WAVE_QUERIES


def _depths():
    wd, _ = _consts()
    return sorted({1, 2, 63, 64, 65, 128, 255, 256, wd, wd + 1})


def _nqs():
    _, wq = _consts()
    return sorted({1, 3, 4, 5, 257, wq - 1, wq, wq + 1})


# ---- table -------------------------------------------------------------------------------------------------------------
def _doc_pages(seed=3, sizes=(7, 0, 12, 1, 9, 30, 0, 5, 64, 3, 17, 2)):
    rng = np.random.default_rng(seed)
    return [rng.integers(-2, 9, size=n).astype(np.int32) for n in sizes]


def _append(table, docs):
    from hiprag.pages import doc_offsets
    table.append(np.concatenate(docs) if docs else np.zeros(0, np.int32), doc_offsets([len(d) for d in docs]))


def _same(table, rows):
    """rows: [(document key, page)] of the survivors in order"""
    pages, tags = table.export()
    assert pages.dtype == np.int32 and tags.dtype == np.int32
    assert pages.tolist() == [p for _d, p in rows]
    docs = [d for d, _p in rows]
    assert len(tags) == len(docs)
    eq_tags = tags[:, None] == tags[None, :]
    eq_docs = np.asarray(docs)[:, None] == np.asarray(docs)[None, :] if docs else eq_tags
    assert np.array_equal(eq_tags, eq_docs)                       # tags are equal exactly where the documents are
    assert len(table) == len(rows)


def _rows_of(docs, first_key=0):
    return [(first_key + j, int(p)) for j, d in enumerate(docs) for p in d]


def _drop(rows, ranges):
    gone = set()
    for lo, hi in ranges:
        gone.update(range(lo, hi))
    return [r for i, r in enumerate(rows) if i not in gone]


def test_append_remove_append_equals_a_fresh_table(gpu):
    from hiprag import PageTable
    docs = _doc_pages()
    t = PageTable()
    _same(t, [])
    assert t.sizes() == (0, 0, 0, 0)
    _append(t, docs[:5])
    rows = _rows_of(docs[:5])
    _same(t, rows)
    cap0 = t.sizes()[2]
    assert t.sizes()[:2] == (29, 5) and cap0 >= 29
    _append(t, docs[5:9])                                  # grows past the first allocation
    rows += _rows_of(docs[5:9], 5)
    _same(t, rows)
    assert t.sizes()[2] > cap0 and t.sizes()[1] == 9
    n = len(rows)                                          # 128
    # empty, touching, document-cutting ranges (7..19 is document 2; 16 cuts it; 29..59 is document 5), the last row
    ranges = [(0, 0), (3, 7), (7, 16), (20, 20), (40, 41), (n - 1, n)]
    t.remove_ranges(ranges)
    rows = _drop(rows, ranges)
    _same(t, rows)
    _append(t, docs[9:])
    rows += _rows_of(docs[9:], 9)
    _same(t, rows)
    assert t.sizes()[1] == len(docs)                       # a removal gives no tag back
    fresh = PageTable()
    for key in sorted({d for d, _p in rows}):              # the survivors, one document each
        fresh.append([p for d, p in rows if d == key])
    assert fresh.export()[0].tobytes() == t.export()[0].tobytes()
    _same(fresh, rows)
    # no-ops; an empty batch and empty documents are valid and take tags
    t.remove_ranges([])
    t.remove_ranges([(3, 3), (len(rows), len(rows))])
    _append(t, [])
    issued = t.sizes()[1]
    _append(t, [np.zeros(0, np.int32), np.zeros(0, np.int32), np.asarray([5], np.int32)])
    rows += [(1002, 5)]
    _same(t, rows)
    assert t.sizes()[1] == issued + 3
    t.remove_ranges([(0, 1)])
    rows = rows[1:]
    _same(t, rows)
    t.remove_ranges([(0, len(rows))])                      # everything
    _same(t, [])
    _append(t, docs[2:4])                                  # and it is usable again
    _same(t, _rows_of(docs[2:4]))


def test_refused_calls_leave_the_table_as_it_was(gpu):
    from hiprag import HipRagError, PageTable
    from hiprag import _native as nat
    docs = _doc_pages(7)[:6]
    t = PageTable()
    _append(t, docs)
    before = ([a.tobytes() for a in t.export()], t.sizes())
    ok = np.asarray([5, 6, 7, 8], dtype=np.int32)
    for offsets in ([1, 2, 4], [0, 3, 2, 4], [-1, 4]):                                  # start, descent
        with pytest.raises(HipRagError) as e:
            nat.call("hippage_append", t._h, ok.ctypes.data, np.asarray(offsets, np.int64).ctypes.data, len(offsets) - 1)
        assert e.value.code == -1
    for args in ((None, np.asarray([0, 2], np.int64).ctypes.data, 1), (ok.ctypes.data, None, 1),
                 (ok.ctypes.data, np.asarray([0, 2], np.int64).ctypes.data, -1)):       # null pages, null offsets, n_docs
        with pytest.raises(HipRagError) as e:
            nat.call("hippage_append", t._h, *args)
        assert e.value.code == -1
    n = len(t)
    for ranges in ([(3, 2)], [(-1, 2)], [(0, n + 1)], [(4, 6), (5, 7)], [(6, 8), (1, 2)]):   # the range table rules
        with pytest.raises(HipRagError) as e:
            t.remove_ranges(ranges)
        assert e.value.code == -1
    with pytest.raises(HipRagError):
        nat.call("hippage_remove_ranges", t._h, None, 2)
    with pytest.raises(HipRagError):
        nat.call("hippage_sizes", t._h, None)
    assert ([a.tobytes() for a in t.export()], t.sizes()) == before
    nat.call("hippage_export", t._h, None, None)                                         # either pointer may be NULL
    t.close()
    with pytest.raises(HipRagError) as e:
        nat.call("hippage_sizes", 0xdead, np.zeros(4, np.int64).ctypes.data)
    assert e.value.code == -3


# ---- ranking -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(gpu):
    from hiprag import PageTable
    from hiprag.pages import doc_offsets
    rng = np.random.default_rng(17)
    pages = rng.integers(1, 7, size=sum(DOC_ROWS)).astype(np.int32)
    t = PageTable()
    t.append(pages, doc_offsets(DOC_ROWS))
    got_pages, tags = t.export()
    assert got_pages.tobytes() == pages.tobytes()
    return t, pages, tags


def _lists(pages, tags, nq, depth, dense_depth, id_base, scale, seed):
    """Candidate and dense lists with everything the ranking has to get right, see the module docstring of the test."""
    rng = np.random.default_rng(seed)
    rows = len(pages)
    cand = rng.integers(0, rows, size=(nq, depth)).astype(np.int64) + id_base          # with repeats
    kind = rng.integers(0, 20, size=(nq, depth))
    cand[kind == 0] = -1
    cand[kind == 1] = id_base - 1 - rng.integers(0, 5)                                  # below id_base (negative at base 0)
    cand[kind == 2] = id_base + rows + rng.integers(0, 5, size=int((kind == 2).sum()))  # at or beyond id_base + rows
    if nq >= 3:
        cand[1] = np.resize(np.asarray([-1, id_base - 1, id_base + rows], np.int64), depth)      # a query of only padding
    d_ids = np.full((nq, dense_depth), -1, np.int64)
    d_vals = rng.normal(0.5, 0.6, size=(nq, dense_depth)) * scale                      # arbitrary fp64, outside [0, 1] too
    for q in range(nq):
        pool = np.concatenate([rng.permutation(cand[q])[:max(1, (3 * depth) // 4)],     # candidates in another order
                               id_base + rng.integers(0, rows + 40, size=max(2, dense_depth // 5)),    # ids that may be none
                               np.full(max(1, dense_depth // 8), -1)])                  # holes
        take = rng.permutation(pool)[:dense_depth]
        d_ids[q, :len(take)] = take
        if q % 3 == 0:       # engineered exact ties: one score per page, from three values; eighteen pages share them
            for p in range(dense_depth):
                r = int(d_ids[q, p]) - id_base
                if 0 <= r < rows:
                    s = 0.25 * (1 + (int(tags[r]) + int(pages[r])) % 3)
                    d_vals[q, p] = s if scale == 1.0 else 2.0 * (1.0 - s)              # L2: 1 - v / 2 gives s back exactly
    # one page of only sparse-only members, in the last query: its rows leave the dense list
    q = nq - 1
    ok = (cand[q] >= id_base) & (cand[q] < id_base + rows)
    if ok.any():
        row = int(cand[q][ok][-1] - id_base)
        on_page = {id_base + r for r in range(rows) if tags[r] == tags[row] and pages[r] == pages[row]}
        d_ids[q][np.isin(d_ids[q], list(on_page))] = -1
    return cand, d_ids, d_vals


def _device(t, cand, d_ids, d_vals, max_pages, id_base, metric):
    import torch
    from hiprag import rank_pages_device
    out = rank_pages_device(t, torch.from_numpy(cand).cuda(), torch.from_numpy(d_ids).cuda(), torch.from_numpy(d_vals).cuda(),
                            max_pages, id_base=id_base, metric=metric)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name)
        assert g.tobytes() == w.tobytes(), (tag, name, g, w)


@pytest.mark.parametrize("nq", _nqs())
@pytest.mark.parametrize("depth", _depths())
def test_ranking_equals_the_reference(table, depth, nq):
    from hiprag import METRIC_IP, METRIC_L2, rank_pages_reference
    t, pages, tags = table
    seen_tie = seen_sparse_page = seen_cut = False
    for metric, id_base, dense_depth in ((METRIC_IP, 0, min(256, depth + 3)), (METRIC_L2, 1000, max(1, min(256, 2 * depth) - 1))):
        scale = 2.0 if metric == METRIC_L2 else 1.0
        cand, d_ids, d_vals = _lists(pages, tags, nq, depth, dense_depth, id_base, scale, seed=depth * 1000 + nq + metric)
        for max_pages in sorted({1, min(depth, 3), depth}):
            want = rank_pages_reference(pages, tags, cand, d_ids, d_vals, max_pages, id_base=id_base, metric=metric)
            _check(_device(t, cand, d_ids, d_vals, max_pages, id_base, metric), want, (metric, id_base, max_pages))
            seen_cut |= bool((want[0] > max_pages).any())
        # the engineered cases are really there (want: max_pages = depth, nothing cut)
        n_pages, scores, _first, members, _no, cand_rank, dpos, _s = want
        if nq >= 3:
            assert n_pages[1] == 0
        for q in range(nq):
            k = int(n_pages[q])
            seen_tie |= len(set(scores[q, :k].tolist())) < k
            for r in range(k):
                seen_sparse_page |= bool((dpos[q][cand_rank[q] == r] < 0).all())
    if depth >= 63:
        assert seen_tie and seen_sparse_page and seen_cut


def test_argument_checks_return_invalid(table):
    import torch
    from hiprag import HipRagError
    from hiprag import _native as nat
    t, _pages, _tags = table
    i64 = torch.zeros(4 * 300, dtype=torch.int64, device="cuda")
    f64 = torch.zeros(4 * 300, dtype=torch.float64, device="cuda")
    i32 = [torch.zeros(4 * 300, dtype=torch.int32, device="cuda") for _ in range(6)]
    good = dict(cand=i64.data_ptr(), depth=8, d_ids=i64.data_ptr(), d_sc=f64.data_ptr(), dd=8, nq=2, id_base=0, metric=0, mp=3,
                o0=i32[0].data_ptr(), o1=f64.data_ptr(), o2=i32[1].data_ptr(), o3=i32[2].data_ptr(), o4=i32[3].data_ptr(),
                o5=i32[4].data_ptr(), o6=i32[5].data_ptr(), o7=f64.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        nat.call("hippage_rank_dev", t._h, a["cand"], a["depth"], a["d_ids"], a["d_sc"], a["dd"], a["nq"], a["id_base"], a["metric"],
                 a["mp"], a["o0"], a["o1"], a["o2"], a["o3"], a["o4"], a["o5"], a["o6"], a["o7"], None)

    call()
    bad = [dict(nq=0), dict(nq=-1), dict(depth=0), dict(depth=257), dict(dd=0), dict(dd=257), dict(mp=0), dict(mp=9), dict(id_base=-1),
           dict(metric=2), dict(metric=-1)]
    bad += [{k: None} for k in ("cand", "d_ids", "d_sc", "o0", "o1", "o2", "o3", "o4", "o5", "o6", "o7")]
    for kw in bad:
        with pytest.raises(HipRagError) as e:
            call(**kw)
        assert e.value.code == -1, kw
    torch.cuda.synchronize()


def test_two_runs_give_identical_bytes(table):
    from hiprag import METRIC_L2
    t, pages, tags = table
    for depth, nq in ((50, 33), (200, 9)):
        cand, d_ids, d_vals = _lists(pages, tags, nq, depth, depth, 1000, 2.0, seed=5)
        a = _device(t, cand, d_ids, d_vals, 5, 1000, METRIC_L2)
        b = _device(t, cand, d_ids, d_vals, 5, 1000, METRIC_L2)
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b]


def test_golden_page_ranking_cases_through_the_device(gpu):
    from hiprag import METRIC_IP, PageTable
    from test_pages_cpu import check_golden, golden_case_arrays
    gold = json.load(open(os.path.join(HERE, "golden", "reference_wrapper_golden.json")))
    for case in gold["page_ranking"]:
        pages, _tags, cand, d_ids, d_vals = golden_case_arrays(case)
        t = PageTable()
        t.append(pages)
        max_pages = min(case["max_pages"], len(pages))             # the call takes max_pages <= depth
        check_golden(case, _device(t, cand, d_ids, d_vals, max_pages, 0, METRIC_IP))
