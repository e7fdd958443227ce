"""
CPU: hiprag.rank_pages_reference, the stated semantics of hippage_rank_dev, against the reference's own output (the
page_ranking cases of tests/golden) and against the host rank_pages of rag/query/retriever.py.  Everything is compared bit
for bit.
"""
import json
import os

import numpy as np

from hiprag import METRIC_IP, METRIC_L2, rank_pages_reference
from hiprag.pages import NEG_DBL_MAX

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "reference_wrapper_golden.json")))


def golden_case_arrays(case):
    """One document, IP metric, candidates = the rows in order: (pages, tags, cand, dense ids, dense values)."""
    n = len(case["chunks"])
    pages = np.array([p for _s, p in case["chunks"]], dtype=np.int32)
    ids = np.arange(n, dtype=np.int64)[None, :]
    vals = np.array([[s for s, _p in case["chunks"]]], dtype=np.float64)
    return pages, np.zeros(n, np.int32), ids, ids.copy(), vals


def check_golden(case, out):
    n_pages, scores, first, members, page_no, cand_rank, dpos, cand_scores = out
    exp = case["expected"]
    k = min(int(n_pages[0]), case["max_pages"])
    assert k == len(exp)
    for r, e in enumerate(exp):
        assert page_no[0, r] == e["page"]
        assert np.float64(scores[0, r]).tobytes() == np.float64(e["score"]).tobytes()
        got = [f"c{j}" for j in np.nonzero(cand_rank[0] == r)[0]]
        assert got == e["chunk_ids"] and members[0, r] == len(got) and first[0, r] == int(got[0][1:])
    assert dpos[0].tolist() == list(range(len(case["chunks"])))


def test_reference_reproduces_every_golden_page_ranking_case():
    assert len(GOLD["page_ranking"]) >= 5
    for case in GOLD["page_ranking"]:
        pages, tags, cand, d_ids, d_vals = golden_case_arrays(case)
        check_golden(case, rank_pages_reference(pages, tags, cand, d_ids, d_vals, case["max_pages"], metric=METRIC_IP))


def _host_rank(chunk_rows, key_of):
    """rag.query.retriever's grouping and rank_pages over [(position, score, sparse_only, row)], pages keyed by key_of(row)"""
    from rag.query.retriever import RetrievedChunk, group_chunks_by_page, rank_pages
    chunks = [RetrievedChunk(str(j), "", s, key_of(row), {"sparse_only": True} if sp else {}) for j, s, sp, row in chunk_rows]
    return [(r.page, r.score, [int(c.chunk_id) for c in r.chunks]) for r in rank_pages(group_chunks_by_page(chunks))]


def test_reference_equals_the_host_rank_pages_on_random_lists_with_sparse_only_members():
    rng = np.random.default_rng(11)
    for trial in range(40):
        rows, depth, dd = 60, int(rng.integers(1, 50)), int(rng.integers(1, 50))
        pages = rng.integers(1, 7, size=rows).astype(np.int32)
        tags = np.zeros(rows, np.int32)
        cand = rng.choice(rows, size=depth, replace=False).astype(np.int64)[None, :]
        d_ids = rng.choice(rows, size=dd, replace=False).astype(np.int64)[None, :]
        # scores on the 2^-24 grid in [0, 1]: every sum of at most 2^29 of them is exact in fp64, whatever the order
        d_vals = (rng.integers(0, (1 << 24) + 1, size=(1, dd)) / float(1 << 24)).astype(np.float64)
        out = rank_pages_reference(pages, tags, cand, d_ids, d_vals, depth, metric=METRIC_IP)
        n_pages, scores, first, members, page_no, cand_rank, dpos, cand_scores = out
        pos_of = {int(i): p for p, i in enumerate(d_ids[0])}
        listed = [(j, float(d_vals[0, pos_of[int(c)]]) if int(c) in pos_of else 0.0, int(c) not in pos_of, int(c))
                  for j, c in enumerate(cand[0])]
        want = _host_rank(listed, lambda row: int(pages[row]))
        assert n_pages[0] == len(want)
        for r, (page, score, ids) in enumerate(want):
            assert page_no[0, r] == page and np.float64(scores[0, r]).tobytes() == np.float64(score).tobytes()
            assert np.nonzero(cand_rank[0] == r)[0].tolist() == ids and members[0, r] == len(ids) and first[0, r] == ids[0]
        assert [d >= 0 for d in dpos[0]] == [not sp for _j, _s, sp, _row in listed]


def test_two_documents_with_equal_page_numbers_are_grouped_apart():
    pages = np.array([3, 3, 4, 3, 3], dtype=np.int32)
    tags = np.array([0, 0, 0, 1, 1], dtype=np.int32)
    ids = np.array([[0, 3, 1, 4, 2]], dtype=np.int64)
    vals = np.array([[0.5, 0.25, 0.75, 0.125, 1.0]], dtype=np.float64)
    n_pages, scores, first, members, page_no, cand_rank, _dpos, _s = rank_pages_reference(pages, tags, ids, ids, vals, 5)
    assert n_pages[0] == 3                                   # (doc 0, page 3), (doc 1, page 3), (doc 0, page 4)
    assert page_no[0, :3].tolist() == [4, 3, 3] and first[0, :3].tolist() == [4, 0, 1] and members[0, :3].tolist() == [1, 2, 2]
    assert scores[0, :3].tolist() == [1.05, 0.625 + 0.1, 0.1875 + 0.1]
    assert cand_rank[0].tolist() == [1, 2, 1, 2, 0]
    assert scores[0, 3] == NEG_DBL_MAX and first[0, 3] == -1 and members[0, 3] == 0 and page_no[0, 3] == 0
    # the same list under ONE tag: the host path's grouping by page number alone
    one = rank_pages_reference(pages, np.zeros(5, np.int32), ids, ids, vals, 5)
    assert one[0][0] == 2 and one[3][0, :2].tolist() == [1, 4]


def test_ties_clamp_and_padding_behave_as_specified():
    pages = np.array([1, 2, 3, 4, 5, 6], dtype=np.int32)
    tags = np.zeros(6, np.int32)
    # ties: three pages of equal score keep their first-seen order
    ids = np.array([[2, 0, 1]], dtype=np.int64)
    out = rank_pages_reference(pages, tags, ids, ids, np.full((1, 3), 0.5), 3)
    assert out[4][0].tolist() == [3, 1, 2] and out[5][0].tolist() == [0, 1, 2]
    # clamp: IP below 0 and above 1; L2 beyond 2 (below 0 after the transform) and below 0 (above 1 after it)
    ids = np.array([[0, 1, 2, 3]], dtype=np.int64)
    vals = np.array([[-0.25, 1.5, 0.25, float("inf")]], dtype=np.float64)
    assert rank_pages_reference(pages, tags, ids, ids, vals, 4, metric=METRIC_IP)[7][0].tolist() == [0.0, 1.0, 0.25, 1.0]
    vals = np.array([[2.5, -1.0, 0.5, 2.0]], dtype=np.float64)
    assert rank_pages_reference(pages, tags, ids, ids, vals, 4, metric=METRIC_L2)[7][0].tolist() == [0.0, 1.0, 0.75, 0.0]
    # padding of all three kinds, id_base 1000; a -1 hole of the dense list matches nothing; the same id twice is two members
    cand = np.array([[-1, 999, 1006, 1001, -7, 1001]], dtype=np.int64)
    d_ids = np.array([[-1, 1001, 1001]], dtype=np.int64)
    n_pages, scores, first, members, page_no, cand_rank, dpos, cs = rank_pages_reference(
        pages, tags, cand, d_ids, np.array([[0.9, 0.5, 0.25]]), 2, id_base=1000)
    assert n_pages[0] == 1 and page_no[0].tolist() == [2, 0] and first[0].tolist() == [3, -1] and members[0].tolist() == [2, 0]
    assert scores[0].tolist() == [0.5 + 0.1, NEG_DBL_MAX]
    assert cand_rank[0].tolist() == [-1, -1, -1, 0, -1, 0] and dpos[0].tolist() == [-1, -1, -1, 1, -1, 1]
    assert cs[0].tolist() == [0.0, 0.0, 0.0, 0.5, 0.0, 0.5]
    # nothing but padding
    out = rank_pages_reference(pages, tags, np.array([[-1, 6, 77]], dtype=np.int64), ids, vals, 3)
    assert out[0][0] == 0 and out[1][0].tolist() == [NEG_DBL_MAX] * 3 and out[2][0].tolist() == [-1] * 3
    assert out[5][0].tolist() == [-1] * 3 and out[6][0].tolist() == [-1] * 3 and out[7][0].tolist() == [0.0] * 3
    # a page of sparse-only members alone scores its boost
    out = rank_pages_reference(pages, tags, np.array([[4, 4, 4, 4]], dtype=np.int64), np.array([[0]], dtype=np.int64), np.array([[0.5]]), 1)
    assert out[1][0, 0] == 0.15 and out[3][0, 0] == 4


def test_the_overlay_takes_only_pages_that_fit_int32():
    import pytest
    from rag.storage.hip_index.pages import PageValueError, page_values
    got = page_values([0, 7, -3, np.int64(2 ** 31 - 1), -2 ** 31])
    assert got.dtype == np.int32 and got.tolist() == [0, 7, -3, 2 ** 31 - 1, -2 ** 31]
    assert page_values([]).dtype == np.int32 and page_values([]).size == 0
    for bad in ("iv", None, 2.0, True, 2 ** 31, -2 ** 31 - 1):
        with pytest.raises(PageValueError):
            page_values([1, bad])
