"""
Scoring rows by id, the parts that need no GPU: hiprag.score_ids_reference (the stated summation order of
hipidx_score_ids) against numpy's fp64 dot product, and the wiring of HIP_HYBRID_SCORE_ALL in the collection's hybrid
search over a fake index whose score_ids returns known values -- setting on: the fused rows the dense list lacks carry
the transformed score and "dense_scored"; setting off: the dicts of today, key for key -- and the case that motivates
the setting, as data: a page whose only chunk came from the sparse leg.
"""
import numpy as np
import pytest

U = 2.0 ** -53          # unit roundoff of fp64
DBL_MAX = float(np.finfo(np.float64).max)


# ---- 1. the reference against numpy ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 7, 136, 1000])
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_reference_against_numpy_fp64(d, metric):
    """Any summation order of n terms is within (n - 1) u / (1 - (n - 1) u) of the exact sum of |terms| (Higham, Accuracy
    and Stability, eq. 4.4); the terms themselves are exact (IP: a product of two fp32 values) or carry two more roundings
    (L2: the difference and the square).  n = d_pad terms: (d_pad + 2) 2^-52 x sum |terms| covers both, as the GPU test
    uses it, and np.dot's own error in the same form."""
    from hiprag import score_ids_reference
    rng = np.random.default_rng(100 + d)
    n, nq, base = 75, 3, 1000
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    ids = np.stack([np.arange(n)[::-1], rng.integers(0, n, n), rng.permutation(n)]).astype(np.int64)
    got = score_ids_reference(x, q, ids, metric)
    assert got.dtype == np.float64 and got.shape == ids.shape
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    d_pad = (d + 7) // 8 * 8
    for i in range(nq):
        rows = x64[ids[i]]
        if metric == "ip":
            want, mag = rows @ q64[i], np.abs(rows * q64[i]).sum(axis=1)
        else:
            want = mag = ((rows - q64[i]) ** 2).sum(axis=1)
        assert np.all(np.abs(got[i] - want) <= 2 * (d_pad + 2) * 2.0 ** -52 * mag), (d, metric, i)     # both sides' error
    # the same row twice is the same bits; ids shifted by id_base name the same rows; padding values
    assert np.array_equal(score_ids_reference(x, q, ids + base, metric, id_base=base), got)
    pad = np.array([[-1, base - 1, base + n, base + n - 1]] * nq, dtype=np.int64)
    p = score_ids_reference(x, q, pad, metric, id_base=base)
    assert np.all(p[:, :3] == (DBL_MAX if metric == "l2" else -DBL_MAX))
    assert np.array_equal(p[:, 3], score_ids_reference(x, q, np.full((nq, 1), n - 1), metric)[:, 0])


def test_reference_order_is_the_stated_one():
    """d = 136 = 17 pieces: partial sum (pq = 0, hh) holds pieces 0, 8 and 16, the others two pieces; restated with Python
    floats, add by add."""
    from hiprag import score_ids_reference
    rng = np.random.default_rng(7)
    d = 136
    x = rng.standard_normal((5, d)).astype(np.float32)
    q = rng.standard_normal((1, d)).astype(np.float32)
    got = score_ids_reference(x, q, np.arange(5)[None, :], "ip")
    for r in range(5):
        acc = [[0.0, 0.0] for _ in range(8)]
        for pq in range(8):
            for hh in range(2):
                for p in range(pq, 17, 8):
                    for e in range(4):
                        k = 8 * p + 4 * hh + e
                        acc[pq][hh] = acc[pq][hh] + float(x[r, k]) * float(q[0, k])
        s = [a[0] + a[1] for a in acc]
        s = [s[0] + s[1], s[2] + s[3], s[4] + s[5], s[6] + s[7]]
        s = [s[0] + s[1], s[2] + s[3]]
        assert np.float64(s[0] + s[1]).tobytes() == got[0, r].tobytes()


# ---- 2. the wiring over a fake index --------------------------------------------------------------------------------
class _FakeIndex:
    def __init__(self, metric, values):
        self.metric, self.values, self.calls = metric, values, []

    def score_ids(self, q, ids, return64=False):
        self.calls.append((np.asarray(q).copy(), np.asarray(ids).copy(), return64))
        out = np.array([[self.values[int(c)] for c in row] for row in np.asarray(ids)], dtype=np.float64)
        return out if return64 else out.astype(np.float32)


class _FakeColl:
    def __init__(self, metric, values):
        self.index = _FakeIndex(metric, values)


def _fake_enrich(page_of):
    def enrich(_coll, results):
        return [{"chunk_id": f"c{row}", "text": f"text {row}", "score": score, "page": page_of[row], "doc_id": "doc"}
                for row, score in results]
    return enrich


def _clamp(v):
    return float(max(0.0, min(1.0, v)))


@pytest.mark.parametrize("metric", [0, 1])
def test_setting_on_scores_the_rows_the_dense_list_lacks(monkeypatch, metric):
    import rag.query.retriever as rt
    from rag.storage.hip_index import collection as col
    page_of = {3: 1, 5: 1, 8: 2, 9: 2, 11: 3}
    monkeypatch.setattr(col, "_enrich", _fake_enrich(page_of))
    monkeypatch.setenv("HIP_HYBRID_SCORE_ALL", "true")
    raw = {8: 0.625, 11: 0.25} if metric == 0 else {8: 0.75, 11: 1.5}        # L2: 1 - v / 2 = 0.625, 0.25
    coll = _FakeColl(metric, raw)
    dense = ([0.5, 0.75, 0.125] if metric == 0 else [1.0, 0.5, 1.75], [3, 5, 9])          # similarities 0.5, 0.75, 0.125
    sparse = ([7.0, 6.0, 5.0, -3.4e38], [8, 3, 11, -1])
    f_ids, f_scores = [3, 8, 5, 11, 9, -1], [0.032, 0.0164, 0.016, 0.0159, 0.0158, 0.0]
    query = [0.25] * 4
    rows = col._fused_rows(coll, query, f_scores, f_ids, dense, sparse)
    assert [r["chunk_id"] for r in rows] == ["c3", "c8", "c5", "c11", "c9"]
    assert [r["score"] for r in rows] == [0.5, 0.625, 0.75, 0.25, 0.125]
    assert [r.get("dense_scored", False) for r in rows] == [False, True, False, True, False]
    assert not any("sparse_only" in r for r in rows)
    assert [r.get("bm25_score") for r in rows] == [6.0, 7.0, None, 5.0, None]
    assert [r["rrf_score"] for r in rows] == f_scores[:5]
    # one call, for exactly the missing rows in fusion order, in fp64, with the query
    assert len(coll.index.calls) == 1
    q, ids, return64 = coll.index.calls[0]
    assert return64 and ids.tolist() == [[8, 11]] and ids.dtype == np.int64
    assert q.dtype == np.float32 and q.tolist() == [query]
    # the chunks carry the key, and rank_pages over them is the reference's arithmetic: mean + min(0.05 n, 0.15)
    chunks = [rt._as_chunk(r) for r in rows]
    assert [c.metadata.get("dense_scored") for c in chunks] == [None, True, None, True, None]
    ranked = rt.rank_pages(rt.group_chunks_by_page(chunks))
    want = {1: (0.5 + 0.75) / 2 + min(2 * 0.05, 0.15), 2: (0.625 + 0.125) / 2 + min(2 * 0.05, 0.15), 3: 0.25 / 1 + min(0.05, 0.15)}
    assert [(p.page, p.score) for p in ranked] == sorted(want.items(), key=lambda kv: -kv[1])


def test_setting_on_with_nothing_missing_makes_no_call(monkeypatch):
    from rag.storage.hip_index import collection as col
    monkeypatch.setattr(col, "_enrich", _fake_enrich({3: 1, 5: 2}))
    monkeypatch.setenv("HIP_HYBRID_SCORE_ALL", "true")
    coll = _FakeColl(0, {})
    rows = col._fused_rows(coll, [0.0], [0.03, 0.02], [5, 3], ([0.5, 0.25], [3, 5]), ([1.0, -3.4e38], [5, -1]))
    assert coll.index.calls == [] and [r["score"] for r in rows] == [0.25, 0.5]
    assert not any("dense_scored" in r or "sparse_only" in r for r in rows)


@pytest.mark.parametrize("setting", [None, "false"])
def test_setting_off_is_todays_output_key_for_key(monkeypatch, setting):
    from rag.storage.hip_index import collection as col
    page_of = {3: 1, 5: 1, 8: 2, 9: 2}
    monkeypatch.setattr(col, "_enrich", _fake_enrich(page_of))
    if setting is None:
        monkeypatch.delenv("HIP_HYBRID_SCORE_ALL", raising=False)
    else:
        monkeypatch.setenv("HIP_HYBRID_SCORE_ALL", setting)
    coll = _FakeColl(1, {8: 0.75})
    rows = col._fused_rows(coll, [0.0], [0.032, 0.0164, 0.016, 0.0158, 0.0], [3, 8, 5, 9, -1], ([1.0, 0.5, 1.75], [3, 5, 9]),
                           ([7.0, 6.0, -3.4e38], [8, 3, -1]))
    assert coll.index.calls == []
    base = [{"chunk_id": f"c{r}", "text": f"text {r}", "score": s, "page": page_of[r], "doc_id": "doc"}
            for r, s in ((3, 0.5), (8, 0.0), (5, 0.75), (9, 0.125))]
    base[0].update(rrf_score=0.032, bm25_score=6.0)
    base[1].update(rrf_score=0.0164, bm25_score=7.0, sparse_only=True)
    base[2].update(rrf_score=0.016)
    base[3].update(rrf_score=0.0158)
    assert rows == base and [list(r) for r in rows] == [list(b) for b in base]


# ---- 3. the motivating case, as data --------------------------------------------------------------------------------
def test_a_page_the_sparse_leg_found_can_win(monkeypatch):
    """limit = 4.  Four dense hits on pages A = 1 and B = 2; row 20 on page C = 3 is found only by the sparse leg (first
    there: its fused score equals the best dense row's, and it displaces the fourth dense hit).  Its true similarity 0.75 is
    above page B's mean (0.5625 in the fused list, 0.5 over both of B's hits): off, C scores exactly 0.05; on, 0.75 + 0.05,
    above B."""
    import rag.query.retriever as rt
    from rag.storage.hip_index import collection as col
    page_of = {10: 1, 11: 1, 12: 2, 13: 2, 20: 3}
    monkeypatch.setattr(col, "_enrich", _fake_enrich(page_of))
    dense = ([0.875, 0.8125, 0.5625, 0.4375], [10, 11, 12, 13])              # inner products = similarities
    sparse = ([9.0, -3.4e38, -3.4e38, -3.4e38], [20, -1, -1, -1])
    fused = sorted([(1 / 61, 10), (1 / 62, 11), (1 / 63, 12), (1 / 64, 13), (1 / 61, 20)], key=lambda t: (-t[0], t[1]))[:4]
    f_scores, f_ids = [s for s, _ in fused], [i for _, i in fused]
    assert f_ids == [10, 20, 11, 12]

    def pages(setting):
        monkeypatch.setenv("HIP_HYBRID_SCORE_ALL", setting)
        coll = _FakeColl(0, {20: 0.75})
        rows = col._fused_rows(coll, [1.0], f_scores, f_ids, dense, sparse)
        return {p.page: p.score for p in rt.rank_pages(rt.group_chunks_by_page([rt._as_chunk(r) for r in rows]))}, \
               [p.page for p in rt.rank_pages(rt.group_chunks_by_page([rt._as_chunk(r) for r in rows]))]

    off, off_order = pages("false")
    assert off[3] == 0.05 and off_order == [1, 2, 3]
    assert off[2] == 0.5625 + 0.05
    on, on_order = pages("true")
    assert on[3] == 0.75 + 0.05 and on[3] > on[2] == off[2] and on_order == [1, 3, 2]
    assert on[1] == off[1] == (0.875 + 0.8125) / 2 + 0.1


def test_the_setting_is_off_by_default_and_read_at_use(monkeypatch):
    from rag.config import config
    monkeypatch.delenv("HIP_HYBRID_SCORE_ALL", raising=False)
    assert config.HIP_HYBRID_SCORE_ALL is False
    monkeypatch.setenv("HIP_HYBRID_SCORE_ALL", "True")
    assert config.HIP_HYBRID_SCORE_ALL is True
    import rag.query.retriever as rt
    assert rt._HYBRID_KEYS == ("rrf_score", "bm25_score", "sparse_only", "dense_scored")
