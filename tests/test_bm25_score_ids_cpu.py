"""
The parts of the BGE-M3 combined score that need no GPU: hiprag.sparse.bm25_score_ids_reference against
weighted_search_reference, hiprag.m3.m3_score_reference's rules, and the HIP_M3_SCORE / HIP_M3_WEIGHTS settings.

The postings of the reference test are chosen so that the ORDER of the adds and the TWO roundings of a weighted step both
show in the bits (asserted here): 3000 documents, 40 terms, two terms in about 90 % of the documents and the rest in about
30 %, impacts exp(N(0, 2)) as float32, 4 queries of 12 distinct terms with weights uniform in [0.05, 2].
"""
import functools

import numpy as np
import pytest

from hiprag.m3 import m3_score_reference
from hiprag.sparse import PostingsCSR, bm25_score_ids_reference, weighted_search_reference

F32_MAX = np.finfo(np.float32).max
F64_MAX = np.finfo(np.float64).max
N_DOCS, N_TERMS, NQ, NT = 3000, 40, 4, 12


@functools.lru_cache(maxsize=None)
def recipe():
    rng = np.random.default_rng(7)
    lists = []
    for t in range(N_TERMS):
        share = 0.9 if t < 2 else 0.3
        lists.append(np.flatnonzero(rng.random(N_DOCS) < share).astype(np.uint32))
    off = np.zeros(N_TERMS + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists]).astype(np.uint64)
    imp = np.exp(rng.normal(0.0, 2.0, size=int(off[-1]))).astype(np.float32)
    p = PostingsCSR(N_DOCS, N_TERMS, off, np.concatenate(lists), imp)
    qs = [rng.choice(N_TERMS, size=NT, replace=False).tolist() for _ in range(NQ)]
    ws = [rng.uniform(0.05, 2.0, size=NT).astype(np.float32) for _ in range(NQ)]
    return p, qs, ws


def all_ids():
    return np.tile(np.arange(N_DOCS, dtype=np.int64), (NQ, 1))


def test_reference_is_the_search_reference_for_every_document():
    p, qs, ws = recipe()
    ref = bm25_score_ids_reference(p, qs, ws, all_ids())
    s, i = weighted_search_reference(p, qs, ws, N_DOCS)
    for b in range(NQ):
        found = i[b] >= 0
        assert found.any()
        assert np.array_equal(ref[b, i[b][found]].view(np.uint32), s[b][found].view(np.uint32))
        rest = np.setdiff1d(np.arange(N_DOCS), i[b][found])
        assert np.array_equal(ref[b, rest].view(np.uint32), np.zeros(len(rest), np.float32).view(np.uint32))


def test_inputs_have_power_order_and_two_roundings():
    p, qs, ws = recipe()
    ref = bm25_score_ids_reference(p, qs, ws, all_ids())
    rev = bm25_score_ids_reference(p, [q[::-1] for q in qs], [w[::-1] for w in ws], all_ids())
    n_order = int((ref.view(np.uint32) != rev.view(np.uint32)).sum())
    # one rounding per step instead of two: acc = fl32(float64(acc) + float64(w) * float64(impact))
    off, docs, imp = p.offsets.astype(np.int64), p.doc_ids.astype(np.int64), p.impacts
    fused = np.zeros((NQ, N_DOCS), dtype=np.float32)
    for b in range(NQ):
        for t, w in zip(qs[b], ws[b]):
            d = docs[off[t]:off[t + 1]]
            fused[b, d] = (fused[b, d].astype(np.float64) + np.float64(w) * imp[off[t]:off[t + 1]].astype(np.float64)).astype(np.float32)
    n_round = int((ref.view(np.uint32) != fused.view(np.uint32)).sum())
    print(f"pairs whose bits change: reversed order {n_order}, single rounding {n_round} of {NQ * N_DOCS}")
    assert n_order > 0
    assert n_round > 0


def test_reference_ids_padding_duplicates_and_base():
    p, qs, ws = recipe()
    base = 500
    ids = np.array([[base, base + N_DOCS - 1, -1, base - 1, base + N_DOCS, base + 7, base + 7, base + 3]] * NQ, dtype=np.int64)
    ref = bm25_score_ids_reference(p, qs, ws, ids, id_base=base)
    full = bm25_score_ids_reference(p, qs, ws, all_ids())
    for b in range(NQ):
        assert np.array_equal(ref[b, [0, 1, 5, 6, 7]].view(np.uint32), full[b, [0, N_DOCS - 1, 7, 7, 3]].view(np.uint32))
        assert np.all(ref[b, [2, 3, 4]] == -F32_MAX)
    # weights None is every weight 1.0; an unknown term and an empty query score 0.0 for valid entries
    ones = [np.ones(NT, np.float32)] * NQ
    assert np.array_equal(bm25_score_ids_reference(p, qs, None, all_ids()).view(np.uint32),
                          bm25_score_ids_reference(p, qs, ones, all_ids()).view(np.uint32))
    odd = bm25_score_ids_reference(p, [[], [N_TERMS + 3]], None, np.array([[0, -1], [5, 6]], dtype=np.int64))
    assert odd.tolist() == [[0.0, -F32_MAX], [0.0, 0.0]]


# ---- m3_score_reference ---------------------------------------------------------------------------------------------

def test_m3_reference_order_duplicates_and_padding():
    dense = np.array([[0.5, 0.9, 0.5, 0.1, 0.9]], dtype=np.float64)
    sparse = np.zeros((1, 5), np.float32)
    ms = np.zeros((1, 5), np.float32)
    valid = np.array([[True, True, True, False, True]])
    pairs, scores, pos = m3_score_reference(dense, sparse, ms, valid, (1.0, 1.0, 1.0), 5)
    assert pos.tolist() == [[1, 4, 0, 2, -1]]                    # score descending, equal scores by position
    assert scores[0, 4] == -F64_MAX and pairs[0, 3] == -F64_MAX
    assert scores[0, 0] == ((1.0 * 0.9 + 0.0) + 0.0) / 3.0
    _, s2, p2 = m3_score_reference(dense, sparse, ms, valid, (1.0, 1.0, 1.0), 2)
    assert p2.tolist() == [[1, 4]] and s2[0, 0] == scores[0, 0]


def test_m3_reference_arithmetic_order_and_dropped_leg():
    rng = np.random.default_rng(3)
    d = rng.normal(size=(2, 9))
    s = rng.uniform(0, 30, size=(2, 9)).astype(np.float32)
    c = rng.uniform(-1, 1, size=(2, 9)).astype(np.float32)
    valid = np.ones((2, 9), bool)
    w = (0.4, 0.2, 0.4)
    pairs, _, _ = m3_score_reference(d, s, c, valid, w, 3)
    total = (np.float64(0.4) + np.float64(0.2)) + np.float64(0.4)
    want = ((np.float64(0.4) * d + np.float64(0.2) * s.astype(np.float64)) + np.float64(0.4) * c.astype(np.float64)) / total
    assert np.array_equal(pairs.view(np.uint64), want.view(np.uint64))
    # a zero weight DROPS the leg: its array is not read (None, or values that would poison a product)
    poison = np.full((2, 9), np.inf, dtype=np.float32)
    a, _, _ = m3_score_reference(d, None, c, valid, (0.4, 0.0, 0.4), 3)
    b, _, _ = m3_score_reference(d, poison, c, valid, (0.4, 0.0, 0.4), 3)
    want = (np.float64(0.4) * d + np.float64(0.4) * c.astype(np.float64)) / (np.float64(0.4) + np.float64(0.0) + np.float64(0.4))
    assert np.array_equal(a.view(np.uint64), want.view(np.uint64)) and np.array_equal(b.view(np.uint64), want.view(np.uint64))
    only_s, _, _ = m3_score_reference(None, s, None, valid, (0.0, 2.0, 0.0), 3)
    assert np.array_equal(only_s.view(np.uint64), ((np.float64(2.0) * s.astype(np.float64)) / np.float64(2.0)).view(np.uint64))


def test_m3_reference_l2_mapping_and_maxsim_padding():
    dist = np.array([[0.0, 0.5, 2.0, 4.0]], dtype=np.float64)
    ms = np.array([[0.25, -F32_MAX, 0.5, -F32_MAX]], dtype=np.float32)
    valid = np.ones((1, 4), bool)
    pairs, _, pos = m3_score_reference(dist, None, ms, valid, (1.0, 0.0, 1.0), 4, l2=True)
    assert pairs.tolist() == [[(1.0 + 0.25) / 2.0, (0.75 + 0.0) / 2.0, (0.0 + 0.5) / 2.0, (-1.0 + 0.0) / 2.0]]
    assert pos.tolist() == [[0, 1, 2, 3]]
    for bad in ((0, 0, 0), (1, -1, 1), (1, float("nan"), 1), (1, 1), (float("inf"), 0, 0)):
        with pytest.raises(ValueError):
            m3_score_reference(dist, None, ms, valid, bad, 1)


# ---- the settings ---------------------------------------------------------------------------------------------------

SETTINGS = ("HIP_COLLECTION", "HIP_COLLECTION_SPARSE", "HIP_SPARSE_MODE", "HIP_LATE_INTERACTION", "HIP_IVF_HYBRID", "HIP_RERANK",
            "HIP_LATE_SEARCH", "HIP_PAGES", "HIP_M3_SCORE", "HIP_M3_WEIGHTS")


@pytest.fixture
def cfg(monkeypatch):
    from rag.config import Config
    for name in SETTINGS:
        monkeypatch.delenv(name, raising=False)
    return Config()


def m3_env(monkeypatch):
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_COLLECTION_SPARSE", "lexical")
    monkeypatch.setenv("HIP_LATE_INTERACTION", "true")
    monkeypatch.setenv("HIP_M3_SCORE", "true")


def test_m3_setting_defaults_and_what_it_needs(cfg, monkeypatch):
    assert cfg.HIP_M3_SCORE is False
    assert cfg.HIP_M3_WEIGHTS == (0.4, 0.2, 0.4)
    monkeypatch.setenv("HIP_M3_SCORE", "true")
    with pytest.raises(ValueError, match="needs HIP_COLLECTION=true"):
        cfg.HIP_M3_SCORE
    monkeypatch.setenv("HIP_COLLECTION", "true")
    with pytest.raises(ValueError, match="needs HIP_COLLECTION_SPARSE=lexical"):
        cfg.HIP_M3_SCORE
    monkeypatch.setenv("HIP_COLLECTION_SPARSE", "lexical")
    with pytest.raises(ValueError, match="needs HIP_LATE_INTERACTION=true"):
        cfg.HIP_M3_SCORE
    monkeypatch.setenv("HIP_LATE_INTERACTION", "true")
    assert cfg.HIP_M3_SCORE is True


def test_m3_setting_lifts_one_refusal_and_only_when_set(cfg, monkeypatch):
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_COLLECTION_SPARSE", "lexical")
    monkeypatch.setenv("HIP_LATE_INTERACTION", "true")
    with pytest.raises(ValueError, match="one forward gives one extra output today"):
        cfg.HIP_COLLECTION_SPARSE                                  # unset: the refusal and its message stay
    monkeypatch.setenv("HIP_M3_SCORE", "false")
    with pytest.raises(ValueError, match="one forward gives one extra output today"):
        cfg.HIP_COLLECTION_SPARSE
    monkeypatch.setenv("HIP_M3_SCORE", "true")
    assert cfg.HIP_COLLECTION_SPARSE == "lexical"
    assert cfg.HIP_LATE_INTERACTION is True
    monkeypatch.setenv("HIP_IVF_HYBRID", "true")                   # the other refusals of the lexical leg still hold
    with pytest.raises(ValueError, match="HIP_IVF_HYBRID"):
        cfg.HIP_M3_SCORE


@pytest.mark.parametrize("name, match", [("HIP_RERANK", "two second stages"), ("HIP_LATE_SEARCH", "HIP_LATE_SEARCH"),
                                         ("HIP_PAGES", "device page path is out of scope")])
def test_m3_setting_refusals(cfg, monkeypatch, name, match):
    m3_env(monkeypatch)
    assert cfg.HIP_M3_SCORE is True
    monkeypatch.setenv(name, "true")
    with pytest.raises(ValueError, match=match):
        cfg.HIP_M3_SCORE


def test_m3_weights_parser(cfg, monkeypatch):
    from rag.config import parse_m3_weights
    assert parse_m3_weights("0.4,0.2,0.4") == (0.4, 0.2, 0.4)
    assert parse_m3_weights(" 1 , 0,2.5 ") == (1.0, 0.0, 2.5)
    for bad in ("", "1,2", "1,2,3,4", "a,b,c", "1,-1,1", "0,0,0", "nan,1,1", "inf,1,1", "1;2;3"):
        with pytest.raises(ValueError, match="HIP_M3_WEIGHTS"):
            parse_m3_weights(bad)
    monkeypatch.setenv("HIP_M3_WEIGHTS", "1,0,0")
    assert cfg.HIP_M3_WEIGHTS == (1.0, 0.0, 0.0)
    m3_env(monkeypatch)
    monkeypatch.setenv("HIP_M3_WEIGHTS", "0,0,0")
    with pytest.raises(ValueError, match="at least one weight"):
        cfg.HIP_M3_SCORE                                           # a malformed mix fails when the setting is read
