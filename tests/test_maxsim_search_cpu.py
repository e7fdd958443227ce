"""
CPU: maxsim_search_reference, the numpy statement of hipmaxsim_search_scoped's order and padding, on hand-made score tables
-- and the proof that those tables can fail: every one-line slip of the selection (an inclusive range end, ties to the
higher id, a document without vectors ranked, a query ranked over another query's scope, padding score 0) changes the result
on EVERY case set.  Then the HIP_LATE_SEARCH setting and the argument checks of the wrappers, none of which needs a GPU.
"""
import numpy as np
import pytest

NEG_MAX = -float(np.finfo(np.float32).max)
MUTANTS = ("inclusive_end", "ties_to_higher_id", "invalid_ranked", "other_querys_scope", "padding_zero")


def _select(pairs, valid, ranges, offsets, soq, k, id_base=0, mutant=None):
    """The selection written out once more, with the slips it can suffer."""
    nq, n_docs = pairs.shape
    scores = np.full((nq, k), 0.0 if mutant == "padding_zero" else NEG_MAX, dtype=np.float32)
    ids = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        s = soq[(i + 1) % nq] if mutant == "other_querys_scope" else soq[i]
        docs = []
        for lo, hi in ranges[offsets[s]:offsets[s + 1]]:
            for d in range(lo, min(hi + 1 if mutant == "inclusive_end" else hi, n_docs)):
                if (valid[i, d] or mutant == "invalid_ranked") and d not in docs:
                    docs.append(d)
        docs.sort(key=lambda d: (-float(pairs[i, d]), -d if mutant == "ties_to_higher_id" else d))
        for r, d in enumerate(docs[:k]):
            scores[i, r], ids[i, r] = pairs[i, d], d + id_base
    return scores, ids


def _case_two_scopes():
    # 8 documents, document 2 holds no vector (and would win); query 0 over [1,3) + [5,6), query 1 over [3,5) + [6,8)
    pairs = np.asarray([[9, 4, 99, 8, 1, 4, 7, 2],
                        [1, 2, 3, 5, 5, 6, 5, 0.5]], dtype=np.float32)
    valid = np.ones((2, 8), dtype=bool)
    valid[:, 2] = False
    ranges = np.asarray([[1, 3], [5, 6], [3, 5], [6, 8]], dtype=np.int64)
    return dict(pairs=pairs, valid=valid, ranges=ranges, offsets=np.asarray([0, 2, 4]), soq=np.asarray([0, 1]), k=4,
                want_ids=[[1, 5, -1, -1], [3, 4, 6, 7]], want_scores=[[4, 4, NEG_MAX, NEG_MAX], [5, 5, 5, 0.5]])


def _case_three_scopes():
    # 7 documents, document 0 and (for query 2) document 6 hold no vector; an empty range; ties between 4 and 5
    pairs = np.asarray([[50, -1, 7, 7, 7, 7, 7],
                        [3, 3, 2, 2.5, 9, 9, 9],
                        [0, 0, 8, 8, 6, 6, 60]], dtype=np.float32)
    valid = np.ones((3, 7), dtype=bool)
    valid[:, 0] = False
    valid[2, 6] = False
    ranges = np.asarray([[0, 2], [2, 2], [2, 4], [4, 7]], dtype=np.int64)
    return dict(pairs=pairs, valid=valid, ranges=ranges, offsets=np.asarray([0, 1, 3, 4]), soq=np.asarray([0, 1, 2]), k=3,
                want_ids=[[1, -1, -1], [3, 2, -1], [4, 5, -1]], want_scores=[[-1, NEG_MAX, NEG_MAX], [2.5, 2, NEG_MAX], [6, 6, NEG_MAX]])


CASES = {"two_scopes": _case_two_scopes, "three_scopes": _case_three_scopes}


@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_on_hand_made_tables(case):
    from hiprag import maxsim_search_reference
    c = CASES[case]()
    for id_base in (0, 1000):
        scores, ids = maxsim_search_reference(c["pairs"], c["valid"], c["ranges"], c["offsets"], c["soq"], c["k"], id_base)
        want_ids = np.asarray(c["want_ids"], dtype=np.int64)
        assert np.array_equal(ids, np.where(want_ids >= 0, want_ids + id_base, -1))
        assert scores.dtype == np.float32 and scores.tobytes() == np.asarray(c["want_scores"], dtype=np.float32).tobytes()
        again = _select(c["pairs"], c["valid"], c["ranges"], c["offsets"], c["soq"], c["k"], id_base)
        assert again[0].tobytes() == scores.tobytes() and np.array_equal(again[1], ids)     # the mutants below mutate THIS statement


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_every_case_set_catches_every_mutant(case, mutant):
    from hiprag import maxsim_search_reference
    c = CASES[case]()
    want = maxsim_search_reference(c["pairs"], c["valid"], c["ranges"], c["offsets"], c["soq"], c["k"])
    got = _select(c["pairs"], c["valid"], c["ranges"], c["offsets"], c["soq"], c["k"], mutant=mutant)
    assert got[0].tobytes() != want[0].tobytes() or not np.array_equal(got[1], want[1]), (case, mutant)


def test_the_reference_takes_what_pack_scopes_gives():
    from hiprag import maxsim_search_reference
    from hiprag.index import pack_scopes
    c = _case_two_scopes()
    ranges, offsets, soq = pack_scopes([[(1, 3), (5, 6)], [(3, 5), (6, 8)]], None, 2)
    scores, ids = maxsim_search_reference(c["pairs"], c["valid"], ranges, offsets, soq, c["k"])
    assert np.array_equal(ids, np.asarray(c["want_ids"]))
    ranges, offsets, soq = pack_scopes([[]], None, 2)                   # a scope without documents: all padding
    scores, ids = maxsim_search_reference(c["pairs"], c["valid"], ranges[:0], offsets, soq, 2)
    assert np.all(ids == -1) and np.all(scores == np.float32(NEG_MAX))


def test_late_search_setting(monkeypatch):
    from rag.config import config
    import rag.query.retriever as rt
    for name in ("HIP_LATE_SEARCH", "HIP_LATE_INTERACTION", "HIP_COLLECTION", "HIP_RERANK"):
        monkeypatch.delenv(name, raising=False)
    assert config.HIP_LATE_SEARCH is False                               # off by default
    assert rt.HybridRetriever(hybrid=True)._late_search() is False       # and then nothing is checked
    monkeypatch.setenv("HIP_LATE_INTERACTION", "true")
    monkeypatch.setenv("HIP_COLLECTION", "true")
    assert config.HIP_LATE_SEARCH is False                               # late interaction alone stays a second stage
    monkeypatch.delenv("HIP_LATE_INTERACTION")
    monkeypatch.delenv("HIP_COLLECTION")
    monkeypatch.setenv("HIP_LATE_SEARCH", "true")
    with pytest.raises(ValueError, match="HIP_LATE_INTERACTION"):
        config.HIP_LATE_SEARCH
    monkeypatch.setenv("HIP_LATE_INTERACTION", "true")
    with pytest.raises(ValueError, match="HIP_COLLECTION"):
        config.HIP_LATE_SEARCH
    monkeypatch.setenv("HIP_COLLECTION", "true")
    monkeypatch.setenv("HIP_RERANK", "true")
    with pytest.raises(ValueError, match="two second stages"):
        config.HIP_LATE_SEARCH
    monkeypatch.setenv("HIP_RERANK", "false")
    assert config.HIP_LATE_SEARCH is True                                # read at use
    assert rt.HybridRetriever(hybrid=False, rerank=False)._late_search() is True
    with pytest.raises(ValueError, match="hybrid"):
        rt.HybridRetriever(hybrid=True, rerank=False)._late_search()
    with pytest.raises(ValueError, match="two second stages"):
        rt.HybridRetriever(hybrid=False, rerank=True)._late_search()
    import asyncio
    with pytest.raises(ValueError, match="hybrid"):                      # before anything is embedded or searched
        asyncio.run(rt.HybridRetriever(hybrid=True, rerank=False).retrieve_chunks("q", "p"))


def test_wrapper_argument_checks_need_no_gpu():
    import torch
    from hiprag import maxsim_search, maxsim_search_device

    class Store:                                                          # the checks come before any native call
        dim, _h = 64, 0
    qv, qc = np.zeros((2, 4, 64), np.uint16), np.asarray([1, 2], np.int32)
    with pytest.raises(ValueError, match="q_vecs"):
        maxsim_search(Store(), qv.reshape(2, 8, 32), qc, [[(0, 1)]], None, 1)            # another dim
    with pytest.raises(ValueError, match="q_vecs"):
        maxsim_search(Store(), qv[0], qc, [[(0, 1)]], None, 1)                            # not [nq, q_stride, dim]
    with pytest.raises(ValueError, match="q_vecs"):
        maxsim_search(Store(), qv, qc[:1], [[(0, 1)]], None, 1)                           # one count per query
    with pytest.raises(ValueError, match="scope_of_query"):
        maxsim_search(Store(), qv, qc, [[(0, 1)], [(1, 2)], [(2, 3)]], None, 1)           # neither one scope nor one per query
    with pytest.raises(ValueError, match="scope_of_query"):
        maxsim_search(Store(), qv, qc, [[(0, 1)]], [0], 1)
    tq, tc = torch.zeros((2, 4, 64), dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        maxsim_search_device(Store(), tq, tc, [[(0, 1)]], None, 1)                        # host tensors
    with pytest.raises(ValueError, match="bfloat16"):
        maxsim_search_device(Store(), tq.float(), tc, [[(0, 1)]], None, 1)
