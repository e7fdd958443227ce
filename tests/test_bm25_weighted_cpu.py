"""
CPU: the numpy restatements the weighted sparse leg is tested against -- hiprag.sparse.weighted_search_reference against a
brute-force dense accumulation, LexicalIndex's document-major -> term-major transpose against a loop, and the dedupe rule of
hiprag.lexical.lexical_reference on a hand-made sequence.  No GPU, no library call.
"""
import numpy as np

from hiprag.lexical import dedupe_token_weights, lexical_reference, lexical_token_weights, transpose_doc_weights
from hiprag.sparse import PostingsCSR, weighted_search_reference

F32_MAX = np.finfo(np.float32).max


def small_postings(n_docs=200, n_terms=12, seed=5, exact=False):
    rng = np.random.default_rng(seed)
    lists = [np.sort(rng.choice(n_docs, size=int(rng.integers(0, 120)), replace=False)).astype(np.uint32) for _ in range(n_terms)]
    off = np.zeros(n_terms + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists]).astype(np.uint64)
    n = int(off[-1])
    imp = (rng.integers(1, 9, size=n) / 4.0).astype(np.float32) if exact else rng.uniform(0.1, 3.0, size=n).astype(np.float32)
    return PostingsCSR(n_docs, n_terms, off, np.concatenate(lists), imp)


def brute_force(p, query, weights, k, ranges=None):
    """a dense [n_docs] fp32 accumulator filled posting by posting, then a plain sort by (score desc, id asc)"""
    acc = [np.float32(0)] * p.n_docs
    for t, w in zip(query, weights):
        if not 0 <= t < p.n_terms:
            continue
        for i in range(int(p.offsets[t]), int(p.offsets[t + 1])):
            d = int(p.doc_ids[i])
            acc[d] = np.float32(acc[d] + np.float32(np.float32(w) * p.impacts[i]))
    docs = [d for d in range(p.n_docs) if acc[d] > 0 and (ranges is None or any(lo <= d < hi for lo, hi in ranges))]
    docs.sort(key=lambda d: (-float(acc[d]), d))
    docs = docs[:k]
    s = np.full(k, -F32_MAX, dtype=np.float32)
    i = np.full(k, -1, dtype=np.int64)
    s[:len(docs)] = [acc[d] for d in docs]
    i[:len(docs)] = docs
    return s, i


def test_weighted_reference_equals_brute_force():
    for exact in (True, False):
        p = small_postings(exact=exact)
        rng = np.random.default_rng(9)
        queries = [[], [3], [1, 5, 1, 7], rng.integers(0, 12, size=9).tolist(), [2, 40, 11]]
        choice = np.asarray([0.5, 1.0, 1.5, 2.0], np.float32)
        weights = [rng.choice(choice, size=len(q)) if exact else rng.uniform(0.1, 2.0, size=len(q)).astype(np.float32) for q in queries]
        for k in (1, 10, 250):
            s, i = weighted_search_reference(p, queries, weights, k)
            for b, (q, w) in enumerate(zip(queries, weights)):
                es, ei = brute_force(p, q, w, k)
                assert np.array_equal(i[b], ei) and np.array_equal(s[b].view(np.uint32), es.view(np.uint32)), (exact, k, b)
        if exact:   # ties: equal scores inside a top 10, ordered by id
            s, i = weighted_search_reference(p, queries, weights, 10)
            tie = (s[:, :-1] == s[:, 1:]) & (i[:, 1:] >= 0)
            assert tie.any() and np.all(i[:, :-1][tie] < i[:, 1:][tie])
        scope = [(10, 60), (150, 151)]
        s, i = weighted_search_reference(p, queries, weights, 10, [scope] * len(queries))
        for b, (q, w) in enumerate(zip(queries, weights)):
            es, ei = brute_force(p, q, w, 10, scope)
            assert np.array_equal(i[b], ei) and np.array_equal(s[b].view(np.uint32), es.view(np.uint32))


def test_weighted_reference_rounds_the_product_before_the_add():
    """two roundings: a case where fl32(acc + fl32(w * x)) differs from the fused fl32(acc + w * x)"""
    rng = np.random.default_rng(3)
    found = False
    for _ in range(2000):
        a, w, x = (np.float32(v) for v in rng.uniform(0.1, 3.0, size=3))
        two = np.float32(a + np.float32(w * x))
        fused = np.float32(np.float64(a) + np.float64(w) * np.float64(x))
        if two != fused:
            p = PostingsCSR(1, 2, np.asarray([0, 1, 2], np.uint64), np.asarray([0, 0], np.uint32), np.asarray([a, x], np.float32))
            s, _ = weighted_search_reference(p, [[0, 1]], [[1.0, w]], 1)
            assert s[0, 0] == two
            found = True
            break
    assert found


def test_transpose_against_a_loop():
    rng = np.random.default_rng(21)
    n_docs, L, n_terms = 57, 9, 23
    counts = rng.integers(0, L + 1, size=n_docs)
    counts[0], counts[1] = 0, L
    terms = np.full((n_docs, L), -1, dtype=np.int32)
    weights = np.zeros((n_docs, L), dtype=np.float32)
    triples = set()
    for d in range(n_docs):
        t = np.sort(rng.choice(n_terms - 1, size=counts[d], replace=False))      # term n_terms - 1 never occurs: an empty list
        terms[d, :counts[d]] = t
        weights[d, :counts[d]] = rng.uniform(0.01, 2.0, size=counts[d]).astype(np.float32)
        triples |= {(d, int(x), float(w)) for x, w in zip(t, weights[d, :counts[d]])}
    p = transpose_doc_weights(terms, weights, counts, n_terms)
    assert p.n_docs == n_docs and p.n_terms == n_terms and p.offsets.dtype == np.uint64 and p.doc_ids.dtype == np.uint32
    assert int(p.offsets[0]) == 0 and int(p.offsets[-1]) == counts.sum() == len(p.doc_ids) == len(p.impacts)
    seen = []
    for t in range(n_terms):
        lo, hi = int(p.offsets[t]), int(p.offsets[t + 1])
        assert np.all(np.diff(p.doc_ids[lo:hi].astype(np.int64)) > 0), "doc ids must ascend within a list"
        seen += [(int(d), t, float(w)) for d, w in zip(p.doc_ids[lo:hi], p.impacts[lo:hi])]
    assert len(seen) == len(triples) and set(seen) == triples       # every (doc, term, weight) once
    assert int(p.offsets[n_terms]) == int(p.offsets[n_terms - 1])


def test_dedupe_rule_on_a_hand_made_sequence():
    #        position  0    1    2    3    4    5    6    7
    ids = [0, 7, 9, 7, 5, 3, 9, 2]
    wts = [0.875, 0.25, 0.0, 0.75, 0.5, 0.8125, 0.0, 0.375]
    t, w = dedupe_token_weights(ids, wts, unused_ids=(0, 1, 2, 3))
    # 0, 3 and 2 are unused; 9 occurs twice with weight 0 and is dropped; 7 occurs twice and keeps its larger weight
    assert t.tolist() == [5, 7] and w.tolist() == [0.5, 0.75] and t.dtype == np.int32 and w.dtype == np.float32
    # the same through lexical_reference: hidden rows whose only non-zero column carries the wanted dot product
    H = 64
    weight = np.zeros(H, np.float32)
    weight[0] = 1.0
    hidden = np.zeros((len(ids), H), np.float32)
    hidden[:, 0] = np.asarray(wts, np.float32) - 0.125          # bias 0.125 restores the weights; position 2: relu(-0.125 + 0.125) = 0
    hidden[6, 0] = -3.0                                         # a negative dot: relu clamps it
    assert np.array_equal(lexical_token_weights(hidden, weight, 0.125), np.asarray(wts, np.float32))
    terms, weights, counts = lexical_reference([hidden, np.zeros((0, H), np.float32)], [ids, []], weight, 0.125, (0, 1, 2, 3), max_len=10)
    assert counts.tolist() == [2, 0]
    assert terms[0].tolist() == [5, 7] + [-1] * 8 and weights[0].tolist() == [0.5, 0.75] + [0.0] * 8
    assert np.all(terms[1] == -1) and np.all(weights[1] == 0)


def test_token_weights_follow_the_stated_order():
    """lane partial sums over columns l, l + 64, .., then the butterfly 32, 16, .., 1 -- against a scalar restatement"""
    rng = np.random.default_rng(8)
    H = 256
    x = rng.standard_normal((5, H)).astype(np.float32)
    w = (rng.standard_normal(H) * 0.02).astype(np.float32)
    got = lexical_token_weights(x, w, 0.01)
    for r in range(5):
        lanes = [np.float32(0)] * 64
        for c in range(H):
            lanes[c % 64] = np.float32(lanes[c % 64] + np.float32(x[r, c] * w[c]))
        for off in (32, 16, 8, 4, 2, 1):
            lanes = [np.float32(lanes[l] + lanes[l ^ off]) for l in range(64)]
        assert len({v.tobytes() for v in lanes}) == 1, "every lane of the butterfly ends with the same bits"
        assert got[r] == max(np.float32(0), np.float32(lanes[0] + np.float32(0.01)))
