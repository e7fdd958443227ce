"""
CPU: the numpy specifications of the centroid codes and of the interaction stage (hiprag.colbert) against direct float64
loops; the comparison helper of the GPU tests (pruned_cases.check_candidates) against mutants of the interaction reference;
and the data of the GPU tests against the margins those tests quote.
"""
import numpy as np
import pytest

import pruned_cases as pc
from oracle.linear_cases import bf16_bits, bf16_values


def _small(seed=3, dim=64, ncent=32, lengths=(0, 1, 5, 9, 0, 5, 5, 12, 3, 5)):
    cent = pc.random_centroids(ncent, dim, seed)
    docs, drawn = pc.clustered_docs(cent, lengths, seed + 1)
    docs[6], drawn[6] = docs[2][::-1].copy(), drawn[2][::-1].copy()      # the multiset of codes of document 2: a tie
    docs[5], drawn[5] = docs[2].copy(), drawn[2].copy()                 # and again
    rng = np.random.default_rng(seed + 2)
    q = bf16_bits(pc.unit(rng.standard_normal((7, dim))).astype(np.float32))
    return cent, docs, drawn, q


def test_codes_reference_is_the_lowest_index_of_the_largest_fp64_dot():
    from hiprag.colbert import centroid_codes_reference
    cent, docs, drawn, _ = _small()
    c = bf16_values(cent).astype(np.float64)
    c[9] = c[4]                                                         # identical centroids: the lower index wins
    v = bf16_values(np.concatenate(docs)).astype(np.float64)
    want = np.zeros(len(v), np.int32)
    for i in range(len(v)):
        best, arg = -np.inf, -1
        for j in range(len(c)):
            s = float(np.dot(v[i], c[j]))
            if s > best:
                best, arg = s, j
        want[i] = arg
    got = centroid_codes_reference(v, c)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert 9 not in got.tolist() and 4 in got.tolist()
    assert centroid_codes_reference(np.zeros((0, 64)), c).shape == (0,)


def test_interaction_reference_is_mean_of_max_over_codes_in_fp64():
    from hiprag.colbert import centroid_codes_reference, centroid_interaction_reference
    cent, docs, _, q = _small()
    c, qv = bf16_values(cent).astype(np.float64), bf16_values(q).astype(np.float64)
    codes = [centroid_codes_reference(bf16_values(d), c) for d in docs]
    got = centroid_interaction_reference(qv, codes, c)
    for d, cd in enumerate(codes):
        if len(cd) == 0:
            assert got[d] == -np.inf
            continue
        total = 0.0
        for i in range(len(qv)):
            total += max(float(np.dot(qv[i], c[j])) for j in cd)
        assert abs(got[d] - total / len(qv)) <= 1e-12
    assert got[2] == got[5] == got[6]                                   # equal multisets of codes: exactly equal scores


def _mutant_scores(kind, qv, codes, c):
    table = qv @ c.T
    out = np.full(len(codes), -np.inf)
    for d, cd in enumerate(codes):
        if len(cd) == 0:
            if kind == "empty_ranked":
                out[d] = 0.0
            continue
        per_i = table[:, cd].sum(axis=1) if kind == "sum" else table[:, cd].max(axis=1)
        out[d] = per_i.sum() / (len(cd) if kind == "div_ld" else len(qv))
    return out


@pytest.mark.parametrize("kind", ["none", "sum", "div_ld", "empty_ranked", "tie_position"])
def test_the_comparison_helper_catches_mutants_of_the_interaction(kind):
    """What the GPU tests call on the library's candidates, called on a correct ranking (passes) and on four wrong ones."""
    from hiprag.colbert import centroid_codes_reference, centroid_interaction_reference
    cent, docs, _, q = _small()
    c, qv = bf16_values(cent).astype(np.float64), bf16_values(q).astype(np.float64)
    codes = [centroid_codes_reference(bf16_values(d), c) for d in docs]
    ref = centroid_interaction_reference(qv, codes, c)
    in_scope, ncand, tol = list(range(len(docs))), 8, pc.product_tolerance(64)
    scores = ref if kind in ("none", "tie_position") else _mutant_scores(kind, qv, codes, c)
    tie_order = None if kind != "tie_position" else {d: -d for d in in_scope}      # the later document first
    ids, sc = pc.rank_candidates(scores, in_scope, ncand, id_base=100, tie_order=tie_order)
    verdict = pc.check_candidates(ids, sc, ref, in_scope, ncand, tol, id_base=100)
    if kind == "none":
        assert verdict is None, verdict
        # and with fewer candidates than documents, a multi-part scope, a scope of empty documents
        for scope, nc in ((in_scope, 3), ([1, 2, 3, 7, 8], 8), ([0, 4], 4)):
            i2, s2 = pc.rank_candidates(ref, scope, nc)
            assert pc.check_candidates(i2, s2, ref, scope, nc, tol) is None
    else:
        assert verdict is not None, kind


def test_the_helper_notices_a_missing_better_document_and_a_wrong_padding():
    ref = np.asarray([0.9, 0.5, -np.inf, 0.7])
    tol = 1e-6
    assert pc.check_candidates([0, 3], [0.9, 0.7], ref, [0, 1, 2, 3], 2, tol) is None
    assert "missing" in pc.check_candidates([0, 1], [0.9, 0.5], ref, [0, 1, 2, 3], 2, tol)
    assert "padding" in pc.check_candidates([0, 3, 1, 2], [0.9, 0.7, 0.5, 0.0], ref, [0, 1, 2, 3], 4, tol)
    assert pc.check_candidates([0, 3, 1, -1], [0.9, 0.7, 0.5, pc.NEG_MAX], ref, [0, 1, 2, 3], 4, tol) is None


@pytest.mark.parametrize("dim", [64, 128])
def test_clustered_vectors_are_far_from_a_second_centroid(dim):
    """The codes test asks for EQUAL codes: the best and second-best float64 dots of its data lie >= 0.36 apart, three orders
    above the fp32 accumulation error, and the best centroid is the one the vector was drawn around."""
    from hiprag.colbert import centroid_codes_reference
    cent = pc.random_centroids(256, dim, 5)
    docs, drawn = pc.clustered_docs(cent, [200] * 10, 7)
    v, c = bf16_values(np.concatenate(docs)), bf16_values(cent)
    assert pc.top2_margin(v, c) >= 0.36
    assert np.array_equal(centroid_codes_reference(v, c), np.concatenate(drawn))
    assert pc.product_tolerance(1024) < 1e-3 * 0.36


@pytest.mark.parametrize("seed", range(5))
def test_planted_documents_stand_out_by_the_margins_quoted(seed):
    """The usefulness test allows no miss at ncand = 16 because, in float64: the planted document is rank 0 by centroid
    interaction, >= 0.46 above rank 16, and the exact top 1 by more than 1e-2."""
    from hiprag.colbert import centroid_codes_reference, centroid_interaction_reference, maxsim_reference
    cent, docs, q, targets = pc.planted(seed)
    c = bf16_values(cent).astype(np.float64)
    codes = [centroid_codes_reference(bf16_values(d), c) for d in docs]
    assert len(docs) == 400 and all(20 <= len(d) <= 40 for d in docs) and q.shape == (16, 8, 128)
    for i, t in enumerate(targets):
        qv = bf16_values(q[i]).astype(np.float64)
        a = centroid_interaction_reference(qv, codes, c)
        order = np.argsort(-a, kind="stable")
        assert order[0] == t and a[order[0]] - a[order[pc.PLANT_NCAND]] >= 0.46
        exact = np.asarray([maxsim_reference(qv, bf16_values(d)) for d in docs])
        eo = np.argsort(-exact, kind="stable")
        assert eo[0] == t and exact[eo[0]] - exact[eo[1]] > 1e-2
