"""
CPU: the data and the model of tests/pruned_shape_cases.py.  The sets have the shapes test_maxsim_pruned_shapes_gpu.py relies
on; the exact regime is exact in bf16 and in MXFP4; the unmutated model of the stage is centroid_interaction_reference +
rank_candidates; every mutant is caught by the comparison the GPU file makes (pruned_shape_cases.verdict, or the equality of
the codes) on the data the GPU file runs; and the random data keep the margin the codes comparison needs.  No GPU.
"""
import numpy as np
import pytest

import maxsim_width_cases as wc
import pruned_cases as pc
import pruned_shape_cases as ps
from oracle.linear_cases import bf16_bits, bf16_values


# ---- the sets ----------------------------------------------------------------------------------------------------------------
def test_set_l_has_the_shape_the_gpu_file_relies_on():
    for regime in ps.REGIMES:
        cent, docs, drawn = ps.documents("L", regime)
        lens = [len(d) for d in docs]
        assert len(docs) == ps.N_DOCS == 600 and len(ps.slices_of([(0, ps.N_DOCS)])) == 3
        assert all(lens[d] == n for d, n in ps.FIXED.items()) and max(lens) == ps.CAP
        assert {lens[d] for d in ps.FIXED} >= {63, 64, 65, 127, 128, 129, 200, 511}
        rest = [n for d, n in enumerate(lens) if d not in ps.FIXED and d not in dict((b, a) for a, b in ps.PAIRS)]
        assert set(rest) == {0, 1, 2, 3}
        print(f"set L ({regime}): {sum(lens)} vectors, {sum(1 for n in lens if n)} documents with vectors")
        for c in ps.COPIES_OF_5:                                        # the same lane of the codes kernel, another tile or trip
            assert np.array_equal(cent[c], cent[5]) and c % ps.ROW_TILE == 5
        assert [c // ps.ROW_TILE for c in (5,) + ps.COPIES_OF_5] == [0, 1, 2]
        for src, dst in ps.PAIRS:
            assert np.array_equal(docs[dst], docs[src][::-1]) and lens[src] >= 63
        assert ps.PAIRS[0][0] // 256 == ps.PAIRS[0][1] // 256 and ps.PAIRS[1][0] // 256 != ps.PAIRS[1][1] // 256
        if drawn is not None:
            assert not np.isin(np.concatenate(drawn), ps.COPIES_OF_5).any() and 5 in np.concatenate(drawn).tolist()
    # the scopes: one, two, three and five slices; a slice of one document
    assert [len(ps.slices_of(sc)) for sc in ps.SCOPES_L] == [3, 1, 5, 1]
    assert [len(ps.slices_of(sc)) for sc in ps.EDGE_SCOPES] == [1, 1, 2, 3, 1, 3, 2]
    b_q, b_s = ps.batch(10, len(ps.SCOPES_L))
    assert ps.expected_items(ps.SCOPES_L, b_s) == 2 * (3 + 1 + 5 + 1)   # ten queries a scope: a group of eight and one of two
    assert [len(d) for d in ps.documents("T", "exact")[1]][:10] == list(ps.FIXED.values())


def test_the_counts_reach_every_path_of_the_interaction_kernel():
    for q_stride in ps.STRIDES:
        qc = ps.raw_counts(q_stride)
        qv, _ = ps.queries("exact", q_stride)
        assert qc[-1] == q_stride + 5 and qc[-2] == -3 and qc[-3] == 0 and len(qc) > ps.GROUP
        for i, c in enumerate(qc):
            n = ps.clamp(c, q_stride)
            assert not np.any(qv[i, :n] == ps.POISON) and np.all(qv[i, n:] == ps.POISON)
    full = ps.raw_counts(512)
    assert full[:7].tolist() == [1, 31, 32, 33, 64, 65, 130]             # both sides of 32 (lane halves) and of 64 (a second trip over i)
    assert {q % 32 for q in ps.STRIDES} >= {0, 1} and 512 in ps.STRIDES and 1 in ps.STRIDES
    assert any((-(-q // 32)) % 2 for q in ps.STRIDES if q > 32)         # P an odd multiple of 32: the last trip's second tile is behind P


@pytest.mark.parametrize("dim", (128,) + wc.BF16_WIDTHS + wc.FP8_WIDTHS)
def test_the_exact_regime_is_exact_in_bf16_and_in_mxfp4(dim):
    from hiprag.colbert import mxfp4_dequantize, mxfp4_quantize_reference
    rng = np.random.default_rng(dim)
    cent = ps.centroids("exact", 96, dim, 3)
    for bits in (cent, ps.integer_vectors(200, dim, rng), ps.integers_around(cent, [5, 37, 0, 95], rng)):
        v = bf16_values(bits).astype(np.float64)
        assert set(np.unique(v)) <= {-1.0, 0.0, 1.0} and np.array_equal(bf16_bits(v.astype(np.float32)), bits)
        if dim % 128 == 0:
            assert np.array_equal(mxfp4_dequantize(*mxfp4_quantize_reference(bits)), bits)
    assert 512 * dim < 2 ** 24


def test_integer_vectors_tie_for_their_maximum_and_vectors_around_a_centroid_do_not():
    cent, docs, _ = ps.documents("L", "exact")
    c = bf16_values(cent).astype(np.float64)
    s = bf16_values(np.concatenate(docs)).astype(np.float64) @ c.T
    tied = ((s == s.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean()
    print(f"{tied:.3f} of set L's integer vectors tie for their maximum")
    assert tied > 0.05
    codes = ps.model_codes(bf16_values(np.concatenate(docs)), c)
    assert not np.isin(codes, ps.COPIES_OF_5).any() and 5 in codes.tolist()
    rng = np.random.default_rng(1)
    near = bf16_values(ps.integers_around(cent, [5] * 64 + [37] * 32 + [69] * 33, rng)).astype(np.float64) @ c.T
    top = np.sort(near, axis=1)
    assert np.all(top[:, -1] == top[:, -3]) and np.all(top[:, -3] - top[:, -4] >= 20)     # the three copies, far above the rest
    assert np.all(np.argmax(near, axis=1) == 5)


# ---- the model is the reference ----------------------------------------------------------------------------------------------
def _set_l(regime, mutant=None):
    cent, docs, _ = ps.documents("L", regime)
    codes, off = ps.stored_codes(docs, cent, mutant if mutant in ps.CODE_MUTANTS else None)
    return cent, docs, codes, off


@pytest.mark.parametrize("regime", ps.REGIMES)
@pytest.mark.parametrize("q_stride", ps.STRIDES)
def test_the_unmutated_model_is_the_reference_and_its_ranking(regime, q_stride):
    cent, docs, codes, off = _set_l(regime)
    qv, qc = ps.queries(regime, q_stride)
    ref = ps.reference_scores(qv, qc, codes, off, cent)
    scores = ps.stage_scores(qv, qc, codes, off, cent)
    ties = []
    for i in range(len(qc)):
        n = ps.clamp(qc[i], q_stride)
        for scope in ps.SCOPES_L + ps.EDGE_SCOPES[3:4]:
            for ncand in ps.NCANDS:
                got = ps.model_rank(*scores[i], scope, ncand, id_base=50)
                want = ps.expected_candidates(ref[i], n, scope, ncand, id_base=50)
                assert got[1].tobytes() == want[1].tobytes(), (i, scope, ncand)
                if regime == "exact":
                    assert ps.same_candidates(*got, *want), (i, scope, ncand)
                assert ps.verdict(regime, *got, ref[i], n, scope, ncand, ps.DIM, id_base=50) is None
        if n:
            top = ps.model_rank(*scores[i], ps.SCOPES_L[0], 256)[1]
            ties.append(int((top[1:] == top[:-1]).sum()))
    print(f"{regime} q_stride {q_stride}: equal-score neighbours among 256 candidates, per query: {ties}")
    if regime == "exact":
        assert min(ties) >= 10                                         # genuine ties that only the id order resolves
    # a count above q_stride is the count q_stride; a count <= 0 ranks nothing
    again = ps.model_scores(ps.model_table(bf16_values(qv[-1]).astype(np.float64), bf16_values(cent).astype(np.float64)), q_stride, q_stride, codes, off)
    assert again[0].tobytes() == scores[-1][0].tobytes()
    assert not scores[-2][1].any() and not scores[-3][1].any()


# ---- every mutant is caught -------------------------------------------------------------------------------------------------
def _caught(regime, q_stride, mutant, which="L", ncent=ps.NCENT, scopes=ps.SCOPES_L, ncands=ps.NCANDS):
    """Whether the GPU file's comparisons notice the mutant on this case: the codes against centroid_codes_reference, the
    candidates of every (query, scope, ncand) through verdict()."""
    from hiprag.colbert import centroid_codes_reference
    cent, docs, _ = ps.documents(which, regime, ps.DIM, ncent)
    right, off = ps.stored_codes(docs, cent)
    codes, _ = ps.stored_codes(docs, cent, mutant if mutant in ps.CODE_MUTANTS else None)
    assert np.array_equal(right, centroid_codes_reference(bf16_values(np.concatenate(docs)), bf16_values(cent)))
    if not np.array_equal(codes, right):
        return True
    qv, qc = ps.queries(regime, q_stride, ps.DIM, ncent)
    ref = ps.reference_scores(qv, qc, right, off, cent)
    scores = ps.stage_scores(qv, qc, codes, off, cent, mutant if mutant in ps.SCORE_MUTANTS + ps.TABLE_MUTANTS else None)
    for i in range(len(qc)):
        for scope in scopes:
            for ncand in ncands:
                got = ps.model_rank(*scores[i], scope, ncand, mutant=mutant if mutant in ps.RANK_MUTANTS else None)
                if ps.verdict(regime, *got, ref[i], ps.clamp(qc[i], q_stride), scope, ncand, ps.DIM) is not None:
                    return True
    return False


@pytest.mark.parametrize("regime", ps.REGIMES)
@pytest.mark.parametrize("q_stride", ps.STRIDES)
def test_every_mutant_is_caught_on_set_l_wherever_it_applies(regime, q_stride):
    assert not _caught(regime, q_stride, None)
    for m in ps.MUTANTS:
        if ps.applies(m, regime, q_stride):
            assert _caught(regime, q_stride, m), (m, regime, q_stride)


def test_every_mutant_applies_somewhere_and_the_exclusions_are_real():
    for m in ps.MUTANTS:
        assert any(ps.applies(m, r, q) for r in ps.REGIMES for q in ps.STRIDES), m
    # where a mutant is excluded it changes nothing: the exclusion is no convenience
    assert not _caught("exact", 33, "query_rows_past_64_dropped") and not _caught("exact", 32, "rows_past_first_tile_zeroed")


@pytest.mark.parametrize("ncent", ps.TABLE_NCENTS)
def test_the_table_mutants_are_caught_on_set_t_at_every_table_shape(ncent):
    for regime in ps.REGIMES:
        for q_stride in ps.TABLE_STRIDES:
            assert not _caught(regime, q_stride, None, "T", ncent, ps.SCOPES_T, (16, 256))
            for m in ps.TABLE_MUTANTS + ("codes_past_64_dropped",):
                if ps.applies(m, regime, q_stride, ncent):
                    assert _caught(regime, q_stride, m, "T", ncent, ps.SCOPES_T, (16, 256)), (m, regime, q_stride, ncent)
    assert ncent % ps.ROW_BLOCK                                          # every shape has a partial block of streamed centroids


def test_the_same_lane_tie_mutant_shows_on_copies_of_one_lane_only():
    """The existing tie test copies centroid 5 to 40 and 77, three different lanes: there the slip changes nothing."""
    rng = np.random.default_rng(4)
    cent = ps.centroids("random", 96, 128, 9)
    other = cent.copy()
    other[37], other[69] = pc.random_centroids(96, 128, 10)[[37, 69]]
    other[40], other[77] = other[5], other[5]
    v = bf16_values(pc.vectors_around(cent, [5] * 40, rng))
    assert np.all(ps.model_codes(v, bf16_values(other)) == 5) and np.all(ps.model_codes(v, bf16_values(other), "argmax_tie_to_higher_centroid") == 5)
    assert np.all(ps.model_codes(v, bf16_values(cent)) == 5) and np.all(ps.model_codes(v, bf16_values(cent), "argmax_tie_to_higher_centroid") == 69)


# ---- the random data keep their margin --------------------------------------------------------------------------------------
def _margin(values, cent, ncent):
    keep = [c for c in range(ncent) if c not in ps.copies(ncent)]       # a copy of centroid 5 is no second centroid
    return pc.top2_margin(values, bf16_values(cent)[keep])


@pytest.mark.parametrize("which,dim,ncent", [("L", 128, 96)] + [("T", 128, n) for n in ps.TABLE_NCENTS] + [("W", d, 96) for d in sorted(set(wc.BF16_WIDTHS + wc.FP8_WIDTHS))])
def test_random_vectors_are_far_from_a_second_centroid(which, dim, ncent):
    from hiprag.colbert import centroid_codes_reference
    if which == "W":
        cent, docs, drawn = ps.width_documents("random", dim)
    else:
        cent, docs, drawn = ps.documents(which, "random", dim, ncent)
    v = bf16_values(np.concatenate(docs))
    gap = _margin(v, cent, ncent)
    print(f"{which} {dim}-d {ncent} centroids: top-2 gap {gap:.3f}, 100 x the accumulation bound {100 * pc.product_tolerance(dim):.2e}")
    assert gap > 100 * pc.product_tolerance(dim)
    assert np.array_equal(centroid_codes_reference(v, bf16_values(cent)), np.concatenate(drawn))
