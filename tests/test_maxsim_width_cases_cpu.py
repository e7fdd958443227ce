"""
The MaxSim width cases (tests/maxsim_width_cases.py) judged on the CPU: the width lists reach every tile count, chunk count and
line count they are meant for; the exactness preconditions of colbert_cases and fp8_cases hold at every width; the model of a
work item is maxsim_expected pair by pair; and every mutant changes the expected result of the GPU tests on every width it
is meant for.  No GPU, no library call.
"""
import numpy as np
import pytest

import fp8_cases as fc
import maxsim_width_cases as wc
from colbert_cases import NEG_MAX, maxsim_expected
from oracle.linear_cases import bf16_bits, bf16_values


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the lists -------------------------------------------------------------------------------------------------------------
def test_the_widths_reach_every_path_they_name():
    assert [wc.tiles_of(d) for d in (64, 128, 576, 640, 768, 832, 1024)] == [4, 4, 4, 3, 3, 2, 2]      # hand-worked from the rule
    for widths in (wc.BF16_WIDTHS, wc.FP8_WIDTHS):
        assert {wc.tiles_of(d) for d in widths} == {2, 3, 4}
        assert all(d % 64 == 0 and 64 <= d <= 1024 for d in widths)
    assert all(d % 128 == 0 for d in wc.FP8_WIDTHS)
    # both edges of every T in bf16; T = 3 and T = 2 twice each in fp8
    assert wc.tiles_of(576) == 4 and wc.tiles_of(640) == 3 and wc.tiles_of(768) == 3 and wc.tiles_of(832) == 2
    assert [wc.tiles_of(d) for d in wc.FP8_WIDTHS] == [4, 4, 3, 3, 2, 2]
    chunks = [d // 64 for d in wc.BF16_WIDTHS]
    assert 1 in chunks and any(c % 2 for c in chunks if c > 1)                     # one chunk; an odd count off the 128 grid
    assert 192 in wc.BF16_WIDTHS and 192 % 128
    lines = [d // 128 for d in wc.FP8_WIDTHS]
    assert min(lines) == 2 and {5, 7} <= set(lines) and max(lines) == 8           # a second line everywhere; odd counts; the maximum


def test_set_a_has_the_shape_the_issue_asks_for():
    lens = [wc.LENGTHS[i % 6] for i in range(wc.N_DOCS)]
    assert set(lens) == {0, 1, 31, 32, 33, 65} and 35 <= wc.N_DOCS <= 48
    for src, dst in wc.COPIES:
        assert lens[src] == lens[dst] > 0
    assert wc.COUNTS[:6] == (0, 1, 8, 8, 33, 70)
    first = np.cumsum((0,) + wc.COUNTS[:wc.GROUP])
    assert first[-1] > 128                                                          # T = 4 takes two passes over the first group
    for tiles in (2, 3, 4):                                                         # and a query straddles a pass at every T
        R = 32 * tiles
        assert any(lo < p * R < hi for lo, hi in zip(first[:-1], first[1:]) for p in range(1, 5)), tiles
    assert max(wc.COUNTS) <= wc.Q_STRIDE and len(wc.COUNTS) > wc.GROUP             # a second, smaller group
    # scopes: starts and ends off the 16-document slices, one range that ends where the next begins, an empty range, a scope
    # of empty documents only
    offs = [b % wc.SLICE for sc in wc.SCOPES for r in sc for b in r]
    assert sum(1 for o in offs if o) >= 8
    for s in wc.EMPTY_SCOPES:
        assert all(lens[d] == 0 for d in wc.scope_docs(wc.SCOPES[s]))
    assert any(len(wc.scope_docs(sc)) and all(lens[d] == 0 for d in wc.scope_docs(sc)) for sc in wc.SCOPES)
    both = [d for src_dst in wc.COPIES for d in src_dst]
    assert set(both) <= set(wc.scope_docs(wc.SCOPES[0]).tolist())                   # the ties are all inside the whole-store scope


# ---- the preconditions at every width -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,fmt", wc.SETS)
def test_exactness_preconditions_hold_at_every_width(dim, fmt):
    docs, queries = wc.doc_vectors("exact", dim), wc.query_vectors("exact", dim)
    stored = wc.stored_values(docs, fmt)
    for d, s in zip(docs, stored):
        assert np.array_equal(d, s)                                                 # integers in [-4, 4] are lossless in fp8 too
    long_q, long_d = queries[5], docs[5]
    maxsim_expected(long_q, long_d, "exact")                                        # its own assert: every partial sum < 2^24
    assert (np.abs(long_q) @ np.abs(long_d).T).max() <= 16 * dim < 2 ** 14 + 1
    for v in docs + queries:                                                        # every value is a bf16
        assert np.array_equal(bf16_values(bf16_bits(v)).astype(np.float64), v)
    for v in wc.doc_vectors("random", dim)[1:3]:
        assert np.array_equal(bf16_values(bf16_bits(v)).astype(np.float64), v)


@pytest.mark.parametrize("dim", (128,) + wc.FP8_WIDTHS)
def test_fp8_statements_agree_and_stay_exact_at_every_width(dim):
    from hiprag import fp8_dequantize, fp8_quantize_reference
    bits = wc.store_vectors(dim)
    codes, scales = fp8_quantize_reference(bits)
    c2, s2 = fc.quantize(bits)
    assert codes.tobytes() == c2.tobytes() and scales.tobytes() == s2.tobytes()
    assert not np.any((codes & 0x7F) == 0x7F) and not np.any(codes == 0x80)
    back = fp8_dequantize(codes, scales)                                            # asserts that code * scale is a bf16
    assert np.array_equal(bf16_values(back).astype(np.float64), fc.dequantized(codes, scales))
    ints = fc.integer_vectors(12, dim, 4)
    assert np.array_equal(bf16_values(fp8_dequantize(*fp8_quantize_reference(ints))), bf16_values(ints))
    finite = np.concatenate([fc.unit_vectors(24, dim, 3), wc.lane_sweep_vectors(dim)])      # (the special vectors hold inf and nan)
    assert fc.error_ratio(finite, *fc.quantize(finite)) <= 1.0
    assert fc.guarded_count(fc.special_vectors(dim)) == fc.N_GUARDED_SPECIAL


# ---- the model is the reference; its mutants are not ------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,fmt", [(64, "bf16"), (192, "bf16"), (640, "fp8"), (1024, "fp8")])
def test_the_model_of_a_work_item_is_maxsim_expected(dim, fmt):
    for regime in wc.REGIMES:
        stored = wc.stored_values(wc.doc_vectors(regime, dim), fmt)
        queries = wc.query_vectors(regime, dim)
        qv, qc = wc.query_block(queries, wc.Q_STRIDE, dim)
        scores, valid = wc.score_table(qv, qc, np.arange(len(qc)), stored, wc.tiles_of(dim))
        for i, q in enumerate(queries):
            for j, d in enumerate(stored):
                assert valid[i, j] == (len(q) > 0 and len(d) > 0)
                if not valid[i, j]:
                    assert scores[i, j] == np.float32(NEG_MAX)
                    continue
                want, bound = maxsim_expected(q, d, regime)
                if regime == "exact":
                    assert _bits32(scores[i, j]) == _bits32(want), (i, j)
                else:
                    assert abs(float(scores[i, j]) - want) <= 2.0 ** -23 * abs(want) + 1e-12     # one rounding to fp32


def _searched(scores, valid, b_q, b_s, k):
    return wc.rank_rows(scores[b_q], valid[b_q], wc.SCOPES, b_s, k)


@pytest.mark.parametrize("dim,fmt", wc.SETS)
def test_every_width_mutant_changes_pairs_and_search_results_at_every_width(dim, fmt):
    """What the GPU tests compare: the pair table (hipmaxsim over all documents) and, from it, the search rows of every
    (query, scope) at the largest k.  A row's groups are formed as the batch forms them: the queries of a scope in order."""
    b_q, b_s = wc.batch_of_every_query_under_every_scope()
    for regime in wc.REGIMES:
        stored = wc.stored_values(wc.doc_vectors(regime, dim), fmt)
        qv, qc = wc.query_block(wc.query_vectors(regime, dim), wc.Q_STRIDE, dim)
        order = np.arange(len(qc))
        right, valid = wc.score_table(qv, qc, order, stored, wc.tiles_of(dim))
        want = _searched(right, valid, b_q, b_s, 256)
        for m in wc.WIDTH_MUTANTS:
            if not wc.applies(m, dim, fmt):
                continue
            wrong, v2 = wc.score_table(qv, qc, order, stored, wc.tiles_of(dim), mutant=m)
            assert np.array_equal(valid, v2)
            moved = (_bits32(right) != _bits32(wrong)) & valid
            share = moved.sum() / valid.sum()
            print(f"{m} {regime} {dim} {fmt}: {share:.2f} of the valid pairs change")
            assert share >= (0.05 if m == "tile_reads_tile0" else 0.5), (m, regime, dim, fmt, share)
            got = _searched(wrong, v2, b_q, b_s, 256)
            assert got[0].tobytes() != want[0].tobytes(), (m, regime, dim, fmt)
            for k in (1, 10):                                                       # the small k see it too
                a, b = _searched(right, valid, b_q, b_s, k), _searched(wrong, v2, b_q, b_s, k)
                assert a[0].tobytes() != b[0].tobytes() or a[1].tobytes() != b[1].tobytes(), (m, regime, dim, fmt, k)


def test_second_line_mutant_is_the_format_itself_at_one_line():
    """The control: at 128-d, where the existing fp8 search tests run, the slip changes nothing."""
    stored = wc.stored_values(wc.doc_vectors("exact", 128), "fp8")
    qv, qc = wc.query_block(wc.query_vectors("exact", 128), wc.Q_STRIDE, 128)
    a = wc.score_table(qv, qc, np.arange(len(qc)), stored, 4)
    b = wc.score_table(qv, qc, np.arange(len(qc)), stored, 4, mutant="second_line_reads_first")
    assert a[0].tobytes() == b[0].tobytes()


def test_rank_rows_is_maxsim_search_reference():
    from hiprag import maxsim_search_reference
    from hiprag.index import pack_scopes
    stored = wc.stored_values(wc.doc_vectors("exact", 64), "bf16")
    qv, qc = wc.query_block(wc.query_vectors("exact", 64), wc.Q_STRIDE, 64)
    scores, valid = wc.score_table(qv, qc, np.arange(len(qc)), stored, 4)
    b_q, b_s = wc.batch_of_every_query_under_every_scope()
    ranges, offsets, soq = pack_scopes(wc.SCOPES, b_s, len(b_s))
    for k in wc.KS:
        want = maxsim_search_reference(scores[b_q], valid[b_q], ranges[:int(offsets[-1])], offsets, soq, k)
        got = _searched(scores, valid, b_q, b_s, k)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        if k == 256:                                                                # the copies tie and fall in id order
            for r in np.flatnonzero((b_s == 0) & (qc[b_q] > 0)):
                ids = got[1][r].tolist()
                for src, dst in wc.COPIES:
                    assert ids.index(src) < ids.index(dst) and got[0][r][ids.index(src)] == got[0][r][ids.index(dst)]


# ---- several items per workgroup ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", (2, 3, 6, 64, 96, 256, 304))
def test_the_many_items_case_fits_any_cu_count(cus):
    nq = wc.many_items_queries(cus)
    groups = -(-nq // wc.GROUP)
    assert nq >= 20 and groups >= 3 and nq % wc.GROUP and (4 * cus) % groups
    n_docs = wc.SLICE * (4 * cus + 300)
    scopes = [[(0, n_docs)], [(5, 40), (57, n_docs - 23)]]
    b_q, b_s = wc.batch_of_every_query_under_every_scope(nq, 2)
    counts = np.asarray([wc.MANY_COUNTS[i % len(wc.MANY_COUNTS)] for i in range(nq)])[b_q]
    items = wc.work_items(scopes, b_s)
    assert len(items) > 4 * cus and len(items) == groups * ((4 * cus + 300) + 3 + (n_docs - 23 - 1) // 16 - 57 // 16 + 1)
    assert wc.consecutive_items_differ(scopes, b_s, counts, cus)
    assert any(p_lo > 0 for _, _, _, p_lo, _, _ in items) and any(p_hi < 16 for _, _, _, _, p_hi, _ in items)


@pytest.mark.parametrize("cus,dim", [(2, 64), (5, 128)])
def test_stale_sums_change_the_many_items_result(cus, dim):
    lens, vecs, queries, scopes, b_q, b_s = wc.many_items_case(cus, dim)
    qc = np.asarray([len(q) for q in queries])
    assert int(lens.sum()) * 16 * dim < 2 ** 24 and set(np.unique(lens)) == {0, 1, 2, 3}
    sums = wc.sum_table(queries, lens, vecs)[b_q]
    right = wc.scores_of_sums(sums, qc[b_q], lens)
    stale = wc.scores_of_sums(wc.stale_sum_table(sums, qc[b_q], lens, scopes, b_s, cus), qc[b_q], lens)
    assert np.array_equal(right[1], stale[1])
    grid = wc.grid_of(len(wc.work_items(scopes, b_s)), cus)
    assert grid == 4 * cus
    first = wc.work_items(scopes, b_s)[:grid]                                       # a workgroup's first item is right either way
    for _, _, base, p_lo, p_hi, rows in first[:5]:
        assert np.array_equal(right[0][np.ix_(rows, range(base + p_lo, base + p_hi))], stale[0][np.ix_(rows, range(base + p_lo, base + p_hi))])
    for k in (1, 16, 256):
        a, b = wc.rank_rows(*right, scopes, b_s, k), wc.rank_rows(*stale, scopes, b_s, k)
        live = qc[b_q] > 0
        changed = (a[1] != b[1]).any(axis=1) | (_bits32(a[0]) != _bits32(b[0])).any(axis=1)
        print(f"stale_sums cus {cus} k {k}: {changed[live].mean():.2f} of the rows with a vector change")
        assert changed[live].mean() >= 0.5 and not changed[~live].any()
    # the sums table itself is the loop-free statement of maxsim_expected
    for i in (0, 3, 7):
        off = np.concatenate([[0], np.cumsum(lens)])
        for d in (int(np.flatnonzero(lens == 3)[0]), int(np.flatnonzero(lens == 1)[2])):
            want, _ = maxsim_expected(queries[i], vecs[off[d]:off[d + 1]], "exact")
            assert _bits32(right[0][i * 2, d]) == _bits32(want)


# ---- two chunks of queries ---------------------------------------------------------------------------------------------------------
def test_chunk_offsets_lost_change_the_two_chunk_result():
    lens, vecs, q, counts, soq = wc.two_chunk_case()
    o = wc.CHUNK_QUERIES
    assert len(counts) == o + 5 and np.all(counts[o:] != counts[:5]) and np.all(soq[o:] != soq[:5])
    assert set(np.unique(counts)) == {0, 1, 2} and set(np.unique(soq)) == {0, 1, 2}
    scores, valid = wc.two_chunk_scores(lens, vecs, q, counts)
    want = wc.rank_rows(scores, valid, wc.TWO_CHUNK_SCOPES, soq, 10)
    wrong_counts = wc.rank_rows(*wc.two_chunk_scores(lens, vecs, q, wc.chunk_lost(counts)), wc.TWO_CHUNK_SCOPES, soq, 10)
    wrong_scopes = wc.rank_rows(scores, valid, wc.TWO_CHUNK_SCOPES, wc.chunk_lost(soq), 10)
    wrong_queries = wc.rank_rows(*wc.two_chunk_scores(lens, vecs, wc.chunk_lost(q), counts), wc.TWO_CHUNK_SCOPES, soq, 10)
    for name, got in (("counts", wrong_counts), ("scopes", wrong_scopes), ("queries", wrong_queries)):
        assert got[0][:o].tobytes() == want[0][:o].tobytes() and got[1][:o].tobytes() == want[1][:o].tobytes(), name
        for i in range(o, o + 5):                                                   # EVERY query of chunk 2 shows it
            assert got[0][i].tobytes() != want[0][i].tobytes() or got[1][i].tobytes() != want[1][i].tobytes(), (name, i)
    # the vectorised expectation is the reference's on the first and last queries
    from hiprag import maxsim_search_reference
    from hiprag.index import pack_scopes
    ranges, offsets, soq32 = pack_scopes(wc.TWO_CHUNK_SCOPES, soq, len(soq))
    for sl in (slice(0, 32), slice(len(soq) - 32, len(soq))):
        ref = maxsim_search_reference(scores[sl], valid[sl], ranges, offsets, soq32[sl], 10)
        assert ref[0].tobytes() == want[0][sl].tobytes() and ref[1].tobytes() == want[1][sl].tobytes()
    for i in (1, o + 1):                                                            # and its scores are maxsim_expected's
        off = np.concatenate([[0], np.cumsum(lens)])
        d = int(np.flatnonzero(lens == 3)[0])
        w, _ = maxsim_expected(q[i, :counts[i]], vecs[off[d]:off[d + 1]], "exact")
        assert _bits32(scores[i, d]) == _bits32(w)


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,fmt", [(128, "bf16"), (1024, "bf16"), (256, "fp8")])
def test_unclamped_counts_change_the_count_case(dim, fmt):
    stored = wc.stored_values(wc.doc_vectors("exact", dim), fmt)
    qv, raw = wc.count_case(dim)
    by_hand = np.minimum(np.maximum(raw.astype(np.int64), 0), wc.COUNT_STRIDE)
    assert {int(c) for c in raw} >= {-3, 0, wc.COUNT_STRIDE + 5, 2 ** 31 - 1} and all(1 <= raw[i] <= wc.COUNT_STRIDE for i in wc.ORDINARY)
    assert np.array_equal(wc.clamped(raw, wc.COUNT_STRIDE), by_hand)
    order = np.arange(len(raw))
    tiles = wc.tiles_of(dim)
    right = wc.score_table(qv, raw, order, stored, tiles)
    hand = wc.score_table(qv, by_hand, order, stored, tiles)
    assert right[0].tobytes() == hand[0].tobytes() and np.array_equal(right[1], hand[1])
    for i in wc.ORDINARY:                                                           # an ordinary query's row is its row alone
        alone = wc.score_table(qv, raw, np.asarray([i]), stored, tiles)
        assert alone[0][0].tobytes() == right[0][i].tobytes()
    for m in wc.COUNT_MUTANTS:
        wrong = wc.score_table(qv, raw, order, stored, tiles, mutant=m)
        rows = [i for i in range(len(raw)) if wrong[0][i].tobytes() != right[0][i].tobytes() or not np.array_equal(wrong[1][i], right[1][i])]
        print(f"{m} {dim} {fmt}: rows {rows} change")
        # a count of -3 pulls the prefix back under the member behind it, an ORDINARY query: its first three rows become
        # the last three of the member in front.  A count above q_stride runs on into the next query's rows.  Members
        # further behind find their own rows again, since the same prefix says where a member's rows lie and whose they are.
        assert set(rows) == ({2} if m == "count_not_clamped_low" else {4, 6}), (m, rows)
        assert 2 in wc.ORDINARY and raw[1] < 0 and raw[4] > wc.COUNT_STRIDE and raw[6] > wc.COUNT_STRIDE


# ---- the quantiser ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (128,) + wc.FP8_WIDTHS)
def test_lane_sweep_catches_a_reduction_that_loses_any_lane(dim):
    bits = wc.lane_sweep_vectors(dim)
    n = dim // 16
    assert bits.shape == (n, dim)
    codes, scales = fc.quantize(bits)
    mag = (bits & 0x7FFF).astype(np.int64)
    assert np.array_equal(mag.argmax(axis=1), 16 * np.arange(n))
    for lane in range(n):                                                           # lane `lane` lost: another scale, other codes
        lost = bits[lane:lane + 1].copy()
        lost[0, 16 * lane:16 * lane + 16] = 0
        assert fc.quantize(lost)[1][0] <= scales[lane] / 8
    c128, s128 = fc.quantize(bits, "amax_first_128")
    if dim == 128:
        assert c128.tobytes() == codes.tobytes() and s128.tobytes() == scales.tobytes()      # a no-op where the old tests ran
    else:
        differ = np.flatnonzero(s128 != scales)
        assert np.array_equal(differ, np.arange(8, n))                              # every lane from 8 on
        assert np.all((c128 != codes).any(axis=1)[8:])
    c64, s64 = fc.quantize(bits, "amax_first_64")
    assert np.array_equal(np.flatnonzero(s64 != scales), np.arange(4, n))


def test_the_quantiser_mutants_are_caught_by_the_case_vectors_at_1024():
    cases = {"unit": fc.unit_vectors(16, 1024, 2), "int": fc.integer_vectors(8, 1024, 4), "special": fc.special_vectors(1024),
             "exhaustive": fc.exhaustive_vectors(1024), "lanes": wc.lane_sweep_vectors(1024)}
    ref = {name: fc.quantize(bits) for name, bits in cases.items()}
    from hiprag import fp8_quantize_reference
    for name, bits in cases.items():
        assert all(a.tobytes() == b.tobytes() for a, b in zip(fp8_quantize_reference(bits), ref[name])), name
    for m in fc.MUTANTS + fc.WIDE_MUTANTS:
        differs = [name for name, bits in cases.items() if any(a.tobytes() != b.tobytes() for a, b in zip(fc.quantize(bits, m), ref[name]))]
        print(f"mutant {m} at 1024-d: differs on {differs}")
        assert differs, m
    for m in ("truncate", "e_plus_one", "e_minus_one", "keep_neg_zero", "scale_is_2e"):
        assert any(a.tobytes() != b.tobytes() for a, b in zip(fc.quantize(cases["exhaustive"], m), ref["exhaustive"])), m
    for m in ("amax_first_64", "amax_first_128"):
        assert any(a.tobytes() != b.tobytes() for a, b in zip(fc.quantize(cases["lanes"], m), ref["lanes"])), m
