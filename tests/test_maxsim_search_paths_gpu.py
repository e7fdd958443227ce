"""
The paths of the late-interaction search (hipmaxsim_search_scoped*, maxsim_scope_kernel<Docs, T>) that no shape of
test_maxsim_search_gpu.py reaches, at the cases of tests/maxsim_width_cases.py:

  every instantiation   both formats at T = 4, 3 and 2 (pass_rows 128, 96, 64), with one chunk, odd chunk counts and two to
                        eight fp8 lines per row, a first group that packs 137 rows (two passes at T = 4, a query across a pass)
  several items         more work items than the grid of 4 x CUs workgroups: the item loop, the re-zeroed sums, the re-used
                        member and document tables, a merge over more than 1000 slices
  two chunks            16389 queries: the offsets of the second chunk into the queries, counts, scopes and outputs
  counts                negative, zero, above q_stride and 2^31 - 1 inside one group; a 512-vector query at 1024-d (8 passes)

Expectations are float64 numpy throughout: hipmaxsim's pair table (held against maxsim_expected at the same width by
test_maxsim_widths_gpu.py) under maxsim_search_reference, or integer data, where a score is exact and is compared bit for bit.
"""
import numpy as np
import pytest

import maxsim_width_cases as wc
from colbert_cases import NEG_MAX, maxsim_expected, maxsim_vectors
from oracle.linear_cases import bf16_bits, bf16_values

pytestmark = pytest.mark.gpu


def _same(got, want):
    return got[1].tobytes() == want[1].tobytes() and got[0].view(np.uint32).tobytes() == want[0].view(np.uint32).tobytes()


def _assert_rows(got, want, tag):
    for row in range(len(want[1])):
        assert np.array_equal(got[1][row], want[1][row]), (tag, row, got[1][row][:12], want[1][row][:12])
        assert np.array_equal(got[0][row].view(np.uint32), want[0][row].view(np.uint32)), (tag, row, got[0][row][:6], want[0][row][:6])


# ---- 1. every instantiation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", wc.REGIMES)
@pytest.mark.parametrize("dim,fmt", wc.SETS)
def test_every_query_under_every_scope_at_every_width(gpu, dim, fmt, regime):
    from hiprag import maxsim_search, maxsim_search_reference
    from hiprag.index import pack_scopes
    s = wc.gpu_setup(regime, dim, fmt)
    b_q, b_s = wc.batch_of_every_query_under_every_scope()
    ranges, offsets, _ = pack_scopes(wc.SCOPES, b_s, len(b_s))
    qv, qc = s["qv"][b_q], s["qc"][b_q]
    for k in wc.KS:
        want = maxsim_search_reference(s["pairs"][b_q], s["valid"][b_q], ranges[:int(offsets[-1])], offsets, b_s, k)
        got = maxsim_search(s["store"], qv, qc, wc.SCOPES, b_s, k)
        _assert_rows(got, want, (regime, dim, fmt, k))
        for r in range(len(b_q)):
            if b_s[r] in wc.EMPTY_SCOPES or qc[r] == 0:                                # all padding
                assert np.all(got[1][r] == -1) and np.all(got[0][r] == np.float32(NEG_MAX))
        if k == 256 and regime == "exact":                                            # the copies tie and fall in id order
            for r in np.flatnonzero((b_s == 0) & (qc > 0)):
                ids = list(got[1][r])
                for src, dst in wc.COPIES:
                    assert ids.index(src) < ids.index(dst) and got[0][r][ids.index(src)] == got[0][r][ids.index(dst)]
    info = s["store"].search_info()
    T = wc.tiles_of(dim)
    assert info["pass_rows"] == 32 * T and info["group_queries"] == wc.GROUP and info["slice_docs"] == wc.SLICE and info["chunks"] == 1
    # what the last call read: every group of a scope reads the scope's vectors once per pass
    reads = 0
    for sc, scope in enumerate(wc.SCOPES):
        rows = np.flatnonzero(b_s == sc)
        stored = sum(int(s["lens"][lo:hi].sum()) for lo, hi in scope)
        for g0 in range(0, len(rows), wc.GROUP):
            reads += -(-int(qc[rows[g0:g0 + wc.GROUP]].sum()) // (32 * T)) * stored
    assert info["doc_vectors_read"] == reads, (info, reads)
    assert info["work_items"] == len(wc.work_items(wc.SCOPES, b_s))
    assert -(-int(qc[np.flatnonzero(b_s == 0)[:wc.GROUP]].sum()) // (32 * T)) == {4: 2, 3: 2, 2: 3}[T]      # the first group's passes


def test_the_widths_run_all_three_tile_counts_in_both_formats(gpu):
    for fmt, widths in (("bf16", wc.BF16_WIDTHS), ("fp8", wc.FP8_WIDTHS)):
        seen = {wc.gpu_setup("exact", d, fmt)["store"].search_info()["pass_rows"] for d in widths}
        assert seen == {64, 96, 128}, (fmt, seen)


# ---- 2. a workgroup takes several items ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,fmt", [(64, "bf16"), (128, "fp8")])
def test_more_work_items_than_workgroups(gpu, dim, fmt):
    import torch
    from hiprag import MultiVectorStore, maxsim_search
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lens, vecs, queries, scopes, b_q, b_s = wc.many_items_case(cus, dim)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    store = MultiVectorStore(dim, max_doc_vectors=4, format=fmt)
    store.append(bf16_bits(vecs), off)                                                # the bulk form; integers are lossless in fp8
    assert store.sizes()[:2] == (len(lens), int(lens.sum()))
    q_stride = max(wc.MANY_COUNTS)
    qv, qc = wc.query_block(queries, q_stride, dim)
    # the host-side statement of what this case is for
    items = wc.work_items(scopes, b_s)
    assert len(items) > 4 * cus and wc.grid_of(len(items), cus) == 4 * cus
    assert -(-len(queries) // wc.GROUP) >= 3
    assert wc.consecutive_items_differ(scopes, b_s, qc[b_q], cus)
    scores, valid = wc.scores_of_sums(wc.sum_table(queries, lens, vecs), qc, lens)   # one matmul per query, exact
    T = wc.tiles_of(dim)
    for k in (1, 16, 256):
        want = wc.rank_rows(scores[b_q], valid[b_q], scopes, b_s, k)
        got = maxsim_search(store, qv[b_q], qc[b_q], scopes, b_s, k)
        _assert_rows(got, want, (dim, fmt, k))
        info = store.search_info()
        assert info["work_items"] == len(items) > 4 * cus and info["chunks"] == 1
        reads = 0
        for sc, scope in enumerate(scopes):
            rows = np.flatnonzero(b_s == sc)
            stored = sum(int(lens[lo:hi].sum()) for lo, hi in scope)
            for g0 in range(0, len(rows), wc.GROUP):
                reads += -(-int(qc[b_q][rows[g0:g0 + wc.GROUP]].sum()) // (32 * T)) * stored
        assert info["doc_vectors_read"] == reads
        n_valid = sum(int((qc[b_q][b_s == sc] > 0).sum()) * sum(int((lens[lo:hi] > 0).sum()) for lo, hi in scope) for sc, scope in enumerate(scopes))
        assert info["valid_pairs"] == n_valid
    # ties across more than 1000 slices fall in id order: integer scores of short documents repeat many times
    full = np.flatnonzero((b_s == 0) & (b_q == 1))[0]                                 # a one-vector query: its scores are integers
    sc, ids = got[0][full], got[1][full]
    assert (np.diff(sc) == 0).sum() > 50 and np.all((np.diff(sc) < 0) | (np.diff(ids) > 0))
    assert (ids.max() - ids.min()) // wc.SLICE > 1000


# ---- 3. two chunks of queries ----------------------------------------------------------------------------------------------------
def test_two_chunks_of_queries(gpu):
    import torch
    from hiprag import MultiVectorStore, maxsim_search, maxsim_search_device, maxsim_search_reference
    from hiprag.index import pack_scopes
    dim, k = 64, 10
    lens, vecs, q, counts, soq = wc.two_chunk_case(dim)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    store = MultiVectorStore(dim, max_doc_vectors=4)
    store.append(bf16_bits(vecs), off)
    qv = bf16_bits(q)
    qv[counts == 0] = 0x7FC5                                                         # poison behind every count
    qv[counts == 1, 1] = 0x7FC5
    scores, valid = wc.two_chunk_scores(lens, vecs, q, counts)
    want = wc.rank_rows(scores, valid, wc.TWO_CHUNK_SCOPES, soq, k)
    ranges, offsets, soq32 = pack_scopes(wc.TWO_CHUNK_SCOPES, soq, len(soq))
    for sl in (slice(0, 32), slice(len(soq) - 32, len(soq))):                        # the vectorised expectation is the reference's
        ref = maxsim_search_reference(scores[sl], valid[sl], ranges, offsets, soq32[sl], k)
        assert _same((want[0][sl], want[1][sl]), ref)
    got = maxsim_search(store, qv, counts, wc.TWO_CHUNK_SCOPES, soq, k)            # the host entry
    info = store.search_info()
    assert info["chunks"] == 2, info
    o = wc.CHUNK_QUERIES
    assert _same((got[0][:o], got[1][:o]), (want[0][:o], want[1][:o])), "the first chunk"
    _assert_rows((got[0][o:], got[1][o:]), (want[0][o:], want[1][o:]), "the second chunk")
    assert np.any(want[1][o:] >= 0)
    dq = torch.from_numpy(qv.view(np.int16)).cuda().view(torch.bfloat16)              # the device entry
    ds, di = maxsim_search_device(store, dq, torch.from_numpy(counts).cuda(), wc.TWO_CHUNK_SCOPES, soq, k)
    torch.cuda.synchronize()
    assert _same((ds.cpu().numpy(), di.cpu().numpy()), want)
    assert store.search_info()["chunks"] == 2


# ---- 4. counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,fmt", [(128, "bf16"), (1024, "bf16"), (256, "fp8")])
def test_counts_are_clamped_inside_a_group(gpu, dim, fmt):
    from hiprag import maxsim_search
    s = wc.gpu_setup("exact", dim, fmt) if (dim, fmt) in wc.SETS else None
    if s is None:
        from hiprag import MultiVectorStore
        docs = wc.doc_vectors("exact", dim)
        store = MultiVectorStore(dim, max_doc_vectors=wc.CAP, format=fmt)
        store.append([bf16_bits(d) for d in docs])
    else:
        store, docs = s["store"], s["docs"]
    qv, raw = wc.count_case(dim)
    by_hand = np.minimum(np.maximum(raw.astype(np.int64), 0), wc.COUNT_STRIDE).astype(np.int32)
    assert by_hand.tolist() == [7, 0, 33, 0, 40, 12, 40, 40]
    scope = [wc.SCOPES[2]]
    for k in (10, 256):
        got = maxsim_search(store, qv, raw, scope, None, k)
        hand = maxsim_search(store, qv, by_hand, scope, None, k)
        _assert_rows(got, hand, (dim, fmt, k, "clamped by hand"))
        # and both are right: float64 over the stored integers, bit for bit
        scores, valid = wc.score_table(qv, by_hand, np.arange(len(raw)), wc.stored_values(docs, fmt), wc.tiles_of(dim))
        _assert_rows(got, wc.rank_rows(scores, valid, scope, np.zeros(len(raw), np.int32), k), (dim, fmt, k, "fp64"))
        for i in wc.ORDINARY:                                                         # an ordinary query's row is its row alone
            alone = maxsim_search(store, qv[i:i + 1], raw[i:i + 1], scope, None, k)
            assert _same(alone, (got[0][i:i + 1], got[1][i:i + 1])), (dim, fmt, k, i)
        for i in (1, 3):
            assert np.all(got[1][i] == -1) and np.all(got[0][i] == np.float32(NEG_MAX))


def test_a_query_of_512_vectors_at_1024_d_takes_eight_passes(gpu):
    from hiprag import maxsim_search
    dim = 1024
    s = wc.gpu_setup("exact", dim, "fp8")                                             # (for its documents)
    from hiprag import MultiVectorStore
    store = MultiVectorStore(dim, max_doc_vectors=wc.CAP)
    store.append([bf16_bits(d) for d in s["docs"]])
    q = maxsim_vectors("exact", wc.MAX_Q_STRIDE, dim, 991)
    qv = bf16_bits(q)[None]
    scope = [[(2, 37)]]
    got = maxsim_search(store, qv, [wc.MAX_Q_STRIDE], scope, None, 256)
    info = store.search_info()
    stored = int(s["lens"][2:37].sum())
    assert info["pass_rows"] == 64 and info["doc_vectors_read"] == 8 * stored, info
    scores = np.full((1, wc.N_DOCS), NEG_MAX, np.float32)
    for j, d in enumerate(s["docs"]):
        if len(d):
            scores[0, j] = np.float32(maxsim_expected(q, d, "exact")[0])
    want = wc.rank_rows(scores, s["lens"][None, :] > 0, scope, [0], 256)
    _assert_rows(got, want, "512 vectors")
    got_big = maxsim_search(store, qv, [2 ** 31 - 1], scope, None, 256)               # clamped to q_stride = 512
    assert _same(got_big, got)
