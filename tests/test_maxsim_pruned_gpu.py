"""
The pruned late-interaction search (hipmaxsim_search_pruned*, csrc/maxsim_codes.hip) against its contract in include/hiprag.h:
(a) every returned score is hipmaxsim's pair score; (b) with ncand >= the scope's documents the result is
hipmaxsim_search_scoped's, bit for bit; (c) the candidates are hipmaxsim_search_scoped(k = ncand) over a bf16 store whose
every vector is replaced by its centroid, bit for bit; (d) a query's rows do not depend on the call; (e) on all three formats.
Beside (c) the candidates are held against the float64 interaction reference with pruned_cases.check_candidates, the helper
test_maxsim_pruned_cpu.py shows to catch the usual wrong interactions.  Shapes: 128-d (one case at 1024-d), 64..256
centroids, 300 documents of 0..40 vectors: two slices of the interaction stage.  The other shapes -- documents of up to 511
vectors over three and five slices, q_stride 1 .. 512 with counts of -3 .. q_stride + 5, 32 .. 288 centroids, every width, stores
of 1, 128 and 129 vectors, integer data compared bit for bit with the float64 ranking -- are test_maxsim_pruned_shapes_gpu.py's
(data and model: pruned_shape_cases.py; its mutants: test_pruned_shape_cases_cpu.py).
"""
import functools

import numpy as np
import pytest

import pruned_cases as pc
from oracle.linear_cases import bf16_values

pytestmark = pytest.mark.gpu

N_DOCS, NCENT, CAP = 300, 128, 40
LENGTHS = (3, 0, 1, 5, 31, 32, 33, 40, 12, 20)                      # cycled; document 10 i + 1 holds no vector
COUNTS = (1, 31, 32, 33, 64, 65, 130, 0, 8)
Q_STRIDE = 136
FORMATS = ("bf16", "fp8", "mxfp4")


def _same(got, want):
    return got[1].tobytes() == want[1].tobytes() and got[0].view(np.uint32).tobytes() == want[0].view(np.uint32).tobytes()


@functools.lru_cache(maxsize=None)
def _setup(fmt, dim=128, n_docs=N_DOCS, ncent=NCENT):
    from hiprag import MultiVectorStore
    cent = pc.random_centroids(ncent, dim, 21)
    docs, _ = pc.clustered_docs(cent, [LENGTHS[i % 10] for i in range(n_docs)], 22)
    for i in range(10):
        docs[50 + i] = docs[i][::-1].copy()                         # the same multiset of codes: equal interaction scores
    if n_docs > 270:
        docs[270] = docs[4].copy()                                  # and one in the second slice
    store = MultiVectorStore(dim, max_doc_vectors=CAP, format=fmt)
    store.append(docs)
    store.attach_centroids(cent)
    rng = np.random.default_rng(23)
    qv = np.full((len(COUNTS), Q_STRIDE, dim), 0x7FC5, dtype=np.uint16)   # poison behind every count
    for i, n in enumerate(COUNTS):
        qv[i, :n] = pc.vectors_around(cent, rng.integers(0, ncent, size=n), rng, noise=0.5)
    qc = np.asarray(COUNTS, np.int32)
    # the bf16 store of contract (c): every vector replaced by its centroid
    off, _ = store.export()
    codes = store.codes()
    sub = MultiVectorStore(dim, max_doc_vectors=CAP)
    sub.append(cent[codes], off)
    lens = np.diff(off)
    return dict(store=store, sub=sub, cent=cent, docs=docs, qv=qv, qc=qc, off=off, codes=codes, lens=lens)


def _batch(s, scopes):
    """every query under every scope"""
    nq, ns = len(s["qc"]), len(scopes)
    b_q, b_s = np.repeat(np.arange(nq), ns), np.tile(np.arange(ns), nq).astype(np.int32)
    return s["qv"][b_q], s["qc"][b_q], b_q, b_s


SMALL_SCOPES = ([(0, 16)], [(3, 3)], [(10, 20), (40, 45), (250, 262)], [(1, 2), (11, 12)], [(284, 300)])   # the 2nd: empty; the 4th: no vectors


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("k,ncand,id_base", [(5, 32, 0), (32, 32, 1000), (1, 27, 7)])
def test_b_with_enough_candidates_the_result_is_the_exact_search(gpu, fmt, k, ncand, id_base):
    from hiprag import maxsim_search, maxsim_search_pruned
    s = _setup(fmt)
    qv, qc, b_q, b_s = _batch(s, SMALL_SCOPES)
    want = maxsim_search(s["store"], qv, qc, SMALL_SCOPES, b_s, k, id_base=id_base)
    got = maxsim_search_pruned(s["store"], qv, qc, SMALL_SCOPES, b_s, k, ncand, id_base=id_base)
    assert _same(got, want)
    assert np.all(got[1][s["qc"][b_q] == 0] == -1) and np.all(got[1][(b_s == 1) | (b_s == 3)] == -1)
    assert np.any(got[1][:, 0] >= id_base)
    info = s["store"].pruned_info()
    assert info["slice_docs"] == 256 and info["chunks"] == 1 and info["exact_pairs"] > 0 and info["valid_pairs"] > 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_b_a_whole_slice_of_documents_at_256_candidates(gpu, fmt):
    from hiprag import maxsim_search, maxsim_search_pruned
    s = _setup(fmt)
    scopes = ([(0, 256)], [(30, 300)])                               # 256 and 270 documents, of which 243 hold a vector
    qv, qc, _, b_s = _batch(s, scopes)
    assert _same(maxsim_search_pruned(s["store"], qv, qc, scopes, b_s, 10, 256), maxsim_search(s["store"], qv, qc, scopes, b_s, 10))


SLICE_SCOPES = ([(0, 256)], [(0, 255)], [(0, 257)], [(1, 257)], [(200, 300)], [(0, 3), (254, 258), (290, 300)])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("ncand", [1, 16, 256])
def test_c_candidates_are_the_exact_search_over_the_centroid_store(gpu, fmt, ncand):
    from hiprag import maxsim_search, maxsim_search_pruned
    from hiprag.colbert import centroid_interaction_reference
    s = _setup(fmt)
    qv, qc, b_q, b_s = _batch(s, SLICE_SCOPES)
    k = min(ncand, 4)
    scores, ids, cids, csc = maxsim_search_pruned(s["store"], qv, qc, SLICE_SCOPES, b_s, k, ncand, id_base=50, want_candidates=True)
    want = maxsim_search(s["sub"], qv, qc, SLICE_SCOPES, b_s, ncand, id_base=50)
    assert _same((csc, cids), want)
    # the copies tie and come in id order
    full = [r for r in range(len(b_q)) if b_s[r] == 0 and qc[r] > 0]
    if ncand == 256:
        for r in full:
            pos = {int(d) - 50: p for p, d in enumerate(cids[r]) if d >= 0}
            for i in (0, 3, 4, 7):
                assert csc[r][pos[i]] == csc[r][pos[50 + i]] and pos[i] < pos[50 + i]
    # and against the float64 definition
    c = bf16_values(s["cent"]).astype(np.float64)
    codes_of = [s["codes"][s["off"][d]:s["off"][d + 1]] for d in range(N_DOCS)]
    tol = pc.product_tolerance(128)
    for qi in range(len(COUNTS)):
        ref = centroid_interaction_reference(bf16_values(s["qv"][qi, :COUNTS[qi]]), codes_of, c)
        for r in np.nonzero(b_q == qi)[0]:
            in_scope = [d for lo, hi in SLICE_SCOPES[b_s[r]] for d in range(lo, hi)] if COUNTS[qi] else []
            verdict = pc.check_candidates(cids[r], csc[r], ref, in_scope, ncand, tol, id_base=50)
            assert verdict is None, (qi, SLICE_SCOPES[b_s[r]], verdict)
    # (a): the exact stage ranks the candidates, and its scores are hipmaxsim's
    _assert_scores_are_maxsims(s["store"], qv, qc, scores, ids, 50)
    for r in range(len(b_q)):
        assert set(ids[r][ids[r] >= 0].tolist()) <= set(cids[r].tolist())


def _assert_scores_are_maxsims(store, qv, qc, scores, ids, id_base):
    from hiprag import maxsim
    cand = ids.copy()
    pairs = maxsim(store, qv, qc, cand, k=1, id_base=id_base)[3]
    assert np.array_equal(pairs.view(np.uint32), scores.view(np.uint32))
    assert np.all(scores[ids < 0] == np.float32(pc.NEG_MAX))
    for r in range(len(ids)):                                       # (score descending, id ascending)
        n = int((ids[r] >= 0).sum())
        assert np.all(ids[r][n:] == -1)
        for p in range(1, n):
            assert scores[r][p] < scores[r][p - 1] or (scores[r][p] == scores[r][p - 1] and ids[r][p] > ids[r][p - 1])


@pytest.mark.parametrize("fmt", ["bf16", "mxfp4"])
def test_a_scores_of_a_truly_pruned_search_are_maxsims(gpu, fmt):
    from hiprag import maxsim_search_pruned
    s = _setup(fmt)
    scopes = ([(0, 300)], [(20, 290)])
    qv, qc, _, b_s = _batch(s, scopes)
    scores, ids = maxsim_search_pruned(s["store"], qv, qc, scopes, b_s, 10, 16)
    _assert_scores_are_maxsims(s["store"], qv, qc, scores, ids, 0)
    assert np.all((ids[qc > 0] >= 0).sum(axis=1) == 10)


def test_b_and_c_at_1024_dimensions(gpu):
    from hiprag import maxsim_search, maxsim_search_pruned
    s = _setup("bf16", dim=1024, n_docs=60, ncent=64)
    scopes = ([(0, 60)], [(5, 33)])
    qv, qc, _, b_s = _batch(s, scopes)
    got = maxsim_search_pruned(s["store"], qv, qc, scopes, b_s, 10, 64, want_candidates=True)
    assert _same(got[:2], maxsim_search(s["store"], qv, qc, scopes, b_s, 10))
    assert _same((got[3], got[2]), maxsim_search(s["sub"], qv, qc, scopes, b_s, 64))


def test_d_rows_do_not_depend_on_the_call_or_on_its_chunks(gpu, monkeypatch):
    from hiprag import maxsim_search_pruned
    s = _setup("bf16")
    scopes = ([(0, 300)], [(3, 3)], [(10, 20), (40, 45), (250, 262)], [(100, 290)])
    nq = 70
    b_q = np.arange(nq) % len(COUNTS)
    b_s = ((np.arange(nq) * 7) % len(scopes)).astype(np.int32)
    qv, qc = s["qv"][b_q], s["qc"][b_q]
    whole = maxsim_search_pruned(s["store"], qv, qc, scopes, b_s, 5, 16, want_candidates=True)
    assert s["store"].pruned_info()["chunks"] == 1
    for i in range(nq):
        one = maxsim_search_pruned(s["store"], qv[i:i + 1], qc[i:i + 1], [scopes[b_s[i]]], [0], 5, 16, want_candidates=True)
        assert all(a[i].tobytes() == b[0].tobytes() for a, b in zip(whole, one)), i
    # a budget of 64 KiB: a query's table alone is 128 x 160 x 4 = 80 KiB, so every query is a chunk of its own
    monkeypatch.setenv("HIPRAG_PRUNED_BUDGET", str(64 << 10))
    cut = maxsim_search_pruned(s["store"], qv, qc, scopes, b_s, 5, 16, want_candidates=True)
    assert s["store"].pruned_info()["chunks"] == nq
    monkeypatch.setenv("HIPRAG_PRUNED_BUDGET", str(1 << 20))        # and chunks of several queries
    cut2 = maxsim_search_pruned(s["store"], qv, qc, scopes, b_s, 5, 16, want_candidates=True)
    assert 1 < s["store"].pruned_info()["chunks"] < nq
    monkeypatch.delenv("HIPRAG_PRUNED_BUDGET")
    for other in (cut, cut2):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, other))


def test_d_the_device_entry_gives_the_host_entry_s_bytes(gpu):
    import torch
    from hiprag import maxsim_search_pruned, maxsim_search_pruned_device
    s = _setup("fp8")
    qv, qc, _, b_s = _batch(s, SLICE_SCOPES)
    want = maxsim_search_pruned(s["store"], qv, qc, SLICE_SCOPES, b_s, 5, 16, want_candidates=True)
    tq = torch.from_numpy(qv.view(np.int16)).cuda().view(torch.bfloat16)
    got = maxsim_search_pruned_device(s["store"], tq, torch.from_numpy(qc).cuda(), SLICE_SCOPES, b_s, 5, 16, want_candidates=True)
    torch.cuda.synchronize()
    assert all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip(got, want))
    two = maxsim_search_pruned_device(s["store"], tq, torch.from_numpy(qc).cuda(), SLICE_SCOPES, b_s, 5, 16)
    torch.cuda.synchronize()
    assert len(two) == 2 and all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip(two, want[:2]))


@pytest.mark.parametrize("seed", range(5))
def test_every_planted_document_comes_first_at_16_candidates(gpu, seed):
    """A condition, not a measurement: test_maxsim_pruned_cpu.py shows the planted document is rank 0 by float64 centroid
    interaction, >= 0.46 above rank 16, and the exact top 1 by > 1e-2 -- margins thousands of times the fp32 error -- so the
    share of misses allowed is 0."""
    from hiprag import MultiVectorStore, maxsim_search_pruned
    cent, docs, q, targets = pc.planted(seed)
    store = MultiVectorStore(pc.PLANT_DIM, max_doc_vectors=64)
    store.append(docs)
    store.attach_centroids(cent)                                    # the true centroids
    qc = np.full(len(q), pc.PLANT_LQ, np.int32)
    scores, ids, cids, _ = maxsim_search_pruned(store, q, qc, [[(0, len(docs))]], np.zeros(len(q), np.int32), 1, pc.PLANT_NCAND,
                                                want_candidates=True)
    assert ids[:, 0].tolist() == targets.tolist()
    assert cids[:, 0].tolist() == targets.tolist()
    assert store.pruned_info()["exact_pairs"] == len(q) * pc.PLANT_NCAND     # 16 of 400 documents reached the exact kernel


def test_refused_calls_leave_the_outputs_untouched(gpu):
    from hiprag import HipRagError, MultiVectorStore
    from hiprag import _native as nat
    from hiprag.index import pack_scopes
    s = _setup("bf16")
    qv, qc = np.ascontiguousarray(s["qv"][:2]), np.ascontiguousarray(s["qc"][:2])
    ranges, offsets, soq = pack_scopes([[(0, 300)]], [0, 0], 2)

    def call(store, k, ncand, ranges=ranges, q_stride=Q_STRIDE):
        scores, ids = np.full((2, 300), 7.0, np.float32), np.full((2, 300), 7, np.int64)
        cids, csc = np.full((2, 300), 7, np.int64), np.full((2, 300), 7.0, np.float32)
        with pytest.raises(HipRagError) as e:
            nat.call("hipmaxsim_search_pruned", store._h, qv.ctypes.data, qc.ctypes.data, q_stride, 2, k, ncand, ranges.ctypes.data,
                     offsets.ctypes.data, 1, soq.ctypes.data, 0, scores.ctypes.data, ids.ctypes.data, cids.ctypes.data, csc.ctypes.data)
        assert np.all(scores == 7.0) and np.all(ids == 7) and np.all(cids == 7) and np.all(csc == 7.0)
        return e.value

    assert call(s["store"], 17, 16).code == -1                      # k > ncand
    assert call(s["store"], 5, 257).code == -1                      # ncand > 256
    assert call(s["store"], 0, 16).code == -1
    assert call(s["store"], 5, 16, q_stride=513).code == -1
    assert call(s["store"], 5, 16, ranges=np.asarray([[0, 301]], np.int64)).code == -1    # the scoped entry's checks
    bare = MultiVectorStore(128, max_doc_vectors=CAP)
    bare.append(s["docs"])
    e = call(bare, 5, 16)
    assert e.code == -6 and "hipmv_attach_centroids" in str(e)
