"""
The centroid codes and the pruned late-interaction search (csrc/maxsim_codes.hip) at the shapes test_maxsim_pruned_gpu.py and
test_multivec_codes_gpu.py do not reach (tests/pruned_shape_cases.py holds the data; test_pruned_shape_cases_cpu.py shows that
every comparison made here fails on a model of the stage with a one-line slip):
  a  set L: 600 documents of up to 511 vectors (several trips over a document's codes, 64 codes exactly, odd last chunks,
     three and five slices in the merge), every q_stride of 1 .. 512, counts of -3 .. q_stride + 5;
  b  scopes that end on, before and behind the slice boundaries 256 and 512, and the work items they make;
  c  the query table at 32, 96, 160 and 288 centroids;
  d  the codes and one search at every width of maxsim_width_cases;
  e  stores of 1, 128 and 129 vectors, equal centroids on ONE lane of the codes kernel, natural ties of integer data;
  f  hiprag.train_token_centroids.
In the EXACT regime (integers in [-1, 1], bf16 and mxfp4 stores) candidates and codes are compared with the float64 definition
bit for bit, ties included; in the RANDOM regime with pruned_cases.check_candidates at product_tolerance(dim), and the codes
after the measured top-2 gap of the stored values has been required to be 100 times that bound.  The contract of
include/hiprag.h is asserted beside it as in test_maxsim_pruned_gpu.py: (a) scores are hipmaxsim's, (b) enough candidates give
the exact search, (c) the candidates are the exact search over the centroid-substituted bf16 store.
"""
import functools

import numpy as np
import pytest

import maxsim_width_cases as wc
import pruned_cases as pc
import pruned_shape_cases as ps
from oracle.linear_cases import bf16_values

pytestmark = pytest.mark.gpu

ID_BASE = 50
FORMAT_REGIMES = [("bf16", "exact"), ("bf16", "random"), ("mxfp4", "exact"), ("mxfp4", "random"), ("fp8", "random")]
NEG = np.float32(pc.NEG_MAX)


def _same(got, want):
    return got[1].tobytes() == want[1].tobytes() and got[0].view(np.uint32).tobytes() == want[0].view(np.uint32).tobytes()


def _new_store(dim, fmt, docs, cent):
    from hiprag import MultiVectorStore
    store = MultiVectorStore(dim, max_doc_vectors=ps.CAP, format=fmt)
    store.append(docs)
    store.attach_centroids(cent)
    return store


def _stored_values(store):
    return store.gather_f32(np.arange(store.sizes()[1], dtype=np.int64)).cpu().numpy()


def _assert_codes_are_the_argmax(store, cent, dim, regime):
    """exact regime: every product is an integer, the codes ARE the float64 argmax, ties to the lowest index.  random regime:
    the measured-gap assertion of test_multivec_codes_gpu.py (a copy of centroid 5 is no second centroid)."""
    from hiprag.colbert import centroid_codes_reference
    vals, c = _stored_values(store), bf16_values(cent)
    if regime == "random":
        keep = [i for i in range(len(cent)) if i not in ps.copies(len(cent))]
        gap = pc.top2_margin(vals, c[keep])
        print(f"top-2 gap of the stored values: {gap:.4f}; accumulation bound {pc.product_tolerance(dim):.2e}")
        assert gap > 100 * pc.product_tolerance(dim)
    codes = store.codes()
    assert codes.dtype == np.int32 and len(codes) == len(vals)
    want = centroid_codes_reference(vals, c)
    assert np.array_equal(codes, want), np.flatnonzero(codes != want)[:8]
    return codes


@functools.lru_cache(maxsize=None)
def _setup(which, fmt, regime, ncent=ps.NCENT):
    """the store of set L or T, and the bf16 store of contract (c): every vector replaced by its centroid"""
    from hiprag import MultiVectorStore
    cent, docs, _ = ps.documents(which, regime, ps.DIM, ncent)
    store = _new_store(ps.DIM, fmt, docs, cent)
    off, _ = store.export()
    codes = store.codes()
    sub = MultiVectorStore(ps.DIM, max_doc_vectors=ps.CAP)
    sub.append(cent[codes], off)
    return dict(store=store, sub=sub, cent=cent, docs=docs, off=off, codes=codes, lens=np.diff(off))


@functools.lru_cache(maxsize=None)
def _reference(which, fmt, regime, ncent, q_stride):
    """float64 [queries, documents], computed once per store and stride and left unchanged"""
    s = _setup(which, fmt, regime, ncent)
    qv, qc = ps.queries(regime, q_stride, ps.DIM, ncent)
    ref = ps.reference_scores(qv, qc, s["codes"], s["off"], s["cent"])
    ref.setflags(write=False)
    return ref


def _assert_scores_are_maxsims(store, qv, qc, scores, ids, id_base):
    from hiprag import maxsim
    pairs = maxsim(store, qv, qc, ids.copy(), k=1, id_base=id_base)[3]
    assert np.array_equal(pairs.view(np.uint32), scores.view(np.uint32))
    assert np.all(scores[ids < 0] == NEG)
    for r in range(len(ids)):                                       # (score descending, id ascending)
        n = int((ids[r] >= 0).sum())
        assert np.all(ids[r][n:] == -1)
        for p in range(1, n):
            assert scores[r][p] < scores[r][p - 1] or (scores[r][p] == scores[r][p - 1] and ids[r][p] > ids[r][p - 1])


def _check_search(which, fmt, regime, ncent, q_stride, scopes, ncand):
    """every query of the stride under every scope: the float64 definition, contracts (c), (a), (b), the counts"""
    from hiprag import maxsim_search, maxsim_search_pruned
    s = _setup(which, fmt, regime, ncent)
    qv, qc = ps.queries(regime, q_stride, ps.DIM, ncent)
    ref = _reference(which, fmt, regime, ncent, q_stride)
    b_q, b_s = ps.batch(len(qc), len(scopes))
    bv, bc = qv[b_q], qc[b_q]
    k = min(ncand, 4)
    scores, ids, cids, csc = maxsim_search_pruned(s["store"], bv, bc, scopes, b_s, k, ncand, id_base=ID_BASE, want_candidates=True)
    assert s["store"].pruned_info()["work_items"] == ps.expected_items(scopes, b_s)
    # the float64 definition: bit for bit on integers, within the accumulation bound on unit vectors
    for r in range(len(b_q)):
        n = ps.clamp(qc[b_q[r]], q_stride)
        v = ps.verdict(regime, cids[r], csc[r], ref[b_q[r]], n, scopes[b_s[r]], ncand, ps.DIM, id_base=ID_BASE)
        assert v is None, (int(qc[b_q[r]]), scopes[b_s[r]], v)
    # (c): the exact search over the centroid-substituted store
    assert _same((csc, cids), maxsim_search(s["sub"], bv, bc, scopes, b_s, ncand, id_base=ID_BASE))
    # (a): the exact stage ranks the candidates, and its scores are hipmaxsim's
    _assert_scores_are_maxsims(s["store"], bv, bc, scores, ids, ID_BASE)
    for r in range(len(b_q)):
        assert set(ids[r][ids[r] >= 0].tolist()) <= set(cids[r].tolist())
    # (b): where every document of the scope with a vector is a candidate, the result is the exact search's
    exact = maxsim_search(s["store"], bv, bc, scopes, b_s, k, id_base=ID_BASE)
    full = [i for i, sc in enumerate(scopes) if ncand >= sum(1 for d in ps.scope_docs(sc) if s["lens"][d] > 0)]
    for r in np.flatnonzero(np.isin(b_s, full)):
        assert scores[r].tobytes() == exact[0][r].tobytes() and ids[r].tobytes() == exact[1][r].tobytes(), (int(bc[r]), scopes[b_s[r]])
    # counts <= 0: padding only
    none = bc <= 0
    assert none.sum() == 2 * len(scopes)
    assert np.all(ids[none] == -1) and np.all(cids[none] == -1) and np.all(scores[none] == NEG) and np.all(csc[none] == NEG)
    assert np.any(cids[~none] >= ID_BASE)
    # a count above q_stride: the rows of the same vectors under the count q_stride
    over = np.flatnonzero(bc > q_stride)
    assert len(over) == len(scopes)
    twin = maxsim_search_pruned(s["store"], bv[over], np.full(len(over), q_stride, np.int32), scopes, b_s[over], k, ncand, id_base=ID_BASE,
                                want_candidates=True)
    for got, want in zip((scores, ids, cids, csc), twin):
        assert got[over].tobytes() == want.tobytes()
    return cids, csc, b_q, b_s


# ---- a: long documents, every stride ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,regime", FORMAT_REGIMES)
def test_a_codes_of_set_l_are_the_float64_argmax(gpu, fmt, regime):
    s = _setup("L", fmt, regime)
    codes = _assert_codes_are_the_argmax(s["store"], s["cent"], ps.DIM, regime)
    assert not np.isin(codes, ps.COPIES_OF_5).any() and 5 in codes.tolist()     # the copies on centroid 5's lane never win
    assert s["store"].sizes()[3] == ps.CAP and len(s["lens"]) == ps.N_DOCS


@pytest.mark.parametrize("fmt,regime", FORMAT_REGIMES)
@pytest.mark.parametrize("q_stride", ps.STRIDES)
@pytest.mark.parametrize("ncand", ps.NCANDS)
def test_a_long_documents_at_every_stride(gpu, fmt, regime, q_stride, ncand):
    cids, csc, b_q, b_s = _check_search("L", fmt, regime, ps.NCENT, q_stride, ps.SCOPES_L, ncand)
    if ncand == 256:                                                # the reversed copies tie and come in id order
        for r in np.flatnonzero((b_s == 0) & (ps.raw_counts(q_stride)[b_q] > 0)):
            pos = {int(d) - ID_BASE: p for p, d in enumerate(cids[r]) if d >= 0}
            for src, dst in ps.PAIRS:
                if src in pos and dst in pos:
                    assert csc[r][pos[src]] == csc[r][pos[dst]] and pos[src] < pos[dst]


# ---- b: slice edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncand", ps.EDGE_NCANDS)
def test_b_scopes_on_before_and_behind_the_slice_boundaries(gpu, ncand):
    from hiprag import maxsim_search_pruned
    q_stride = 33
    s = _setup("L", "bf16", "exact")
    qv, qc = ps.queries("exact", q_stride)
    ref = _reference("L", "bf16", "exact", ps.NCENT, q_stride)
    scopes = ps.EDGE_SCOPES
    b_q, b_s = ps.batch(len(qc), len(scopes))
    _, _, cids, csc = maxsim_search_pruned(s["store"], qv[b_q], qc[b_q], scopes, b_s, 1, ncand, want_candidates=True)
    info = s["store"].pruned_info()
    assert info["slice_docs"] == ps.SLICE and info["chunks"] == 1
    assert info["work_items"] == ps.expected_items(scopes, b_s) == 2 * (1 + 1 + 2 + 3 + 1 + 3 + 2)
    for r in range(len(b_q)):
        want = ps.expected_candidates(ref[b_q[r]], ps.clamp(qc[b_q[r]], q_stride), scopes[b_s[r]], ncand)
        assert ps.same_candidates(cids[r], csc[r], *want), (int(qc[b_q[r]]), scopes[b_s[r]])


# ---- c: table shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncent", ps.TABLE_NCENTS)
@pytest.mark.parametrize("regime", ps.REGIMES)
def test_c_codes_at_every_table_shape(gpu, ncent, regime):
    s = _setup("T", "bf16", regime, ncent)
    codes = _assert_codes_are_the_argmax(s["store"], s["cent"], ps.DIM, regime)
    assert not np.isin(codes, ps.copies(ncent)).any() and codes.max() < ncent


@pytest.mark.parametrize("ncent", ps.TABLE_NCENTS)
@pytest.mark.parametrize("regime", ps.REGIMES)
@pytest.mark.parametrize("q_stride", ps.TABLE_STRIDES)
@pytest.mark.parametrize("ncand", [16, 256])
def test_c_the_query_table_at_every_centroid_count(gpu, ncent, regime, q_stride, ncand):
    _check_search("T", "bf16", regime, ncent, q_stride, ps.SCOPES_T, ncand)


# ---- d: widths --------------------------------------------------------------------------------------------------------------------
WIDTH_CASES = ([(d, "bf16", r) for d in wc.BF16_WIDTHS for r in ps.REGIMES] + [(d, "fp8", "random") for d in wc.FP8_WIDTHS]
               + [(d, "mxfp4", r) for d in wc.FP8_WIDTHS for r in ps.REGIMES])


@pytest.mark.parametrize("dim,fmt,regime", WIDTH_CASES)
def test_d_codes_and_a_search_at_every_width(gpu, dim, fmt, regime):
    from hiprag import MultiVectorStore, maxsim_search, maxsim_search_pruned
    cent, docs, _ = ps.width_documents(regime, dim)
    store = _new_store(dim, fmt, docs, cent)
    assert store.sizes()[:2] == (3, 129)
    codes = _assert_codes_are_the_argmax(store, cent, dim, regime)
    off, _ = store.export()
    qv, qc = ps.width_queries(regime, cent, dim)
    scopes, soq, ncand = [[(0, 3)]], np.zeros(2, np.int32), 3
    scores, ids, cids, csc = maxsim_search_pruned(store, qv, qc, scopes, soq, 3, ncand, want_candidates=True)
    ref = ps.reference_scores(qv, qc, codes, off, cent)
    for r in range(2):
        v = ps.verdict(regime, cids[r], csc[r], ref[r], int(qc[r]), scopes[0], ncand, dim)
        assert v is None, (r, v)
    sub = MultiVectorStore(dim, max_doc_vectors=ps.CAP)
    sub.append(cent[codes], off)
    assert _same((csc, cids), maxsim_search(sub, qv, qc, scopes, soq, ncand))
    assert _same((scores, ids), maxsim_search(store, qv, qc, scopes, soq, 3))      # three candidates of three documents: (b)


# ---- e: codes ------------------------------------------------------------------------------------------------------------------------
def _split(n):
    return {1: (1,), 128: (64, 64), 129: (1, 64, 64)}[n]


@pytest.mark.parametrize("stored", [1, 128, 129])
@pytest.mark.parametrize("fmt,regime", FORMAT_REGIMES)
def test_e_equal_centroids_on_one_lane_give_the_lowest(gpu, stored, fmt, regime):
    """Centroids 5, 37 and 69 hold the same bits: one lane of the codes kernel meets them in tile 0 and tile 1 of its first trip
    and in tile 0 of its second, and only a GREATER product may replace what it holds."""
    cent = ps.centroids(regime, ps.NCENT, ps.DIM, 41)
    rng = np.random.default_rng(42 + stored)
    around = ps.integers_around if regime == "exact" else pc.vectors_around
    docs = [around(cent, [5] * n, rng) for n in _split(stored)]
    store = _new_store(ps.DIM, fmt, docs, cent)
    vals = _stored_values(store).astype(np.float64) @ bf16_values(cent).astype(np.float64).T
    top = np.sort(vals, axis=1)
    assert np.all(top[:, -1] == top[:, -3]) and np.all(top[:, -3] - top[:, -4] > 100 * pc.product_tolerance(ps.DIM))
    codes = store.codes()
    assert len(codes) == stored and codes.tolist() == [5] * stored


@pytest.mark.parametrize("stored", [1, 128, 129])
@pytest.mark.parametrize("fmt", ["bf16", "mxfp4"])
@pytest.mark.parametrize("ncent", [96, 1024])
def test_e_natural_ties_of_integer_vectors_resolve_to_the_lowest_centroid(gpu, stored, fmt, ncent):
    cent = ps.centroids("exact", ncent, ps.DIM, 43)
    rng = np.random.default_rng(44 + stored)
    docs = [ps.integer_vectors(n, ps.DIM, rng) for n in _split(stored)]
    store = _new_store(ps.DIM, fmt, docs, cent)
    products = _stored_values(store).astype(np.float64) @ bf16_values(cent).astype(np.float64).T
    tied = int(((products == products.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    print(f"{tied} of {stored} vectors tie for their maximum over {ncent} centroids")
    assert stored == 1 or tied >= 5
    _assert_codes_are_the_argmax(store, cent, ps.DIM, "exact")


# ---- f: train_token_centroids -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clustered_store():
    true = pc.random_centroids(32, ps.DIM, 51)
    docs, _ = pc.clustered_docs(true, [30] * 40, 52)
    from hiprag import MultiVectorStore
    store = MultiVectorStore(ps.DIM, max_doc_vectors=ps.CAP)
    store.append(docs)
    return store


def test_f_trained_centroids_are_unit_bf16_rows_and_the_same_for_the_same_seed(gpu):
    from hiprag import train_token_centroids
    store = _clustered_store()
    table = train_token_centroids(store, 32, seed=3)
    assert table.dtype == np.uint16 and table.shape == (32, ps.DIM)
    norms = np.linalg.norm(bf16_values(table).astype(np.float64), axis=1)
    print(f"norms of the trained centroids: {norms.min():.5f} .. {norms.max():.5f}")
    assert np.all(np.abs(norms - 1.0) <= 2.0 ** -8)                 # every component rounds by at most 2^-9 of itself: one bf16 step of 1
    assert train_token_centroids(store, 32, seed=3).tobytes() == table.tobytes()
    assert store.centroid_info() == (0, 0, 0)                       # training attaches nothing


def test_f_ncent_zero_follows_the_default_rule_and_bad_counts_are_refused(gpu):
    from hiprag import MultiVectorStore, train_token_centroids
    from hiprag.colbert import default_ncent
    store = _clustered_store()
    nv = store.sizes()[1]
    assert nv == 1200 and default_ncent(nv) == 512                  # 16 sqrt(1200) = 554: the nearest power of two
    assert train_token_centroids(store, 0).shape == (512, ps.DIM)
    small = MultiVectorStore(ps.DIM, max_doc_vectors=ps.CAP)
    small.append([pc.random_centroids(100, ps.DIM, 53)])
    assert default_ncent(100) == 128                                # above the 100 stored vectors: cut to 64
    got = train_token_centroids(small, 0)
    assert got.shape[0] % 32 == 0 and got.shape == (64, ps.DIM)
    for bad in (33, 48, 16, 65536 + 32):
        with pytest.raises(ValueError):
            train_token_centroids(store, bad)
    with pytest.raises(ValueError):
        train_token_centroids(small, 128)                           # more centroids than stored vectors
    with pytest.raises(ValueError):
        train_token_centroids(store, 1216)


def test_f_trained_centroids_fit_clustered_data_better_than_random_ones(gpu):
    from hiprag import train_token_centroids
    store = _clustered_store()
    vals = _stored_values(store).astype(np.float64)

    def fit(table):
        store.attach_centroids(table)
        codes = store.codes()
        store.detach_centroids()
        return float(np.einsum("ij,ij->i", vals, bf16_values(table).astype(np.float64)[codes]).mean())

    trained, random = fit(train_token_centroids(store, 32)), fit(pc.random_centroids(32, ps.DIM, 54))
    print(f"mean product of a stored vector with its coded centroid: trained {trained:.4f}, random {random:.4f}")
    assert trained > random
