"""
Late interaction over an MXFP4 multi-vector store.  THE IDENTITY the format is defined for: hipmaxsim_dev's pair scores, orders
and counters, and hipmaxsim_search_scoped's scores and ids, equal byte for byte those over a bf16 store that holds the
dequantised vectors (export() of the MXFP4 store), at every width at which the search kernel takes another instance (128 and
384: four query tiles, 640: three, 1024: two), on integer data and on unit vectors, for document and query lengths around the
32-row tile, k below and above the entries a slice keeps, scopes that cut slices at both ends and more queries on a scope than
a work item takes.  RIGHTNESS: on integer data every product and sum is exact and the format is lossless, so the scores are
the float64 MaxSim of the dequantised vectors bit for bit; on unit vectors they lie within colbert_cases' accumulation bound
plus mxfp4_cases' quantisation term of the float64 MaxSim of the ORIGINAL vectors.  The search follows removals and appends;
hipm3_score_dev with only the ColBERT weight gives hipmaxsim_dev's bits.
"""
import functools

import numpy as np
import pytest

import mxfp4_cases as mc
from colbert_cases import NEG_MAX, drop_ranges, maxsim_expected, maxsim_vectors, score_ratio
from oracle.linear_cases import bf16_bits, bf16_values

pytestmark = pytest.mark.gpu

DIMS = (128, 384, 640, 1024)                                    # scope-kernel query tiles 4, 4, 3, 2
TILES = {128: 4, 384: 4, 640: 3, 1024: 2}
REGIMES = ("exact", "random")                                   # integers in [-4, 4] | unit vectors
N_DOCS = 40
LD = (1, 31, 32, 33, 65, 0)                                     # stored lengths, cycled; every sixth document is empty
LQ = (1, 32, 33, 33, 1, 32, 33, 1, 32, 33, 32)                  # 11 queries
Q_STRIDE = 33
CAP = 80
KS = (1, 5, 16, 17)                                             # a slice keeps min(k, 16) entries
SCOPES = ([(0, 40)], [(3, 37)], [(5, 9), (18, 35)])                # whole slices | cut at both ends | two ranges, all four ends cut
SOQ = (0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2)                         # nine queries on scope 0: two groups of a work item's 8
ID_BASE = 500


def _twin_of(store, cap=CAP):
    from hiprag import MultiVectorStore
    off, deq = store.export()
    twin = MultiVectorStore(store.dim, max_doc_vectors=cap)     # bf16, holding the dequantised vectors
    twin.append(deq, off)
    return twin, off, deq


@functools.lru_cache(maxsize=None)
def _setup(regime, dim):
    import torch
    from hiprag import MultiVectorStore
    docs = [maxsim_vectors(regime, LD[i % len(LD)], dim, 100 + i) for i in range(N_DOCS)]
    for i in range(1, 5):
        docs[24 + i] = docs[i].copy()                           # equal scores: they must fall in id order in both stores
    queries = [maxsim_vectors(regime, n, dim, 200 + i) for i, n in enumerate(LQ)]
    store = MultiVectorStore(dim, max_doc_vectors=CAP, format="mxfp4")
    store.append([bf16_bits(d) for d in docs])
    twin, off, deq = _twin_of(store)
    qv = np.full((len(LQ), Q_STRIDE, dim), 0x7FC5, dtype=np.uint16)      # poison behind every count: it must not be read
    for i, q in enumerate(queries):
        qv[i, :len(q)] = bf16_bits(q)
    qc = np.asarray(LQ, np.int32)
    dev = dict(qv=torch.from_numpy(qv.view(np.int16)).cuda().view(torch.bfloat16), qc=torch.from_numpy(qc).cuda())
    return dict(store=store, twin=twin, off=off, deq=deq, docs=docs, queries=queries, qv=qv, qc=qc, dev=dev)


def _bytes(tensors):
    return [None if t is None else (t.dtype, t.cpu().numpy().tobytes()) for t in tensors]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("regime", REGIMES)
def test_the_identity_with_the_bf16_store_of_the_dequantised_vectors(gpu, regime, dim):
    import torch
    from hiprag import maxsim_search_device, maxsim_device
    s = _setup(regime, dim)
    assert s["store"].format == "mxfp4" and s["twin"].format == "bf16"
    cand = torch.from_numpy(np.tile(ID_BASE + np.arange(-1, N_DOCS + 1, dtype=np.int64), (len(LQ), 1))).cuda()   # padding at both ends
    for k in KS:
        got = maxsim_device(s["store"], s["dev"]["qv"], s["dev"]["qc"], cand, k, id_base=ID_BASE)
        info = s["store"].maxsim_info()
        want = maxsim_device(s["twin"], s["dev"]["qv"], s["dev"]["qc"], cand, k, id_base=ID_BASE)
        assert _bytes(got) == _bytes(want), ("hipmaxsim_dev", k)
        assert info == s["twin"].maxsim_info() and info[0] == len(LQ) * sum(1 for d in s["docs"] if len(d)), k
        got = maxsim_search_device(s["store"], s["dev"]["qv"], s["dev"]["qc"], SCOPES, SOQ, k, id_base=ID_BASE)
        sinfo = s["store"].search_info()
        want = maxsim_search_device(s["twin"], s["dev"]["qv"], s["dev"]["qc"], SCOPES, SOQ, k, id_base=ID_BASE)
        assert _bytes(got) == _bytes(want), ("hipmaxsim_search_scoped", k)
        assert sinfo == s["twin"].search_info() and sinfo["pass_rows"] == 32 * TILES[dim] and sinfo["valid_pairs"] > 0, k
        ids = got[1].cpu().numpy()
        assert np.all(ids[9, :1] >= ID_BASE + 3) and np.all(ids[9] < ID_BASE + 37)              # the cut scope keeps to its documents
        assert np.all(np.isin(ids[10][ids[10] >= 0] - ID_BASE, list(range(5, 9)) + list(range(18, 35))))
    # the search's scores are the pair scores' bits, and the copies 25..28 of documents 1..4 rank behind them
    pairs = maxsim_device(s["store"], s["dev"]["qv"], s["dev"]["qc"], cand, 1, id_base=ID_BASE)[3].cpu().numpy()[:, 1:-1]
    sc, ids = (t.cpu().numpy() for t in maxsim_search_device(s["store"], s["dev"]["qv"], s["dev"]["qc"], SCOPES, SOQ, 17, id_base=ID_BASE))
    for i in range(len(LQ)):
        for r in range(17):
            if ids[i, r] >= 0:
                assert sc[i, r].tobytes() == pairs[i, ids[i, r] - ID_BASE].tobytes(), (i, r)
                if r and sc[i, r] == sc[i, r - 1]:
                    assert ids[i, r] > ids[i, r - 1], (i, r)
            else:
                assert sc[i, r] == np.float32(NEG_MAX)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("regime", REGIMES)
def test_the_scores_are_right(gpu, regime, dim):
    from hiprag import maxsim, maxsim_reference
    s = _setup(regime, dim)
    cand = np.tile(np.arange(N_DOCS, dtype=np.int64), (len(LQ), 1))
    pairs = maxsim(s["store"], s["qv"], s["qc"], cand, k=1)[3]
    _, codes, scales = s["store"].export_mxfp4()
    off, deq = s["off"], s["deq"]
    worst = dev = 0.0
    for j, d in enumerate(s["docs"]):
        if not len(d):
            assert np.all(pairs[:, j] == np.float32(NEG_MAX))
            continue
        rows = slice(int(off[j]), int(off[j + 1]))
        dq = bf16_values(deq[rows]).astype(np.float64)
        for i, q in enumerate(s["queries"]):
            if regime == "exact":                                # integers in [-4, 4] are codes times a power of two: lossless
                assert np.array_equal(dq, d)
                r = score_ratio(pairs[i, j], maxsim_reference(q, dq), None)
            else:
                want, _ = maxsim_expected(q, d, regime)          # of the ORIGINAL vectors
                _, acc = maxsim_expected(q, dq, regime)          # the accumulation bound on the dequantised vectors
                bound = acc + mc.maxsim_quant_bound(q, bf16_bits(d), scales[rows])
                r = abs(float(pairs[i, j]) - want) / bound
                dev = max(dev, abs(float(pairs[i, j]) - want))
            worst = max(worst, r)
            assert r <= 1.0, (regime, dim, i, j, float(pairs[i, j]))
    print(f"mxfp4 maxsim {regime} dim {dim}: worst |got - ref| / bound = {worst:.3g} (exact: 0 = bits); "
          f"largest |score - float64 score of the original vectors| = {dev:.3g}")


def test_vectors_of_many_magnitudes_zero_and_guarded_rows(gpu):
    """The identity where the block scales differ from block to block and row to row, the special vectors among the rows."""
    from hiprag import MultiVectorStore, maxsim, maxsim_search
    docs = mc.mixed_docs((1, 33, 64, 0, 97), 256, 21) + [mc.special_vectors(256)]
    store = MultiVectorStore(256, max_doc_vectors=128, format="mxfp4")
    store.append(docs)
    twin, off, deq = _twin_of(store, 128)
    qv = np.concatenate(mc.mixed_docs((40, 40), 256, 22)).reshape(2, 40, 256)
    qv[qv == 0x7F80] = 0                                        # finite queries
    cand = np.asarray([[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]], np.int64)
    got, want = maxsim(store, qv, [40, 33], cand, k=6), maxsim(twin, qv, [40, 33], cand, k=6)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert np.all(np.isfinite(got[3][cand != 3])) and store.maxsim_info() == twin.maxsim_info()
    for a, b in zip(maxsim_search(store, qv, [40, 33], [[(0, 6)]], None, 6), maxsim_search(twin, qv, [40, 33], [[(0, 6)]], None, 6)):
        assert a.tobytes() == b.tobytes()


def test_the_search_follows_removals_and_appends(gpu):
    from hiprag import MultiVectorStore, maxsim_search
    s = _setup("random", 128)
    docs = [bf16_bits(d) for d in s["docs"]]
    gone = [(5, 12), (20, 21), (33, 40)]
    extra = [bf16_bits(maxsim_vectors("random", n, 128, 900 + n)) for n in (40, 0, 33)]
    store = MultiVectorStore(128, max_doc_vectors=CAP, format="mxfp4")
    store.append(docs)
    store.remove_ranges(gone)
    store.append(extra)
    survivors = drop_ranges(docs, gone) + extra
    fresh = MultiVectorStore(128, max_doc_vectors=CAP, format="mxfp4")
    fresh.append(survivors)
    twin, _, _ = _twin_of(fresh)
    n = len(survivors)
    assert len(store) == n
    scopes = [[(0, n)], [(3, 20), (20, 21), (n - 5, n)]]
    soq = [i % 2 for i in range(len(LQ))]
    for k in (5, 17):
        got = maxsim_search(store, s["qv"], s["qc"], scopes, soq, k)
        for other in (fresh, twin):                             # the same answer as a fresh store, and the right one
            want = maxsim_search(other, s["qv"], s["qc"], scopes, soq, k)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), k
        assert np.any(got[1] >= n - 3)                          # the appended documents are found


def test_m3_score_with_only_the_colbert_weight_gives_the_maxsim_bits(gpu):
    import torch
    from hiprag import HipFlatIndex, m3_score_device, maxsim_device
    s = _setup("random", 128)
    rng = np.random.default_rng(3)
    index = HipFlatIndex(128, metric="ip")
    index.add(rng.standard_normal((N_DOCS, 128)).astype(np.float32))
    index.set_id_base(ID_BASE)
    cand = torch.from_numpy(ID_BASE + rng.integers(-2, N_DOCS + 2, size=(len(LQ), 64)).astype(np.int64)).cuda()
    out = m3_score_device(index, None, s["store"], None, None, None, s["dev"]["qv"], s["dev"]["qc"], cand, 16, weights=(0, 0, 1))
    scores, ids, pos, pairs = maxsim_device(s["store"], s["dev"]["qv"], s["dev"]["qc"], cand, 16, id_base=ID_BASE)
    torch.cuda.synchronize()
    parts = out["parts"][..., 2].contiguous().cpu().numpy()
    assert parts.tobytes() == pairs.cpu().numpy().tobytes()
    assert bool((parts > NEG_MAX).any()) and bool((parts == np.float32(NEG_MAX)).any())
    top = out["pos"].cpu().numpy()[:, 0]                         # the best candidate's combined score is its MaxSim, times 1.0
    assert np.array_equal(out["scores"].cpu().numpy()[:, 0], parts[np.arange(len(LQ)), top].astype(np.float64))
    twin_out = m3_score_device(index, None, s["twin"], None, None, None, s["dev"]["qv"], s["dev"]["qc"], cand, 16, weights=(0, 0, 1))
    torch.cuda.synchronize()
    for name in out:
        assert torch.equal(out[name], twin_out[name]), name
