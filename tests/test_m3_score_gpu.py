"""
BGE-M3's combined score on the device (hipm3_score_*, hiprag.m3_score*): the three components are the bits the component
entries give the pair (hipidx_score_ids_dev, hipbm25_score_ids_dev, hipmaxsim_dev's pair scores), and the combination, the
order, the ids and the positions are hiprag.m3_score_reference fed with those components.  No tolerance anywhere: the
arithmetic on top of the components is a few correctly rounded fp64 operations.

Setup: 40 documents -- an IP and an L2 flat index at d = 128, a multi-vector store at dim 128 with 0 to 9 vectors per document
(some have none), lexical postings over 50 terms; 3 queries, one without ColBERT vectors and one without terms.
"""
import functools

import numpy as np
import pytest

from oracle.linear_cases import bf16_bits

pytestmark = pytest.mark.gpu

E_INVALID = -1
F32_MAX = np.finfo(np.float32).max
F64_MAX = np.finfo(np.float64).max
N, D, N_TERMS, NQ, Q_STRIDE = 40, 128, 50, 3, 12
ID_BASE = 300
MIX = (0.4, 0.2, 0.4)
SHAPES = [(1, 1), (7, 1), (7, 4), (7, 7), (64, 1), (64, 33), (64, 64), (256, 1), (256, 100), (256, 256)]


def unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def setup():
    import torch
    from hiprag import HipBM25, HipFlatIndex, MultiVectorStore, PostingsCSR
    rng = np.random.default_rng(31)
    x = unit(rng, N, D).astype(np.float32)
    idx = {}
    for metric in ("ip", "l2"):
        idx[metric] = HipFlatIndex(D, metric=metric)
        idx[metric].add(x)
        idx[metric].set_id_base(ID_BASE)
    n_vecs = rng.integers(0, 10, size=N)
    n_vecs[[3, 17]] = 0                                              # documents without vectors
    n_vecs[5] = 9
    docs = [bf16_bits(unit(rng, int(n), D)) if n else np.zeros((0, D), np.uint16) for n in n_vecs]
    store = MultiVectorStore(D, max_doc_vectors=16)
    store.append(docs)
    lists = [np.sort(rng.choice(N, size=int(rng.integers(0, N + 1)), replace=False)) for _ in range(N_TERMS)]
    off = np.zeros(N_TERMS + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(v) for v in lists]).astype(np.uint64)
    post = PostingsCSR(N, N_TERMS, off, np.concatenate(lists).astype(np.uint32), np.exp(rng.normal(0, 1, size=int(off[-1]))).astype(np.float32))
    bm = HipBM25(post, id_base=ID_BASE)
    q = unit(rng, NQ, D).astype(np.float32)
    q_counts = np.asarray([7, 0, Q_STRIDE], dtype=np.int32)          # query 1 has no ColBERT vectors
    q_vecs = np.full((NQ, Q_STRIDE, D), 0x7FC5, dtype=np.uint16)     # poison behind every count
    for i, c in enumerate(q_counts):
        q_vecs[i, :c] = bf16_bits(unit(rng, int(c), D))
    terms = [rng.integers(0, N_TERMS, size=9).tolist(), rng.integers(0, N_TERMS + 3, size=70).tolist(), []]   # query 2 has no terms
    tw = [rng.uniform(0.05, 2.0, size=len(t)).astype(np.float32) for t in terms]
    dev = dict(q=torch.from_numpy(q).cuda(), q_vecs=torch.from_numpy(q_vecs.view(np.int16)).cuda().view(torch.bfloat16),
               q_counts=torch.from_numpy(q_counts).cuda())
    return dict(idx=idx, store=store, bm=bm, q=q, q_vecs=q_vecs, q_counts=q_counts, terms=terms, tw=tw, dev=dev, n_vecs=n_vecs)


def candidates(depth, seed):
    """rows of the collection with repeats, and every kind of padding: -1, id_base - 1, id_base + N, far outside"""
    rng = np.random.default_rng(seed)
    cand = ID_BASE + rng.integers(0, N, size=(NQ, depth)).astype(np.int64)
    pads = np.asarray([-1, ID_BASE - 1, ID_BASE + N, ID_BASE + 10 ** 12, 0])
    mask = rng.random((NQ, depth)) < 0.2
    cand[mask] = pads[rng.integers(0, len(pads), size=int(mask.sum()))]
    if depth >= 7:
        cand[:, 1], cand[:, 4] = ID_BASE + 5, ID_BASE + 5              # one document twice: a tie broken by position
        cand[:, 2] = ID_BASE + 3                                        # a document without vectors
    return cand


def components(s, metric, cand_dev):
    """the three component entries, called separately -> host arrays (dense64, dense32, sparse32, maxsim32)"""
    import torch
    from hiprag import maxsim_device
    d64, d32 = s["idx"][metric].score_ids_device(s["dev"]["q"], cand_dev)
    sp = s["bm"].score_ids_device(s["terms"], cand_dev, s["tw"])
    pairs = maxsim_device(s["store"], s["dev"]["q_vecs"], s["dev"]["q_counts"], cand_dev, 1, id_base=ID_BASE)[3]
    torch.cuda.synchronize()
    return d64.cpu().numpy(), d32.cpu().numpy(), sp.cpu().numpy(), pairs.cpu().numpy()


def check_against_reference(out, comps, cand, weights, k, l2):
    from hiprag import m3_score_reference
    d64, d32, sp, ms = comps
    valid = (cand >= ID_BASE) & (cand < ID_BASE + N)
    pairs, scores, pos = m3_score_reference(d64, sp, ms, valid, weights, k, l2=l2)
    assert np.array_equal(out["pairs"].view(np.uint64), pairs.view(np.uint64))
    assert np.array_equal(out["scores"].view(np.uint64), scores.view(np.uint64))
    assert np.array_equal(out["pos"], pos)
    want_ids = np.where(pos >= 0, np.take_along_axis(cand, np.maximum(pos, 0), axis=1), -1)
    assert np.array_equal(out["ids"], want_ids)
    want_parts = np.stack([d32 if weights[0] > 0 else np.zeros_like(d32), sp if weights[1] > 0 else np.zeros_like(sp),
                           ms if weights[2] > 0 else np.zeros_like(ms)], axis=2)
    assert np.array_equal(out["parts"].view(np.uint32), want_parts.view(np.uint32))
    return valid, pairs, pos


@pytest.mark.parametrize("metric", ("ip", "l2"))
@pytest.mark.parametrize("depth,k", SHAPES)
def test_parts_are_the_entries_and_the_rest_is_the_reference(gpu, metric, depth, k):
    import torch
    from hiprag import m3_score_device
    s = setup()
    cand = candidates(depth, depth * 1000 + k)
    cand_dev = torch.from_numpy(cand).cuda()
    comps = components(s, metric, cand_dev)
    out = m3_score_device(s["idx"][metric], s["bm"], s["store"], s["dev"]["q"], s["terms"], s["tw"], s["dev"]["q_vecs"], s["dev"]["q_counts"],
                          cand_dev, k, weights=MIX)
    torch.cuda.synchronize()
    out = {name: t.cpu().numpy() for name, t in out.items()}
    valid, pairs, pos = check_against_reference(out, comps, cand, MIX, k, metric == "l2")
    # the setup has power: a query without vectors and documents without vectors are MaxSim padding yet stay candidates
    ms = comps[3]
    assert np.all(ms[1] == -F32_MAX) and np.all(out["pairs"][1][valid[1]] > -F64_MAX)
    assert np.all(comps[2][2][valid[2]] == 0.0)                        # the query without terms scores 0.0, not padding
    if depth >= 7:
        assert ms[0, 2] == -F32_MAX and valid[0, 2]
        r1, r4 = [list(pos[0]).index(p) if p in pos[0] else None for p in (1, 4)]
        assert r4 is None or (r1 is not None and r1 < r4)                # equal scores: the earlier position ranks first
    if metric == "l2" and depth >= 7:
        assert np.all(comps[0][valid] >= 0) and np.all(np.abs(1.0 - 0.5 * comps[0][valid]) <= 1.0 + 1e-6)


@pytest.mark.parametrize("weights", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0.7, 0.3, 0), (0.5, 0, 1.5), (0, 2, 1)])
def test_legs_with_weight_zero_are_not_run_and_need_no_handle(gpu, weights):
    import torch
    from hiprag import m3_score, m3_score_device
    s = setup()
    depth, k = 64, 20
    cand = candidates(depth, 77)
    cand_dev = torch.from_numpy(cand).cuda()
    comps = components(s, "ip", cand_dev)
    use_d, use_s, use_c = (w > 0 for w in weights)
    out = m3_score_device(s["idx"]["ip"], s["bm"] if use_s else None, s["store"] if use_c else None, s["dev"]["q"] if use_d else None,
                          s["terms"] if use_s else None, s["tw"] if use_s else None, s["dev"]["q_vecs"] if use_c else None,
                          s["dev"]["q_counts"] if use_c else None, cand_dev, k, weights=weights)
    torch.cuda.synchronize()
    out = {name: t.cpu().numpy() for name, t in out.items()}
    check_against_reference(out, comps, cand, weights, k, False)
    host = m3_score(s["idx"]["ip"], s["bm"] if use_s else None, s["store"] if use_c else None, s["q"] if use_d else None,
                    s["terms"] if use_s else None, s["tw"] if use_s else None, s["q_vecs"] if use_c else None,
                    s["q_counts"] if use_c else None, cand, k, weights=weights)
    for name in out:
        assert host[name].tobytes() == out[name].tobytes(), name         # the host entry agrees with the device entry


def test_unweighted_terms_and_null_outputs(gpu):
    import torch
    from hiprag import m3_score_device
    s = setup()
    cand = candidates(7, 5)
    cand_dev = torch.from_numpy(cand).cuda()
    args = (s["idx"]["ip"], s["bm"], s["store"], s["dev"]["q"])
    tail = (s["dev"]["q_vecs"], s["dev"]["q_counts"], cand_dev, 3)
    a = m3_score_device(*args, s["terms"], None, *tail)                  # term weights NULL = every weight 1.0f
    b = m3_score_device(*args, s["terms"], [np.ones(len(t), np.float32) for t in s["terms"]], *tail)
    c = m3_score_device(*args, s["terms"], None, *tail, want_parts=False)   # out_parts and out_pair_scores NULL
    torch.cuda.synchronize()
    for name in ("scores", "ids", "pos"):
        assert torch.equal(a[name], b[name]) and torch.equal(a[name], c[name])
    assert torch.equal(a["parts"], b["parts"]) and c["parts"] is None and c["pairs"] is None


def test_mismatched_handles_and_bad_arguments_are_refused(gpu):
    import torch
    from hiprag import HipBM25, HipFlatIndex, HipRagError, MultiVectorStore, m3_score_device
    s = setup()
    cand_dev = torch.from_numpy(candidates(7, 9)).cuda()

    def call(index=None, bm=None, store=None, k=3, weights=MIX, cand=cand_dev):
        return m3_score_device(index or s["idx"]["ip"], bm or s["bm"], store or s["store"], s["dev"]["q"], s["terms"], s["tw"],
                               s["dev"]["q_vecs"], s["dev"]["q_counts"], cand, k, weights=weights)

    call()
    short = HipFlatIndex(D, metric="ip")
    short.add(s["q"])                                                     # 3 rows against 40 documents
    short.set_id_base(ID_BASE)
    other_base = HipBM25(s["bm"].p, id_base=ID_BASE + 1)
    fewer = MultiVectorStore(D, max_doc_vectors=16)
    fewer.append([np.zeros((1, D), np.uint16)] * (N - 1))
    try:
        for name, kw in (("document count of the postings", dict(index=short, weights=(1, 1, 0))),
                         ("document count of the store", dict(index=short, weights=(1, 0, 1))),
                         ("id_base of the postings", dict(bm=other_base)), ("documents of the store", dict(store=fewer)),
                         ("k 0", dict(k=0)), ("k above depth", dict(k=8))):
            with pytest.raises(HipRagError) as e:
                call(**kw)
            assert e.value.code == E_INVALID, name
        with pytest.raises(HipRagError) as e:
            call(cand=torch.zeros((NQ, 257), dtype=torch.int64, device="cuda"))
        assert e.value.code == E_INVALID
        for bad in ((0, 0, 0), (1, -1, 1), (float("nan"), 1, 1)):
            with pytest.raises(ValueError):
                call(weights=bad)
        import hiprag._native as nat
        o = torch.zeros((NQ, 3), dtype=torch.float64, device="cuda")
        oi = torch.zeros((NQ, 3), dtype=torch.int64, device="cuda")
        base = [s["idx"]["ip"]._h, 0, 0, s["dev"]["q"].data_ptr(), None, None, None, None, None, 1, NQ, cand_dev.data_ptr(), 7, 3, 1.0, 0.0, 0.0,
                None, None, o.data_ptr(), oi.data_ptr(), None, None]
        nat.call("hipm3_score_dev", *base)                                # dense alone: every other argument 0 / NULL
        for pos, value in ((14, 0.0), (14, float("inf")), (15, -1.0), (3, None), (11, None), (19, None), (20, None), (10, 0)):
            a = list(base)
            a[pos] = value
            with pytest.raises(HipRagError) as e:
                nat.call("hipm3_score_dev", *a)
            assert e.value.code == E_INVALID, pos
        a = list(base)
        a[15] = 1.0                                                        # w_sparse > 0 without postings: an unknown handle
        with pytest.raises(HipRagError):
            nat.call("hipm3_score_dev", *a)
    finally:
        short.close()
        other_base.close()
        fewer.close()


def test_fp8_store_gives_the_result_of_a_bf16_store_of_the_dequantised_vectors(gpu):
    import torch
    from hiprag import MultiVectorStore, m3_score_device
    s = setup()
    fp8 = s["store"].to_fp8()
    off, deq = fp8.export()
    plain = MultiVectorStore(D, max_doc_vectors=16)
    plain.append(deq, off)
    try:
        cand_dev = torch.from_numpy(candidates(64, 3)).cuda()
        outs = [m3_score_device(s["idx"]["l2"], s["bm"], st, s["dev"]["q"], s["terms"], s["tw"], s["dev"]["q_vecs"], s["dev"]["q_counts"],
                                cand_dev, 64, weights=MIX) for st in (fp8, plain)]
        torch.cuda.synchronize()
        for name in outs[0]:
            assert torch.equal(outs[0][name], outs[1][name]), name
        assert bool((outs[0]["parts"][..., 2] > -F32_MAX).any())
    finally:
        fp8.close()
        plain.close()
