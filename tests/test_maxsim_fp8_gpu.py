"""
Late interaction over an fp8 multi-vector store: every output equals, byte for byte, the outputs over a bf16 store that holds
the dequantised vectors (the identity the format is defined for), on test_maxsim_gpu.py's grid of boundary lengths; bit for
bit against the float64 reference on integer data, which the format keeps losslessly; within the accumulation bound plus the
quantisation term against the reference of the ORIGINAL vectors; padding, selection, ties, position invariance, the device
entry and the counters as for the bf16 store.  Bounds: tests/fp8_cases.py, tests/colbert_cases.py.
"""
import functools

import numpy as np
import pytest

import fp8_cases as fc
from colbert_cases import NEG_MAX, maxsim_expected, maxsim_vectors, score_ratio, select_expected
from oracle.linear_cases import bf16_bits, bf16_values

pytestmark = pytest.mark.gpu

CAP = 160
LQ = (1, 31, 32, 33, 65)
LD = (1, 31, 32, 33, 127, 128, 129, CAP, 0, CAP + 10)      # documents 0..9: document 8 is empty, 9 is cut to the cap
Q_STRIDE = 65
ID_BASE = 1000


@functools.lru_cache(maxsize=None)
def _setup(regime, dim):
    """One fp8 store, the bf16 store of its export, and one query block per (regime, dim); the float64 tables."""
    from hiprag import MultiVectorStore
    docs = [maxsim_vectors(regime, n, dim, 100 + i) for i, n in enumerate(LD)]
    queries = [maxsim_vectors(regime, n, dim, 200 + i) for i, n in enumerate(LQ)]
    store = MultiVectorStore(dim, max_doc_vectors=CAP, format="fp8")
    store.append([bf16_bits(d) for d in docs])
    off, deq = store.export()
    twin = MultiVectorStore(dim, max_doc_vectors=CAP)                    # bf16, holding the dequantised vectors
    twin.append(deq, off)
    _, codes, scales = store.export_fp8()
    qv = np.full((len(LQ), Q_STRIDE, dim), 0x7FC5, dtype=np.uint16)      # poison behind every count: it must not be read
    for i, q in enumerate(queries):
        qv[i, :len(q)] = bf16_bits(q)
    table, qterm = {}, {}
    for j, d in enumerate(docs):
        if not len(d):
            continue
        dq = bf16_values(deq[off[j]:off[j + 1]]).astype(np.float64)
        moved = np.maximum(np.abs(d[:CAP]) / 16.0, scales[off[j]:off[j + 1], None].astype(np.float64) / 1024.0)
        for i, q in enumerate(queries):
            table[i, j] = maxsim_expected(q, d[:CAP], regime)             # of the ORIGINAL vectors
            if regime == "random":
                _, acc = maxsim_expected(q, dq, regime)                   # the accumulation bound on the dequantised vectors
                qterm[i, j] = acc + float((np.abs(q) @ moved.T).max(axis=1).mean())
    return dict(store=store, twin=twin, qv=qv, qc=np.asarray(LQ, np.int32), table=table, qterm=qterm, docs=docs, queries=queries)


def _closed_form_reads(qis, cand_docs):
    return sum(min(LD[j], CAP) * -(-LQ[i] // 32) for i, row in zip(qis, cand_docs) for j in row if j is not None and LD[j] > 0)


def _equal(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("dim", (128, 1024))
@pytest.mark.parametrize("regime", ("exact", "random"))
def test_every_pair_of_the_boundary_lengths(gpu, regime, dim):
    from hiprag import maxsim
    s = _setup(regime, dim)
    cand = np.tile(np.arange(len(LD), dtype=np.int64), (len(LQ), 1))
    out = maxsim(s["store"], s["qv"], s["qc"], cand, k=len(LD))
    info = s["store"].maxsim_info()
    # the identity: every output, and the counters, are those of the bf16 store of the dequantised vectors
    _equal(out, maxsim(s["twin"], s["qv"], s["qc"], cand, k=len(LD)))
    assert info == s["twin"].maxsim_info()
    scores, ids, pos, pairs = out
    worst = 0.0
    for (i, j), (want, bound) in s["table"].items():
        if regime == "exact":
            r = score_ratio(pairs[i, j], want, None)                      # integers in [-4, 4] quantise losslessly: bits
        else:
            r = abs(float(pairs[i, j]) - want) / s["qterm"][i, j]
        worst = max(worst, r)
        assert r <= 1.0, (regime, dim, LQ[i], LD[j], float(pairs[i, j]), want)
    print(f"fp8 maxsim {regime} dim {dim}: worst |got - ref| / bound = {worst:.3g} over {len(s['table'])} pairs (exact: 0 = bits)")
    if regime == "random":
        dev = max(abs(float(pairs[i, j]) - want) for (i, j), (want, _) in s["table"].items())
        print(f"fp8 maxsim dim {dim}: largest |score - float64 score of the original vectors| = {dev:.3g}")
    assert np.all(pairs[:, 8] == np.float32(NEG_MAX))                     # the empty document is padding
    valid = np.asarray([n > 0 for n in LD])
    for i in range(len(LQ)):
        sc, ii, pp = select_expected(pairs[i], cand[i], valid, len(LD))
        assert np.array_equal(ids[i], ii) and np.array_equal(pos[i], pp) and sc.tobytes() == scores[i].tobytes()
    assert info == (len(LQ) * 9, len(LQ), _closed_form_reads(range(len(LQ)), [list(range(len(LD)))] * len(LQ)), 0), info
    _equal(out, maxsim(s["store"], s["qv"], s["qc"], cand, k=len(LD)))    # the same bits from run to run


@pytest.mark.parametrize("depth,k,nq", [(1, 1, 1), (5, 1, 3), (5, 5, 1), (64, 64, 3), (64, 1, 1), (256, 256, 1), (256, 1, 3)])
def test_shapes_padding_order_and_position_invariance(gpu, depth, k, nq):
    import torch
    from hiprag import maxsim, maxsim_device
    s = _setup("random", 128)
    full = maxsim(s["store"], s["qv"], s["qc"], np.tile(np.arange(len(LD), dtype=np.int64), (len(LQ), 1)), k=1)[3]
    rng = np.random.default_rng(depth * 7 + k * 3 + nq)
    qis = [int(v) for v in rng.choice(len(LQ), size=nq, replace=False)]
    qv, qc = s["qv"][qis].copy(), s["qc"][qis].copy()
    zero_q = nq == 3
    if zero_q:
        qc[1] = 0                                                           # a query with no vector: all its candidates are padding
    if LQ[qis[0]] == Q_STRIDE:
        qc[0] = 1000                                                        # a count above q_stride is clamped to it
    pads = [-1, -5, ID_BASE - 1, 0, ID_BASE + len(LD), ID_BASE + 10 ** 12, ID_BASE + 8]     # every kind of padding
    cand = np.zeros((nq, depth), dtype=np.int64)
    docs_of = []
    for a in range(nq):
        row = []
        for b in range(depth):
            if depth > 1 and rng.random() < 0.3:
                cand[a, b] = pads[int(rng.integers(len(pads)))]
                row.append(None)
            else:
                j = int(rng.integers(len(LD)))
                cand[a, b] = ID_BASE + j
                row.append(j)
        if depth >= 5:
            cand[a, 1], cand[a, 3] = ID_BASE + 4, ID_BASE + 4             # one document twice: a tie broken by position
            row[1], row[3] = 4, 4
        docs_of.append(row)
    out = maxsim(s["store"], qv, qc, cand, k=k, id_base=ID_BASE)
    info = s["store"].maxsim_info()
    _equal(out, maxsim(s["twin"], qv, qc, cand, k=k, id_base=ID_BASE))    # the identity, padding and all
    assert info == s["twin"].maxsim_info()
    scores, ids, pos, pairs = out
    for a in range(nq):
        valid = np.asarray([j is not None and LD[j] > 0 and not (zero_q and a == 1) for j in docs_of[a]])
        for b, j in enumerate(docs_of[a]):
            if valid[b]:
                assert pairs[a, b].tobytes() == full[qis[a], j].tobytes(), (a, b, j)     # the bits of the pair, wherever it stands
            else:
                assert pairs[a, b] == np.float32(NEG_MAX)
        sc, ii, pp = select_expected(pairs[a], cand[a], valid, k)
        assert np.array_equal(ids[a], ii) and np.array_equal(pos[a], pp) and sc.tobytes() == scores[a].tobytes()
        if depth >= 5 and valid[1]:
            r1, r3 = list(pos[a]).index(1) if 1 in pos[a] else None, list(pos[a]).index(3) if 3 in pos[a] else None
            assert r3 is None or (r1 is not None and r1 < r3)               # equal scores: the earlier position ranks first
    n_valid = sum(int(j is not None and LD[j] > 0 and not (zero_q and a == 1)) for a in range(nq) for j in docs_of[a])
    reads = _closed_form_reads([qis[a] for a in range(nq) if not (zero_q and a == 1)],
                               [docs_of[a] for a in range(nq) if not (zero_q and a == 1)])
    assert info == (n_valid, nq * depth - n_valid, reads, 0)
    # the device entry: the same bytes, with and without the pair scores
    t = lambda x, dt: torch.from_numpy(x).cuda().view(dt) if dt == torch.bfloat16 else torch.from_numpy(x).cuda()
    dqv, dqc, dcand = t(qv.view(np.int16), torch.bfloat16), t(qc, torch.int32), t(cand, torch.int64)
    ds, di, dp, dpairs = maxsim_device(s["store"], dqv, dqc, dcand, k, id_base=ID_BASE)
    assert ds.cpu().numpy().tobytes() == scores.tobytes() and di.cpu().numpy().tobytes() == ids.tobytes()
    assert dp.cpu().numpy().tobytes() == pos.tobytes() and dpairs.cpu().numpy().tobytes() == pairs.tobytes()
    ds2, di2, dp2, none = maxsim_device(s["store"], dqv, dqc, dcand, k, id_base=ID_BASE, want_pairs=False)
    assert none is None and ds2.cpu().numpy().tobytes() == scores.tobytes() and di2.cpu().numpy().tobytes() == ids.tobytes()
    assert dp2.cpu().numpy().tobytes() == pos.tobytes()


def test_vectors_of_many_magnitudes_zero_and_guarded_rows(gpu):
    """The identity where the scales differ from row to row, with zero vectors and rows the guard zeroed among them."""
    from hiprag import MultiVectorStore, maxsim
    lens = (1, 33, 64, 0, 97)
    docs = fc.mixed_docs(lens, 256, 21)
    store = MultiVectorStore(256, max_doc_vectors=128, format="fp8")
    store.append(docs)
    off, deq = store.export()
    twin = MultiVectorStore(256, max_doc_vectors=128)
    twin.append(deq, off)
    qv = np.concatenate(fc.mixed_docs((40, 40), 256, 22)).reshape(2, 40, 256)
    qv[qv == 0x7F80] = 0                                                    # finite queries
    cand = np.asarray([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]], np.int64)
    out = maxsim(store, qv, [40, 33], cand, k=5)
    _equal(out, maxsim(twin, qv, [40, 33], cand, k=5))
    assert np.all(np.isfinite(out[3][cand != 3])) and store.maxsim_info() == twin.maxsim_info()
    # and the scores are those of the float64 reference of the dequantised vectors, within the accumulation bound
    for a, lq in enumerate((40, 33)):
        q = bf16_values(qv[a, :lq]).astype(np.float64)
        for b, j in enumerate(cand[a]):
            if lens[j]:
                d = bf16_values(deq[off[j]:off[j + 1]]).astype(np.float64)
                want, bound = maxsim_expected(q, d, "random")
                assert abs(float(out[3][a, b]) - want) <= bound, (a, b, float(out[3][a, b]), want, bound)
