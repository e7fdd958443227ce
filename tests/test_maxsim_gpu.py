"""
Late interaction on the device (hipmaxsim_*): pair scores against the float64 reference -- bit for bit on integer data, within
the accumulation bound on unit vectors -- at every tile boundary of the kernel (32 query vectors per LDS tile, 32 document
vectors per wave step, four waves); padding, selection and ties under hiprerank_dev's rules; the bits of a pair do not depend
on where it stands in a call; the counters equal their closed forms.  Bounds: tests/colbert_cases.py.
"""
import functools

import numpy as np
import pytest

from colbert_cases import NEG_MAX, maxsim_expected, maxsim_vectors, score_ratio, select_expected
from oracle.linear_cases import bf16_bits

pytestmark = pytest.mark.gpu

CAP = 160
LQ = (1, 31, 32, 33, 65)
LD = (1, 31, 32, 33, 127, 128, 129, CAP, 0, CAP + 10)      # documents 0..9: document 8 is empty, 9 is cut to the cap
Q_STRIDE = 65
ID_BASE = 1000


@functools.lru_cache(maxsize=None)
def _setup(regime, dim):
    """One store and one query block per (regime, dim), and the float64 table of every (query, document) pair."""
    from hiprag import MultiVectorStore
    docs = [maxsim_vectors(regime, n, dim, 100 + i) for i, n in enumerate(LD)]
    queries = [maxsim_vectors(regime, n, dim, 200 + i) for i, n in enumerate(LQ)]
    store = MultiVectorStore(dim, max_doc_vectors=CAP)
    store.append([bf16_bits(d) for d in docs])
    qv = np.full((len(LQ), Q_STRIDE, dim), 0x7FC5, dtype=np.uint16)      # poison behind every count: it must not be read
    for i, q in enumerate(queries):
        qv[i, :len(q)] = bf16_bits(q)
    table = {}
    for i, q in enumerate(queries):
        for j, d in enumerate(docs):
            if len(d):
                table[i, j] = maxsim_expected(q, d[:CAP], regime)
    return dict(store=store, qv=qv, qc=np.asarray(LQ, np.int32), table=table, docs=docs, queries=queries)


def _closed_form_reads(qis, cand_docs):
    return sum(min(LD[j], CAP) * -(-LQ[i] // 32) for i, row in zip(qis, cand_docs) for j in row if j is not None and LD[j] > 0)


@pytest.mark.parametrize("dim", (128, 1024))
@pytest.mark.parametrize("regime", ("exact", "random"))
def test_every_pair_of_the_boundary_lengths(gpu, regime, dim):
    from hiprag import maxsim
    s = _setup(regime, dim)
    cand = np.tile(np.arange(len(LD), dtype=np.int64), (len(LQ), 1))
    scores, ids, pos, pairs = maxsim(s["store"], s["qv"], s["qc"], cand, k=len(LD))
    worst = 0.0
    for (i, j), (want, bound) in s["table"].items():
        r = score_ratio(pairs[i, j], want, bound)
        worst = max(worst, r)
        assert r <= 1.0, (regime, dim, LQ[i], LD[j], float(pairs[i, j]), want, bound)
    print(f"maxsim {regime} dim {dim}: worst |got - ref| / bound = {worst:.3g} over {len(s['table'])} pairs (bound None = bits)")
    assert np.all(pairs[:, 8] == np.float32(NEG_MAX))                     # the empty document is padding
    valid = np.asarray([n > 0 for n in LD])
    for i in range(len(LQ)):
        sc, ii, pp = select_expected(pairs[i], cand[i], valid, len(LD))
        assert np.array_equal(ids[i], ii) and np.array_equal(pos[i], pp) and sc.tobytes() == scores[i].tobytes()
    info = s["store"].maxsim_info()
    assert info == (len(LQ) * 9, len(LQ), _closed_form_reads(range(len(LQ)), [list(range(len(LD)))] * len(LQ)), 0), info
    again = maxsim(s["store"], s["qv"], s["qc"], cand, k=len(LD))
    for a, b in zip((scores, ids, pos, pairs), again):
        assert a.tobytes() == b.tobytes()                                  # the same bits from run to run


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
    # candidates: stored documents (with repeats), and every kind of padding
    pads = [-1, -5, ID_BASE - 1, 0, ID_BASE + len(LD), ID_BASE + 10 ** 12, ID_BASE + 8]
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
    scores, ids, pos, pairs = maxsim(s["store"], qv, qc, cand, k=k, id_base=ID_BASE)
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
    assert s["store"].maxsim_info() == (n_valid, nq * depth - n_valid, reads, 0)
    # the device entry: the same bits, with and without the optional outputs
    t = lambda x, dt: torch.from_numpy(x).cuda().view(dt) if dt == torch.bfloat16 else torch.from_numpy(x).cuda()
    dqv, dqc, dcand = t(qv.view(np.int16), torch.bfloat16), t(qc, torch.int32), t(cand, torch.int64)
    ds, di, dp, dpairs = maxsim_device(s["store"], dqv, dqc, dcand, k, id_base=ID_BASE)
    assert ds.cpu().numpy().tobytes() == scores.tobytes() and di.cpu().numpy().tobytes() == ids.tobytes()
    assert dp.cpu().numpy().tobytes() == pos.tobytes() and dpairs.cpu().numpy().tobytes() == pairs.tobytes()
    ds2, di2, _, none = maxsim_device(s["store"], dqv, dqc, dcand, k, id_base=ID_BASE, want_pairs=False)
    assert none is None and ds2.cpu().numpy().tobytes() == scores.tobytes() and di2.cpu().numpy().tobytes() == ids.tobytes()


def test_an_empty_store_and_a_single_pair(gpu):
    from hiprag import MultiVectorStore, maxsim
    st = MultiVectorStore(128, max_doc_vectors=4)
    qv = bf16_bits(maxsim_vectors("exact", 2, 128, 1)).reshape(1, 2, 128)
    scores, ids, pos, pairs = maxsim(st, qv, [2], np.asarray([[0, 1, -1]], np.int64), k=2)
    assert np.all(pairs == np.float32(NEG_MAX)) and np.all(ids == -1) and np.all(pos == -1) and np.all(scores == np.float32(NEG_MAX))
    assert st.maxsim_info() == (0, 3, 0, 0)
    d = maxsim_vectors("exact", 5, 128, 2)
    st.append([bf16_bits(d)])                                              # cut to the cap of 4
    scores, ids, pos, pairs = maxsim(st, qv, [2], np.asarray([[0]], np.int64), k=1)
    want, _ = maxsim_expected(maxsim_vectors("exact", 2, 128, 1), d[:4], "exact")
    assert pairs[0, 0].tobytes() == np.float32(want).tobytes() and ids[0, 0] == 0 and pos[0, 0] == 0
    assert st.maxsim_info() == (1, 0, 4, 0)


def test_every_check_raises_with_nothing_written(gpu):
    import torch
    from hiprag import HipRagError
    from hiprag import _native as nat
    s = _setup("exact", 128)
    st = s["store"]
    nq, depth, k = 2, 4, 2
    qv = torch.from_numpy(s["qv"][:nq].view(np.int16).copy()).cuda()
    qc = torch.from_numpy(s["qc"][:nq].copy()).cuda()
    cand = torch.zeros((nq, depth), dtype=torch.int64, device="cuda")
    outs = dict(pairs=torch.full((nq, depth), 7.0, device="cuda"), scores=torch.full((nq, k), 7.0, device="cuda"),   # 7 = untouched
                ids=torch.full((nq, k), 7, dtype=torch.int64, device="cuda"), pos=torch.full((nq, k), 7, dtype=torch.int32, device="cuda"))

    def call(h=st._h, q=qv.data_ptr(), c=qc.data_ptr(), stride=Q_STRIDE, n=nq, cd=cand.data_ptr(), d=depth, base=0, kk=k,
             scores=outs["scores"].data_ptr(), ids=outs["ids"].data_ptr()):
        nat.call("hipmaxsim_dev", h, q, c, stride, n, cd, d, base, kk, outs["pairs"].data_ptr(), scores, ids, outs["pos"].data_ptr(), None)

    bad = [dict(q=None), dict(c=None), dict(cd=None), dict(scores=None), dict(ids=None), dict(n=0), dict(kk=0), dict(kk=depth + 1),
           dict(d=257, kk=1), dict(d=0, kk=0), dict(stride=0), dict(stride=513), dict(base=-1), dict(n=2 ** 24, d=256)]
    for kw in bad:
        with pytest.raises(HipRagError) as e:
            call(**kw)
        assert e.value.code == -1, kw
    with pytest.raises(HipRagError) as e:
        call(h=123456789)
    assert e.value.code == -3
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert bool((t == 7).all()), name
    # the host entry checks the same things
    hq, hc, hcand = s["qv"][:nq].copy(), s["qc"][:nq].copy(), np.zeros((nq, depth), np.int64)
    so, io = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int64)
    for kw in (dict(nq=0), dict(k=0), dict(k=depth + 1), dict(stride=0), dict(stride=513), dict(base=-1)):
        a = dict(nq=nq, k=k, stride=Q_STRIDE, base=0)
        a.update(kw)
        with pytest.raises(HipRagError) as e:
            nat.call("hipmaxsim_host", st._h, hq.ctypes.data, hc.ctypes.data, a["stride"], a["nq"], hcand.ctypes.data, depth, a["base"],
                     a["k"], None, so.ctypes.data, io.ctypes.data, None)
        assert e.value.code == -1, kw
    call()                                                                  # and the unchanged call goes through
    torch.cuda.synchronize()
    assert bool((outs["ids"] == 0).all()) and bool((outs["pos"] < depth).all())
