"""
The device rerank call (hiprerank_*): pair assembly against the pure-Python pair rule, logits against hipenc_score_pairs on
a host-built batch of the same composition (THE SAME BITS), selection against a numpy sort, the host entry against the
device entry, and every documented refusal.
Encoder of tests/test_hybrid_gpu.py's size; about 40 passages at the lengths around room = 124 and the cap; L = 128.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOCAB, L, CAP, ID_BASE = 2000, 128, 130, 1000
ROOM = L - 4
DOC_LENS = [0, 1, 59, 60, 61, 119, 120, 121, 124, 125, CAP] * 3 + [2, 5, 9, 17, 33, 40, 64]       # 40 passages
NEG_MAX = -float(np.finfo(np.float32).max)
RERANK_ATOL = 1.5e-2            # tests/test_encoder_gpu.py::test_reranker_head_logits

_STATE = {}


def _setup():
    """one encoder and one store for the module"""
    if not _STATE:
        from hiprag import EncoderConfig, HipEncoder, TokenStore, random_state
        cfg = EncoderConfig(vocab=VOCAB, hidden=256, layers=2, heads=4, ffn=512, max_pos=200, max_seq_len=L)
        enc = HipEncoder(cfg, random_state(cfg, seed=9, with_head=True), with_head=True)
        rng = np.random.default_rng(21)
        docs = [rng.integers(3, VOCAB, size=n).tolist() for n in DOC_LENS]
        store = TokenStore(VOCAB, bos=0, eos=2, pad=cfg.pad_id, max_doc_tokens=CAP)
        store.append(docs[:25])
        store.append(docs[25:])
        _STATE.update(cfg=cfg, enc=enc, docs=docs, store=store)
    return _STATE["cfg"], _STATE["enc"], _STATE["docs"], _STATE["store"]


def _queries(lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(3, VOCAB, size=n).tolist() for n in lens]


def _candidates(nq, depth, n_docs, seed):
    """ids of stored documents with padding of every kind and repeats mixed in"""
    rng = np.random.default_rng(seed)
    cand = ID_BASE + rng.integers(0, n_docs, size=(nq, depth)).astype(np.int64)
    odd = [-1, ID_BASE - 1, ID_BASE + n_docs, -5, ID_BASE + n_docs + 7, 0]
    for q in range(nq):
        for j, v in enumerate(odd):
            cand[q, (3 * q + 5 * j) % depth] = v
        if depth >= 4:
            cand[q, depth - 1] = cand[q, depth // 2] = ID_BASE + (q % n_docs)       # the same document twice
    cand[0, 0] = ID_BASE + n_docs - 1                                              # the last document is a valid one
    return cand


def _valid(cand, n_docs):
    return (cand >= ID_BASE) & (cand < ID_BASE + n_docs)


def _expected_rows(queries, cand, docs, S, pad):
    """the pure-Python rule: tokens [nq * depth][S] and lens"""
    from hiprag import pair_tokens
    nq, depth = cand.shape
    rows = np.full((nq * depth, S), pad, dtype=np.int32)
    lens = np.zeros(nq * depth, dtype=np.int32)
    for q in range(nq):
        for j in range(depth):
            c = int(cand[q, j])
            ok = ID_BASE <= c < ID_BASE + len(docs)
            pair = pair_tokens(queries[q], docs[c - ID_BASE][:CAP], L) if ok else pair_tokens([], [], L)
            rows[q * depth + j, :len(pair)] = pair
            lens[q * depth + j] = len(pair)
    return rows, lens


@pytest.mark.parametrize("depth", [1, 7, 64, 65, 256])
def test_assembly_equals_the_pair_rule(gpu, depth):
    from hiprag.rerank import seq_len_bound
    cfg, _enc, docs, store = _setup()
    queries = _queries([0, 1, 3, ROOM, 130], seed=depth)
    cand = _candidates(len(queries), depth, len(docs), seed=100 + depth)
    tokens, lens = store.assemble(queries, cand, id_base=ID_BASE, max_len=L)
    S = seq_len_bound(L, 130, CAP)
    assert S == 128 and tokens.shape == (len(queries) * depth, S)
    want_tokens, want_lens = _expected_rows(queries, cand, docs, S, cfg.pad_id)
    assert np.array_equal(lens, want_lens)
    assert np.array_equal(tokens, want_tokens)
    pad_rows = ~_valid(cand, len(docs)).reshape(-1)
    assert pad_rows.any() and np.all(lens[pad_rows] == 4) and np.all(tokens[pad_rows, :4] == [0, 2, 2, 2])
    valid, padding, info_S, _ = store.rerank_info()
    assert (valid, padding, info_S) == (int((~pad_rows).sum()), int(pad_rows.sum()), S)
    if depth == 7:      # a short batch under a shorter limit: S follows min(max_len, ...), and a store-wide bound below max_len
        t2, l2 = store.assemble(queries[:3], cand[:3], id_base=ID_BASE, max_len=70)
        assert t2.shape[1] == 128 and int(l2.max()) <= 70
        t3, l3 = store.assemble(queries[:3], cand[:3], id_base=ID_BASE, max_len=60)
        assert t3.shape[1] == 64 and int(l3.max()) <= 60


def _score_pairs_host(enc, rows, lens, S):
    """hipenc_score_pairs on a host-built batch exactly as given: no sorting, max_len = S"""
    import torch
    from hiprag import _native as nat
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    out = torch.empty(len(rows), dtype=torch.float32, device="cuda")
    nat.call("hipenc_score_pairs", enc._h, rows.ctypes.data, lens.ctypes.data, len(rows), S, out.data_ptr(),
             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_logits_are_the_bits_of_score_pairs_on_the_same_batch(gpu):
    import torch
    from hiprag import rerank_device
    cfg, enc, docs, store = _setup()
    queries = _queries([3, 0, 2], seed=4)
    depth = 7
    cand = _candidates(3, depth, len(docs), seed=40)
    cand_dev = torch.from_numpy(cand).cuda()
    valid = _valid(cand, len(docs)).reshape(-1)
    for batch_tokens in (0, None):           # one sub-batch, then 4 x S tokens: sub-batches of four pairs
        _, _, _, logits = rerank_device(enc, store, queries, cand_dev, 1, id_base=ID_BASE, max_len=L,
                                        max_batch_tokens=4 * 128 if batch_tokens is None else 0)
        torch.cuda.synchronize()
        n_valid, n_pad, S, batches = store.rerank_info()
        assert S == 128 and n_valid + n_pad == 3 * depth and n_valid == int(valid.sum())
        per = 3 * depth if batch_tokens == 0 else 4
        assert batches == -(-3 * depth // per)
        rows, lens = _expected_rows(queries, cand, docs, S, cfg.pad_id)
        want = np.concatenate([_score_pairs_host(enc, rows[o:o + per], lens[o:o + per], S) for o in range(0, len(rows), per)])
        got = logits.cpu().numpy().reshape(-1)
        assert got[valid].tobytes() == want[valid].tobytes(), np.abs(got[valid] - want[valid]).max()
        assert np.all(got[~valid] == np.float32(NEG_MAX))


@pytest.mark.parametrize("k", [1, 7])
def test_selection_equals_a_sort_of_the_calls_own_logits(gpu, k):
    import torch
    from hiprag import rerank_device
    _cfg, enc, docs, store = _setup()
    depth = 7
    queries = _queries([3, 5, 1, 0], seed=6)
    cand = _candidates(4, depth, len(docs), seed=60)
    cand[3, :] = [-1, ID_BASE - 1, ID_BASE + len(docs), -9, -1, -1, -1]          # a query with no valid candidate
    scores, ids, pos, logits = (t.cpu().numpy() for t in rerank_device(enc, store, queries, torch.from_numpy(cand).cuda(), k,
                                                                       id_base=ID_BASE, max_len=L))
    valid = _valid(cand, len(docs))
    n_valid, n_pad, _S, batches = store.rerank_info()
    assert n_valid + n_pad == 4 * depth and n_valid == int(valid.sum()) and batches == 1
    for q in range(4):
        # the repeated document: two candidates, the same bits, the earlier position first
        a, b = depth // 2, depth - 1
        if q < 3:
            assert cand[q, a] == cand[q, b] and logits[q, a].tobytes() == logits[q, b].tobytes()
        order = sorted([j for j in range(depth) if valid[q, j]], key=lambda j: (-logits[q, j], j))
        for r in range(k):
            if r < len(order):
                j = order[r]
                assert (ids[q, r], pos[q, r]) == (cand[q, j], j) and scores[q, r].tobytes() == logits[q, j].tobytes()
            else:
                assert ids[q, r] == -1 and pos[q, r] == -1 and scores[q, r] == np.float32(NEG_MAX)
        assert np.all(logits[q][~valid[q]] == np.float32(NEG_MAX))
    assert np.all(ids[3] == -1)


def test_host_entry_agrees_with_the_device_entry_at_its_tighter_bound(gpu):
    import torch
    from hiprag import rerank, rerank_device
    from hiprag.rerank import seq_len_bound
    _cfg, enc, docs, store = _setup()
    short = [i for i, n in enumerate(DOC_LENS) if n <= 40]
    rng = np.random.default_rng(8)
    depth = 7
    cand = ID_BASE + rng.choice(short, size=(3, depth)).astype(np.int64)
    cand[1, 2] = -1
    cand[2, 5] = ID_BASE + len(docs)
    queries = _queries([3, 7, 0], seed=80)
    d_scores, d_ids, d_pos, d_logits = (t.cpu().numpy() for t in rerank_device(enc, store, queries, torch.from_numpy(cand).cuda(), depth,
                                                                               id_base=ID_BASE, max_len=L))
    assert store.rerank_info()[2] == 128                    # the store-wide bound
    h_scores, h_ids, h_pos, h_logits = rerank(enc, store, queries, cand, depth, id_base=ID_BASE, max_len=L)
    longest = max(min(DOC_LENS[int(c) - ID_BASE], CAP) for c in cand.reshape(-1) if ID_BASE <= c < ID_BASE + len(docs))
    assert store.rerank_info()[2] == seq_len_bound(L, 7, longest) == 64      # the tight one
    valid = _valid(cand, len(docs))
    print(f"\n[rerank host vs dev] max |logit delta| {np.abs(h_logits[valid] - d_logits[valid]).max():.3e}")
    assert np.array_equal(h_ids, d_ids) and np.array_equal(h_pos, d_pos)
    assert np.allclose(h_logits[valid], d_logits[valid], rtol=0, atol=RERANK_ATOL)
    assert np.all(h_logits[~valid] == np.float32(NEG_MAX)) and np.all(d_logits[~valid] == np.float32(NEG_MAX))
    live = h_ids >= 0
    assert np.allclose(h_scores[live], d_scores[live], rtol=0, atol=RERANK_ATOL) and np.array_equal(h_scores[~live], d_scores[~live])


def test_every_documented_check_refuses_before_anything_is_enqueued(gpu):
    import torch
    from hiprag import EncoderConfig, HipEncoder, HipRagError, TokenStore, rerank_device
    from hiprag import _native as nat
    cfg, enc, docs, store = _setup()
    depth, nq, k = 7, 2, 3
    cand = torch.from_numpy(_candidates(nq, depth, len(docs), seed=90)).cuda()
    rerank_device(enc, store, _queries([2, 3], 9), cand, k, id_base=ID_BASE, max_len=L)      # a good call: the info to keep
    info = store.rerank_info()
    qt = np.asarray([5, 6, 7, 8, 9], dtype=np.int32)
    qo = np.asarray([0, 2, 5], dtype=np.int32)
    logits = torch.full((nq, depth), 7.0, device="cuda")
    scores = torch.full((nq, k), 7.0, device="cuda")
    ids = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    pos = torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
    no_head = HipEncoder(EncoderConfig(vocab=VOCAB, hidden=128, layers=1, heads=2, ffn=128, max_pos=200, max_seq_len=L))
    wide = TokenStore(VOCAB + 1, pad=cfg.pad_id)
    other_pad = TokenStore(VOCAB, pad=3)
    for st in (wide, other_pad):
        st.append([[5, 6]])

    def call(**kw):
        a = dict(enc=enc._h, st=store._h, qt=qt.ctypes.data, qo=qo.ctypes.data, nq=nq, cand=cand.data_ptr(), depth=depth, base=ID_BASE,
                 max_len=L, k=k, B=0, logits=logits.data_ptr(), scores=scores.data_ptr(), ids=ids.data_ptr(), pos=pos.data_ptr())
        a.update(kw)
        nat.call("hiprerank_dev", a["enc"], a["st"], a["qt"], a["qo"], a["nq"], a["cand"], a["depth"], a["base"], a["max_len"], a["k"],
                 a["B"], a["logits"], a["scores"], a["ids"], a["pos"], None)

    def arr(v):
        keep.append(np.asarray(v, dtype=np.int32))
        return keep[-1].ctypes.data

    keep = []
    refused = [
        dict(cand=None), dict(scores=None), dict(ids=None), dict(qo=None), dict(qt=None),
        dict(nq=0), dict(k=0), dict(k=depth + 1), dict(depth=257, k=1), dict(depth=0, k=0),
        dict(max_len=4), dict(max_len=200 - cfg.pad_id - 1),                   # the position-table rule of hipenc_forward
        dict(qo=arr([1, 2, 5])), dict(qo=arr([0, 3, 2])), dict(qt=arr([5, 6, VOCAB, 8, 9])), dict(qt=arr([5, -1, 7, 8, 9])),
        dict(st=wide._h), dict(st=other_pad._h), dict(enc=no_head._h), dict(base=-1), dict(B=-1),
    ]
    for kw in refused:
        with pytest.raises(HipRagError) as e:
            call(**kw)
        assert e.value.code == -1, kw
    for kw in (dict(enc=12345), dict(st=12345)):                               # unknown handles: HIPRAG_E_HANDLE
        with pytest.raises(HipRagError) as e:
            call(**kw)
        assert e.value.code == -3, kw
    torch.cuda.synchronize()
    for t in (logits, scores, ids, pos):                                       # nothing was enqueued: no output was written
        assert bool((t == 7).all())
    assert store.rerank_info() == info
    call(logits=None, pos=None)                                                # the two optional outputs
    torch.cuda.synchronize()
    assert bool((ids != 7).all()) and bool((pos == 7).all())
    # the host entry and the test hook check the same way
    out = np.zeros(64, dtype=np.float32)
    oid = np.zeros(64, dtype=np.int64)
    host_cand = np.full((nq, depth), ID_BASE, dtype=np.int64)
    for kw in (dict(k=0), dict(depth=257), dict(nq=0)):
        a = dict(nq=nq, depth=depth, k=k)
        a.update(kw)
        with pytest.raises(HipRagError):
            nat.call("hiprerank_host", enc._h, store._h, qt.ctypes.data, qo.ctypes.data, a["nq"], host_cand.ctypes.data, a["depth"], ID_BASE, L,
                     a["k"], 0, None, out.ctypes.data, oid.ctypes.data, None)
    with pytest.raises(HipRagError):
        store.assemble([[5], [VOCAB]], host_cand, id_base=ID_BASE, max_len=L)
    with pytest.raises(HipRagError):
        store.assemble([[5], [6]], host_cand, id_base=ID_BASE, max_len=4)
