"""
The PACKED device rerank (hiprerank_packed_*): every pair costs its own length rounded up to 64 rows, not the store's longest
document.  Pair assembly at the packed rows against the pure-Python pair rule, the row count against Python's arithmetic, the
logits against hipenc_score_pairs_packed on a host-built batch of each sub-batch (THE SAME BITS), selection against a numpy
sort, the host entry against the device entry (bit for bit), the padded call within the reranker's tolerance, and every
documented refusal.
The store and queries are those of tests/test_rerank_gpu.py (builders copied), with a longer limit (L = 512) and ONE 400-token
document that no candidate names: the store-wide bound of hiprerank_dev is then 512 rows per pair.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOCAB, L, CAP, ID_BASE = 2000, 512, 508, 1000
SHORT_L = 128                                      # the limit of tests/test_rerank_gpu.py: pairs are cut at room = 124
DOC_LENS = [0, 1, 59, 60, 61, 119, 120, 121, 124, 125, 130] * 3 + [2, 5, 9, 17, 33, 40, 64]       # 40 passages
LONG_DOC = 400                                     # document 40: never a candidate
NEG_MAX = -float(np.finfo(np.float32).max)
RERANK_ATOL = 1.5e-2            # tests/test_encoder_gpu.py::test_reranker_head_logits

_STATE = {}


def _setup():
    """one encoder and one store for the module"""
    if not _STATE:
        from hiprag import EncoderConfig, HipEncoder, TokenStore, random_state
        cfg = EncoderConfig(vocab=VOCAB, hidden=256, layers=2, heads=4, ffn=512, max_pos=600, max_seq_len=L)
        enc = HipEncoder(cfg, random_state(cfg, seed=9, with_head=True), with_head=True)
        rng = np.random.default_rng(21)
        docs = [rng.integers(3, VOCAB, size=n).tolist() for n in DOC_LENS + [LONG_DOC]]
        store = TokenStore(VOCAB, bos=0, eos=2, pad=cfg.pad_id, max_doc_tokens=CAP)
        store.append(docs[:25])
        store.append(docs[25:])
        _STATE.update(cfg=cfg, enc=enc, docs=docs, store=store)
    return _STATE["cfg"], _STATE["enc"], _STATE["docs"], _STATE["store"]


def _queries(lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(3, VOCAB, size=n).tolist() for n in lens]


def _candidates(nq, depth, n_docs, seed):
    """ids of stored documents (never the last, long one) with padding of every kind and repeats mixed in"""
    rng = np.random.default_rng(seed)
    cand = ID_BASE + rng.integers(0, n_docs - 1, size=(nq, depth)).astype(np.int64)
    odd = [-1, ID_BASE - 1, ID_BASE + n_docs, -5, ID_BASE + n_docs + 7, 0]     # negative, below id_base, beyond the store
    for q in range(nq):
        for j, v in enumerate(odd):
            cand[q, (3 * q + 5 * j) % depth] = v
        if depth >= 4:
            cand[q, depth - 1] = cand[q, depth // 2] = ID_BASE + (q % (n_docs - 1))       # the same document twice
    cand[0, 0] = ID_BASE + n_docs - 2                                                  # the last short document is a valid one
    assert not np.any(cand == ID_BASE + n_docs - 1)
    return cand


def _valid(cand, n_docs):
    return (cand >= ID_BASE) & (cand < ID_BASE + n_docs)


def _pairs(queries, cand, docs, max_len):
    """the pure-Python rule: the token list of every slot, padding slots as the 4-token pair"""
    from hiprag import pair_tokens
    out = []
    for q in range(cand.shape[0]):
        for c in cand[q].tolist():
            ok = ID_BASE <= c < ID_BASE + len(docs)
            out.append(pair_tokens(queries[q], docs[c - ID_BASE][:CAP], max_len) if ok else pair_tokens([], [], max_len))
    return out


def _round64(n):
    return -(-n // 64) * 64


def _greedy(lens, B):
    """the stated cut: a sub-batch takes the next pair while its packed rows stay <= B; it holds at least one pair"""
    cuts, o, rows = [], 0, 0
    for i, n in enumerate(lens):
        if i > o and rows + _round64(n) > B:
            cuts.append((o, i))
            o, rows = i, 0
        rows += _round64(n)
    return cuts + [(o, len(lens))]


@pytest.mark.parametrize("max_len", [SHORT_L, L])
@pytest.mark.parametrize("depth", [1, 3, 50])
def test_packed_assembly_equals_the_pair_rule_at_the_packed_rows(gpu, depth, max_len):
    from hiprag.rerank import seq_len_bound
    cfg, _enc, docs, store = _setup()
    queries = _queries([0, 1, 3, SHORT_L - 4, 130], seed=depth)
    cand = _candidates(len(queries), depth, len(docs), seed=100 + depth)
    tokens, row_off, lens = store.assemble_packed(queries, cand, id_base=ID_BASE, max_len=max_len)
    pairs = _pairs(queries, cand, docs, max_len)
    want_lens = np.asarray([len(p) for p in pairs], dtype=np.int32)
    assert np.array_equal(lens, want_lens) and int(lens.max()) <= max_len
    want_off = np.concatenate([[0], np.cumsum([_round64(n) for n in want_lens])]).astype(np.int32)
    assert np.array_equal(row_off, want_off) and tokens.shape == (int(want_off[-1]),)
    want = np.full(int(want_off[-1]), cfg.pad_id, dtype=np.int32)
    for p, o in zip(pairs, want_off):
        want[o:o + len(p)] = p
    assert np.array_equal(tokens, want)
    pad_slots = ~_valid(cand, len(docs)).reshape(-1)
    assert pad_slots.any() and np.all(lens[pad_slots] == 4)
    assert all(tokens[o:o + 4].tolist() == [0, 2, 2, 2] for o in row_off[:-1][pad_slots])
    valid, padding, rows, _ = store.rerank_packed_info()
    assert (valid, padding, rows) == (int((~pad_slots).sum()), int(pad_slots.sum()), int(want_off[-1]))
    # the point of the packed call: fewer rows than pairs x S of the store-wide bound, which the 400-token document sets
    S = seq_len_bound(max_len, 130, LONG_DOC)
    assert S == max_len
    if max_len == L:
        assert rows < len(pairs) * S, (rows, len(pairs) * S)


def _score_pairs_packed(enc, pairs):
    """hipenc_score_pairs_packed on a host-built batch exactly as given"""
    import torch
    from hiprag import _native as nat
    flat = np.ascontiguousarray([t for p in pairs for t in p], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum([len(p) for p in pairs])]).astype(np.int32)
    out = torch.empty(len(pairs), dtype=torch.float32, device="cuda")
    nat.call("hipenc_score_pairs_packed", enc._h, flat.ctypes.data, off.ctypes.data, len(pairs), out.data_ptr(),
             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_packed_logits_are_the_bits_of_score_pairs_packed_on_each_sub_batch(gpu):
    import torch
    from hiprag import rerank_device
    _cfg, enc, docs, store = _setup()
    queries = _queries([3, 0, 20], seed=4)
    depth = 7
    cand = _candidates(3, depth, len(docs), seed=40)
    cand_dev = torch.from_numpy(cand).cuda()
    valid = _valid(cand, len(docs)).reshape(-1)
    pairs = _pairs(queries, cand, docs, L)
    lens = [len(p) for p in pairs]
    total = sum(_round64(n) for n in lens)
    for B in (0, 512):                      # one sub-batch (131072 rows), then sub-batches of at most 512 packed rows
        _, _, _, logits = rerank_device(enc, store, queries, cand_dev, 1, id_base=ID_BASE, max_len=L, max_batch_tokens=B, packed=True)
        torch.cuda.synchronize()
        cuts = _greedy(lens, B or 131072)
        n_valid, n_pad, rows, batches = store.rerank_packed_info()
        assert (n_valid, n_pad, rows, batches) == (int(valid.sum()), int((~valid).sum()), total, len(cuts))
        assert len(cuts) == 1 if B == 0 else len(cuts) >= 3
        want = np.concatenate([_score_pairs_packed(enc, pairs[a:b]) for a, b in cuts])
        got = logits.cpu().numpy().reshape(-1)
        assert got[valid].tobytes() == want[valid].tobytes(), np.abs(got[valid] - want[valid]).max()
        assert np.all(got[~valid] == np.float32(NEG_MAX))
    # a limit below one pair's rows: every sub-batch holds exactly one pair
    rerank_device(enc, store, queries, cand_dev, 1, id_base=ID_BASE, max_len=L, max_batch_tokens=1, packed=True)
    assert store.rerank_packed_info()[3] == len(pairs)


@pytest.mark.parametrize("k", [1, 7])
def test_packed_selection_equals_a_sort_of_the_calls_own_logits(gpu, k):
    import torch
    from hiprag import rerank_device
    _cfg, enc, docs, store = _setup()
    depth = 7
    queries = _queries([3, 5, 1, 0], seed=6)
    cand = _candidates(4, depth, len(docs), seed=60)
    cand[3, :] = [-1, ID_BASE - 1, ID_BASE + len(docs), -9, -1, -1, -1]          # a query with no valid candidate
    scores, ids, pos, logits = (t.cpu().numpy() for t in rerank_device(enc, store, queries, torch.from_numpy(cand).cuda(), k,
                                                                       id_base=ID_BASE, max_len=L, packed=True))
    valid = _valid(cand, len(docs))
    for q in range(4):
        order = sorted([j for j in range(depth) if valid[q, j]], key=lambda j: (-logits[q, j], j))
        for r in range(k):
            if r < len(order):
                j = order[r]
                assert (ids[q, r], pos[q, r]) == (cand[q, j], j) and scores[q, r].tobytes() == logits[q, j].tobytes()
            else:
                assert ids[q, r] == -1 and pos[q, r] == -1 and scores[q, r] == np.float32(NEG_MAX)
        assert np.all(logits[q][~valid[q]] == np.float32(NEG_MAX))
    assert np.all(ids[3] == -1) and np.all(pos[3] == -1)


def test_packed_host_entry_is_the_device_entry_and_the_padded_call_is_close(gpu):
    import torch
    from hiprag import rerank, rerank_device
    _cfg, enc, docs, store = _setup()
    depth = 7
    cand = _candidates(3, depth, len(docs), seed=70)
    queries = _queries([3, 7, 0], seed=80)
    cand_dev = torch.from_numpy(cand).cuda()
    d = [t.cpu().numpy() for t in rerank_device(enc, store, queries, cand_dev, depth, id_base=ID_BASE, max_len=L, packed=True)]
    info = store.rerank_packed_info()
    h = rerank(enc, store, queries, cand, depth, id_base=ID_BASE, max_len=L, packed=True)
    assert store.rerank_packed_info() == info                       # the same layout: no tighter bound exists any more
    assert all(a.tobytes() == b.tobytes() for a, b in zip(d, h))
    # against the padded call (the 400-token document sets S for every pair): the same pairs on another plan
    from hiprag.rerank import seq_len_bound
    p_scores, p_ids, p_pos, p_logits = (t.cpu().numpy() for t in rerank_device(enc, store, queries, cand_dev, depth, id_base=ID_BASE,
                                                                               max_len=L))
    S = seq_len_bound(L, 7, LONG_DOC)
    assert S == 448 and store.rerank_info()[2] == S and info[2] < 3 * depth * S
    valid = _valid(cand, len(docs))
    print(f"\n[packed rerank vs padded] {info[2]} packed rows against {3 * depth * S}; max |logit delta| "
          f"{np.abs(d[3][valid] - p_logits[valid]).max():.3e}")
    assert np.allclose(d[3][valid], p_logits[valid], rtol=0, atol=RERANK_ATOL)
    assert np.all(d[3][~valid] == np.float32(NEG_MAX))


def test_packed_rerank_refuses_what_the_padded_call_refuses_before_anything_is_enqueued(gpu):
    import torch
    from hiprag import EncoderConfig, HipEncoder, HipRagError, TokenStore, rerank_device
    from hiprag import _native as nat
    cfg, enc, docs, store = _setup()
    depth, nq, k = 7, 2, 3
    cand = torch.from_numpy(_candidates(nq, depth, len(docs), seed=90)).cuda()
    rerank_device(enc, store, _queries([2, 3], 9), cand, k, id_base=ID_BASE, max_len=L, packed=True)      # a good call: the info to keep
    info = store.rerank_packed_info()
    qt = np.asarray([5, 6, 7, 8, 9], dtype=np.int32)
    qo = np.asarray([0, 2, 5], dtype=np.int32)
    logits = torch.full((nq, depth), 7.0, device="cuda")
    scores = torch.full((nq, k), 7.0, device="cuda")
    ids = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    pos = torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
    no_head = HipEncoder(EncoderConfig(vocab=VOCAB, hidden=128, layers=1, heads=2, ffn=128, max_pos=600, max_seq_len=L))
    wide = TokenStore(VOCAB + 1, pad=cfg.pad_id)
    other_pad = TokenStore(VOCAB, pad=3)
    for st in (wide, other_pad):
        st.append([[5, 6]])

    def call(**kw):
        a = dict(enc=enc._h, st=store._h, qt=qt.ctypes.data, qo=qo.ctypes.data, nq=nq, cand=cand.data_ptr(), depth=depth, base=ID_BASE,
                 max_len=L, k=k, B=0, logits=logits.data_ptr(), scores=scores.data_ptr(), ids=ids.data_ptr(), pos=pos.data_ptr())
        a.update(kw)
        nat.call("hiprerank_packed_dev", a["enc"], a["st"], a["qt"], a["qo"], a["nq"], a["cand"], a["depth"], a["base"], a["max_len"],
                 a["k"], a["B"], a["logits"], a["scores"], a["ids"], a["pos"], None)

    def arr(v):
        keep.append(np.asarray(v, dtype=np.int32))
        return keep[-1].ctypes.data

    keep = []
    refused = [
        dict(cand=None), dict(scores=None), dict(ids=None), dict(qo=None), dict(qt=None),
        dict(nq=0), dict(k=0), dict(k=depth + 1), dict(depth=257, k=1), dict(depth=0, k=0),
        dict(max_len=4), dict(max_len=600 - cfg.pad_id - 1),                   # the position-table rule of hipenc_forward
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
    assert store.rerank_packed_info() == info
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
            nat.call("hiprerank_packed_host", enc._h, store._h, qt.ctypes.data, qo.ctypes.data, a["nq"], host_cand.ctypes.data, a["depth"],
                     ID_BASE, L, a["k"], 0, None, out.ctypes.data, oid.ctypes.data, None)
    with pytest.raises(HipRagError):
        store.assemble_packed([[5], [VOCAB]], host_cand, id_base=ID_BASE, max_len=L)
    with pytest.raises(HipRagError):
        store.assemble_packed([[5], [6]], host_cand, id_base=ID_BASE, max_len=4)
