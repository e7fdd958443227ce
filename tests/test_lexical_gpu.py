"""
The encoder's lexical head (libhiprag hipenc_set_lexical_head / hipenc_forward_lexical, HipEncoder.encode_lexical): BGE-M3's
per-token weights relu(sparse_linear(hidden)) from the forward that makes the embedding, deduplicated per sequence on the
device.  Expected values: hiprag.lexical.lexical_reference (numpy, the kernel's summation order) applied to the hidden rows
of the SAME batch (HipEncoder.hidden_tokens: the GEMM plan depends on the batch) -- bit for bit -- and the fp64 dot of the
same bf16 inputs within a bound derived from the summation depth.

vocab = 48 so that ids repeat inside a sequence; lengths 0, 1, 2, 63, 64, 65 and 130 in one batch.  Seed and bias were
chosen on the CPU (oracle.encoder_oracle.xlmr_hidden_bf16sim) so that some token weight is 0, some is positive and some id
occurs twice with different weights; test_the_batch_has_the_cases asserts all three from the reference.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -6   # include/hiprag.h
CONFIGS = {"h128": dict(hidden=128, heads=2, ffn=256, layers=2), "h256": dict(hidden=256, heads=4, ffn=512, layers=2)}
LENS = (0, 1, 2, 63, 64, 65, 130)
UNUSED = (0, 1, 2, 3)
SEED = 11


def bf16_f32(t):
    import torch
    return t.detach().to(torch.bfloat16).float().cpu().numpy()


@functools.lru_cache(maxsize=None)
def setup(name):
    """encoder, tokens, the device's four outputs, the hidden rows of the same batch and the reference over them"""
    import torch
    from hiprag import EncoderConfig, HipEncoder, random_state
    from hiprag.lexical import lexical_reference
    cfg = EncoderConfig(vocab=48, max_pos=200, max_seq_len=192, **CONFIGS[name])
    sd = random_state(cfg, seed=SEED, with_lexical=True)
    rng = np.random.default_rng(SEED)
    toks = []
    for n in LENS:
        body = rng.integers(3, cfg.vocab, size=max(n - 2, 0)).tolist()       # 3 (unk) is an unused id that occurs in bodies
        toks.append(([0] + body + [2])[:n] if n >= 2 else [0][:n])
    enc = HipEncoder(cfg, sd)
    enc.set_lexical_head(sd["sparse_linear.weight"], sd["sparse_linear.bias"], UNUSED)
    out = enc.encode_lexical(toks, batch_size=256)
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in out)
    hidden = enc.hidden_tokens(toks, batch_size=256)
    w = bf16_f32(sd["sparse_linear.weight"].reshape(-1))
    b = float(sd["sparse_linear.bias"].float().reshape(-1)[0])
    ref = lexical_reference(hidden, toks, w, b, UNUSED, max_len=max(LENS))
    return enc, cfg, toks, out, hidden, (w, b), ref


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_batch_has_the_cases(gpu, name):
    from hiprag.lexical import lexical_token_weights
    _, _, toks, _, hidden, (w, b), _ = setup(name)
    wt = [lexical_token_weights(h, w, b) if len(t) else np.zeros(0, np.float32) for h, t in zip(hidden, toks)]
    allw = np.concatenate(wt)
    assert np.any(allw == 0) and np.any(allw > 0)
    twice = False
    for t, x in zip(toks, wt):
        t = np.asarray(t)
        for i in np.unique(t):
            v = x[t == i]
            twice = twice or (v.size >= 2 and np.unique(v).size >= 2)
    assert twice, "no id occurs twice with different weights"
    assert any(3 in t for t in toks)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_outputs_equal_the_reference_bit_for_bit(gpu, name):
    _, _, toks, (dense, terms, weights, counts), _, _, (rt, rw, rc) = setup(name)
    assert terms.shape == rt.shape == (len(LENS), max(LENS)) and terms.dtype == np.int32 and counts.dtype == np.int32
    assert np.array_equal(counts, rc)
    assert counts[0] == 0 and counts.max() > 1
    assert np.array_equal(terms, rt)
    assert np.array_equal(weights.view(np.uint32), rw.view(np.uint32))
    for i, n in enumerate(counts):
        assert np.all(np.diff(terms[i, :n]) > 0), "ids of a row must ascend strictly"
        assert np.all(terms[i, n:] == -1) and np.all(weights[i, n:].view(np.uint32) == 0)
        assert np.all(weights[i, :n] > 0) and not set(terms[i, :n].tolist()) & set(UNUSED)
        assert set(terms[i, :n].tolist()) <= set(toks[i])


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_dense_output_is_hipenc_forwards(gpu, name):
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    enc, cfg, toks, (dense, terms, weights, counts), _, _, _ = setup(name)
    plain = enc.encode_tokens(toks, batch_size=256).cpu().numpy()
    assert np.array_equal(dense.view(np.uint32), plain.view(np.uint32))
    assert np.all(dense[0] == 0)
    # out_dense_dev = NULL: the sparse outputs alone, the same bits; and a second run gives the same bits
    order = sorted(range(len(toks)), key=lambda i: -len(toks[i]))
    ids, lens, max_len = enc._pad([toks[i] for i in order])
    pt = torch.empty((len(toks), max_len), dtype=torch.int32, device="cuda")
    pw = torch.empty((len(toks), max_len), dtype=torch.float32, device="cuda")
    pc = torch.empty((len(toks),), dtype=torch.int32, device="cuda")
    nat.call("hipenc_forward_lexical", enc._h, ids.ctypes.data, lens.ctypes.data, len(toks), max_len, None, pt.data_ptr(), pw.data_ptr(),
             pc.data_ptr(), _stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(pt.cpu().numpy(), terms[order]) and np.array_equal(pc.cpu().numpy(), counts[order])
    assert np.array_equal(pw.cpu().numpy().view(np.uint32), weights[order].view(np.uint32))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_weights_against_the_fp64_dot(gpu, name):
    """|w - max(0, dot64 + b)| <= (H/64 + 8) * 2^-24 * (sum |x_c w_c| + |b|) per token: the summation depth is H/64 - 1 adds per
    lane + 6 butterfly steps + 1 bias add = H/64 + 6 roundings, each at most 2^-24 relative to a partial sum that
    sum |x_c w_c| + |b| bounds (the products are exact, relu is 1-Lipschitz); H/64 + 8 leaves the second-order terms room.
    The row's weight of an id is a maximum over positions, and |max a - max b| <= max |a - b|, so the bound of an id is the
    largest bound of its positions."""
    _, cfg, toks, (_, terms, weights, counts), hidden, (w, b), _ = setup(name)
    H = cfg.hidden
    checked = 0
    for i, t in enumerate(toks):
        if not len(t):
            continue
        x = hidden[i].astype(np.float64)
        ref = np.maximum(0.0, x @ w.astype(np.float64) + b)
        bound = (H / 64 + 8) * 2.0 ** -24 * (np.abs(x * w.astype(np.float64)[None, :]).sum(axis=1) + abs(b))
        t = np.asarray(t)
        got = dict(zip(terms[i, :counts[i]].tolist(), weights[i, :counts[i]].astype(np.float64)))
        for tid in np.unique(t):
            if int(tid) in UNUSED:
                continue
            sel = t == tid
            err = abs(got.get(int(tid), 0.0) - ref[sel].max())
            assert err <= bound[sel].max(), f"sequence {i} id {tid}: error {err} above the bound {bound[sel].max()}"
            checked += 1
    assert checked > 50


def test_refusals(gpu):
    import torch
    from hiprag import EncoderConfig, HipEncoder, random_state
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    cfg = EncoderConfig(vocab=48, max_pos=200, max_seq_len=192, **CONFIGS["h128"])
    sd = random_state(cfg, seed=SEED, with_lexical=True)
    head = {k: sd.pop(k) for k in ("sparse_linear.weight", "sparse_linear.bias")}
    enc = HipEncoder(cfg, sd)
    assert not enc.has_lexical
    ids, lens = np.asarray([[0, 5, 2]], np.int32), np.asarray([3], np.int32)
    pt = torch.full((1, 3), 7, dtype=torch.int32, device="cuda")
    pw = torch.full((1, 3), 7.0, dtype=torch.float32, device="cuda")
    pc = torch.full((1,), 7, dtype=torch.int32, device="cuda")

    def forward(max_len=3, terms=pt):
        nat.call("hipenc_forward_lexical", enc._h, ids.ctypes.data, lens.ctypes.data, 1, max_len, None,
                 terms.data_ptr() if terms is not None else None, pw.data_ptr(), pc.data_ptr(), _stream_ptr())

    with pytest.raises(nat.HipRagError) as e:     # no head set
        forward()
    assert e.value.code == E_INVALID
    with pytest.raises(ValueError):
        enc.encode_lexical([[0, 5, 2]])
    wt = head["sparse_linear.weight"].reshape(-1).to(device="cuda", dtype=torch.bfloat16)
    bt = head["sparse_linear.bias"].to(device="cuda", dtype=torch.float32)
    un = np.arange(17, dtype=np.int32)
    with pytest.raises(nat.HipRagError) as e:     # n_unused = 17
        nat.call("hipenc_set_lexical_head", enc._h, wt.data_ptr(), bt.data_ptr(), un.ctypes.data, 17)
    assert e.value.code == E_INVALID
    with pytest.raises(nat.HipRagError) as e:     # still no head
        forward()
    assert e.value.code == E_INVALID
    enc.set_lexical_head(head["sparse_linear.weight"], head["sparse_linear.bias"], UNUSED)
    with pytest.raises(nat.HipRagError) as e:
        forward(max_len=2049)
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(nat.HipRagError) as e:     # a null output
        forward(terms=None)
    assert e.value.code == E_INVALID
    torch.cuda.synchronize()
    assert torch.all(pt == 7) and torch.all(pw == 7.0) and torch.all(pc == 7), "a refused call wrote its outputs"
    forward()                                      # and the same call with a head runs
    torch.cuda.synchronize()
    assert int(pc[0]) in (0, 1) and torch.all(pt[0, int(pc[0]):] == -1)
    enc.close()
