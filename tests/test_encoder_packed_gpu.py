"""
GPU: the encoder's PACKED forward (hipenc_*_packed, csrc/encoder_packed.h) -- sequences one after another, each rounded up to
whole 64-row granules, no GEMM row for the padding up to a batch's longest sequence.

  * the packed instantiation of attention2_kernel through hipenc_attention_packed, the launch helper the packed forward
    uses: every real row against oracle.encoder_oracle.attention_f64 within oracle.encoder_cases.attention_bound, and bit for
    bit against hipenc_attention's row of the same sequence; 128-query tiles that overhang into the next sequence and past Tp;
  * every real hidden row of every model case against float64 within the bf16-emulation yardstick, recomputed on the CPU, and
    -- wherever the padded and the packed plan agree in path and K splits -- bit for bit against the padded entry;
  * one more model case that reaches the 256-tile path packed, with a last row tile that is part padding;
  * embeddings, logits, independence of the batch's other sequences, the documented checks.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import encoder_cases as ec
from oracle import encoder_oracle as eo

pytestmark = pytest.mark.gpu
RERANK_ATOL = 1.5e-2          # tests/test_encoder_gpu.py: reranker logits against the fp32 oracle

# packed, big_h1024 has only 10 304 rows and falls to the tiled path: this one keeps the 256-tile path when packed
BIG_PACKED = dict(cfg=dict(vocab=3000, hidden=1024, layers=2, heads=16, ffn=4096, max_pos=300), std=0.05, seed=24,
                  lens=(191, 129, 65, 64, 16, 1) * 24 + (192, 130, 2), env={}, path="big", sample=(0, 1, 5, 40, 144, 145, 146))
CASES = dict(ec.MODEL_CASES, big_packed_h1024=BIG_PACKED)


# ---- attention ---------------------------------------------------------------------------------------------------------
ATT_ORDER = (1, 192, 65, 0, 129)      # len 1 directly before len 192 (its tile overhangs into it); len 129 last (past Tp)


def _relay(case):
    """The sequences of lengths ATT_ORDER of an attention case, re-laid into the packed layout on the host."""
    import torch
    from hiprag.encoder import packed_layout
    lens = case["lens"].tolist()
    pick = [lens.index(n) for n in ATT_ORDER]
    row_off, Tp, _, items = packed_layout(ATT_ORDER)
    assert Tp == 576 and row_off.tolist() == [0, 64, 256, 384, 384, 576]
    h = case["heads"]
    q = torch.zeros((h, Tp, 64), dtype=torch.bfloat16)
    k = torch.zeros_like(q)
    vt = torch.zeros((h, 64, Tp), dtype=torch.bfloat16)
    for s, i in enumerate(pick):
        r0, R = int(row_off[s]), int(row_off[s + 1] - row_off[s])
        q[:, r0:r0 + R], k[:, r0:r0 + R], vt[:, :, r0:r0 + R] = case["q"][i, :, :R], case["k"][i, :, :R], case["vt"][i, :, :, :R]
    return pick, row_off, Tp, items, q, k, vt


def _attention_packed(row_off, Tp, items, q, k, vt, heads, fill, guard=128):
    """-> (ctx bf16 [Tp, heads * 64], the `guard` rows behind it) on the host; ctx starts out as `fill`."""
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    dev = torch.device("cuda", 0)
    qd, kd, vd = (t.to(dev).contiguous() for t in (q, k, vt))
    ro = torch.from_numpy(row_off).to(dev)
    ln = torch.tensor(ATT_ORDER, dtype=torch.int32, device=dev)
    it = torch.from_numpy(np.ascontiguousarray(items)).to(dev)
    ctx = torch.full((Tp + guard, heads * 64), fill, dtype=torch.bfloat16, device=dev)
    nat.call("hipenc_attention_packed", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), ro.data_ptr(), ln.data_ptr(), it.data_ptr(),
             len(items), len(ATT_ORDER), Tp, heads, ctx.data_ptr(), _stream_ptr())
    torch.cuda.synchronize()
    return ctx[:Tp].cpu(), ctx[Tp:].cpu()


def _attention_padded(case):
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    dev = torch.device("cuda", 0)
    q, k, vt = (case[n].to(dev).contiguous() for n in ("q", "k", "vt"))
    lens = torch.from_numpy(case["lens"]).to(dev)
    nseq, heads, S, _ = q.shape
    ctx = torch.full((nseq, S, heads * 64), 7.0, dtype=torch.bfloat16, device=dev)
    nat.call("hipenc_attention", q.data_ptr(), k.data_ptr(), vt.data_ptr(), lens.data_ptr(), ctx.data_ptr(), nseq, S, heads,
             _stream_ptr())
    torch.cuda.synchronize()
    return ctx.cpu()


@pytest.mark.parametrize("regime", ec.ATT_REGIMES)
def test_packed_attention_every_row_against_fp64_and_the_padded_kernel(gpu, regime):
    import torch
    case = ec.attention_case(regime, 192)
    pick, row_off, Tp, items, q, k, vt = _relay(case)
    got, guard = _attention_packed(row_off, Tp, items, q, k, vt, case["heads"], fill=7.0)
    assert bool((guard == 7.0).all()), "the tile that overhangs past Tp wrote behind ctx"
    assert bool(torch.isfinite(got.float()).all())
    ref, A = eo.attention_f64(case["q"], case["k"], case["vt"], case["lens"])
    bound = ec.attention_bound(ref, A)
    padded = _attention_padded(case)
    worst = 0.0
    for s, i in enumerate(pick):
        n, r0 = ATT_ORDER[s], int(row_off[s])
        if n == 0:
            continue
        g = got[r0:r0 + n]
        ratio = float(((g.double() - ref[i, :n]).abs() / bound[i, :n]).max())
        worst = max(worst, ratio)
        assert torch.equal(g.view(torch.int16), padded[i, :n].view(torch.int16)), (regime, n, "differs from hipenc_attention")
    print(f"\n[packed attention {regime}] worst |err| / bound {worst:.3f} over lens {ATT_ORDER}, Tp {Tp}")
    assert worst <= 1.0, (regime, worst)
    again, guard = _attention_packed(row_off, Tp, items, q, k, vt, case["heads"], fill=-3.0)
    assert torch.equal(again.view(torch.int16), got.view(torch.int16)) and bool((guard == -3.0).all())


def test_packed_attention_entry_validates_its_arguments(gpu):
    import torch
    from hiprag import HipRagError, _native as nat
    dev = torch.device("cuda", 0)
    t = torch.zeros((1, 64, 64), dtype=torch.bfloat16, device=dev)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)
    ro, ln, it = i32(0, 64), i32(1), i32(0, 0)
    ctx = torch.zeros((64, 64), dtype=torch.bfloat16, device=dev)
    ok = dict(q=t.data_ptr(), k=t.data_ptr(), vt=t.data_ptr(), ro=ro.data_ptr(), ln=ln.data_ptr(), it=it.data_ptr(), n_items=1, nseq=1,
              Tp=64, heads=1, ctx=ctx.data_ptr())
    for bad in (dict(q=None), dict(k=None), dict(vt=None), dict(ro=None), dict(ln=None), dict(it=None), dict(ctx=None), dict(Tp=0),
                dict(Tp=96), dict(Tp=-64), dict(nseq=0), dict(heads=0), dict(n_items=-1)):
        a = dict(ok, **bad)
        with pytest.raises(HipRagError):
            nat.call("hipenc_attention_packed", a["q"], a["k"], a["vt"], a["ro"], a["ln"], a["it"], a["n_items"], a["nseq"], a["Tp"],
                     a["heads"], a["ctx"], None)


# ---- whole model, every row ---------------------------------------------------------------------------------------------
def _pool_reference(cls_row):
    """pool_kernel's arithmetic on one bf16 CLS row (as float32), operation for operation (tests/test_encoder_kernels_gpu.py)."""
    v = cls_row.astype(np.float32)
    lanes = np.zeros(64, dtype=np.float32)
    for r in v.reshape(-1, 64):
        lanes = lanes + r * r
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ off]
    inv = np.float32(1.0) / np.maximum(np.sqrt(lanes[0]), np.float32(1e-12))
    return v * inv


def _set_env(monkeypatch, env):
    for var in ("HIPENC_SMALL_ROWS", "HIPENC_GEMM256"):
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, val)


def _plans(enc, lens):
    """(P1, P2, agree): the plan of the padded batch of all sequences, that of the packed one, and whether a row's bits must agree."""
    from hiprag.encoder import forward_plan, packed_layout
    shape = enc.shape()
    p1 = forward_plan(shape, len(lens), -(-max(max(lens), 1) // 64) * 64)
    p2 = forward_plan(shape, 1, packed_layout(lens)[1])
    return p1, p2, (p1.path, p1.osplit, p1.dsplit) == (p2.path, p2.osplit, p2.dsplit)


def _path_name(p):
    return {0: "small", 1: "big"}.get(p.path) or ("tiled_splitk" if max(p.osplit, p.dsplit) > 1 else "tiled")


@functools.lru_cache(maxsize=None)
def _references(name, big_batch):
    """(pick, fp64 rows, yardstick) of a case's sampled sequences: computed once on the CPU, never from the GPU."""
    from hiprag import EncoderConfig, random_state
    case = CASES[name]
    cfg = EncoderConfig(**case["cfg"])
    toks = ec.model_tokens(case)
    pick = list(range(len(toks))) if case["sample"] is None else list(case["sample"])
    sub = [toks[i] for i in pick]
    args = (eo.bf16_round_state(random_state(cfg, seed=case["seed"], std=case["std"])), sub, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps)
    ref = eo.xlmr_hidden_f64(*args)
    sim = eo.xlmr_hidden_bf16sim(*args, big_batch=big_batch)
    yard = max(float(eo.row_rel_err(sim[j, :len(t)], ref[j, :len(t)]).max()) for j, t in enumerate(sub))
    return pick, ref, yard


@pytest.mark.parametrize("name", list(CASES))
def test_every_packed_hidden_row_against_fp64_and_the_padded_entry(gpu, monkeypatch, name):
    import torch
    from hiprag import EncoderConfig, HipEncoder, random_state
    case = CASES[name]
    cfg = EncoderConfig(**case["cfg"])
    _set_env(monkeypatch, case["env"])
    toks = ec.model_tokens(case)
    lens = [len(t) for t in toks]
    enc = HipEncoder(cfg, random_state(cfg, seed=case["seed"], std=case["std"]))
    p1, p2, agree = _plans(enc, lens)
    assert _path_name(p1) == case["path"], (name, _path_name(p1))
    if name == "big_packed_h1024":
        assert (p2.T, p2.path, p2.M) == (17344, 1, 17408)          # the 256-tile path, its last row tile part padding
    if name in ("small_h256", "tiled_h256"):
        assert (p1.T, p2.T) == (1536, 768) and agree                # so the bit-equality branch cannot be skipped everywhere
    if name == "big_packed_h1024":
        assert agree
    hid = enc.hidden_tokens(toks, packed=True, max_tokens=1 << 20)                 # ONE packed batch
    assert enc.packed_info() == (p2.T, sum(lens), len(toks), p2.path)
    assert all(h.shape == (len(t), cfg.hidden) and np.all(np.isfinite(h)) for h, t in zip(hid, toks))
    H, F = cfg.hidden, cfg.ffn
    flops = sum(lens) * cfg.layers * (8.0 * H * H + 4.0 * H * F) + cfg.layers * 4.0 * sum((-(-n // 64) * 64) ** 2 for n in lens) * H
    assert enc.last_flops() == flops

    pick, ref, yard = _references(name, p2.path == 1)
    assert 0 in pick and len(toks) - 1 in pick
    bar = ec.YARDSTICK_FACTOR * yard
    worst, where = 0.0, None
    for j, i in enumerate(pick):
        err = eo.row_rel_err(torch.from_numpy(hid[i]).double(), ref[j, :len(toks[i])])
        if float(err.max()) > worst:
            worst, where = float(err.max()), (i, len(toks[i]), int(err.argmax()))
    branch = "bit for bit against the padded entry" if agree else "plans differ: the fp64 bar alone"
    print(f"\n[packed hidden rows {name}: padded {_path_name(p1)} {p1.T} rows ({p1.osplit}, {p1.dsplit}), packed {_path_name(p2)} "
          f"{p2.T} rows ({p2.osplit}, {p2.dsplit}): {branch}] GPU worst row {worst:.3e} at (seq, len, row) {where}; "
          f"bf16-sim yardstick {yard:.3e}, bar {bar:.3e}")
    assert worst <= bar, (name, worst, bar, where)
    if agree:
        padded = enc.hidden_tokens(toks, batch_size=len(toks))
        for i, (a, b) in enumerate(zip(hid, padded)):
            assert np.array_equal(a, b), (name, i, len(toks[i]))
    # the packed CLS row, normalised as pool_kernel does it, IS encode_tokens(packed=True): bit for bit
    emb = enc.encode_tokens(toks, packed=True, max_tokens=1 << 20).cpu().numpy()
    for i in pick:
        assert np.array_equal(emb[i], _pool_reference(hid[i][0])), (name, i)
    again = enc.hidden_tokens(toks, packed=True, max_tokens=1 << 20)
    assert all(np.array_equal(a, b) for a, b in zip(hid, again))


# ---- embeddings, logits, batches ----------------------------------------------------------------------------------------
def _tokens(rng, lens, vocab):
    return [([0] + rng.integers(3, vocab, size=max(0, n - 2)).tolist() + [2])[:max(n, 0)] if n > 0 else [] for n in lens]


def test_packed_embeddings_empty_sequences_and_batching(gpu, monkeypatch):
    from hiprag import EncoderConfig, HipEncoder, random_state
    _set_env(monkeypatch, {})
    cfg = EncoderConfig(vocab=1000, hidden=256, layers=3, heads=4, ffn=512, max_pos=300)
    lens = [0, 9, 33, 70, 0, 4, 120, 64, 18, 0]
    toks = _tokens(np.random.default_rng(5), lens, cfg.vocab)
    enc = HipEncoder(cfg, random_state(cfg, seed=5))
    padded = enc.encode_tokens(toks, batch_size=256).cpu().numpy()
    packed = enc.encode_tokens(toks, packed=True).cpu().numpy()
    hid = enc.hidden_tokens(toks, packed=True)
    for i, n in enumerate(lens):
        if n == 0:
            assert np.all(packed[i] == 0) and hid[i].shape == (0, cfg.hidden)
        else:
            assert np.array_equal(packed[i], _pool_reference(hid[i][0])), i
    assert np.allclose(packed, padded, atol=2e-3)           # the bar of test_batching_does_not_change_results
    # input-order batches cut by packed rows: 64 | 64 + 128 (the next would pass 192) | ...
    cut = enc.encode_tokens(toks, packed=True, max_tokens=192).cpu().numpy()
    assert enc.packed_info()[2] < len(toks) and np.allclose(cut, padded, atol=2e-3)
    assert np.all(cut[[0, 4, 9]] == 0)


def test_packed_logits_against_the_oracle_and_the_padded_entry(gpu, monkeypatch):
    from hiprag import EncoderConfig, HipEncoder, random_state
    cfg = EncoderConfig(vocab=1000, hidden=256, layers=2, heads=4, ffn=1024, max_pos=300)
    sd = random_state(cfg, seed=7, with_head=True)
    lens = [20, 50, 7, 100]
    toks = _tokens(np.random.default_rng(7), lens, cfg.vocab)
    ref = eo.rerank_logits_fp32(eo.bf16_round_state(sd), toks, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps)
    took = []
    for env in ({}, {"HIPENC_SMALL_ROWS": "0"}):
        _set_env(monkeypatch, env)
        enc = HipEncoder(cfg, sd, with_head=True)
        p1, p2, agree = _plans(enc, lens)
        got = enc.score_tokens(toks, packed=True).cpu().numpy()
        print(f"\n[packed reranker head, padded {_path_name(p1)} / packed {_path_name(p2)}] max |logit delta| {np.abs(got - ref).max():.3e}")
        assert np.allclose(got, ref, atol=RERANK_ATOL), (got, ref)
        padded = enc.score_tokens(toks, batch_size=len(toks)).cpu().numpy()
        assert np.allclose(got, padded, atol=RERANK_ATOL)
        if agree:
            assert np.array_equal(got, padded)
        took.append(agree)
    assert took[1], "with the small-batch path off both batches take 128-tiles with the same splits"


def test_a_packed_result_does_not_depend_on_the_batch(gpu, monkeypatch):
    """One sequence in two different batches of equal plan: identical bits, wherever its rows start."""
    from hiprag import EncoderConfig, HipEncoder, random_state
    from hiprag.encoder import forward_plan, packed_layout
    case = ec.MODEL_CASES["tiled_h256"]
    _set_env(monkeypatch, case["env"])
    cfg = EncoderConfig(**case["cfg"])
    enc = HipEncoder(cfg, random_state(cfg, seed=case["seed"], std=case["std"]))
    toks = ec.model_tokens(case)                       # lens 200, 129, 65, 64, 16, 1
    x = toks[1]
    a, b = [x, toks[0], toks[4]], [toks[2], toks[5], x, toks[3], toks[0]]
    plans = [forward_plan(enc.shape(), 1, packed_layout([len(t) for t in batch])[1]) for batch in (a, b)]
    assert plans[0].T != plans[1].T
    assert len({(p.path, p.osplit, p.dsplit) for p in plans}) == 1
    ha, hb = enc.hidden_tokens(a, packed=True), enc.hidden_tokens(b, packed=True)
    assert np.array_equal(ha[0], hb[2]) and np.array_equal(ha[1], hb[4])
    ea, eb = enc.encode_tokens(a, packed=True).cpu().numpy(), enc.encode_tokens(b, packed=True).cpu().numpy()
    assert np.array_equal(ea[0], eb[2])


# ---- checks ---------------------------------------------------------------------------------------------------------------
def test_packed_entries_refuse_bad_batches_and_leave_the_outputs_alone(gpu, monkeypatch):
    import torch
    from hiprag import EncoderConfig, HipEncoder, HipRagError, random_state, _native as nat
    _set_env(monkeypatch, {})
    cfg = EncoderConfig(vocab=100, hidden=128, layers=1, heads=2, ffn=128, max_pos=40)
    enc = HipEncoder(cfg, random_state(cfg, seed=3, with_head=True), with_head=True)
    bare = HipEncoder(cfg, random_state(cfg, seed=3))
    dev = torch.device("cuda", 0)
    out = torch.full((4, cfg.hidden), 5.0, dtype=torch.float32, device=dev)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    tok, off = i32([0, 5, 2, 0, 6, 7, 2]), i32([0, 3, 7])

    def call(fn, h, t, o, n, dst):
        nat.call(fn, h, None if t is None else t.ctypes.data, None if o is None else o.ctypes.data, n, dst, None)

    entries = ("hipenc_forward_packed", "hipenc_score_pairs_packed", "hipenc_forward_hidden_packed")
    for fn in entries:
        for t, o, n, dst in ((None, off, 2, out.data_ptr()), (tok, None, 2, out.data_ptr()), (tok, off, 2, None),      # null pointers
                             (tok, off, -1, out.data_ptr()),                                                          # nseq < 0
                             (tok, i32([1, 3, 7]), 2, out.data_ptr()),                                                # offsets start at 0
                             (tok, i32([0, 5, 3]), 2, out.data_ptr()),                                                # ... and do not descend
                             (i32([0, 100, 2, 0, 6, 7, 2]), off, 2, out.data_ptr()),                                  # id = vocab
                             (i32([0, -1, 2, 0, 6, 7, 2]), off, 2, out.data_ptr()),                                   # id < 0
                             (i32([5] * 38), i32([0, 38]), 1, out.data_ptr())):                                       # 38 + pad_id + 1 = max_pos
            with pytest.raises(HipRagError) as e:
                call(fn, enc._h, t, o, n, dst)
            assert e.value.code == -1, (fn, n, str(e.value))                                                          # HIPRAG_E_INVALID
        with pytest.raises(HipRagError) as e:
            call(fn, 987654321, tok, off, 2, out.data_ptr())                                                          # unknown handle
        assert e.value.code == -3
    call("hipenc_forward_packed", enc._h, i32([5] * 37), i32([0, 37]), 1, out.data_ptr())                             # the longest that fits
    out.fill_(5.0)
    with pytest.raises(HipRagError):
        call("hipenc_score_pairs_packed", enc._h, tok, i32([0, 3, 3, 7]), 3, out.data_ptr())                         # an empty pair
    with pytest.raises(HipRagError):
        call("hipenc_score_pairs_packed", bare._h, tok, off, 2, out.data_ptr())                                      # no head
    # 2^24 one-token sequences are 2^30 packed rows
    many = 1 << 24
    with pytest.raises(HipRagError):
        call("hipenc_forward_packed", enc._h, np.full(many, 5, dtype=np.int32), np.arange(many + 1, dtype=np.int32), many, out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()), "a refused call wrote to its output"

    # nseq = 0 and an all-empty batch succeed; the latter writes zeros and runs no GEMM
    for fn in entries:
        call(fn, enc._h, None, None, 0, None)
    assert bool((out == 5.0).all())
    call("hipenc_forward_packed", enc._h, None, i32([0, 0, 0]), 2, out.data_ptr())
    call("hipenc_forward_hidden_packed", enc._h, None, i32([0, 0, 0]), 2, out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out[:2] == 0).all()) and bool((out[2:] == 5.0).all())
    assert enc.packed_info() == (0, 0, 2, -1) and enc.last_flops() == 0.0
    v = (ctypes.c_int64 * 4)()
    with pytest.raises(HipRagError):
        nat.call("hipenc_packed_info", 987654321, v)
    with pytest.raises(HipRagError):
        nat.call("hipenc_packed_info", enc._h, None)
