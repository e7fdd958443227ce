"""
GPU: the encoder's attention kernel alone, and EVERY hidden row of whole models with peaked attention, against float64.

tests/test_encoder_gpu.py sees the encoder through one normalised CLS row per sequence of a model whose softmax is almost
uniform (weights of std 0.02); DESIGN.md ("How the encoder is tested") lists wrong attentions that pass there.  Here:

  * attention2_kernel through hipenc_attention -- the launch helper the forward uses -- on every query row, head and column
    against oracle.encoder_oracle.attention_f64, within a bound DERIVED from the two bf16 roundings the kernel has
    (oracle.encoder_cases.attention_bound), at S in {64, 128, 192, 512}, every length that crosses a wave, a key tile or a
    query tile, five score regimes, finite poison behind the lengths, twice for identical bits;
  * HipEncoder.hidden_tokens (hipenc_forward_hidden) on every path the forward can take, weights drawn wide enough for a
    peaked softmax, every real row within 3 x the worst row of the bf16 emulation xlmr_hidden_bf16sim -- a yardstick
    recomputed on the CPU for each case, never taken from the GPU.

tests/test_encoder_reference_cpu.py shows on the CPU that wrong forwards miss these bars by >= 3 x.  Every case prints
what it measured beside its bound.
"""
import numpy as np
import pytest

from oracle import encoder_cases as ec
from oracle import encoder_oracle as eo

pytestmark = pytest.mark.gpu


def _attention(case, fill=7.0):
    """-> ctx bf16 [nseq, S, heads * 64] on the host.  ctx starts out non-zero: the entry has to zero-fill it itself."""
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    dev = torch.device("cuda", 0)
    q, k, vt = (case[n].to(dev).contiguous() for n in ("q", "k", "vt"))
    lens = torch.from_numpy(case["lens"]).to(dev)
    nseq, heads, S, _ = q.shape
    assert int(case["lens"].min()) >= 0 and int(case["lens"].max()) <= S          # the entry's precondition
    ctx = torch.full((nseq, S, heads * 64), fill, dtype=torch.bfloat16, device=dev)
    nat.call("hipenc_attention", q.data_ptr(), k.data_ptr(), vt.data_ptr(), lens.data_ptr(), ctx.data_ptr(), nseq, S, heads,
             _stream_ptr())
    torch.cuda.synchronize()
    return ctx.cpu()


@pytest.mark.parametrize("S", ec.ATT_S)
@pytest.mark.parametrize("regime", ec.ATT_REGIMES)
def test_attention_kernel_every_row_against_fp64(gpu, regime, S):
    """|ctx_gpu - ctx_ref| <= u (A + |ctx_ref|) (1 + 2^-6) + 1e-6 with u = 2^-8 and A = sum_j p_j |v_j|, element-wise, from
    the reference alone: q, k, v are bf16-exact and their products exact in fp32, so the kernel's only bf16 roundings are the
    probabilities in front of P.V (the row sum adds the unrounded ones) and the output."""
    import torch
    case = ec.attention_case(regime, S)
    got = _attention(case)
    ref, A = eo.attention_f64(case["q"], case["k"], case["vt"], case["lens"])
    bound = ec.attention_bound(ref, A)
    worst, where = 0.0, None
    for i, n in enumerate(case["lens"].tolist()):
        g = got[i].double()
        assert bool(torch.isfinite(g).all()), (regime, S, n)
        tile_end = -(-n // 128) * 128
        assert bool((g[tile_end:] == 0).all()), (regime, S, n, "rows of query tiles wholly beyond len must be zero")
        if n == 0:
            continue
        ratio = ((g[:n] - ref[i, :n]).abs() / bound[i, :n])
        if float(ratio.max()) > worst:
            worst, where = float(ratio.max()), (n, int(ratio.argmax()) // ratio.shape[1], int(ratio.argmax()) % ratio.shape[1])
    print(f"\n[attention {regime} S={S}] worst |err| / bound {worst:.3f} at (len, row, col) {where}; "
          f"lens {case['lens'].tolist()}")
    assert worst <= 1.0, (regime, S, worst, where)
    again = _attention(case, fill=-3.0)
    assert torch.equal(again.view(torch.int16), got.view(torch.int16))           # identical bits, whatever ctx held before


def test_attention_entry_validates_its_arguments(gpu):
    import torch
    from hiprag import HipRagError, _native as nat
    dev = torch.device("cuda", 0)
    t = torch.zeros((1, 1, 64, 64), dtype=torch.bfloat16, device=dev)
    lens = torch.ones(1, dtype=torch.int32, device=dev)
    ctx = torch.zeros((64, 64), dtype=torch.bfloat16, device=dev)
    ok = dict(q=t.data_ptr(), k=t.data_ptr(), vt=t.data_ptr(), lens=lens.data_ptr(), ctx=ctx.data_ptr(), nseq=1, S=64, heads=1)
    for bad in (dict(q=None), dict(k=None), dict(vt=None), dict(lens=None), dict(ctx=None), dict(S=0), dict(S=96), dict(S=-64),
                dict(nseq=0), dict(heads=0)):
        a = dict(ok, **bad)
        with pytest.raises(HipRagError):
            nat.call("hipenc_attention", a["q"], a["k"], a["vt"], a["lens"], a["ctx"], a["nseq"], a["S"], a["heads"], None)


# ---- whole model, every row -----------------------------------------------------------------------------------------
def _pool_reference(cls_row):
    """pool_kernel's arithmetic on one bf16 CLS row (as float32), operation for operation: lane-strided sums of squares
    (exact products: bf16 x bf16 fits fp32), the xor-butterfly of wave_sum, one correctly rounded sqrt and division."""
    v = cls_row.astype(np.float32)
    lanes = np.zeros(64, dtype=np.float32)
    for r in v.reshape(-1, 64):
        lanes = lanes + r * r
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ off]
    inv = np.float32(1.0) / np.maximum(np.sqrt(lanes[0]), np.float32(1e-12))
    return v * inv


@pytest.mark.parametrize("name", list(ec.MODEL_CASES))
def test_every_hidden_row_against_fp64_with_peaked_attention(gpu, monkeypatch, name):
    import torch
    from hiprag import EncoderConfig, HipEncoder, random_state
    case = ec.MODEL_CASES[name]
    cfg = EncoderConfig(**case["cfg"])
    for var in ("HIPENC_SMALL_ROWS", "HIPENC_GEMM256"):
        monkeypatch.delenv(var, raising=False)
    for var, val in case["env"].items():
        monkeypatch.setenv(var, val)
    toks = ec.model_tokens(case)
    # the path this case is meant for is the path its sizes and switches select (one batch: all sequences together)
    rows = len(toks) * (-(-max(len(t) for t in toks) // 64) * 64)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    path = ec.forward_path(cfg.hidden, cfg.ffn, rows, int(case["env"].get("HIPENC_SMALL_ROWS", 384)), True, n_cu)
    assert path == case["path"], (name, path, rows, n_cu)
    if name == "big_h1024":
        assert rows % 256 != 0                     # the last 256-row tile is part padding

    sd = random_state(cfg, seed=case["seed"], std=case["std"])
    enc = HipEncoder(cfg, sd)
    # ... and it is the path the library itself plans for this handle: the shape it read at creation, the same batch
    from hiprag.encoder import forward_plan
    shape = enc.shape()
    assert (shape.hidden, shape.ffn, shape.n_cu, shape.small_rows, shape.use256) == \
        (cfg.hidden, cfg.ffn, n_cu, int(case["env"].get("HIPENC_SMALL_ROWS", 384)), 1)
    p = forward_plan(shape, len(toks), rows // len(toks))
    lib_path = {0: "small", 1: "big"}.get(p.path) or ("tiled_splitk" if max(p.osplit, p.dsplit) > 1 else "tiled")
    assert p.T == rows and lib_path == case["path"], (name, lib_path, p.osplit, p.dsplit)
    hid = enc.hidden_tokens(toks, batch_size=len(toks))
    assert all(h.shape == (len(t), cfg.hidden) and np.all(np.isfinite(h)) for h, t in zip(hid, toks))

    pick = list(range(len(toks))) if case["sample"] is None else list(case["sample"])
    assert 0 in pick and len(toks) - 1 in pick
    sub = [toks[i] for i in pick]
    args = (eo.bf16_round_state(sd), sub, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps)
    ref = eo.xlmr_hidden_f64(*args)
    sim = eo.xlmr_hidden_bf16sim(*args, big_batch=(path == "big"))
    yard = max(float(eo.row_rel_err(sim[j, :len(t)], ref[j, :len(t)]).max()) for j, t in enumerate(sub))
    bar = ec.YARDSTICK_FACTOR * yard
    worst, where = 0.0, None
    for j, i in enumerate(pick):
        err = eo.row_rel_err(torch.from_numpy(hid[i]).double(), ref[j, :len(toks[i])])
        if float(err.max()) > worst:
            worst, where = float(err.max()), (i, len(toks[i]), int(err.argmax()))
    print(f"\n[hidden rows {name}: path {path}, {rows} rows] GPU worst row {worst:.3e} at (seq, len, row) {where}; "
          f"bf16-sim yardstick {yard:.3e}, bar {bar:.3e}")
    assert worst <= bar, (name, worst, bar, where)

    # the CLS row of hidden_tokens, normalised as pool_kernel does it, IS encode_tokens: bit for bit
    emb = enc.encode_tokens(toks, batch_size=len(toks)).cpu().numpy()
    for i in pick:
        assert np.array_equal(emb[i], _pool_reference(hid[i][0])), (name, i)
    again = enc.hidden_tokens(toks, batch_size=len(toks))
    assert all(np.array_equal(a, b) for a, b in zip(hid, again))


def test_hidden_tokens_restores_input_order_across_batches(gpu, monkeypatch):
    """Length-sorted batches of two: every sequence comes back at its own index with its own length, holding exactly the rows
    that the same pair gives when it is run on its own (no tolerance: the forward has no atomics)."""
    from hiprag import EncoderConfig, HipEncoder, random_state
    for var in ("HIPENC_SMALL_ROWS", "HIPENC_GEMM256"):
        monkeypatch.delenv(var, raising=False)
    case = ec.MODEL_CASES["tiled_h256"]
    cfg = EncoderConfig(**case["cfg"])
    toks = ec.model_tokens(case)[::-1] + [[0, 7, 2]]          # shortest first, so the sort has something to undo
    enc = HipEncoder(cfg, random_state(cfg, seed=case["seed"], std=case["std"]))
    got = enc.hidden_tokens(toks, batch_size=2)
    order = sorted(range(len(toks)), key=lambda i: -len(toks[i]))
    for o in range(0, len(toks), 2):
        pair = order[o:o + 2]
        alone = enc.hidden_tokens([toks[i] for i in pair], batch_size=2)
        for i, a in zip(pair, alone):
            assert got[i].shape == (len(toks[i]), cfg.hidden) and np.array_equal(got[i], a), i
