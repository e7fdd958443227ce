"""
GPU parity of the MFMA encoder (hipenc_*) against the fp32 oracle on the SAME bf16-rounded weights.
Tolerance (bf16 operands, fp32 accumulation), derived from what the 24-layer H = 1024 case measures on MI355X
(tests/test_configs_gpu.py prints it: min cosine 0.999946, largest element error 0.037 / sqrt(H)): cosine >= 0.9998 per
embedding, i.e. ||gpu - ref|| <= 2e-2 on the unit-norm outputs, and max |diff| <= 0.1 / sqrt(H) per element; reranker
logits within 1.5e-2 absolute.  Each case prints what it measured.  The retrieval ids computed FROM these embeddings are then
exact (dense search is bit-exact for whatever vectors it is given).

What these whole-model cases see: ONE row per sequence, the normalised CLS row, of models whose weights all have std 0.02.
That exercises the GEMMs and their epilogues, the LayerNorms, the embedding and the pooling.  It does NOT validate the
attention kernel: at this scale the softmax is almost uniform (largest probability ~0.013 at H = 256), and only query row 0
of the last layer reaches the output -- a uniform softmax, a missed rescale between key tiles or zeroed non-CLS rows pass
these bars ("How the encoder is tested").  The attention kernel and every hidden row are checked against fp64 in
tests/test_encoder_kernels_gpu.py.
"""
import numpy as np
import pytest

from oracle import encoder_oracle as eo

pytestmark = pytest.mark.gpu
MIN_COS = 0.9998
MAX_ABS_SQRT_H = 0.1
RERANK_ATOL = 1.5e-2


def _tokens(rng, lens, vocab):
    return [([0] + rng.integers(3, vocab, size=max(0, n - 2)).tolist() + [2])[:max(n, 0)] if n > 0 else [] for n in lens]


def _check(cfg, lens, seed, with_head=False, batch_size=256):
    import torch
    from hiprag import HipEncoder, random_state
    sd = random_state(cfg, seed=seed, with_head=with_head)
    enc = HipEncoder(cfg, sd, with_head=with_head)
    rng = np.random.default_rng(seed)
    toks = _tokens(rng, lens, cfg.vocab)
    got = enc.encode_tokens(toks, batch_size=batch_size).cpu().numpy()
    ref = eo.embed_fp32(eo.bf16_round_state(sd), toks, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps)
    worst_cos, worst_abs = 1.0, 0.0
    for i, t in enumerate(toks):
        if len(t) == 0:
            assert np.all(got[i] == 0)
            continue
        cos = float(np.dot(got[i], ref[i]))
        worst_cos, worst_abs = min(worst_cos, cos), max(worst_abs, float(np.max(np.abs(got[i] - ref[i]))))
        assert cos >= MIN_COS, (i, len(t), cos)
        assert np.max(np.abs(got[i] - ref[i])) <= MAX_ABS_SQRT_H / np.sqrt(cfg.hidden)
        assert abs(np.linalg.norm(got[i]) - 1.0) < 1e-3
    print(f"\n[encoder H={cfg.hidden} L={cfg.layers}] min cosine {worst_cos:.6f}  max |delta| {worst_abs:.3e} "
          f"= {worst_abs * np.sqrt(cfg.hidden):.3f} / sqrt(H)")
    return enc, sd, toks, got, ref


def test_small_config_mixed_lengths(gpu):
    from hiprag import EncoderConfig
    cfg = EncoderConfig(vocab=1000, hidden=256, layers=2, heads=4, ffn=1024, max_pos=600, max_seq_len=512)
    _check(cfg, [16, 64, 128, 5, 1, 2, 65, 200, 0, 63, 127, 129], seed=1)


def test_large_width_two_layers_512_tokens(gpu):
    from hiprag import EncoderConfig
    cfg = EncoderConfig(vocab=5000, hidden=1024, layers=2, heads=16, ffn=4096, max_pos=600, max_seq_len=512)
    _check(cfg, [512, 512, 17, 300], seed=2)


def test_batching_does_not_change_results(gpu):
    from hiprag import EncoderConfig
    cfg = EncoderConfig(vocab=1000, hidden=256, layers=3, heads=4, ffn=512, max_pos=300)
    lens = [9, 33, 70, 4, 120, 64, 18]
    enc, sd, toks, got, _ = _check(cfg, lens, seed=5, batch_size=256)
    again = enc.encode_tokens(toks, batch_size=2).cpu().numpy()
    assert np.allclose(got, again, atol=2e-3)          # same kernels, different padding: only rounding-order noise


def test_small_batch_gemm_path_matches_tiled_path_and_oracle(gpu, monkeypatch):
    """The single-query latency path (weight-streaming GEMMs with split-K partials summed in the LayerNorm, rows <=
    HIPENC_SMALL_ROWS) against the 128x128-tile path on the same inputs, and both against the fp32 oracle."""
    from hiprag import EncoderConfig, HipEncoder, random_state
    for cfg, lens in [(EncoderConfig(vocab=3000, hidden=1024, layers=2, heads=16, ffn=4096, max_pos=300), [12, 40, 64, 100, 1, 129]),
                      (EncoderConfig(vocab=1000, hidden=384, layers=2, heads=6, ffn=1536, max_pos=300), [7, 64, 65, 130, 200])]:
        monkeypatch.setenv("HIPENC_SMALL_ROWS", "1024")
        enc, sd, toks, small, ref = _check(cfg, lens, seed=11, batch_size=4)          # T <= 4 * 256 rows: the small path
        # (rows 64..1024: one and two column tiles per wave, one and several row blocks per workgroup)
        one = enc.encode_tokens(toks[:1], batch_size=1).cpu().numpy()                  # one query alone
        monkeypatch.setenv("HIPENC_SMALL_ROWS", "0")
        tiled = HipEncoder(cfg, sd).encode_tokens(toks, batch_size=4).cpu().numpy()
        assert np.allclose(small, tiled, atol=2e-3)
        assert np.allclose(one[0], small[0], atol=2e-3)
        again = enc.encode_tokens(toks, batch_size=4).cpu().numpy()
        assert np.array_equal(again, small)                                            # no atomics: run-to-run identical


def test_reranker_head_logits(gpu):
    from hiprag import EncoderConfig
    cfg = EncoderConfig(vocab=1000, hidden=256, layers=2, heads=4, ffn=1024, max_pos=300)
    enc, sd, toks, _, _ = _check(cfg, [20, 50, 7, 100], seed=7, with_head=True)
    got = enc.score_tokens(toks).cpu().numpy()
    ref = eo.rerank_logits_fp32(eo.bf16_round_state(sd), toks, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps)
    print(f"\n[reranker head] max |logit delta| {np.abs(got - ref).max():.3e}")
    assert np.allclose(got, ref, atol=RERANK_ATOL), (got, ref)
    assert np.array_equal(np.argsort(-got), np.argsort(-ref)) or np.max(np.abs(np.sort(ref)[1:] - np.sort(ref)[:-1])) < 2 * RERANK_ATOL


def test_bad_inputs_raise(gpu):
    from hiprag import EncoderConfig, HipEncoder, HipRagError
    with pytest.raises(HipRagError):
        HipEncoder(EncoderConfig(vocab=100, hidden=200, layers=1, heads=3, ffn=256, max_pos=64))      # hidden % 128
    cfg = EncoderConfig(vocab=100, hidden=128, layers=1, heads=2, ffn=128, max_pos=40)
    enc = HipEncoder(cfg)
    with pytest.raises(HipRagError):
        enc.encode_tokens([[0, 500, 2]])                 # token id outside the vocabulary
    with pytest.raises(HipRagError):
        enc.encode_tokens([[0] + [5] * 60 + [2]])        # longer than the position table
    with pytest.raises(ValueError):
        enc.score_tokens([[0, 5, 2]])                    # no classification head


def _linear(epi, impl, a, w, bias, resid=None, S=64, heads=16):
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr as sp
    M, K = a.shape
    N = w.shape[0]
    dev = a.device
    if epi == 0:
        q = torch.zeros((M // S, heads, S, 64), dtype=torch.bfloat16, device=dev)
        k = torch.zeros_like(q)
        vt = torch.zeros((M // S, heads, 64, S), dtype=torch.bfloat16, device=dev)
        nat.call("hipenc_linear", a.data_ptr(), w.data_ptr(), bias.data_ptr(), M, N, K, 0, None, q.data_ptr(), k.data_ptr(),
                 vt.data_ptr(), S, heads, impl, sp())
        return q, k, vt
    out = torch.zeros((M, N), dtype=torch.float32 if epi == 2 else torch.bfloat16, device=dev)
    nat.call("hipenc_linear", a.data_ptr(), w.data_ptr(), bias.data_ptr(), M, N, K, epi,
             resid.data_ptr() if resid is not None else None, out.data_ptr(), None, None, 0, 0, impl, sp())
    return (out,)


@pytest.mark.parametrize("epi,N,K", [(0, 3072, 1024), (1, 4096, 1024), (2, 1024, 4096), (3, 1024, 1024)])
def test_linear_layers_both_tiled_kernels_against_fp32_reference(gpu, epi, N, K):
    """hipenc_linear: the 128 x 128 kernel and the persistent 256 x 256 ping-pong kernel (csrc/gemm256.h) on the encoder's
    four layer shapes with their fused epilogues -- QKV scatter (q scaled, head-major q / k, TRANSPOSED v through the
    swapped-role tiles), exact GELU, bias + residual in fp32 and in bf16 -- against an fp32 torch reference on the same bf16
    operands, and against each other BIT FOR BIT (same ascending-k fp32 accumulation).  1536 rows = 6 row tiles: more tiles
    than one pass of a small grid, partial XCD super-rows."""
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7 + epi)
    M, S, heads = 1536, 64, 16
    a = (torch.randn((M, K), generator=g, device=dev) * 0.5).to(torch.bfloat16)
    w = (torch.randn((N, K), generator=g, device=dev) * 0.03).to(torch.bfloat16)
    bias = torch.randn((N,), generator=g, device=dev) * 0.1
    resid = torch.randn((M, N), generator=g, device=dev).to(torch.bfloat16) if epi >= 2 else None
    c = a.float() @ w.float().T + bias
    if epi == 0:
        H = N // 3
        nseq = M // S
        ref = ((c[:, :H] * 0.125).view(nseq, S, heads, 64).permute(0, 2, 1, 3), c[:, H:2 * H].view(nseq, S, heads, 64).permute(0, 2, 1, 3),
               c[:, 2 * H:].view(nseq, S, heads, 64).permute(0, 2, 3, 1))
    elif epi == 1:
        ref = (torch.nn.functional.gelu(c),)
    else:
        ref = (c + resid.float(),)
    outs = {}
    for impl in ((2,) if epi == 3 else (1, 2)):
        out = _linear(epi, impl, a, w, bias, resid, S, heads)
        torch.cuda.synchronize()
        outs[impl] = out
        for o, r in zip(out, ref):
            tol = 5e-4 if epi == 2 else 2.0 ** -8          # fp32 output: accumulation-order noise over K <= 4096; bf16 outputs: one rounding
            err = ((o.float() - r).abs() / (r.abs() + 0.05)).max().item()
            assert err <= tol, (epi, impl, err)
    if len(outs) == 2:
        assert all(torch.equal(x, y) for x, y in zip(outs[1], outs[2]))


def test_residual_epilogues_of_the_256_tile_kernel_repeat_bit_exact(gpu):
    """The bias + residual epilogues of gemm256 read the residual through hand-counted `s_waitcnt vmcnt` (a count
    that also allowed for younger stores could pass with a residual load in flight -- a timing-dependent wrong row).
    16384 rows = 64 x 4 = 256 tiles, thirty launches each: the fp32 form must equal the 128-tile kernel's output bit for bit
    every time, and the bf16 form its one rounding.  The grid is min(tiles, CUs): on a 256-CU device every workgroup owns ONE
    tile here, so nothing between two tiles of a workgroup is exercised -- the capped-grid test below does that."""
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    M = 16384
    for N, K in ((1024, 1024), (1024, 4096)):
        a = (torch.randn((M, K), generator=g, device=dev) * 0.5).to(torch.bfloat16)
        w = (torch.randn((N, K), generator=g, device=dev) * 0.03).to(torch.bfloat16)
        bias = torch.randn((N,), generator=g, device=dev) * 0.1
        resid = torch.randn((M, N), generator=g, device=dev).to(torch.bfloat16)
        ref32 = _linear(2, 1, a, w, bias, resid)[0]
        ref16 = ref32.to(torch.bfloat16)
        for _ in range(30):
            assert torch.equal(_linear(2, 2, a, w, bias, resid)[0], ref32)
            assert torch.equal(_linear(3, 2, a, w, bias, resid)[0], ref16)


def test_residual_epilogues_of_the_256_tile_kernel_many_tiles_per_workgroup_bit_exact(gpu):
    """The same check with MANY tiles per workgroup on any device: hipenc_linear_ex caps the persistent grid, so 2048 rows = 32
    tiles are walked by 4 workgroups (8 tiles each, XCD order off) and by 8 (4 each, XCD order on).  Between two tiles the
    residual loads and stores of one epilogue are followed at once by the next tile's staging stream and its counted waits."""
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr as sp
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(98)
    M = 2048
    for N, K in ((1024, 1024), (1024, 4096)):
        a = (torch.randn((M, K), generator=g, device=dev) * 0.5).to(torch.bfloat16)
        w = (torch.randn((N, K), generator=g, device=dev) * 0.03).to(torch.bfloat16)
        bias = torch.randn((N,), generator=g, device=dev) * 0.1
        resid = torch.randn((M, N), generator=g, device=dev).to(torch.bfloat16)
        ref32 = _linear(2, 1, a, w, bias, resid)[0]
        ref16 = ref32.to(torch.bfloat16)
        for cap in (4, 8):
            for _ in range(30):
                for epi, ref in ((2, ref32), (3, ref16)):
                    out = torch.zeros((M, N), dtype=ref.dtype, device=dev)
                    nat.call("hipenc_linear_ex", a.data_ptr(), w.data_ptr(), bias.data_ptr(), M, N, K, epi, resid.data_ptr(),
                             out.data_ptr(), None, None, 0, 0, 2, M, 0, cap, None, sp())
                    assert torch.equal(out, ref), (N, K, cap, epi)


def test_big_batch_path_with_padded_row_tiles_and_masks(gpu, monkeypatch):
    """261 x 64-token rows = 16704 token rows: enough for the persistent 256-tile GEMMs (>= 16 k rows), and NOT a multiple of
    256, so the last row tile is padding -- the QKV epilogue has to mask its scatter, the pad rows must never reach a real
    token.  Checked against the fp32 oracle on a sample of sequences (incl. the last ones) and against the 128-tile path."""
    from hiprag import EncoderConfig, HipEncoder, random_state
    cfg = EncoderConfig(vocab=3000, hidden=1024, layers=2, heads=16, ffn=4096, max_pos=100, max_seq_len=64)
    sd = random_state(cfg, seed=13)
    rng = np.random.default_rng(13)
    lens = [64] * 200 + rng.integers(3, 65, size=61).tolist()
    toks = _tokens(rng, lens, cfg.vocab)
    big = HipEncoder(cfg, sd).encode_tokens(toks, batch_size=512).cpu().numpy()
    pick = [0, 1, 199, 200, 230, 259, 260]
    ref = eo.embed_fp32(eo.bf16_round_state(sd), [toks[i] for i in pick], cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps)
    cos = np.sum(big[pick] * ref, axis=1)
    print(f"\n[big-batch path, 16704 rows] min cosine {cos.min():.6f}  max |delta| {np.abs(big[pick] - ref).max():.3e}")
    assert cos.min() >= MIN_COS and np.abs(big[pick] - ref).max() <= MAX_ABS_SQRT_H / np.sqrt(cfg.hidden)
    monkeypatch.setenv("HIPENC_GEMM256", "0")
    small_tiles = HipEncoder(cfg, sd).encode_tokens(toks, batch_size=512).cpu().numpy()
    assert np.allclose(big, small_tiles, atol=3e-3)       # bf16 pre-LN rows vs fp32 ones: rounding noise only
    assert np.all(np.isfinite(big)) and np.allclose(np.linalg.norm(big, axis=1), 1.0, atol=1e-3)
