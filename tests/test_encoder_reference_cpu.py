"""
CPU: the bars of tests/test_encoder_kernels_gpu.py can fail.  Each wrong forward below is applied to the float64 CPU
reference (oracle/encoder_oracle.py) on the inputs the GPU tests use (oracle/encoder_cases.py) and must VIOLATE the bar it
is aimed at by at least MARGIN = 3 times -- a condition, not a measurement.  The bars:
  kernel  |ctx - ctx_ref| <= attention_bound(ctx_ref, A) element-wise (derived in oracle/encoder_cases.py);
  model   per real row, ||x - x_ref|| / ||x_ref|| <= 3 * yardstick, the yardstick being the worst row of
          xlmr_hidden_bf16sim against xlmr_hidden_f64 on the same case.
Also here: the bf16 emulation stays within the old whole-model bars on the old inputs, and attention_f64 is the attention
inside xlmr_hidden_f64.
"""
import numpy as np
import pytest
import torch

from oracle import encoder_cases as ec
from oracle import encoder_oracle as eo

MARGIN = 3.0


# ---- wrong attentions: (q, k, v, lens, layer) -> ctx [n, heads, S, dh], q already scaled -------------------------------
def _probs(q, k, lens):
    S = q.shape[2]
    keep = (torch.arange(S)[None, :] < torch.as_tensor(np.asarray(lens, dtype=np.int64))[:, None])[:, None, None, :]
    s = (q @ k.transpose(-1, -2)).masked_fill(~keep, float("-inf"))
    p = torch.softmax(s, -1)
    return torch.where(torch.isnan(p), torch.zeros_like(p), p), keep        # no key at all: zeros


def uniform_softmax(q, k, v, lens, layer):
    _, keep = _probs(q, k, lens)
    p = keep.to(q.dtype).expand(q.shape[0], q.shape[1], q.shape[2], -1)
    return (p / p.sum(-1, keepdim=True).clamp_min(1)) @ v


def late_keys_double(q, k, v, lens, layer):
    """A missed rescale between key tiles: keys >= 64 weigh double."""
    p, _ = _probs(q, k, lens)
    p = p.clone()
    p[..., 64:] *= 2
    return (p / p.sum(-1, keepdim=True).clamp_min(1e-300)) @ v


def last_key_dropped(q, k, v, lens, layer):
    return _probs(q, k, [max(0, n - 1) for n in lens])[0] @ v


def pad_keys_unmasked(q, k, v, lens, layer):
    """The crossing tile's mask is missing: keys up to the next multiple of 64 take part."""
    return _probs(q, k, [-(-n // 64) * 64 for n in lens])[0] @ v


def logits_scaled(q, k, v, lens, layer):
    return _probs(q * 1.05, k, lens)[0] @ v


def no_max_subtraction_fp32(q, k, v, lens, layer):
    S = q.shape[2]
    keep = (torch.arange(S)[None, :] < torch.as_tensor(np.asarray(lens, dtype=np.int64))[:, None])[:, None, None, :]
    e = torch.exp((q.float() @ k.float().transpose(-1, -2))) * keep
    return ((e @ v.float()) / e.sum(-1, keepdim=True)).double()


def _kernel_violation(case, wrong):
    """max over the real rows of |wrong - ref| / bound; inf if the wrong result is not finite."""
    q, k, vt, lens = case["q"].double(), case["k"].double(), case["vt"].double(), case["lens"]
    ref, A = eo.attention_f64(q, k, vt, lens)
    got = wrong(q, k, vt.transpose(-1, -2), lens.tolist(), 0)
    n, h, S, dh = q.shape
    got = got.transpose(1, 2).reshape(n, S, h * dh)
    worst = 0.0
    for i, n_i in enumerate(lens):
        if n_i == 0:
            continue
        g = got[i, :n_i]
        if not bool(torch.isfinite(g).all()):
            return float("inf")
        worst = max(worst, float(((g - ref[i, :n_i]).abs() / ec.attention_bound(ref[i, :n_i], A[i, :n_i])).max()))
    return worst


@pytest.mark.parametrize("wrong,regime,S", [
    (uniform_softmax, "peaked", 128), (late_keys_double, "peaked", 192), (late_keys_double, "first_tile", 512),
    (last_key_dropped, "peaked", 192), (pad_keys_unmasked, "peaked", 192), (logits_scaled, "peaked", 512),
    (logits_scaled, "rising", 512), (no_max_subtraction_fp32, "huge", 64)])
def test_wrong_attention_violates_the_kernel_bound(wrong, regime, S):
    v = _kernel_violation(ec.attention_case(regime, S), wrong)
    print(f"\n[kernel bound] {wrong.__name__} on {regime} S={S}: {v:.1f} x the bound")
    assert v >= MARGIN
    if wrong is no_max_subtraction_fp32:
        assert v == float("inf")            # exp(80+) overflows fp32: not finite


def test_the_correct_attention_meets_the_kernel_bound_with_bf16_roundings():
    """The bound is not vacuous the other way: the reference with the kernel's two bf16 roundings (P, output) meets it."""
    for regime in ec.ATT_REGIMES:
        case = ec.attention_case(regime, 192)
        q, k, vt, lens = case["q"].double(), case["k"].double(), case["vt"].double(), case["lens"]
        ref, A = eo.attention_f64(q, k, vt, lens)
        ctx = eo.round_bf16(eo.softmax_context(q, k, vt.transpose(-1, -2), lens, eo.round_bf16)[0])
        n, h, S, dh = q.shape
        ctx = ctx.transpose(1, 2).reshape(n, S, h * dh)
        for i, n_i in enumerate(lens):
            assert bool(((ctx[i, :n_i] - ref[i, :n_i]).abs() <= ec.attention_bound(ref[i, :n_i], A[i, :n_i])).all()), (regime, n_i)


# ---- whole model -----------------------------------------------------------------------------------------------------
def _model(case_name):
    from hiprag import EncoderConfig, random_state
    case = ec.MODEL_CASES[case_name]
    cfg = EncoderConfig(**case["cfg"])
    sd = eo.bf16_round_state(random_state(cfg, seed=case["seed"], std=case["std"]))
    return cfg, sd, ec.model_tokens(case)


def _worst_row(x, ref, toks):
    return max(float(eo.row_rel_err(x[i, :len(t)], ref[i, :len(t)]).max()) for i, t in enumerate(toks))


def zero_all_but_cls_in_last_layer(layers):
    def attention(q, k, v, lens, layer):
        ctx = eo.softmax_context(q, k, v, lens)[0]
        if layer == layers - 1:
            ctx = ctx.clone()
            ctx[:, :, 1:, :] = 0
        return ctx
    return attention


@pytest.mark.parametrize("case_name,wrongs", [
    ("tiled_h256", ("uniform", "late_double", "last_dropped", "pad_unmasked", "non_cls_zeroed")),
    ("tiled_splitk_h1024", ("uniform", "late_double", "non_cls_zeroed"))])
def test_wrong_forward_violates_the_model_bar(case_name, wrongs):
    cfg, sd, toks = _model(case_name)
    args = (sd, toks, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps)
    ref = eo.xlmr_hidden_f64(*args, pad_multiple=64)
    yard = _worst_row(eo.xlmr_hidden_bf16sim(*args), ref, toks)
    bar = ec.YARDSTICK_FACTOR * yard
    table = {"uniform": uniform_softmax, "late_double": late_keys_double, "last_dropped": last_key_dropped,
             "pad_unmasked": pad_keys_unmasked, "non_cls_zeroed": zero_all_but_cls_in_last_layer(cfg.layers)}
    print(f"\n[model bar] {case_name}: yardstick {yard:.3e}, bar {bar:.3e}")
    for name in wrongs:
        err = _worst_row(eo.xlmr_hidden_f64(*args, attention=table[name], pad_multiple=64), ref, toks)
        print(f"    {name:15s} worst row {err:.3e} = {err / bar:.1f} x the bar")
        assert err >= MARGIN * bar, (name, err, bar)


def test_bf16_emulation_stays_within_the_old_whole_model_bars_on_the_old_inputs():
    """Sanity of the emulation: on the inputs of tests/test_encoder_gpu.py's H = 256 case (std 0.02) its normalised CLS rows
    meet the bars that file sets for the GPU (cosine >= 0.9998, max |delta| <= 0.1 / sqrt(H))."""
    from hiprag import EncoderConfig, random_state
    cfg = EncoderConfig(vocab=1000, hidden=256, layers=2, heads=4, ffn=1024, max_pos=600, max_seq_len=512)
    sd = eo.bf16_round_state(random_state(cfg, seed=1))
    rng = np.random.default_rng(1)
    toks = [([0] + rng.integers(3, cfg.vocab, size=max(0, n - 2)).tolist() + [2])[:n] for n in [16, 64, 128, 5, 1, 2, 65, 200, 63, 127, 129]]
    ref = eo.embed_fp32(sd, toks, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps)
    for big in (False, True):
        cls = eo.xlmr_hidden_bf16sim(sd, toks, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps, big_batch=big)[:, 0, :]
        emb = (cls / cls.norm(dim=1, keepdim=True)).numpy()
        assert np.sum(emb * ref, axis=1).min() >= 0.9998
        assert np.abs(emb - ref).max() <= 0.1 / np.sqrt(cfg.hidden)


def test_f64_forward_agrees_with_the_pinned_fp32_forward():
    cfg, sd, toks = _model("tiled_h256")
    a = eo.xlmr_hidden_f64(sd, toks, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps)
    b = eo.xlmr_hidden_fp32(sd, toks, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps).double()
    assert _worst_row(b, a, toks) < 1e-5


def test_attention_f64_is_the_attention_inside_the_f64_forward():
    cfg, sd, toks = _model("tiled_h256")
    seen = []

    def spy(q, k, v, lens, layer):
        ctx = eo.softmax_context(q, k, v, lens)[0]
        seen.append((q, k, v, lens, ctx))
        return ctx
    spied = eo.xlmr_hidden_f64(sd, toks, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps, attention=spy, pad_multiple=64)
    plain = eo.xlmr_hidden_f64(sd, toks, cfg.layers, cfg.heads, cfg.pad_id, cfg.ln_eps, pad_multiple=64)
    assert torch.equal(spied, plain) and len(seen) == cfg.layers
    for q, k, v, lens, ctx in seen:
        n, h, S, dh = q.shape
        mine, A = eo.attention_f64(q, k, v.transpose(-1, -2).contiguous(), lens)
        want = ctx.transpose(1, 2).reshape(n, S, h * dh)
        indep = (_probs(q, k, lens)[0] @ v).transpose(1, 2).reshape(n, S, h * dh)       # torch.softmax, not softmax_context
        for i, n_i in enumerate(lens):
            assert float((mine[i, :n_i] - want[i, :n_i]).abs().max()) <= 1e-12
            assert float((mine[i, :n_i] - indep[i, :n_i]).abs().max()) <= 1e-12
            assert bool((A[i, :n_i] >= mine[i, :n_i].abs() - 1e-12).all())
