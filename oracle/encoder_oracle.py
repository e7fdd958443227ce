"""
oracle/encoder_oracle.py -- fp32 CPU restatement of the XLM-RoBERTa forward the reference runs through
sentence-transformers (rag/providers/hf/embeddings.py:32-35,54,77): CLS pooling + L2 normalisation, and of
XLMRobertaForSequenceClassification's head for the reranker the reference only configures (rag/config.py:25-27).

TEST INFRASTRUCTURE ONLY (see oracle/hybrid_oracle.py header).  The third-party implementation it restates is
`transformers` (requirements.txt:29 pins >=4.37; 5.15 is installed here): tests/test_encoder_oracle.py pins this file
against transformers' own XLMRobertaModel / XLMRobertaForSequenceClassification built from a local config with the same
seeded weights.  No BGE-M3 checkpoint or tokenizer exists offline, so parity with the released model's numbers is
UNPINNED; what is pinned is the architecture's arithmetic.

The second half holds the float64 forms the encoder's kernel tests compare against: attention_f64 (the attention kernel's
layouts), xlmr_hidden_f64 (every row) and xlmr_hidden_bf16sim (the same with the GPU's bf16 stores emulated: the yardstick).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch


def _ln(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def xlmr_hidden_fp32(sd: Dict[str, torch.Tensor], token_lists: Sequence[Sequence[int]], layers: int, heads: int,
                     pad_id: int = 1, eps: float = 1e-5) -> torch.Tensor:
    """Last hidden state [n, S, H] (fp32, CPU) for right-padded sequences; padded keys are masked."""
    sd = {k: v.float() for k, v in sd.items()}
    n = len(token_lists)
    S = max(1, max(len(t) for t in token_lists))
    ids = torch.full((n, S), pad_id, dtype=torch.long)
    mask = torch.zeros((n, S), dtype=torch.bool)
    for i, t in enumerate(token_lists):
        ids[i, :len(t)] = torch.as_tensor(list(t), dtype=torch.long)
        mask[i, :len(t)] = True
    pos = torch.cumsum(mask.long(), 1) * mask.long() + pad_id          # create_position_ids_from_input_ids
    x = sd["embeddings.word_embeddings.weight"][ids] + sd["embeddings.position_embeddings.weight"][pos] + \
        sd["embeddings.token_type_embeddings.weight"][0]
    x = _ln(x, sd["embeddings.LayerNorm.weight"], sd["embeddings.LayerNorm.bias"], eps)
    H = x.shape[-1]
    dh = H // heads
    neg = torch.zeros((n, 1, 1, S))
    neg.masked_fill_(~mask[:, None, None, :], float("-inf"))
    for i in range(layers):
        p = f"encoder.layer.{i}."

        def lin(name, t):
            return t @ sd[p + name + ".weight"].T + sd[p + name + ".bias"]

        q = lin("attention.self.query", x).view(n, S, heads, dh).transpose(1, 2)
        k = lin("attention.self.key", x).view(n, S, heads, dh).transpose(1, 2)
        v = lin("attention.self.value", x).view(n, S, heads, dh).transpose(1, 2)
        att = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh) + neg, dim=-1)
        ctx = (att @ v).transpose(1, 2).reshape(n, S, H)
        x = _ln(lin("attention.output.dense", ctx) + x, sd[p + "attention.output.LayerNorm.weight"],
                sd[p + "attention.output.LayerNorm.bias"], eps)
        h = lin("intermediate.dense", x)
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        x = _ln(lin("output.dense", h) + x, sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"], eps)
    return x


def embed_fp32(sd, token_lists, layers, heads, pad_id=1, eps=1e-5) -> np.ndarray:
    """CLS pooling + L2 normalise (sentence-transformers BGE recipe); zero rows for empty inputs."""
    nonempty = [t if len(t) else [pad_id] for t in token_lists]
    cls = xlmr_hidden_fp32(sd, nonempty, layers, heads, pad_id, eps)[:, 0, :]
    out = cls / cls.norm(dim=1, keepdim=True).clamp_min(1e-12)
    for i, t in enumerate(token_lists):
        if len(t) == 0:
            out[i] = 0
    return out.numpy()


def rerank_logits_fp32(sd, token_lists, layers, heads, pad_id=1, eps=1e-5) -> np.ndarray:
    """XLMRobertaClassificationHead: out_proj(tanh(dense(cls)))."""
    cls = xlmr_hidden_fp32(sd, token_lists, layers, heads, pad_id, eps)[:, 0, :]
    sd = {k: v.float() for k, v in sd.items()}
    h = torch.tanh(cls @ sd["classifier.dense.weight"].T + sd["classifier.dense.bias"])
    return (h @ sd["classifier.out_proj.weight"].T + sd["classifier.out_proj.bias"]).reshape(-1).numpy()


def bf16_round_state(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Matrices / embedding tables as the GPU holds them (bf16), biases and LayerNorm parameters fp32."""
    out = {}
    for k, v in sd.items():
        is_mat = v.dim() == 2
        out[k] = v.to(torch.bfloat16).float() if is_mat else v.float()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references for the encoder's kernel tests (tests/test_encoder_kernels_gpu.py, tests/test_encoder_reference_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def round_bf16(t: torch.Tensor) -> torch.Tensor:
    """Round to the nearest bf16 (ties to even), keep the dtype: what one bf16 store on the GPU does to a value."""
    return t.to(torch.bfloat16).to(t.dtype)


def softmax_context(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, lens: Sequence[int],
                    round_p: Optional[Callable[[torch.Tensor], torch.Tensor]] = None):
    """Masked softmax attention in the dtype of its inputs.  q (ALREADY scaled by 1/sqrt(dh)), k, v: [n, heads, S, dh];
    keys at positions >= lens[i] are masked.  -> (ctx, A), both [n, heads, S, dh]: ctx = sum_j p_j v_j and
    A = sum_j p_j |v_j| with p the softmax probabilities.  `round_p` (the bf16 emulation) is applied to exp(s - max)
    before the product with v ONLY; the denominator sums the unrounded values, as attention2_kernel does.  Sequences of
    length 0 give zeros."""
    n, _, S, _ = q.shape
    lens_t = torch.as_tensor(np.asarray(lens, dtype=np.int64))
    keep = (torch.arange(S)[None, :] < lens_t[:, None])[:, None, None, :]
    s = (q @ k.transpose(-1, -2)).masked_fill(~keep, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))            # empty sequence: exp(-inf - 0) = 0 everywhere
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True)
    den = torch.where(den > 0, den, torch.ones_like(den))
    ctx = ((round_p(e) if round_p is not None else e) @ v) / den
    return ctx, ((e / den) @ v.abs())


def attention_f64(q, k, vt, lens):
    """fp64 reference of attention2_kernel in the kernel's own layouts: q, k [nseq, heads, S, 64] (q carries the 1/8
    scale), vt [nseq, heads, 64, S], lens [nseq].  -> (ctx, A) as float64 tensors [nseq, S, heads * 64]; A is the
    softmax-weighted mean of |v| per output element, which the kernel's error bound needs.  Query rows at positions >= len
    are returned as zeros (the kernel leaves them unspecified or zero, see include/hiprag.h)."""
    q, k, vt = (torch.as_tensor(t).to(torch.float64) for t in (q, k, vt))
    n, heads, S, dh = q.shape
    ctx, A = softmax_context(q, k, vt.transpose(-1, -2), lens)
    real = (torch.arange(S)[None, :] < torch.as_tensor(np.asarray(lens, dtype=np.int64))[:, None])[:, None, :, None]
    to_rows = lambda t: (t * real).transpose(1, 2).reshape(n, S, heads * dh)
    return to_rows(ctx), to_rows(A)


def _hidden_f64(sd, token_lists, layers, heads, pad_id, eps, rb, round_pre_ln, attention, pad_multiple):
    sd = {k: v.to(torch.float64) for k, v in sd.items()}
    n = len(token_lists)
    lens = [len(t) for t in token_lists]
    S = max(1, max(lens))
    S = -(-S // pad_multiple) * pad_multiple
    ids = torch.full((n, S), pad_id, dtype=torch.long)
    mask = torch.zeros((n, S), dtype=torch.bool)
    for i, t in enumerate(token_lists):
        ids[i, :len(t)] = torch.as_tensor(list(t), dtype=torch.long)
        mask[i, :len(t)] = True
    pos = torch.cumsum(mask.long(), 1) * mask.long() + pad_id
    x = sd["embeddings.word_embeddings.weight"][ids] + sd["embeddings.position_embeddings.weight"][pos] + \
        sd["embeddings.token_type_embeddings.weight"][0]
    x = rb(_ln(x, sd["embeddings.LayerNorm.weight"], sd["embeddings.LayerNorm.bias"], eps))
    H = x.shape[-1]
    dh = H // heads
    pre = rb if round_pre_ln else (lambda t: t)
    for i in range(layers):
        p = f"encoder.layer.{i}."

        def lin(name, t):
            return t @ sd[p + name + ".weight"].T + sd[p + name + ".bias"]

        split = lambda t: t.view(n, S, heads, dh).transpose(1, 2)
        q = rb(split(lin("attention.self.query", x)) / math.sqrt(dh))
        k = rb(split(lin("attention.self.key", x)))
        v = rb(split(lin("attention.self.value", x)))
        if attention is not None:
            ctx = attention(q, k, v, lens, i)
        else:
            ctx = softmax_context(q, k, v, lens, None if rb is _identity else rb)[0]
        ctx = rb(ctx.transpose(1, 2).reshape(n, S, H))
        x = rb(_ln(pre(lin("attention.output.dense", ctx) + x), sd[p + "attention.output.LayerNorm.weight"],
                   sd[p + "attention.output.LayerNorm.bias"], eps))
        h = lin("intermediate.dense", x)
        h = rb(0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0))))
        x = rb(_ln(pre(lin("output.dense", h) + x), sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"], eps))
    return x


def _identity(t):
    return t


def xlmr_hidden_f64(sd, token_lists, layers, heads, pad_id=1, eps=1e-5, attention=None, pad_multiple=1) -> torch.Tensor:
    """xlmr_hidden_fp32's forward in float64: last hidden state [n, S, H] of every row (rows at positions >= len are
    unspecified).  `attention(q, k, v, lens, layer) -> ctx [n, heads, S, dh]` replaces the softmax attention (q already
    scaled): the mutation tests plug wrong ones in.  `pad_multiple` rounds S up, as the GPU's 64-row padding does."""
    return _hidden_f64(sd, token_lists, layers, heads, pad_id, eps, _identity, False, attention, pad_multiple)


def xlmr_hidden_bf16sim(sd, token_lists, layers, heads, pad_id=1, eps=1e-5, big_batch=False) -> torch.Tensor:
    """The float64 forward with one round-to-nearest-even to bf16 at exactly the places where csrc/encoder.hip stores
    bf16 (read off the kernels, not off their output):
      * the embedding LayerNorm output (embed_ln_kernel);
      * q after the 1/8 scale, k and v (EPI_QKV epilogues of all three GEMM kernels);
      * the unnormalised probabilities exp(s - max) before P.V -- the row sum adds the UNROUNDED values
        (attention2_kernel: `lpart += p; pf = (bf16)p`);
      * the context (attention2_kernel's output staging);
      * the GELU output (EPI_GELU);
      * both LayerNorm outputs of a layer (layernorm_kernel / layernorm16_kernel);
      * with big_batch=True, the bias + residual sum in front of each LayerNorm (EPI_RESID16 of gemm256.h: the
        256-tile path keeps its pre-LayerNorm rows in bf16; the other paths keep them in fp32).
    Everything else (GEMM accumulation, softmax statistics, LayerNorm statistics) stays in float64, where the GPU has
    fp32.  Its distance from xlmr_hidden_f64 is the rounding noise a CORRECT implementation of this design has; the
    whole-model tests use it as their yardstick."""
    return _hidden_f64(sd, token_lists, layers, heads, pad_id, eps, round_bf16, big_batch, None, 1)


def row_rel_err(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """||got - ref|| / ||ref|| per row (last axis)."""
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1)
