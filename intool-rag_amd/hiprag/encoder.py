"""
HipEncoder -- Python handle on libhiprag's XLM-RoBERTa-shaped batch encoder (csrc/encoder.hip).

PyTorch-ROCm only HOLDS the weights (bf16 matrices, fp32 biases / LayerNorm parameters, on the GPU) and hands their
data_ptr()s to the library; every FLOP runs in hand-written HIP kernels.  Stands where the reference keeps
LangChain's HuggingFaceEmbeddings / sentence-transformers (rag/providers/hf/embeddings.py:32-35).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _native as nat


@dataclass
class EncoderConfig:
    """Defaults = XLM-RoBERTa-large, the architecture of BAAI/bge-m3 and BAAI/bge-reranker-v2-m3
    (rag/config.py:9 EMBEDDING_MODEL, :25 RERANKER_MODEL)."""
    vocab: int = 250002
    hidden: int = 1024
    layers: int = 24
    heads: int = 16
    ffn: int = 4096
    max_pos: int = 8194
    pad_id: int = 1
    ln_eps: float = 1e-5
    bos_id: int = 0
    eos_id: int = 2
    max_seq_len: int = 512


def random_state(cfg: EncoderConfig, seed: int = 0, with_head: bool = False, std: float = 0.02,
                 with_lexical: bool = False) -> Dict[str, "object"]:
    """Seeded random weights under transformers' XLM-R parameter names (no checkpoint exists offline).  `with_lexical` adds
    BGE-M3's sparse_linear.weight [1, H] / sparse_linear.bias [1], drawn after everything else (the other tensors do not
    change with it)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    H, F = cfg.hidden, cfg.ffn

    def w(*shape):
        return torch.randn(*shape, generator=g) * std

    sd = {
        "embeddings.word_embeddings.weight": w(cfg.vocab, H),
        "embeddings.position_embeddings.weight": w(cfg.max_pos, H),
        "embeddings.token_type_embeddings.weight": w(1, H),
        "embeddings.LayerNorm.weight": 1.0 + w(H),
        "embeddings.LayerNorm.bias": w(H),
    }
    for i in range(cfg.layers):
        p = f"encoder.layer.{i}."
        for name, shape in (("attention.self.query", (H, H)), ("attention.self.key", (H, H)),
                            ("attention.self.value", (H, H)), ("attention.output.dense", (H, H)),
                            ("intermediate.dense", (F, H)), ("output.dense", (H, F))):
            sd[p + name + ".weight"] = w(*shape)
            sd[p + name + ".bias"] = w(shape[0])
        for name in ("attention.output.LayerNorm", "output.LayerNorm"):
            sd[p + name + ".weight"] = 1.0 + w(H)
            sd[p + name + ".bias"] = w(H)
    if with_head:
        sd["classifier.dense.weight"] = w(H, H)
        sd["classifier.dense.bias"] = w(H)
        sd["classifier.out_proj.weight"] = w(1, H)
        sd["classifier.out_proj.bias"] = w(1)
    if with_lexical:
        sd["sparse_linear.weight"] = w(1, H)
        sd["sparse_linear.bias"] = w(1)
    return sd


def forward_plan(shape: "nat.HipEncShape", nseq: int, S: int) -> "nat.HipEncPlan":
    """hipenc_forward_plan: the forward that nseq rows of S tokens (S a multiple of 64) get from an encoder of `shape`.
    Arithmetic alone: no handle, no device."""
    p = nat.HipEncPlan()
    nat.call("hipenc_forward_plan", ctypes.byref(shape), int(nseq), int(S), ctypes.byref(p))
    return p


def packed_layout(lens: Sequence[int]):
    """hipenc_packed_layout: the layout of a PACKED batch of sequences of these lengths (csrc/encoder_packed.h).  Sequence i
    takes len_i rounded up to 64 rows (none if empty) from row_off[i] on.  -> (row_off int32 [n + 1], Tp, gran_seq int32
    [Tp / 64], items int32 [n_items, 2]): gran_seq names the sequence that owns each 64-row granule, items is the attention
    work list (sequence, 128-query tile j) for every 128 j < len, in sequence order.  Arithmetic alone: no handle, no device."""
    ln = np.ascontiguousarray(lens, dtype=np.int32).reshape(-1)
    n = int(ln.size)
    counts = np.zeros(2, dtype=np.int32)
    row_off = np.zeros(n + 1, dtype=np.int32)
    nat.call("hipenc_packed_layout", ln.ctypes.data, n, row_off.ctypes.data, None, None, counts.ctypes.data)
    gran = np.zeros(int(counts[0]) // 64, dtype=np.int32)
    items = np.zeros((int(counts[1]), 2), dtype=np.int32)
    nat.call("hipenc_packed_layout", ln.ctypes.data, n, None, gran.ctypes.data, items.ctypes.data, counts.ctypes.data)
    return row_off, int(counts[0]), gran, items


def packed_batches(lens: Sequence[int], max_tokens: Optional[int]) -> List[range]:
    """Consecutive sequences in input order, cut greedily: a batch takes the next sequence while its packed rows (every length
    rounded up to 64) stay <= max_tokens; a batch holds at least one sequence.  max_tokens None: one batch."""
    out, o, rows = [], 0, 0
    for i, n in enumerate(lens):
        r = -(-int(n) // 64) * 64
        if max_tokens is not None and i > o and rows + r > max_tokens:
            out.append(range(o, i))
            o, rows = i, 0
        rows += r
    if len(lens) > o:
        out.append(range(o, len(lens)))
    return out


class _Cfg(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("vocab", "hidden", "layers", "heads", "ffn", "max_pos", "pad_id")] + \
               [("ln_eps", ctypes.c_float)]


class _Layer(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("wqkv", "bqkv", "wo", "bo", "ln1_g", "ln1_b", "w1", "b1", "w2", "b2",
                                               "ln2_g", "ln2_b")]


class _Weights(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("word_emb", "pos_emb", "type_emb", "emb_ln_g", "emb_ln_b")] + \
               [("layers", ctypes.POINTER(_Layer))] + \
               [(n, ctypes.c_void_p) for n in ("cls_dense_w", "cls_dense_b", "cls_out_w", "cls_out_b")]


class HipEncoder:
    def __init__(self, cfg: EncoderConfig, state: Optional[Dict[str, "object"]] = None, device: int = 0, seed: int = 0,
                 with_head: bool = False):
        import torch
        self.cfg = cfg
        self.device = int(device)
        dev = torch.device("cuda", self.device)
        if state is None:
            state = random_state(cfg, seed, with_head)
        state = {k.replace("roberta.", "", 1) if k.startswith("roberta.") else k: v for k, v in state.items()}
        self._t: List["torch.Tensor"] = []     # keeps every device tensor alive for the lifetime of the handle

        def mat(t):
            t = t.detach().to(device=dev, dtype=torch.bfloat16).contiguous()
            self._t.append(t)
            return t.data_ptr()

        def vec(t):
            t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
            self._t.append(t)
            return t.data_ptr()

        layers = (_Layer * cfg.layers)()
        for i in range(cfg.layers):
            p = f"encoder.layer.{i}."
            wq, wk, wv = (state[p + f"attention.self.{n}.weight"] for n in ("query", "key", "value"))
            bq, bk, bv = (state[p + f"attention.self.{n}.bias"] for n in ("query", "key", "value"))
            L = layers[i]
            L.wqkv, L.bqkv = mat(torch.cat([wq, wk, wv], 0)), vec(torch.cat([bq, bk, bv], 0))
            L.wo, L.bo = mat(state[p + "attention.output.dense.weight"]), vec(state[p + "attention.output.dense.bias"])
            L.ln1_g, L.ln1_b = vec(state[p + "attention.output.LayerNorm.weight"]), vec(state[p + "attention.output.LayerNorm.bias"])
            L.w1, L.b1 = mat(state[p + "intermediate.dense.weight"]), vec(state[p + "intermediate.dense.bias"])
            L.w2, L.b2 = mat(state[p + "output.dense.weight"]), vec(state[p + "output.dense.bias"])
            L.ln2_g, L.ln2_b = vec(state[p + "output.LayerNorm.weight"]), vec(state[p + "output.LayerNorm.bias"])
        w = _Weights()
        w.word_emb = mat(state["embeddings.word_embeddings.weight"])
        w.pos_emb = mat(state["embeddings.position_embeddings.weight"])
        w.type_emb = mat(state["embeddings.token_type_embeddings.weight"][0])
        w.emb_ln_g, w.emb_ln_b = vec(state["embeddings.LayerNorm.weight"]), vec(state["embeddings.LayerNorm.bias"])
        w.layers = layers
        self.has_head = "classifier.dense.weight" in state
        if self.has_head:
            w.cls_dense_w, w.cls_dense_b = mat(state["classifier.dense.weight"]), vec(state["classifier.dense.bias"])
            w.cls_out_w = mat(state["classifier.out_proj.weight"].reshape(-1))
            w.cls_out_b = vec(state["classifier.out_proj.bias"].reshape(-1))
        c = _Cfg(cfg.vocab, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.pad_id, cfg.ln_eps)
        h = ctypes.c_uint64()
        nat.call("hipenc_create", ctypes.byref(c), ctypes.byref(w), self.device, ctypes.byref(h))
        self._h = h.value
        self.has_lexical = False
        if "sparse_linear.weight" in state:
            self.set_lexical_head(state["sparse_linear.weight"], state["sparse_linear.bias"],
                                  (cfg.bos_id, cfg.pad_id, cfg.eos_id, 3))     # BGE-M3's unused ids: bos, pad, eos, unk

    def set_lexical_head(self, weight, bias, unused_ids: Sequence[int] = ()) -> None:
        """hipenc_set_lexical_head: BGE-M3's sparse_linear (weight [1, H] or [H], bias [1]) and the token ids that never carry
        a lexical weight.  The tensors are kept alive with the handle; a second call replaces the head."""
        import torch
        dev = torch.device("cuda", self.device)
        wt = torch.as_tensor(weight).detach().reshape(-1).to(device=dev, dtype=torch.bfloat16).contiguous()
        bt = torch.as_tensor(bias).detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        if wt.numel() != self.cfg.hidden or bt.numel() != 1:
            raise ValueError("the lexical head is a weight of `hidden` values and one bias")
        un = np.ascontiguousarray(list(unused_ids), dtype=np.int32)
        nat.call("hipenc_set_lexical_head", self._h, wt.data_ptr(), bt.data_ptr(), un.ctypes.data if un.size else None, int(un.size))
        self._lex = (wt, bt)
        self.has_lexical = True

    def close(self) -> None:
        if getattr(self, "_h", None):
            try:
                nat.call("hipenc_destroy", self._h)
            finally:
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def dimension(self) -> int:
        return self.cfg.hidden

    @staticmethod
    def _pad(token_lists: Sequence[Sequence[int]]):
        lens = np.asarray([len(t) for t in token_lists], dtype=np.int32)
        max_len = max(1, int(lens.max()) if len(lens) else 1)
        ids = np.zeros((len(token_lists), max_len), dtype=np.int32)
        for i, t in enumerate(token_lists):
            ids[i, :len(t)] = np.asarray(t, dtype=np.int32)
        return ids, lens, max_len

    def _run(self, fn: str, token_lists: Sequence[Sequence[int]], out_cols: int, batch_size: int,
             max_tokens: Optional[int] = None):
        """Length-sorted batches (what sentence-transformers' encode does with batch_size=32); results are restored
        to input order and do not depend on the batching: padding never reaches a real token.
        `max_tokens`: form batches by PADDED TOKEN COUNT instead of sequence count -- as many of the next-longest
        sequences as fit nseq * S <= max_tokens (S = the batch's longest, rounded up to 64) and nseq <= batch_size; short
        texts then fill the GPU as well as long ones do (32 x 128 tokens is a twentieth of what one forward can take)."""
        import torch
        from .index import _stream_ptr
        n = len(token_lists)
        shape = (n, out_cols) if out_cols > 1 else (n,)
        out = torch.zeros(shape, dtype=torch.float32, device=torch.device("cuda", self.device))
        order = sorted(range(n), key=lambda i: -len(token_lists[i]))
        o = 0
        while o < n:
            take = batch_size
            if max_tokens is not None:
                s_pad = max(64, -(-len(token_lists[order[o]]) // 64) * 64)
                take = max(1, min(batch_size, max_tokens // s_pad))
            idx = order[o:o + take]
            o += take
            ids, lens, max_len = self._pad([token_lists[i] for i in idx])
            part = torch.empty((len(idx), out_cols) if out_cols > 1 else (len(idx),), dtype=torch.float32, device=out.device)
            nat.call(fn, self._h, ids.ctypes.data, lens.ctypes.data, len(idx), max_len, part.data_ptr(), _stream_ptr())
            out[torch.as_tensor(idx, device=out.device)] = part
        return out

    PACKED_MAX_TOKENS = 131072      # packed rows of one forward when max_tokens is not given

    @staticmethod
    def _concat(token_lists: Sequence[Sequence[int]]):
        lens = [len(t) for t in token_lists]
        offsets = np.zeros(len(lens) + 1, dtype=np.int32)
        np.cumsum(lens, out=offsets[1:])
        flat = np.zeros(max(1, int(offsets[-1])), dtype=np.int32)
        for t, o in zip(token_lists, offsets):
            flat[o:o + len(t)] = np.asarray(t, dtype=np.int32)
        return flat, offsets

    def _run_packed(self, fn: str, token_lists: Sequence[Sequence[int]], out_cols: int, max_tokens: Optional[int]):
        """PACKED batches (csrc/encoder_packed.h): consecutive sequences in input order, greedy by packed rows <= max_tokens
        (packed_batches).  No sort: a sequence costs its own length rounded up to 64 whatever its neighbours are."""
        import torch
        from .index import _stream_ptr
        n = len(token_lists)
        out = torch.zeros((n, out_cols) if out_cols > 1 else (n,), dtype=torch.float32, device=torch.device("cuda", self.device))
        for r in packed_batches([len(t) for t in token_lists], max_tokens or self.PACKED_MAX_TOKENS):
            flat, offsets = self._concat(token_lists[r.start:r.stop])
            nat.call(fn, self._h, flat.ctypes.data, offsets.ctypes.data, len(r), out[r.start:r.stop].data_ptr(), _stream_ptr())
        return out

    def encode_tokens(self, token_lists: Sequence[Sequence[int]], batch_size: int = 256, max_tokens: Optional[int] = None,
                      packed: bool = False):
        """-> float32 CUDA tensor [n, hidden]: L2-normalised CLS embeddings (zero rows for empty token lists).  packed=True:
        hipenc_forward_packed over input-order batches (batch_size is not used)."""
        if packed:
            return self._run_packed("hipenc_forward_packed", token_lists, self.cfg.hidden, max_tokens)
        return self._run("hipenc_forward", token_lists, self.cfg.hidden, batch_size, max_tokens)

    def score_tokens(self, token_lists: Sequence[Sequence[int]], batch_size: int = 64, max_tokens: Optional[int] = None,
                     packed: bool = False):
        """-> float32 CUDA tensor [n]: classification-head logits of `<s> query </s></s> passage </s>` sequences.  packed=True:
        hipenc_score_pairs_packed over input-order batches (batch_size is not used)."""
        if not self.has_head:
            raise ValueError("this encoder was created without a classification head")
        if packed:
            return self._run_packed("hipenc_score_pairs_packed", token_lists, 1, max_tokens)
        return self._run("hipenc_score_pairs", token_lists, 1, batch_size, max_tokens)

    def packed_info(self):
        """hipenc_packed_info -> (Tp, real tokens, sequences, path) of the last packed forward on this handle."""
        v = (ctypes.c_int64 * 4)()
        nat.call("hipenc_packed_info", self._h, v)
        return tuple(int(x) for x in v)

    def encode_lexical(self, token_lists: Sequence[Sequence[int]], batch_size: int = 256, max_tokens: Optional[int] = None):
        """hipenc_forward_lexical over the length-sorted batches of _run: ONE forward gives (dense float32 [n, hidden],
        terms int32 [n, L], weights float32 [n, L], counts int32 [n]) as CUDA tensors in input order, L = the longest input
        (at least 1).  Row i holds counts[i] (term id, weight) pairs, ids ascending, then -1 / 0."""
        import torch
        from .index import _stream_ptr
        if not self.has_lexical:
            raise ValueError("this encoder has no lexical head (set_lexical_head)")
        n = len(token_lists)
        dev = torch.device("cuda", self.device)
        L = max(1, max((len(t) for t in token_lists), default=1))
        dense = torch.zeros((n, self.cfg.hidden), dtype=torch.float32, device=dev)
        terms = torch.full((n, L), -1, dtype=torch.int32, device=dev)
        weights = torch.zeros((n, L), dtype=torch.float32, device=dev)
        counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        order = sorted(range(n), key=lambda i: -len(token_lists[i]))
        o = 0
        while o < n:
            take = batch_size
            if max_tokens is not None:
                s_pad = max(64, -(-len(token_lists[order[o]]) // 64) * 64)
                take = max(1, min(batch_size, max_tokens // s_pad))
            idx = order[o:o + take]
            o += take
            ids, lens, max_len = self._pad([token_lists[i] for i in idx])
            m = len(idx)
            pd = torch.empty((m, self.cfg.hidden), dtype=torch.float32, device=dev)
            pt = torch.empty((m, max_len), dtype=torch.int32, device=dev)
            pw = torch.empty((m, max_len), dtype=torch.float32, device=dev)
            pc = torch.empty((m,), dtype=torch.int32, device=dev)
            nat.call("hipenc_forward_lexical", self._h, ids.ctypes.data, lens.ctypes.data, m, max_len, pd.data_ptr(), pt.data_ptr(),
                     pw.data_ptr(), pc.data_ptr(), _stream_ptr())
            sel = torch.as_tensor(idx, device=dev)
            dense[sel] = pd
            terms[sel, :max_len] = pt
            weights[sel, :max_len] = pw
            counts[sel] = pc
        return dense, terms, weights, counts

    def set_colbert_head(self, weight, bias) -> None:
        """hipenc_set_colbert_head: BGE-M3's colbert_linear (weight [H, H] in nn.Linear layout, bias [H]).  The tensors are
        kept alive with the handle; a second call replaces the head."""
        import torch
        dev = torch.device("cuda", self.device)
        H = self.cfg.hidden
        wt = torch.as_tensor(weight).detach().to(device=dev, dtype=torch.bfloat16).contiguous()
        bt = torch.as_tensor(bias).detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        if tuple(wt.shape) != (H, H) or bt.numel() != H:
            raise ValueError("the ColBERT head is a weight [hidden, hidden] and a bias [hidden]")
        nat.call("hipenc_set_colbert_head", self._h, wt.data_ptr(), bt.data_ptr())
        self._col = (wt, bt)

    @property
    def has_colbert(self) -> bool:
        return getattr(self, "_col", None) is not None

    def encode_colbert(self, token_lists: Sequence[Sequence[int]], batch_size: int = 256, max_tokens: Optional[int] = None):
        """hipenc_forward_colbert over the length-sorted batches of _run: ONE forward gives (dense float32 [n, hidden], vecs
        bfloat16 [n, L - 1, hidden], counts int32 [n]) as CUDA tensors in INPUT order, L = the longest input (at least 2).
        Row p < counts[i] of vecs[i] is the unit vector of token position p + 1 (CLS skipped, EOS kept); the rest is zero."""
        import torch
        from .index import _stream_ptr
        if not self.has_colbert:
            raise ValueError("this encoder has no ColBERT head (set_colbert_head)")
        n, H = len(token_lists), self.cfg.hidden
        dev = torch.device("cuda", self.device)
        L = max(2, max((len(t) for t in token_lists), default=2))
        dense = torch.zeros((n, H), dtype=torch.float32, device=dev)
        vecs = torch.zeros((n, L - 1, H), dtype=torch.bfloat16, device=dev)
        counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        order = sorted(range(n), key=lambda i: -len(token_lists[i]))
        o = 0
        while o < n:
            take = batch_size
            if max_tokens is not None:
                s_pad = max(64, -(-len(token_lists[order[o]]) // 64) * 64)
                take = max(1, min(batch_size, max_tokens // s_pad))
            idx = order[o:o + take]
            o += take
            ids, lens, max_len = self._pad([token_lists[i] for i in idx])
            if max_len < 2:                       # the head needs room for one vector; the extra column is padding
                ids, max_len = np.ascontiguousarray(np.pad(ids, ((0, 0), (0, 2 - max_len)))), 2
            m = len(idx)
            pd = torch.empty((m, H), dtype=torch.float32, device=dev)
            pv = torch.empty((m, max_len - 1, H), dtype=torch.bfloat16, device=dev)
            pc = torch.empty((m,), dtype=torch.int32, device=dev)
            nat.call("hipenc_forward_colbert", self._h, ids.ctypes.data, lens.ctypes.data, m, max_len, pd.data_ptr(), pv.data_ptr(),
                     pc.data_ptr(), _stream_ptr())
            sel = torch.as_tensor(idx, device=dev)
            dense[sel] = pd
            vecs[sel, :max_len - 1] = pv
            counts[sel] = pc
        return dense, vecs, counts

    def encode_colbert_into(self, store, token_lists: Sequence[Sequence[int]], batch_size: int = 256,
                            max_tokens: Optional[int] = None, window: int = 1024):
        """encode_colbert straight into a MultiVectorStore: the inputs are taken `window` at a time in INPUT order (inside a
        window the batches are length-sorted as usual) and every window's vectors are appended before the next is encoded,
        so the extra device memory is one window's padded block whatever the collection holds.  -> dense float32 [n, hidden]."""
        import torch
        n = len(token_lists)
        dense = torch.zeros((n, self.cfg.hidden), dtype=torch.float32, device=torch.device("cuda", self.device))
        for o in range(0, n, max(1, int(window))):
            part = token_lists[o:o + window]
            d, v, c = self.encode_colbert(part, batch_size, max_tokens)
            dense[o:o + len(part)] = d
            store.append_device(v, c.cpu().numpy())
        return dense

    def encode_m3(self, token_lists: Sequence[Sequence[int]], batch_size: int = 256, max_tokens: Optional[int] = None):
        """hipenc_forward_m3 over the length-sorted batches of _run: ONE forward gives what encode_lexical and encode_colbert
        give together -- (dense float32 [n, hidden], terms int32 [n, L], weights float32 [n, L], lexical counts int32 [n],
        vecs bfloat16 [n, max(L, 2) - 1, hidden], vector counts int32 [n]) as CUDA tensors in INPUT order, L = the longest
        input (at least 1); every one of them bit for bit what the single-head method returns."""
        import torch
        from .index import _stream_ptr
        if not self.has_lexical:
            raise ValueError("this encoder has no lexical head (set_lexical_head)")
        if not self.has_colbert:
            raise ValueError("this encoder has no ColBERT head (set_colbert_head)")
        n, H = len(token_lists), self.cfg.hidden
        dev = torch.device("cuda", self.device)
        L = max(1, max((len(t) for t in token_lists), default=1))
        dense = torch.zeros((n, H), dtype=torch.float32, device=dev)
        terms = torch.full((n, L), -1, dtype=torch.int32, device=dev)
        weights = torch.zeros((n, L), dtype=torch.float32, device=dev)
        lex_counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        vecs = torch.zeros((n, max(L, 2) - 1, H), dtype=torch.bfloat16, device=dev)
        col_counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        order = sorted(range(n), key=lambda i: -len(token_lists[i]))
        o = 0
        while o < n:
            take = batch_size
            if max_tokens is not None:
                s_pad = max(64, -(-len(token_lists[order[o]]) // 64) * 64)
                take = max(1, min(batch_size, max_tokens // s_pad))
            idx = order[o:o + take]
            o += take
            ids, lens, max_len = self._pad([token_lists[i] for i in idx])
            real_len = max_len
            if max_len < 2:                       # the ColBERT head needs room for one vector; the extra column is padding
                ids, max_len = np.ascontiguousarray(np.pad(ids, ((0, 0), (0, 2 - max_len)))), 2
            m = len(idx)
            pd = torch.empty((m, H), dtype=torch.float32, device=dev)
            pt = torch.empty((m, max_len), dtype=torch.int32, device=dev)
            pw = torch.empty((m, max_len), dtype=torch.float32, device=dev)
            pc = torch.empty((m,), dtype=torch.int32, device=dev)
            pv = torch.empty((m, max_len - 1, H), dtype=torch.bfloat16, device=dev)
            pn = torch.empty((m,), dtype=torch.int32, device=dev)
            nat.call("hipenc_forward_m3", self._h, ids.ctypes.data, lens.ctypes.data, m, max_len, pd.data_ptr(), pt.data_ptr(),
                     pw.data_ptr(), pc.data_ptr(), pv.data_ptr(), pn.data_ptr(), _stream_ptr())
            sel = torch.as_tensor(idx, device=dev)
            dense[sel] = pd
            terms[sel, :real_len] = pt[:, :real_len]      # a column added for the ColBERT head holds no term (-1 / 0)
            weights[sel, :real_len] = pw[:, :real_len]
            lex_counts[sel] = pc
            vecs[sel, :max_len - 1] = pv
            col_counts[sel] = pn
        return dense, terms, weights, lex_counts, vecs, col_counts

    def encode_m3_into(self, store, token_lists: Sequence[Sequence[int]], batch_size: int = 256,
                       max_tokens: Optional[int] = None, window: int = 1024):
        """encode_m3 with the vectors going straight into a MultiVectorStore, `window` inputs at a time in INPUT order as
        encode_colbert_into does.  -> (dense float32 [n, hidden], terms int32 [n, L], weights float32 [n, L], lexical counts
        int32 [n]), L = the longest input (at least 1)."""
        import torch
        n = len(token_lists)
        dev = torch.device("cuda", self.device)
        L = max(1, max((len(t) for t in token_lists), default=1))
        dense = torch.zeros((n, self.cfg.hidden), dtype=torch.float32, device=dev)
        terms = torch.full((n, L), -1, dtype=torch.int32, device=dev)
        weights = torch.zeros((n, L), dtype=torch.float32, device=dev)
        counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        for o in range(0, n, max(1, int(window))):
            part = token_lists[o:o + window]
            d, t, w, c, v, vc = self.encode_m3(part, batch_size, max_tokens)
            dense[o:o + len(part)] = d
            terms[o:o + len(part), :t.shape[1]] = t
            weights[o:o + len(part), :t.shape[1]] = w
            counts[o:o + len(part)] = c
            store.append_device(v, vc.cpu().numpy())
        return dense, terms, weights, counts

    def hidden_tokens(self, token_lists: Sequence[Sequence[int]], batch_size: int = 256, packed: bool = False,
                      max_tokens: Optional[int] = None) -> List[np.ndarray]:
        """Test hook (hipenc_forward_hidden): the last hidden state of EVERY token, per input sequence a float32 array
        [len_i, hidden] holding the bf16 rows the kernels left (the conversion is exact).  Same length-sorted batches as
        encode_tokens, restored to input order.  packed=True: hipenc_forward_hidden_packed over encode_tokens' packed batches."""
        import torch
        from .index import _stream_ptr
        n, H = len(token_lists), self.cfg.hidden
        out: List[Optional[np.ndarray]] = [None] * n
        if packed:
            for r in packed_batches([len(t) for t in token_lists], max_tokens or self.PACKED_MAX_TOKENS):
                flat, offsets = self._concat(token_lists[r.start:r.stop])
                part = torch.empty((max(1, int(offsets[-1])), H), dtype=torch.bfloat16, device=torch.device("cuda", self.device))
                nat.call("hipenc_forward_hidden_packed", self._h, flat.ctypes.data, offsets.ctypes.data, len(r), part.data_ptr(),
                         _stream_ptr())
                host = part.float().cpu().numpy()
                for j, i in enumerate(r):
                    out[i] = host[offsets[j]:offsets[j + 1]].copy()
            return out
        order = sorted(range(n), key=lambda i: -len(token_lists[i]))
        for o in range(0, n, batch_size):
            idx = order[o:o + batch_size]
            ids, lens, max_len = self._pad([token_lists[i] for i in idx])
            S = -(-max_len // 64) * 64
            part = torch.empty((len(idx), S, H), dtype=torch.bfloat16, device=torch.device("cuda", self.device))
            nat.call("hipenc_forward_hidden", self._h, ids.ctypes.data, lens.ctypes.data, len(idx), max_len, part.data_ptr(),
                     _stream_ptr())
            host = part.float().cpu().numpy()
            for j, i in enumerate(idx):
                out[i] = host[j, :len(token_lists[i])].copy()
        return out

    def shape(self) -> "nat.HipEncShape":
        """What the forward's policy sees of this handle (hipenc_shape); with forward_plan: the path a batch takes."""
        s = nat.HipEncShape()
        nat.call("hipenc_shape", self._h, ctypes.byref(s))
        return s

    def last_flops(self) -> float:
        v = ctypes.c_double()
        nat.call("hipenc_last_flops", self._h, ctypes.byref(v))
        return v.value
