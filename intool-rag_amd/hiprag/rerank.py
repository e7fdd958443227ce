"""
TokenStore and rerank -- Python handles on the passage token store (csrc/token_store.hip) and the device rerank call
(csrc/rerank.hip): the cross-encoder the reference only configures (rag/config.py:25-27), run over candidate ids without
tokenising a passage again.  No CPU path: `pair_tokens` below states the pair rule for tests and documentation only.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat

NEG_MAX = -float(np.finfo(np.float32).max)      # -FLT_MAX: the logit of a padding slot, the score of an empty rank
DEFAULT_BATCH_TOKENS = 131072                   # 256 x 512, what CrossEncoderReranker.score passes to score_tokens


def pair_tokens(q: Sequence[int], p: Sequence[int], max_len: int, bos: int = 0, eos: int = 2) -> List[int]:
    """The pair rule of hiprerank_* as a pure function over token bodies: FileTokenizer.encode_pair, token for token."""
    room = max(0, max_len - 4)
    q = list(q)[:room]
    return [bos] + q + [eos, eos] + list(p)[:max(0, room - len(q))] + [eos]


def seq_len_bound(max_len: int, longest_query: int, longest_doc: int) -> int:
    """S of a rerank call: min(max_len, 4 + longest query + longest document), rounded up to 64."""
    return -(-min(int(max_len), 4 + int(longest_query) + int(longest_doc)) // 64) * 64


def csr(lists: Sequence[Sequence[int]], offset_dtype=np.int64) -> Tuple[np.ndarray, np.ndarray]:
    """token lists -> (tokens int32, offsets [n + 1])"""
    offsets = np.zeros(len(lists) + 1, dtype=offset_dtype)
    if len(lists):
        offsets[1:] = np.cumsum([len(t) for t in lists])
    tokens = np.fromiter((v for t in lists for v in t), dtype=np.int32, count=int(offsets[-1]))
    return tokens, offsets


class TokenStore:
    """Device-resident CSR of the token bodies of every chunk; document i is collection row i."""

    def __init__(self, vocab: int, bos: int = 0, eos: int = 2, pad: int = 1, max_doc_tokens: int = 508, device: int = 0):
        self.vocab, self.bos, self.eos, self.pad = int(vocab), int(bos), int(eos), int(pad)
        self.max_doc_tokens, self.device = int(max_doc_tokens), int(device)
        h = ctypes.c_uint64()
        nat.call("hiptok_create", self.vocab, self.bos, self.eos, self.pad, self.max_doc_tokens, self.device, ctypes.byref(h))
        self._h = h.value

    def close(self) -> None:
        if getattr(self, "_h", None):
            try:
                nat.call("hiptok_destroy", self._h)
            finally:
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, tokens, offsets=None) -> None:
        """append(list of token lists) or append(tokens int32, offsets int64 [n + 1])."""
        if offsets is None:
            tokens, offsets = csr(tokens)
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        keep = tokens if tokens.size else np.zeros(1, np.int32)     # an empty batch still passes a pointer
        nat.call("hiptok_append", self._h, keep.ctypes.data, offsets.ctypes.data, len(offsets) - 1)

    def remove_ranges(self, ranges) -> None:
        r = np.ascontiguousarray(ranges, dtype=np.int64).reshape(-1, 2)
        nat.call("hiptok_remove_ranges", self._h, r.ctypes.data if len(r) else None, len(r))

    def sizes(self) -> Tuple[int, int, int, int]:
        """(documents, stored tokens, cap per document, longest stored document)"""
        out = np.zeros(4, dtype=np.int64)
        nat.call("hiptok_sizes", self._h, out.ctypes.data)
        return tuple(int(v) for v in out)

    def __len__(self) -> int:
        return self.sizes()[0]

    def export(self) -> Tuple[np.ndarray, np.ndarray]:
        """(offsets int64 [n + 1], tokens int32): a test hook."""
        n, nt, _, _ = self.sizes()
        offsets, tokens = np.zeros(n + 1, dtype=np.int64), np.zeros(max(nt, 1), dtype=np.int32)
        nat.call("hiptok_export", self._h, offsets.ctypes.data, tokens.ctypes.data)
        return offsets, tokens[:nt]

    def rerank_info(self) -> Tuple[int, int, int, int]:
        """(valid pairs, padding slots, S, sub-batches) of the last rerank call on this store; synchronises."""
        out = np.zeros(4, dtype=np.int64)
        nat.call("hiprerank_info", self._h, out.ctypes.data)
        return tuple(int(v) for v in out)

    def rerank_packed_info(self) -> Tuple[int, int, int, int]:
        """(valid pairs, padding slots, packed rows, sub-batches) of the last PACKED rerank call on this store; synchronises."""
        out = np.zeros(4, dtype=np.int64)
        nat.call("hiprerank_packed_info", self._h, out.ctypes.data)
        return tuple(int(v) for v in out)

    def assemble_packed(self, queries: Sequence[Sequence[int]], cand_ids, id_base: int = 0, max_len: int = 512):
        """Test hook (hiprerank_assemble_packed): ONE packed layout over all the pairs.
        -> (tokens int32 [Tp], row_off int32 [nq * depth + 1], lens int32 [nq * depth])."""
        cand = np.ascontiguousarray(cand_ids, dtype=np.int64)
        nq, depth = cand.shape
        qt, qo = _queries(queries)
        tokens = np.zeros(nq * depth * max(-(-int(max_len) // 64) * 64, 64), dtype=np.int32)
        row_off = np.zeros(nq * depth + 1, dtype=np.int32)
        lens = np.zeros(nq * depth, dtype=np.int32)
        Tp = ctypes.c_int32()
        nat.call("hiprerank_assemble_packed", self._h, qt.ctypes.data, qo.ctypes.data, nq, cand.ctypes.data, depth, int(id_base),
                 int(max_len), tokens.ctypes.data, row_off.ctypes.data, lens.ctypes.data, ctypes.byref(Tp))
        return tokens[:Tp.value].copy(), row_off, lens

    def assemble(self, queries: Sequence[Sequence[int]], cand_ids, id_base: int = 0, max_len: int = 512):
        """Test hook (hiprerank_assemble): -> (tokens int32 [nq * depth, S], lens int32 [nq * depth])."""
        cand = np.ascontiguousarray(cand_ids, dtype=np.int64)
        nq, depth = cand.shape
        qt, qo = csr(queries, np.int32)
        qt = qt if qt.size else np.zeros(1, np.int32)
        s_max = -(-int(max_len) // 64) * 64
        tokens = np.zeros(nq * depth * max(s_max, 64), dtype=np.int32)
        lens = np.zeros(nq * depth, dtype=np.int32)
        S = ctypes.c_int32()
        nat.call("hiprerank_assemble", self._h, qt.ctypes.data, qo.ctypes.data, nq, cand.ctypes.data, depth, int(id_base), int(max_len),
                 tokens.ctypes.data, lens.ctypes.data, ctypes.byref(S))
        return tokens[:nq * depth * S.value].reshape(nq * depth, S.value).copy(), lens


def _queries(queries: Sequence[Sequence[int]]):
    qt, qo = csr(queries, np.int32)
    return (qt if qt.size else np.zeros(1, np.int32)), qo


def rerank(encoder, store: TokenStore, queries: Sequence[Sequence[int]], cand_ids, k: int, id_base: int = 0,
           max_len: Optional[int] = None, max_batch_tokens: int = 0, packed: bool = False):
    """hiprerank_host: queries = token bodies (no bos / eos), cand_ids int64 [nq, depth] on the host.
    -> (scores float32 [nq, k], ids int64 [nq, k], positions int32 [nq, k], logits float32 [nq, depth]).
    packed=True: hiprerank_packed_host -- every pair costs its own length rounded up to 64, not the longest candidate's."""
    cand = np.ascontiguousarray(cand_ids, dtype=np.int64)
    if cand.ndim != 2 or cand.shape[0] != len(queries):
        raise ValueError("cand_ids must be [len(queries), depth]")
    nq, depth = cand.shape
    qt, qo = _queries(queries)
    max_len = int(max_len or encoder.cfg.max_seq_len)
    kk = max(int(k), 1)
    scores, ids = np.zeros((nq, kk), np.float32), np.zeros((nq, kk), np.int64)
    pos, logits = np.zeros((nq, kk), np.int32), np.zeros((nq, depth), np.float32)
    nat.call("hiprerank_packed_host" if packed else "hiprerank_host", encoder._h, store._h, qt.ctypes.data, qo.ctypes.data, nq,
             cand.ctypes.data, depth, int(id_base), max_len,
             int(k), int(max_batch_tokens), logits.ctypes.data, scores.ctypes.data, ids.ctypes.data, pos.ctypes.data)
    return scores, ids, pos, logits


def rerank_device(encoder, store: TokenStore, queries: Sequence[Sequence[int]], cand_ids, k: int, id_base: int = 0,
                  max_len: Optional[int] = None, max_batch_tokens: int = 0, want_logits: bool = True, packed: bool = False):
    """hiprerank_dev on torch's current stream: cand_ids is an int64 CUDA tensor [nq, depth] (what hybrid_search*_device
    returned).  -> CUDA tensors (scores [nq, k], ids [nq, k], positions [nq, k], logits [nq, depth] or None); nothing is
    synchronised.  Calls on one encoder share its workspace: keep them on one stream.
    packed=True: hiprerank_packed_dev -- rows follow every pair's own length instead of the store's longest document, at the
    price of ONE synchronise of the stream inside the call (the pair lengths come to the host)."""
    import torch
    from .index import _stream_ptr
    if cand_ids.dtype != torch.int64 or cand_ids.dim() != 2 or not cand_ids.is_cuda or cand_ids.shape[0] != len(queries):
        raise ValueError("cand_ids must be an int64 CUDA tensor [len(queries), depth]")
    cand = cand_ids.contiguous()
    nq, depth = cand.shape
    qt, qo = _queries(queries)
    max_len = int(max_len or encoder.cfg.max_seq_len)
    kk = max(int(k), 1)
    dev = cand.device
    scores = torch.empty((nq, kk), dtype=torch.float32, device=dev)
    ids = torch.empty((nq, kk), dtype=torch.int64, device=dev)
    pos = torch.empty((nq, kk), dtype=torch.int32, device=dev)
    logits = torch.empty((nq, depth), dtype=torch.float32, device=dev) if want_logits else None
    nat.call("hiprerank_packed_dev" if packed else "hiprerank_dev", encoder._h, store._h, qt.ctypes.data, qo.ctypes.data, nq,
             cand.data_ptr(), depth, int(id_base), max_len,
             int(k), int(max_batch_tokens), logits.data_ptr() if want_logits else None, scores.data_ptr(), ids.data_ptr(),
             pos.data_ptr(), _stream_ptr())
    return scores, ids, pos, logits
