"""
PageTable and rank_pages_device -- Python handles on the page table and the page-ranking call (csrc/page_table.hip): the
last step of the reference's retriever (rag/query/page_retriever.py:145-236: group the retrieved chunks by page, score
every page, keep the best few) over candidate ids that stay on the GPU.  No CPU path: `rank_pages_reference` below states
the semantics for tests and documentation only, as `pair_tokens` does for the rerank call.
"""
from __future__ import annotations

import ctypes
import math
from typing import Sequence, Tuple

import numpy as np

from . import _native as nat

NEG_DBL_MAX = -float(np.finfo(np.float64).max)   # the score of a rank past the pages of a query
MAX_DEPTH = 256                                  # kRankMaxDepth: of the candidate list and of the dense list
# the dispatch constants of the ranking kernel, as csrc/page_table.h names them
RANK_THREADS = 256                               # kRankThreads
RANK_WAVE_DEPTH = 64                             # kRankWaveDepth: depth <= this runs one wave per query ...
RANK_WAVE_QUERIES = 4                            # kRankWaveQueries: ... and this many queries per workgroup


def doc_offsets(doc_rows: Sequence[int]) -> np.ndarray:
    """rows per document -> offsets int64 [n_docs + 1]"""
    off = np.zeros(len(doc_rows) + 1, dtype=np.int64)
    if len(doc_rows):
        off[1:] = np.cumsum(np.asarray(doc_rows, dtype=np.int64))
    return off


class PageTable:
    """Device-resident (page, document tag) of every collection row."""

    def __init__(self, device: int = 0):
        self.device = int(device)
        h = ctypes.c_uint64()
        nat.call("hippage_create", self.device, ctypes.byref(h))
        self._h = h.value

    def close(self) -> None:
        if getattr(self, "_h", None):
            try:
                nat.call("hippage_destroy", self._h)
            finally:
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, pages, offsets=None) -> None:
        """append(pages of ONE document) or append(pages int32 [n_rows], offsets int64 [n_docs + 1]): document j is the
        rows offsets[j] .. offsets[j + 1] - 1 of the batch and gets the next tag."""
        pages = np.ascontiguousarray(pages, dtype=np.int32).reshape(-1)
        if offsets is None:
            offsets = np.array([0, pages.size], dtype=np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.size and int(offsets[-1]) > pages.size:
            raise ValueError(f"offsets end at {int(offsets[-1])}, {pages.size} pages were given")
        keep = pages if pages.size else np.zeros(1, np.int32)       # an empty batch still passes a pointer
        nat.call("hippage_append", self._h, keep.ctypes.data, offsets.ctypes.data if offsets.size else None, len(offsets) - 1)

    def remove_ranges(self, ranges) -> None:
        r = np.ascontiguousarray(ranges, dtype=np.int64).reshape(-1, 2)
        nat.call("hippage_remove_ranges", self._h, r.ctypes.data if len(r) else None, len(r))

    def sizes(self) -> Tuple[int, int, int, int]:
        """(rows, tags issued, capacity in rows, 0)"""
        out = np.zeros(4, dtype=np.int64)
        nat.call("hippage_sizes", self._h, out.ctypes.data)
        return tuple(int(v) for v in out)

    def __len__(self) -> int:
        return self.sizes()[0]

    def export(self) -> Tuple[np.ndarray, np.ndarray]:
        """(pages int32 [rows], tags int32 [rows]): a test hook."""
        n = self.sizes()[0]
        pages, tags = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        nat.call("hippage_export", self._h, pages.ctypes.data, tags.ctypes.data)
        return pages[:n], tags[:n]


class RankedPages(tuple):
    """The eight outputs of rank_pages_device: a tuple of CUDA tensors that are views of one int32 and one float64 buffer."""

    def __new__(cls, outputs, packed, layout):
        self = super().__new__(cls, outputs)
        self._packed, self._layout = packed, layout
        return self

    @staticmethod
    def layout(nq: int, max_pages: int, depth: int):
        """[(buffer 0 = int32 | 1 = float64, first element, shape)] of the eight outputs, then the two buffer sizes"""
        shapes = ((0, (nq,)), (1, (nq, max_pages)), (0, (nq, max_pages)), (0, (nq, max_pages)), (0, (nq, max_pages)),
                  (0, (nq, depth)), (0, (nq, depth)), (1, (nq, depth)))
        used, out = [0, 0], []
        for which, shape in shapes:
            out.append((which, used[which], shape))
            used[which] += math.prod(shape)
        return out + [tuple(used)]

    def host(self):
        """The eight outputs as numpy arrays, through two copies (the first synchronises the stream)."""
        bufs = [b.cpu().numpy() for b in self._packed]
        return tuple(bufs[which][lo:lo + math.prod(shape)].reshape(shape) for which, lo, shape in self._layout[:-1])


def rank_pages_device(table: PageTable, cand_ids, dense_ids, dense_scores64, max_pages: int, id_base: int = 0,
                      metric: int = nat.METRIC_IP):
    """hippage_rank_dev on torch's current stream.  cand_ids int64 [nq, depth], dense_ids int64 [nq, dense_depth] and
    dense_scores64 float64 [nq, dense_depth] are CUDA tensors (a dense-only caller passes its result ids as both id
    lists).  -> RankedPages, a tuple of CUDA tensors (n_pages int32 [nq], page_scores float64 [nq, max_pages], page_first,
    page_members, page_no int32 [nq, max_pages], cand_rank, cand_dense_pos int32 [nq, depth], cand_scores float64
    [nq, depth]); nothing is synchronised.  The eight are views of two buffers: `.host()` brings them over in two copies."""
    import torch
    from .index import _stream_ptr
    for name, t, dt in (("cand_ids", cand_ids, torch.int64), ("dense_ids", dense_ids, torch.int64),
                        ("dense_scores64", dense_scores64, torch.float64)):
        if t.dtype != dt or t.dim() != 2 or not t.is_cuda:
            raise ValueError(f"{name} must be a 2-d {dt} CUDA tensor")
    if dense_ids.shape != dense_scores64.shape or dense_ids.shape[0] != cand_ids.shape[0]:
        raise ValueError("dense_ids and dense_scores64 must be [nq, dense_depth] with the nq of cand_ids")
    cand, d_ids, d_sc = cand_ids.contiguous(), dense_ids.contiguous(), dense_scores64.contiguous()
    nq, depth = cand.shape
    mp = max(int(max_pages), 1)
    dev = cand.device
    layout = RankedPages.layout(nq, mp, depth)
    packed = (torch.empty((layout[-1][0],), dtype=torch.int32, device=dev), torch.empty((layout[-1][1],), dtype=torch.float64, device=dev))
    n_pages, page_scores, page_first, page_members, page_no, cand_rank, cand_dpos, cand_scores = (
        packed[which][lo:lo + math.prod(shape)].view(shape) for which, lo, shape in layout[:-1])
    nat.call("hippage_rank_dev", table._h, cand.data_ptr(), depth, d_ids.data_ptr(), d_sc.data_ptr(), d_ids.shape[1], nq, int(id_base),
             int(metric), int(max_pages), n_pages.data_ptr(), page_scores.data_ptr(), page_first.data_ptr(), page_members.data_ptr(),
             page_no.data_ptr(), cand_rank.data_ptr(), cand_dpos.data_ptr(), cand_scores.data_ptr(), _stream_ptr())
    return RankedPages((n_pages, page_scores, page_first, page_members, page_no, cand_rank, cand_dpos, cand_scores), packed, layout)


def rank_pages_reference(pages, tags, cand_ids, dense_ids, dense_scores64, max_pages: int, id_base: int = 0,
                         metric: int = nat.METRIC_IP):
    """The semantics of hippage_rank_dev as a pure function over numpy arrays (pages, tags: the table's two columns) ->
    the eight outputs of rank_pages_device as numpy arrays.  Python floats are fp64; the sum of a page is explicit
    sequential adds (a compensated `sum` may differ from them in the last bit)."""
    pages, tags = np.asarray(pages), np.asarray(tags)
    cand, d_ids = np.asarray(cand_ids, dtype=np.int64), np.asarray(dense_ids, dtype=np.int64)
    d_sc = np.asarray(dense_scores64, dtype=np.float64)
    nq, depth = cand.shape
    rows = len(pages)
    n_pages = np.zeros(nq, np.int32)
    page_scores = np.full((nq, max_pages), NEG_DBL_MAX, np.float64)
    page_first = np.full((nq, max_pages), -1, np.int32)
    page_members, page_no = np.zeros((nq, max_pages), np.int32), np.zeros((nq, max_pages), np.int32)
    cand_rank, cand_dpos = np.full((nq, depth), -1, np.int32), np.full((nq, depth), -1, np.int32)
    cand_scores = np.zeros((nq, depth), np.float64)
    for q in range(nq):
        dense = d_ids[q].tolist()
        groups = {}                                   # (tag, page) -> member positions; dicts keep first-seen order
        for j, c in enumerate(cand[q].tolist()):
            if c < 0 or not 0 <= c - id_base < rows:
                continue
            if c in dense:
                cand_dpos[q, j] = dense.index(c)
                v = float(d_sc[q, cand_dpos[q, j]])
                s = 1.0 - v / 2.0 if metric == nat.METRIC_L2 else v
                cand_scores[q, j] = max(0.0, min(1.0, s))
            row = c - id_base
            groups.setdefault((int(tags[row]), int(pages[row])), []).append(j)
        ranked = []
        for (_tag, page), members in groups.items():
            acc, m = 0.0, 0
            for j in members:
                if cand_dpos[q, j] >= 0:
                    acc = acc + float(cand_scores[q, j])
                    m += 1
            ranked.append(((acc / m if m else 0.0) + min(len(members) * 0.05, 0.15), page, members))
        ranked.sort(key=lambda r: r[0], reverse=True)     # stable: ties keep first-seen order
        n_pages[q] = len(ranked)
        for r, (score, page, members) in enumerate(ranked):
            cand_rank[q, members] = r
            if r < max_pages:
                page_scores[q, r], page_first[q, r], page_members[q, r], page_no[q, r] = score, members[0], len(members), page
    return n_pages, page_scores, page_first, page_members, page_no, cand_rank, cand_dpos, cand_scores
