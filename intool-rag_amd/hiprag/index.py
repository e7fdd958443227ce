"""
HipFlatIndex -- Python handle on libhiprag's dense flat index (the object that stands where the reference
keeps a faiss.IndexFlatL2: rag/storage/faiss_index.py:123-124, searched at :83).

Host arrays are numpy (C-contiguous float32).  The *_device methods take / return torch CUDA tensors and enqueue
on torch's current stream; torch is only the allocator and stream owner here.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _native as nat
from ._native import METRIC_IP, METRIC_L2, HipRagError

_METRICS = {"ip": METRIC_IP, "l2": METRIC_L2, METRIC_IP: METRIC_IP, METRIC_L2: METRIC_L2}


def _host_f32(a, cols: Optional[int] = None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or (cols is not None and a.shape[1] != cols):
        raise ValueError(f"expected a [n,{cols}] float32 array, got shape {a.shape}")
    return a


def scan_plan(shape: "nat.HipIdxScanShape", nq: int, k: int, cus: int) -> "nat.HipIdxScanPlan":
    """hiprag_scan_plan: the launch that nq queries at depth k get from an index of `shape` on a grid of `cus` scan workgroups.
    Arithmetic only: needs the library, not a GPU."""
    p = nat.HipIdxScanPlan()
    nat.call("hiprag_scan_plan", ctypes.byref(shape), int(nq), int(k), int(cus), ctypes.byref(p))
    return p


def wide_walk(nrt: int, ncol: int, cus: int, wg: int) -> Tuple[np.ndarray, np.ndarray]:
    """hiprag_wide_walk: the (row tiles, columns) that workgroup `wg` of `cus` of the wide scan computes, in its order, for
    an index of `nrt` row tiles and a launch of `ncol` query columns.  Arithmetic only: needs the library, not a GPU."""
    n = ctypes.c_int64()
    nat.call("hiprag_wide_walk", int(nrt), int(ncol), int(cus), int(wg), 0, None, None, ctypes.byref(n))
    rts, cols = np.empty(n.value, np.int64), np.empty(n.value, np.int32)
    nat.call("hiprag_wide_walk", int(nrt), int(ncol), int(cus), int(wg), n.value, rts.ctypes.data, cols.ctypes.data, ctypes.byref(n))
    return rts, cols


def wide_fold(p0: int, n: int, wg: int, wave: int, every: int) -> np.ndarray:
    """hiprag_wide_fold: for pairs p0 .. p0 + n - 1 of its walk, does wave `wave` of workgroup `wg` of the wide scan recompute
    its unit's bound (True) or only read it, under HIPRAG_WIDE_FOLD_EVERY = `every`?  Arithmetic only."""
    out = np.empty(int(n), np.uint8)
    nat.call("hiprag_wide_fold", int(p0), int(n), int(wg), int(wave), int(every), out.ctypes.data, None, None)
    return out.astype(bool)


def wide_fold_constants() -> Tuple[int, int]:
    """(kWideFoldFirst, kWideFoldEvery): the pairs of a walk that always fold, and the default of HIPRAG_WIDE_FOLD_EVERY."""
    first, default = ctypes.c_int32(), ctypes.c_int32()
    nat.call("hiprag_wide_fold", 0, 0, 0, 0, 1, None, ctypes.byref(first), ctypes.byref(default))
    return first.value, default.value


class HipFlatIndex:
    def __init__(self, d: int, metric="l2", device: int = 0, _handle: Optional[int] = None):
        self.device = int(device)
        if _handle is None:
            h = ctypes.c_uint64()
            nat.call("hipidx_create", int(d), _METRICS[metric], self.device, ctypes.byref(h))
            self._h = h.value
        else:
            self._h = _handle
        self.d = int(d)
        self.metric = _METRICS[metric]

    # ---- lifecycle --------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            try:
                nat.call("hipidx_destroy", self._h)
            finally:
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- properties (faiss names: ntotal, d) -------------------------------------------------------
    @property
    def ntotal(self) -> int:
        n = ctypes.c_int64()
        nat.call("hipidx_ntotal", self._h, ctypes.byref(n))
        return n.value

    def set_id_base(self, base: int) -> None:
        nat.call("hipidx_set_id_base", self._h, int(base))

    # ---- build -------------------------------------------------------------------------------------
    def add(self, x) -> None:
        """index.add(float32[n,d]) -- rows get ids ntotal..ntotal+n-1 in insertion order."""
        if _is_cuda_tensor(x):
            return self.add_device(x)
        x = _host_f32(x, self.d)
        nat.call("hipidx_add", self._h, x.ctypes.data, x.shape[0])

    def add_device(self, x) -> None:
        import torch
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.d or x.device.index != self.device:
            raise ValueError("add_device expects a float32 [n,d] tensor on this index's device")
        x = x.contiguous()
        nat.call("hipidx_add_dev", self._h, x.data_ptr(), x.shape[0], _stream_ptr())
        torch.cuda.current_stream().synchronize()   # x may be freed by the caller right after

    # ---- search ------------------------------------------------------------------------------------
    def search(self, q, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """(scores float32 [nq,k], ids int64 [nq,k]) in faiss order; padded with id -1."""
        q = _host_f32(q, self.d)
        nq = q.shape[0]
        scores = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        nat.call("hipidx_search", self._h, q.ctypes.data, nq, int(k), scores.ctypes.data, ids.ctypes.data)
        return scores, ids

    def search_device(self, q, k: int, out=None):
        """q: float32 CUDA tensor [nq,d].  Returns (scores64 [nq,k] f64, scores [nq,k] f32, ids [nq,k] i64) CUDA
        tensors; work is enqueued on torch's current stream, no synchronisation."""
        import torch
        nq = q.shape[0]
        if out is None:
            dev = q.device
            out = (torch.empty((nq, k), dtype=torch.float64, device=dev),
                   torch.empty((nq, k), dtype=torch.float32, device=dev),
                   torch.empty((nq, k), dtype=torch.int64, device=dev))
        s64, s32, ids = out
        nat.call("hipidx_search_dev", self._h, q.data_ptr(), nq, int(k), s64.data_ptr(), s32.data_ptr(), ids.data_ptr(),
                 _stream_ptr())
        return s64, s32, ids

    # ---- scoped search (hipidx_search_scoped*) -----------------------------------------------------
    def search_scoped(self, q, k: int, scopes, scope_of_query=None) -> Tuple[np.ndarray, np.ndarray]:
        """The top k of every query among the rows of ITS scope only: (scores float32 [nq,k], ids int64 [nq,k]).

        `scopes`: a sequence of scopes, each a sequence of half-open local row ranges (lo, hi), ascending and not
        overlapping.  `scope_of_query=None`: the one scope for every query when len(scopes) == 1, else scope i for query i
        (len(scopes) == nq).  Scores are the bits `search` returns for the same rows; slots past the rows of a scope are
        padded with id -1."""
        q = _host_f32(q, self.d)
        nq = q.shape[0]
        ranges, offsets, soq = pack_scopes(scopes, scope_of_query, nq)
        s64 = np.empty((nq, k), dtype=np.float64)
        scores = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        nat.call("hipidx_search_scoped", self._h, q.ctypes.data, nq, int(k), ranges.ctypes.data, offsets.ctypes.data,
                 len(offsets) - 1, soq.ctypes.data, s64.ctypes.data, scores.ctypes.data, ids.ctypes.data)
        return scores, ids

    def search_scoped_device(self, q, k: int, scopes, scope_of_query=None, out=None):
        """search_scoped for a float32 CUDA tensor [nq,d]: (scores64, scores32, ids) CUDA tensors, enqueued on torch's
        current stream, no synchronisation (the scope tables are host data and are copied before the call returns)."""
        import torch
        nq = q.shape[0]
        ranges, offsets, soq = pack_scopes(scopes, scope_of_query, nq)
        if out is None:
            dev = q.device
            out = (torch.empty((nq, k), dtype=torch.float64, device=dev),
                   torch.empty((nq, k), dtype=torch.float32, device=dev),
                   torch.empty((nq, k), dtype=torch.int64, device=dev))
        s64, s32, ids = out
        nat.call("hipidx_search_scoped_dev", self._h, q.data_ptr(), nq, int(k), ranges.ctypes.data, offsets.ctypes.data,
                 len(offsets) - 1, soq.ctypes.data, s64.data_ptr(), s32.data_ptr() if s32 is not None else None,
                 ids.data_ptr(), _stream_ptr())
        return s64, s32, ids

    def scoped_info(self) -> dict:
        """hipidx_scoped_info (synchronises): queries per work item, chunking of the last scoped call, rows it read."""
        v = np.zeros(4, dtype=np.int64)
        nat.call("hipidx_scoped_info", self._h, v.ctypes.data)
        return {"group_queries": int(v[0]), "chunk_queries": int(v[1]), "chunks": int(v[2]), "rows_read": int(v[3])}

    # ---- exact scores of given rows (hipidx_score_ids*) ---------------------------------------------
    def score_ids(self, q, ids, return64: bool = False) -> np.ndarray:
        """The exact score of query i and every row ids[i, j] names (id = local row + id_base), found by a search or not:
        float32 [nq, depth], or the float64 values with `return64=True` -- the bits `search` returns for the same row.
        An id that names no row (negative, or outside the index) is padding: -FLT_MAX / -DBL_MAX (IP), FLT_MAX / DBL_MAX
        (L2).  Duplicates are separate entries; no order is assumed."""
        q = _host_f32(q, self.d)
        nq = q.shape[0]
        ids = _ids_2d(ids, nq)
        s64 = np.empty(ids.shape, dtype=np.float64)
        s32 = None if return64 else np.empty(ids.shape, dtype=np.float32)
        nat.call("hipidx_score_ids", self._h, q.ctypes.data, nq, ids.ctypes.data, ids.shape[1], s64.ctypes.data,
                 None if s32 is None else s32.ctypes.data)
        return s64 if return64 else s32

    def score_ids_device(self, q, ids, out=None):
        """score_ids for a float32 CUDA tensor [nq, d] and an int64 CUDA tensor [nq, depth]: (scores64, scores32) CUDA
        tensors [nq, depth], enqueued on torch's current stream, no synchronisation.  `out` = (scores64, scores32 or None)."""
        import torch
        if q.dtype != torch.float32 or q.dim() != 2 or q.shape[1] != self.d or not q.is_cuda:
            raise ValueError("score_ids_device expects a float32 [nq, d] CUDA tensor of queries")
        if ids.dtype != torch.int64 or ids.dim() != 2 or ids.shape[0] != q.shape[0] or not ids.is_cuda:
            raise ValueError("score_ids_device expects an int64 [nq, depth] CUDA tensor of ids")
        q, ids = q.contiguous(), ids.contiguous()
        nq, depth = ids.shape
        if out is None:
            out = (torch.empty((nq, depth), dtype=torch.float64, device=q.device),
                   torch.empty((nq, depth), dtype=torch.float32, device=q.device))
        s64, s32 = out
        nat.call("hipidx_score_ids_dev", self._h, q.data_ptr(), nq, ids.data_ptr(), depth, s64.data_ptr(),
                 s32.data_ptr() if s32 is not None else None, _stream_ptr())
        return s64, s32

    def score_info(self) -> dict:
        """hipidx_score_info (synchronises), of the last score_ids call: valid and padding entries, workgroups launched."""
        v = np.zeros(4, dtype=np.int64)
        nat.call("hipidx_score_info", self._h, v.ctypes.data)
        return {"valid": int(v[0]), "padding": int(v[1]), "workgroups": int(v[2])}

    # ---- removal (hipidx_remove_ranges) -----------------------------------------------------------
    def remove_ranges(self, ranges) -> int:
        """faiss.IndexFlat.remove_ids over half-open local row ranges [(lo, hi), ...], ascending and not overlapping: the
        rows go, the survivors keep their order and are renumbered densely.  Returns the rows removed.  Synchronous; no
        search may be in flight on this index.  `ranges=None` passes a null table (the library refuses it)."""
        if ranges is None:
            nat.call("hipidx_remove_ranges", self._h, None, 1)
        r = np.ascontiguousarray(np.asarray(list(ranges), dtype=np.int64).reshape(-1, 2))
        nat.call("hipidx_remove_ranges", self._h, r.ctypes.data if r.shape[0] else None, r.shape[0])
        return int(self.remove_info()["rows_removed"])

    def remove_info(self) -> dict:
        """hipidx_remove_info, of the last removal: rows removed, rows moved (the survivors behind the first removed row),
        chunks of the move and the extra device bytes it allocated."""
        v = np.zeros(4, dtype=np.int64)
        nat.call("hipidx_remove_info", self._h, v.ctypes.data)
        return {"rows_removed": int(v[0]), "rows_moved": int(v[1]), "chunks": int(v[2]), "staging_bytes": int(v[3])}

    def row_bounds(self) -> Tuple[np.float32, np.float32]:
        """hipidx_row_bounds (a test hook): (max |x|^2, max |x - bf16(x)|^2) over the rows, as the certificate uses them."""
        v = np.zeros(2, dtype=np.float32)
        nat.call("hipidx_row_bounds", self._h, v.ctypes.data)
        return v[0], v[1]

    def search_begin(self, q, k: int, slot: int = 0, stream: Optional[int] = None) -> None:
        """Phase 1 of a pass (<= 32 queries): enqueue query fragments + the index scan into workspace `slot`.
        `stream` = raw hipStream_t (int) or None for torch's current stream."""
        nat.call("hipidx_search_begin_dev", self._h, q.data_ptr(), q.shape[0], int(k), int(slot),
                 _stream_ptr() if stream is None else ctypes.c_void_p(stream))

    def search_finish(self, q, k: int, slot: int, out, stream: Optional[int] = None):
        """Phase 2: selection, fp64 re-score, top-k, certificate; `out` = (scores64, scores32, ids) CUDA tensors."""
        s64, s32, ids = out
        nat.call("hipidx_search_finish_dev", self._h, q.data_ptr(), q.shape[0], int(k), int(slot), s64.data_ptr(),
                 s32.data_ptr() if s32 is not None else None, ids.data_ptr(),
                 _stream_ptr() if stream is None else ctypes.c_void_p(stream))
        return out

    @property
    def pass_queries(self) -> int:
        """Queries that share one read of the index: 64 by default, 32 in the split / f32 operand modes."""
        n = ctypes.c_int32()
        nat.call("hipidx_pass_queries", self._h, ctypes.byref(n))
        return n.value

    @property
    def launch_queries(self) -> int:
        """Queries one search_begin / search_finish pair takes: the scan runs launch/pass passes inside one launch."""
        n = ctypes.c_int32()
        nat.call("hipidx_launch_queries", self._h, ctypes.byref(n))
        return n.value

    def set_spare_cus(self, n: int) -> None:
        """Leave n CUs out of the scan grid for kernels of other streams (the finish of the previous launch, a BM25 leg, the
        RCCL all-gather); takes effect with the next launch.  See hipidx_set_spare_cus in hiprag.h."""
        nat.call("hipidx_set_spare_cus", self._h, int(n))

    def gate_tail(self, slot: int, stream: int) -> None:
        """hipidx_gate_tail_dev: `stream` waits (in the command processor) until the scan launched after the one of `slot` has
        started -- the finish enqueued behind it then runs on the CUs that scan leaves.  That scan must have been launched."""
        nat.call("hipidx_gate_tail_dev", self._h, int(slot), ctypes.c_void_p(stream))

    @property
    def spare_cus(self) -> int:
        n = ctypes.c_int32()
        nat.call("hipidx_get_spare_cus", self._h, ctypes.byref(n))
        return n.value

    @property
    def pipe_spare_cus(self) -> int:
        """CUs a pipelining host should leave out of the scan grid for the index as it stands (hipidx_pipe_spare_cus)."""
        n = ctypes.c_int32()
        nat.call("hipidx_pipe_spare_cus", self._h, ctypes.byref(n))
        return n.value

    def scan_shape(self) -> "nat.HipIdxScanShape":
        """What the scan's launch policy sees of the index as it stands (hipidx_scan_shape); with scan_plan: the launch a
        search gets."""
        s = nat.HipIdxScanShape()
        nat.call("hipidx_scan_shape", self._h, ctypes.byref(s))
        return s

    def reserve_search(self, k: int) -> None:
        nat.call("hipidx_reserve_search", self._h, int(k))

    def reserve_rows(self, n_rows: int) -> None:
        """Capacity for n_rows rows in one allocation (hipidx_reserve_rows)."""
        nat.call("hipidx_reserve_rows", self._h, int(n_rows))

    # ---- misc --------------------------------------------------------------------------------------
    def reconstruct(self, row: int) -> np.ndarray:
        out = np.empty(self.d, dtype=np.float32)
        nat.call("hipidx_reconstruct", self._h, int(row), out.ctypes.data)
        return out

    def save(self, path: str) -> None:
        nat.call("hipidx_save", self._h, str(path).encode())

    @classmethod
    def load(cls, path: str, device: int = 0) -> "HipFlatIndex":
        h = ctypes.c_uint64()
        nat.call("hipidx_load", str(path).encode(), int(device), ctypes.byref(h))
        d, m = ctypes.c_int32(), ctypes.c_int32()
        nat.call("hipidx_dim", h.value, ctypes.byref(d))
        nat.call("hipidx_metric", h.value, ctypes.byref(m))
        return cls(d.value, m.value, device, _handle=h.value)

    def enable_timing(self, on=True) -> None:
        """True / 1: HIP events around every scan launch; n > 1: around every n-th launch; False / 0: off."""
        nat.call("hipidx_enable_timing", self._h, int(on))

    def stats(self) -> dict:
        st = nat.HipIdxStats()
        nat.call("hipidx_get_stats", self._h, ctypes.byref(st))
        return {f: getattr(st, f) for f, _ in st._fields_}


def pack_scopes(scopes, scope_of_query, nq: int):
    """scopes (a sequence of sequences of (lo, hi)) -> the CSR arrays of hipidx_search_scoped: ranges int64 [n_ranges,2],
    offsets int32 [n_scopes+1], scope_of_query int32 [nq].  Only the shapes are checked here; the library checks the values."""
    scopes = list(scopes)
    offsets = np.zeros(len(scopes) + 1, dtype=np.int32)
    flat = []
    for s, sc in enumerate(scopes):
        sc = np.asarray(list(sc), dtype=np.int64).reshape(-1, 2)
        flat.append(sc)
        offsets[s + 1] = offsets[s] + sc.shape[0]
    ranges = np.ascontiguousarray(np.concatenate(flat, axis=0) if flat else np.zeros((0, 2), dtype=np.int64))
    if ranges.shape[0] == 0:
        ranges = np.zeros((1, 2), dtype=np.int64)      # a valid pointer for the library; no scope refers to it
    if scope_of_query is None:
        if len(scopes) == 1:
            soq = np.zeros(nq, dtype=np.int32)
        elif len(scopes) == nq:
            soq = np.arange(nq, dtype=np.int32)
        else:
            raise ValueError(f"scope_of_query=None needs one scope or one per query: {len(scopes)} scopes, {nq} queries")
    else:
        soq = np.ascontiguousarray(scope_of_query, dtype=np.int32).reshape(-1)
        if soq.shape[0] != nq:
            raise ValueError(f"scope_of_query has {soq.shape[0]} entries for {nq} queries")
    return ranges, offsets, soq


def _ids_2d(ids, nq: int) -> np.ndarray:
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    if ids.ndim == 1:
        ids = ids[None, :]
    if ids.ndim != 2 or ids.shape[0] != nq:
        raise ValueError(f"expected an [{nq}, depth] int64 array of ids, got shape {ids.shape}")
    return ids


def score_ids_reference(x, q, ids, metric, id_base: int = 0) -> np.ndarray:
    """The semantics of hipidx_score_ids as a pure function over numpy arrays (no GPU): float64 [nq, depth], the score of
    query i and row ids[i, j] - id_base of x, padding values where the id names no row.  It restates rescore4's summation
    order (csrc/dense_layout.h): a row's 16 partial sums are indexed (pq = 0..7, hh = 0..1); each sums the pieces p = pq,
    pq + 8, ... in order over the elements 8p + 4hh .. 8p + 4hh + 3, one after the other, in fp64; the xor-4 / 8 / 16 / 32
    butterfly then adds hh = 0 and 1, then pq and pq ^ 1, pq ^ 2, pq ^ 4.  Every add is an explicit numpy fp64 add.  Inner
    product: bit for bit the library's value (a product of two fp32 values is exact in fp64).  L2: the library may contract
    t * t + acc into one rounding where numpy rounds twice, so the two agree to rounding, not always to the bit."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    if x.ndim != 2 or q.ndim != 2 or q.shape[1] != x.shape[1]:
        raise ValueError(f"expected x [n, d] and q [nq, d], got {x.shape} and {q.shape}")
    ids = _ids_2d(ids, q.shape[0])
    n, d = x.shape
    l2 = _METRICS[metric] == METRIC_L2
    steps = (d + 63) // 64                         # pieces per partial sum: P = ceil(d / 8) pieces, 8 partial sums per half
    width = steps * 64                             # zero padding adds +0.0 to a sum that is never -0.0: the bits stay
    big = float(np.finfo(np.float64).max)
    out = np.full(ids.shape, big if l2 else -big, dtype=np.float64)
    valid = (ids >= 0) & (ids >= id_base) & (ids - id_base < n)
    for i in range(q.shape[0]):
        js = np.nonzero(valid[i])[0]
        if js.size == 0:
            continue
        xr = np.zeros((js.size, width), dtype=np.float64)
        xr[:, :d] = x[ids[i, js] - id_base]
        qr = np.zeros(width, dtype=np.float64)
        qr[:d] = q[i]
        xr = xr.reshape(js.size, steps, 8, 2, 4)   # element 8p + 4hh + e of piece p = 8 * step + pq
        qr = qr.reshape(1, steps, 8, 2, 4)
        if l2:
            t = xr - qr
            term = t * t
        else:
            term = xr * qr
        acc = np.zeros((js.size, 8, 2), dtype=np.float64)
        for step in range(steps):
            for e in range(4):
                acc = acc + term[:, step, :, :, e]
        s = acc[:, :, 0] + acc[:, :, 1]            # xor 4
        s = s[:, 0::2] + s[:, 1::2]                # xor 8
        s = s[:, 0::2] + s[:, 1::2]                # xor 16
        out[i, js] = s[:, 0] + s[:, 1]             # xor 32
    return out


def _is_cuda_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def _stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def merge_topk_device(scores64, ids, k_out: int, metric, out=None):
    """Merge [n_parts, nq, k_in] partial lists (CUDA tensors) -> (scores64, scores32, ids) [nq,k_out].

    The two inputs may be strided views along dim 0 (e.g. halves of one all-gathered [G,2,nq,k] buffer) as long
    as each [nq,k_in] part is contiguous and both use the same part stride."""
    import torch
    n_parts, nq, k_in = scores64.shape
    for t in (scores64, ids):
        if t.stride(2) != 1 or t.stride(1) != k_in:
            raise ValueError("each [nq,k_in] part must be contiguous")
    part_stride = scores64.stride(0) if n_parts > 1 else nq * k_in
    if n_parts > 1 and ids.stride(0) != part_stride:
        raise ValueError("scores and ids must use the same part stride")
    dev = scores64.device
    if out is None:
        out = (torch.empty((nq, k_out), dtype=torch.float64, device=dev),
               torch.empty((nq, k_out), dtype=torch.float32, device=dev),
               torch.empty((nq, k_out), dtype=torch.int64, device=dev))
    nat.call("hiprag_merge_topk_dev", scores64.data_ptr(), ids.data_ptr(), n_parts, nq, k_in, int(k_out),
             int(part_stride), _METRICS[metric], out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _stream_ptr())
    return out


__all__ = ["HipFlatIndex", "merge_topk_device", "pack_scopes", "score_ids_reference", "HipRagError", "METRIC_IP", "METRIC_L2"]
