"""
HipIVFIndex -- IVF-Flat on top of the flat index (BASELINE north_star names "the flat-IP / IVF distance scan"; the reference
itself only ever builds faiss.IndexFlatL2, rag/storage/faiss_index.py:123).  The approximate, low-latency mode for ONE query at
a time: a search reads nprobe / nlist of the rows instead of all of them.  For batches the flat index is the faster AND exact
choice (64 queries share one read of its 2-byte filter copy; an IVF probe is per query), see DESIGN.md.

Build: libhiprag's hipivf_build(_dev) -- k-means on the GPU (assignment = the flat index's exact k = 1 search among the
centroids, update = a segmented fp64 mean, no float atomics), then the rows stored permuted by list in a flat index, every
list padded to whole 32-row blocks; the algorithm is specified in include/hiprag.h.  Files: hipivf_save / hipivf_load
("HIPIVF01").  Search: hipivf_search_dev.  At nprobe = nlist every row is scored and the result equals the flat index's bit
for bit.  Scoped search: search_scoped* (hipivf_search_scoped*) -- per-query id-range scopes over the probed lists, the
`project` argument for this index.  Updates: from_centroids (trained elsewhere, no rows yet), add and remove_ranges move the stored rows in place
(hipivf_add*, hipivf_remove_ranges) and leave exactly the index a build's layout step gives over the current rows.  torch is
only the allocator and stream owner here.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _native as nat
from .index import _METRICS, _host_f32, _is_cuda_tensor, _stream_ptr, pack_scopes


class HipIVFIndex:
    def __init__(self, d: int, nlist: int, metric="l2", device: int = 0, nprobe: Optional[int] = None):
        self.d, self.nlist, self.metric, self.device = int(d), int(nlist), _METRICS[metric], int(device)
        self.nprobe = None if nprobe is None else int(nprobe)     # search's default number of probed lists
        self._h = None
        self.ntotal = 0
        self.list_lengths: Optional[np.ndarray] = None

    # ---- build ------------------------------------------------------------------------------------------------------
    def build(self, x, iters: int = 6, seed: int = 0, max_train_rows: int = 0) -> None:
        """x: float32 [n, d] CUDA tensor (on this index's device) or array.  Trains nlist centroids (k-means, `iters`
        rounds, on all rows or on max_train_rows of them) and stores every row; ids are row numbers."""
        if _is_cuda_tensor(x):
            import torch
            if x.dtype != torch.float32 or x.dim() != 2 or x.device.index != self.device:
                raise ValueError(f"build expects a float32 [n, {self.d}] tensor on cuda:{self.device}")
            x = x.contiguous()
            ptr, fn = x.data_ptr(), "hipivf_build_dev"
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            if x.ndim != 2:
                raise ValueError(f"build expects a float32 [n, {self.d}] array, got shape {x.shape}")
            ptr, fn = x.ctypes.data, "hipivf_build"
        n = int(x.shape[0])
        if x.shape[1] != self.d or n < self.nlist:
            raise ValueError(f"need a [n >= nlist = {self.nlist}, {self.d}] float32 matrix, got {tuple(x.shape)}")
        h = ctypes.c_uint64()
        nat.call(fn, ptr, n, self.d, self.metric, self.nlist, int(iters), int(seed) & (2**64 - 1), int(max_train_rows),
                 self.device, _stream_ptr() if fn == "hipivf_build_dev" else None, ctypes.byref(h))
        self.close()
        self._adopt(h.value)

    def train_add(self, x, iters: int = 6, seed: int = 0) -> None:
        """x: float32 [n, d] CUDA tensor or array -- trains the nlist centroids on x and stores x (ids = row numbers)."""
        self.build(x, iters=iters, seed=seed, max_train_rows=0)

    # ---- updates ----------------------------------------------------------------------------------------------------
    @classmethod
    def from_centroids(cls, centroids, metric="l2", device: int = 0, nprobe: Optional[int] = None) -> "HipIVFIndex":
        """hipivf_from_centroids: nlist empty lists over `centroids` (float32 [nlist, d]) -- a trained index without rows."""
        c = np.ascontiguousarray(centroids, dtype=np.float32)
        if c.ndim != 2 or c.shape[0] < 1:
            raise ValueError(f"from_centroids expects a float32 [nlist, d] array, got shape {c.shape}")
        ix = cls(c.shape[1], c.shape[0], metric, device, nprobe)
        h = ctypes.c_uint64()
        nat.call("hipivf_from_centroids", c.ctypes.data, ix.nlist, ix.d, ix.metric, ix.device, ctypes.byref(h))
        ix._adopt(h.value)
        return ix

    def add(self, x) -> None:
        """x: float32 [m, d] CUDA tensor (on this index's device) or array -- stored under the unchanged centroids with the ids
        ntotal .. ntotal + m - 1 (faiss.IndexIVFFlat.add)."""
        self._require()
        if _is_cuda_tensor(x):
            import torch
            if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != self.d or x.device.index != self.device:
                raise ValueError(f"add expects a float32 [m, {self.d}] tensor on cuda:{self.device}")
            x = x.contiguous()
            nat.call("hipivf_add_dev", self._h, x.data_ptr() if x.shape[0] else None, int(x.shape[0]), _stream_ptr())
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
            if x.ndim != 2 or x.shape[1] != self.d:
                raise ValueError(f"add expects a float32 [m, {self.d}] array, got shape {x.shape}")
            nat.call("hipivf_add", self._h, x.ctypes.data if x.shape[0] else None, int(x.shape[0]))
        self._adopt(self._h)

    def remove_ranges(self, ranges) -> None:
        """ranges: int64 [m, 2] half-open id ranges, ascending and non-overlapping within [0, ntotal).  The surviving rows keep
        their order and are renumbered densely, as HipFlatIndex.remove_ranges renumbers (faiss remove_ids)."""
        self._require()
        r = np.ascontiguousarray(ranges, dtype=np.int64)
        if r.size == 0:
            r = r.reshape(0, 2)
        if r.ndim != 2 or r.shape[1] != 2:
            raise ValueError(f"remove_ranges expects an int64 [m, 2] array of [lo, hi) pairs, got shape {r.shape}")
        nat.call("hipivf_remove_ranges", self._h, r.ctypes.data if len(r) else None, len(r))
        self._adopt(self._h)

    def update_info(self) -> dict:
        """Of the last add / remove_ranges: rows added, rows removed, stored rows moved, staging chunks, extra device bytes."""
        self._require()
        v = np.zeros(5, dtype=np.int64)
        nat.call("hipivf_update_info", self._h, v.ctypes.data)
        return {"added": int(v[0]), "removed": int(v[1]), "moved": int(v[2]), "chunks": int(v[3]), "extra_bytes": int(v[4])}

    def _adopt(self, h: int) -> None:
        self._h = h
        d, metric, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        nat.call("hipivf_meta", h, ctypes.byref(d), ctypes.byref(metric), ctypes.byref(n))
        nlist, stored, longest = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        nat.call("hipivf_info", h, ctypes.byref(nlist), ctypes.byref(stored), ctypes.byref(longest))
        self.d, self.metric, self.ntotal, self.nlist = d.value, metric.value, n.value, nlist.value
        offs, orig = self.lists()
        real = np.nonzero(orig >= 0)[0]
        self.list_lengths = np.bincount(np.searchsorted(offs, real, side="right") - 1, minlength=self.nlist).astype(np.int64)

    # ---- files ------------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """HIPIVF01 file (include/hiprag.h)"""
        self._require()
        nat.call("hipivf_save", self._h, str(path).encode())

    @classmethod
    def load(cls, path: str, device: int = 0, nprobe: Optional[int] = None) -> "HipIVFIndex":
        h = ctypes.c_uint64()
        nat.call("hipivf_load", str(path).encode(), int(device), ctypes.byref(h))
        ix = cls.__new__(cls)
        ix.device, ix.nprobe, ix._h = int(device), None if nprobe is None else int(nprobe), None
        ix._adopt(h.value)
        return ix

    @classmethod
    def from_parts(cls, rows, centroids, list_offsets, orig_ids, nprobe: Optional[int] = None) -> "HipIVFIndex":
        """hipivf_create: an IVF view over two flat indexes the caller keeps -- `rows` (stored by list, every list starting on
        a 32-row block) and `centroids`; list_offsets int64 [nlist + 1], orig_ids int64 [rows.ntotal] (-1 = padding).  While
        the view lives, `rows` and `centroids` refuse remove_ranges."""
        offs = np.ascontiguousarray(list_offsets, dtype=np.int64)
        orig = np.ascontiguousarray(orig_ids, dtype=np.int64)
        h = ctypes.c_uint64()
        nat.call("hipivf_create", rows._h, centroids._h, offs.ctypes.data, orig.ctypes.data, len(offs) - 1, ctypes.byref(h))
        ix = cls.__new__(cls)
        ix.device, ix.nprobe, ix._h = rows.device, None if nprobe is None else int(nprobe), None
        ix._adopt(h.value)
        return ix

    # ---- inspection -------------------------------------------------------------------------------------------------
    def centroids(self) -> np.ndarray:
        """fp32 [nlist, d], centroid l = list l's"""
        self._require()
        out = np.empty((self.nlist, self.d), dtype=np.float32)
        nat.call("hipivf_get_centroids", self._h, out.ctypes.data)
        return out

    def lists(self) -> Tuple[np.ndarray, np.ndarray]:
        """(offsets int64 [nlist + 1], original id of every stored row int64 [stored rows], -1 = padding)"""
        self._require()
        nlist, stored, longest = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        nat.call("hipivf_info", self._h, ctypes.byref(nlist), ctypes.byref(stored), ctypes.byref(longest))
        offs = np.empty(nlist.value + 1, dtype=np.int64)
        orig = np.empty(max(stored.value, 1), dtype=np.int64)
        nat.call("hipivf_get_lists", self._h, offs.ctypes.data, orig.ctypes.data)
        return offs, orig[:stored.value]

    def build_times(self) -> dict:
        """ms the last build spent in assignment, update and layout (zeros for a loaded index)"""
        self._require()
        t = (ctypes.c_float * 3)()
        nat.call("hipivf_build_times", self._h, t)
        return {"assign_ms": t[0], "update_ms": t[1], "layout_ms": t[2]}

    # ---- search -----------------------------------------------------------------------------------------------------
    def _require(self) -> None:
        if self._h is None:
            raise RuntimeError("index not built")

    def _probes(self, nprobe: Optional[int]) -> int:
        nprobe = self.nprobe if nprobe is None else nprobe
        if nprobe is None:
            raise ValueError("nprobe not given and the index has no default nprobe")
        return int(nprobe)

    def search_device(self, q, k: int, nprobe: Optional[int] = None, out=None):
        """q: float32 CUDA tensor [nq, d] -> (scores64, scores32, ids) CUDA tensors [nq, k]; enqueued on the current stream."""
        import torch
        self._require()
        nprobe = self._probes(nprobe)
        nq = q.shape[0]
        if out is None:
            out = (torch.empty((nq, k), dtype=torch.float64, device=q.device), torch.empty((nq, k), dtype=torch.float32, device=q.device),
                   torch.empty((nq, k), dtype=torch.int64, device=q.device))
        nat.call("hipivf_search_dev", self._h, q.data_ptr(), nq, int(k), nprobe, out[0].data_ptr(), out[1].data_ptr(),
                 out[2].data_ptr(), _stream_ptr())
        return out

    def search(self, q, k: int, nprobe: Optional[int] = None):
        import torch
        qd = torch.from_numpy(_host_f32(q, self.d)).to(torch.device("cuda", self.device))
        _, s32, ids = self.search_device(qd, k, nprobe)
        torch.cuda.synchronize()
        return s32.cpu().numpy(), ids.cpu().numpy()

    def search_batch_device(self, q, k: int, nprobe: Optional[int] = None, out=None):
        """search_device for a batch, list-major: every slice of a probed list is read once per 16 of the queries that probe
        it.  Same arguments and the same result bit for bit; the entry to call from about 64 queries on."""
        import torch
        self._require()
        nprobe = self._probes(nprobe)
        nq = q.shape[0]
        if out is None:
            out = (torch.empty((nq, k), dtype=torch.float64, device=q.device), torch.empty((nq, k), dtype=torch.float32, device=q.device),
                   torch.empty((nq, k), dtype=torch.int64, device=q.device))
        nat.call("hipivf_search_batch_dev", self._h, q.data_ptr(), nq, int(k), nprobe, out[0].data_ptr(), out[1].data_ptr(),
                 out[2].data_ptr(), _stream_ptr())
        return out

    def search_batch(self, q, k: int, nprobe: Optional[int] = None):
        import torch
        qd = torch.from_numpy(_host_f32(q, self.d)).to(torch.device("cuda", self.device))
        _, s32, ids = self.search_batch_device(qd, k, nprobe)
        torch.cuda.synchronize()
        return s32.cpu().numpy(), ids.cpu().numpy()

    def batch_info(self) -> dict:
        """Workspace budget (bytes), queries per chunk, chunks and stored rows read of the last search_batch* call."""
        self._require()
        v = np.zeros(4, dtype=np.int64)
        nat.call("hipivf_batch_info", self._h, v.ctypes.data)
        return {"budget_bytes": int(v[0]), "chunk_queries": int(v[1]), "chunks": int(v[2]), "rows_read": int(v[3])}

    # ---- scoped search (hipivf_search_scoped*) ----------------------------------------------------------------------
    @staticmethod
    def _probe_mode(probe) -> int:
        """ "any" | "scope" (or HIPIVF_PROBE_ANY / HIPIVF_PROBE_SCOPE) -> the probe_mode argument; other integers go to the
        library, which refuses them"""
        if isinstance(probe, str):
            try:
                return {"any": nat.PROBE_ANY, "scope": nat.PROBE_SCOPE}[probe]
            except KeyError:
                raise ValueError(f"probe={probe!r}: expected 'any' or 'scope'") from None
        return int(probe)

    def search_scoped_device(self, q, k: int, scopes, scope_of_query=None, nprobe: Optional[int] = None, out=None, probe="any"):
        """search_batch_device with a scope per query: the top k of the rows that are in a probed list AND whose id lies in
        a range of the query's scope.  `scopes` / `scope_of_query` as in HipFlatIndex.search_scoped, the ranges over ids in
        [0, ntotal).  probe="any" (default): the probed lists do not depend on the scope; probe="scope": the nprobe best
        lists among those that hold a row of the query's scope (hipivf_search_scoped_probe_dev; the first such call on an
        index may synchronise once).  (scores64, scores32, ids) CUDA tensors, enqueued on torch's current stream, no
        synchronisation (the scope tables are host data, copied before the call returns)."""
        import torch
        self._require()
        nprobe = self._probes(nprobe)
        mode = self._probe_mode(probe)
        nq = q.shape[0]
        ranges, offsets, soq = pack_scopes(scopes, scope_of_query, nq)
        if out is None:
            out = (torch.empty((nq, k), dtype=torch.float64, device=q.device), torch.empty((nq, k), dtype=torch.float32, device=q.device),
                   torch.empty((nq, k), dtype=torch.int64, device=q.device))
        s64, s32, ids = out
        if mode == nat.PROBE_ANY:
            nat.call("hipivf_search_scoped_dev", self._h, q.data_ptr(), nq, int(k), nprobe, ranges.ctypes.data, offsets.ctypes.data,
                     len(offsets) - 1, soq.ctypes.data, s64.data_ptr(), s32.data_ptr() if s32 is not None else None, ids.data_ptr(),
                     _stream_ptr())
        else:
            nat.call("hipivf_search_scoped_probe_dev", self._h, q.data_ptr(), nq, int(k), nprobe, mode, ranges.ctypes.data,
                     offsets.ctypes.data, len(offsets) - 1, soq.ctypes.data, s64.data_ptr(), s32.data_ptr() if s32 is not None else None,
                     ids.data_ptr(), _stream_ptr())
        return s64, s32, ids

    def search_scoped(self, q, k: int, scopes, scope_of_query=None, nprobe: Optional[int] = None,
                      probe="any") -> Tuple[np.ndarray, np.ndarray]:
        """search_scoped_device from and to host arrays (hipivf_search_scoped / hipivf_search_scoped_probe): (scores float32
        [nq, k], ids int64 [nq, k])."""
        self._require()
        nprobe = self._probes(nprobe)
        mode = self._probe_mode(probe)
        q = _host_f32(q, self.d)
        nq = q.shape[0]
        ranges, offsets, soq = pack_scopes(scopes, scope_of_query, nq)
        s64 = np.empty((nq, k), dtype=np.float64)
        scores = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        if mode == nat.PROBE_ANY:
            nat.call("hipivf_search_scoped", self._h, q.ctypes.data, nq, int(k), nprobe, ranges.ctypes.data, offsets.ctypes.data,
                     len(offsets) - 1, soq.ctypes.data, s64.ctypes.data, scores.ctypes.data, ids.ctypes.data)
        else:
            nat.call("hipivf_search_scoped_probe", self._h, q.ctypes.data, nq, int(k), nprobe, mode, ranges.ctypes.data,
                     offsets.ctypes.data, len(offsets) - 1, soq.ctypes.data, s64.ctypes.data, scores.ctypes.data, ids.ctypes.data)
        return scores, ids

    def scope_probe_info(self) -> dict:
        """hipivf_scope_probe_info (synchronises), of the last probe="scope" call: member (scope, list) pairs, (query, probe)
        slots actually probed, chunks, centroid rows the coarse step read."""
        self._require()
        v = np.zeros(4, dtype=np.int64)
        nat.call("hipivf_scope_probe_info", self._h, v.ctypes.data)
        return {"member_pairs": int(v[0]), "probed_slots": int(v[1]), "chunks": int(v[2]), "centroid_rows_read": int(v[3])}

    def scoped_info(self) -> dict:
        """hipivf_scoped_info (synchronises): queries per work item, chunking of the last scoped call, 4 x the quads it loaded."""
        self._require()
        v = np.zeros(4, dtype=np.int64)
        nat.call("hipivf_scoped_info", self._h, v.ctypes.data)
        return {"group_queries": int(v[0]), "chunk_queries": int(v[1]), "chunks": int(v[2]), "rows_read": int(v[3])}

    def close(self) -> None:
        if self._h is not None:
            try:
                nat.call("hipivf_destroy", self._h)
            finally:
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
