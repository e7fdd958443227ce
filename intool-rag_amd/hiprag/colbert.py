"""
MultiVectorStore and maxsim -- Python handles on the multi-vector store (csrc/multivec.hip) and the late-interaction call
(csrc/maxsim.hip): the third output of the reference's model, BAAI/bge-m3 (rag/config.py:9), as a second stage beside the
cross-encoder of rag/config.py:25-27.  No CPU path: `colbert_reference` and `maxsim_reference` below state the arithmetic for
tests and documentation only.

Host-side vectors are bf16 BIT PATTERNS in uint16 arrays (numpy has no bfloat16); `bf16_bits` / `bf16_values` convert.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native as nat

NEG_MAX = -float(np.finfo(np.float32).max)      # -FLT_MAX: the score of a padding candidate and of an empty rank
TILE = 32                                       # query vectors per LDS tile of the kernel


def bf16_bits(x) -> np.ndarray:
    """float values -> bf16 bit patterns (uint16), ONE round to nearest even from fp32."""
    import torch
    x32 = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def bf16_values(bits) -> np.ndarray:
    """bf16 bit patterns (uint16) -> float32 values (exact)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def colbert_reference(hidden_bf16, w, b, splits: int = 1) -> np.ndarray:
    """The ColBERT head of hipenc_forward_colbert in numpy fp32, operation for operation.  hidden_bf16 [n, H] and w [H, H]
    (nn.Linear layout) hold bf16-exact values, b [H] fp32.  -> float32 [n, H] holding the bf16 output values (bf16_bits of it
    gives the stored bits).
      c   the fp32 product, `splits` K ranges added in split order (the order INSIDE a range is numpy's, not the GPU kernel's:
          bit-exact only where every partial sum is exact in fp32 -- otherwise compare within the accumulation bound)
      v   c + b;   ss: lane l of 64 adds the squares of columns l, l + 64, .. in ascending order, then the butterfly over lane
          distances 32 .. 1 (each step v[l] + v[l ^ distance]);   inv = 1 / max(sqrt(ss), 1e-12);   y = bf16(v * inv)."""
    x = np.ascontiguousarray(hidden_bf16, dtype=np.float32)
    w32 = np.ascontiguousarray(w, dtype=np.float32)
    b32 = np.asarray(b, dtype=np.float32).reshape(-1)
    n, H = x.shape
    assert w32.shape == (H, H) and b32.shape == (H,) and H % 64 == 0 and H % splits == 0
    kr = H // splits
    c = (x[:, :kr] @ w32[:, :kr].T).astype(np.float32)
    for s in range(1, splits):
        c = (c + (x[:, s * kr:(s + 1) * kr] @ w32[:, s * kr:(s + 1) * kr].T).astype(np.float32)).astype(np.float32)
    v = (c + b32).astype(np.float32)
    sq = (v * v).astype(np.float32)
    lanes = np.zeros((n, 64), dtype=np.float32)
    for chunk in sq.reshape(n, H // 64, 64).transpose(1, 0, 2):
        lanes = (lanes + chunk).astype(np.float32)
    idx = np.arange(64)
    for dist in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, idx ^ dist]).astype(np.float32)
    ss = lanes[:, :1]
    inv = (np.float32(1.0) / np.maximum(np.sqrt(ss).astype(np.float32), np.float32(1e-12))).astype(np.float32)
    return bf16_values(bf16_bits((v * inv).astype(np.float32)))


def maxsim_reference(q, d) -> float:
    """BGE-M3's colbert_score without a temperature, in float64: q [Lq, dim], d [Ld, dim] -> mean_i max_j q_i . d_j."""
    q = np.asarray(q, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    assert q.ndim == 2 and d.ndim == 2 and q.shape[0] >= 1 and d.shape[0] >= 1 and q.shape[1] == d.shape[1]
    return float((q @ d.T).max(axis=1).sum() / q.shape[0])


FORMATS = {"bf16": 0, "fp8": 1, "mxfp4": 4}     # the store's formats and their numbers in the C-ABI (2 and 3 are none)
FORMAT_NAMES = {number: name for name, number in FORMATS.items()}
FP8_AMAX_LO, FP8_AMAX_HI = 67 << 7, 187 << 7    # bf16 magnitude bits of 2^-60 and 2^60: the domain of the fp8 format


def fp8_quantize_reference(bits) -> Tuple[np.ndarray, np.ndarray]:
    """The fp8 format of the multi-vector store (csrc/multivec.h) in numpy: bf16 bits uint16 [n, dim] -> (codes uint8 [n, dim],
    scales float32 [n]).  Per vector, amax = max |v_k|:
      amax == 0                                      codes 0x00, scale 1.0
      a non-finite component, or amax outside
      [2^-60, 2^60]                                  the zero vector, scale 1.0 (the store counts these)
      otherwise  e = 7 - floor(log2 amax)            (amax's exponent bits), so amax * 2^e lies in [128, 256)
                 code_k = e4m3fn(v_k * 2^e)          OCP, round to nearest even: torch's float8_e4m3fn cast; the product is
                                                     exact in fp32 and <= 256 < 448, so nothing saturates
                 a -0 code (0x80) is stored as 0x00;   scale = 2^-e."""
    import torch
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    assert b.ndim == 2
    n, dim = b.shape
    codes, scales = np.zeros((n, dim), dtype=np.uint8), np.ones(n, dtype=np.float32)
    if n == 0:
        return codes, scales
    amax = (b & 0x7FFF).max(axis=1).astype(np.int64)          # magnitude bits order as magnitudes; non-finite above every finite
    ok = (amax >= FP8_AMAX_LO) & (amax <= FP8_AMAX_HI)
    e = 134 - (amax[ok] >> 7)                                 # 7 - (exponent field - 127)
    scaled = (bf16_values(b[ok]) * np.ldexp(np.float32(1.0), e.astype(np.int32))[:, None]).astype(np.float32)
    c = torch.from_numpy(scaled).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    c[c == 0x80] = 0
    codes[ok] = c
    scales[ok] = np.ldexp(np.float32(1.0), (-e).astype(np.int32))
    return codes, scales


def fp8_dequantize(codes, scales) -> np.ndarray:
    """code * scale as bf16 bits uint16 [n, dim]: exact (4 significant bits, the exponent in range by the domain)."""
    import torch
    c = np.ascontiguousarray(codes, dtype=np.uint8)
    s = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1, 1)
    vals = torch.from_numpy(c).view(torch.float8_e4m3fn).to(torch.float32).numpy() * s
    bits32 = np.ascontiguousarray(vals, dtype=np.float32).view(np.uint32)
    assert not np.any(bits32 & 0xFFFF), "code * scale is not exact in bf16"
    return (bits32 >> 16).astype(np.uint16)


MXFP4_BLOCK = 32                                # components per e8m0 scale
MXFP4_E_MIN = -100                              # the smallest block exponent E; scale bytes E + 127 lie in [27, 185]
_E2M1_MAGNITUDES = np.asarray([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=np.float32)
# the midpoints between neighbouring e2m1 magnitudes; a tie goes to the even mantissa, so it goes UP where the upper code is even
_E2M1_MIDPOINTS = np.asarray([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=np.float32)
_E2M1_TIE_UP = np.asarray([False, True, False, True, False, True, False])


def mxfp4_quantize_reference(bits) -> Tuple[np.ndarray, np.ndarray]:
    """The MXFP4 format of the multi-vector store (csrc/multivec.h) in numpy: bf16 bits uint16 [n, dim], dim % 32 == 0 ->
    (codes uint8 [n, dim / 2], scales uint8 [n, dim / 32]).  Component 2i is the low nibble of byte i, 2i + 1 the high one; a
    nibble is sign | 2 exponent bits | 1 mantissa bit; scale byte s means 2^(s - 127).
      per vector   a non-finite component, or amax outside [2^-60, 2^60]: the zero vector (codes 0x0, scale bytes 127; the
                   store counts these); amax == 0: the zero vector too
      per block of 32 consecutive components
                   bmax == 0                      codes 0, scale byte 127
                   otherwise  E = max(floor(log2 bmax) - 2, -100)   (bmax's exponent bits; a bf16 subnormal takes -100)
                              scale byte = E + 127
                              code_k = e2m1(v_k * 2^-E)   round to nearest, ties to the even mantissa, SATURATING at +-6 (the
                                                          scaled block maximum lies in [4, 8): [7, 8) becomes 6)
                              a -0 code (0x8) is stored as 0x0."""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    assert b.ndim == 2 and b.shape[1] % MXFP4_BLOCK == 0
    n, dim = b.shape
    nb = dim // MXFP4_BLOCK
    codes, scales = np.zeros((n, dim // 2), dtype=np.uint8), np.full((n, nb), 127, dtype=np.uint8)
    if n == 0:
        return codes, scales
    mag = (b & 0x7FFF).astype(np.int64).reshape(n, nb, MXFP4_BLOCK)
    amax = mag.max(axis=(1, 2))                               # magnitude bits order as magnitudes; non-finite above every finite
    ok = (amax >= FP8_AMAX_LO) & (amax <= FP8_AMAX_HI)
    bmax = mag.max(axis=2)
    some = ok[:, None] & (bmax != 0)
    e = np.maximum((bmax >> 7) - 127 - 2, MXFP4_E_MIN)        # floor(log2 bmax) - 2 off the exponent field
    scales[some] = (e[some] + 127).astype(np.uint8)
    mul = np.where(some, np.ldexp(np.float32(1.0), (-e).astype(np.int32)), np.float32(0.0)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        vals = np.where(some[:, :, None], bf16_values(b).reshape(n, nb, MXFP4_BLOCK) * mul[:, :, None], np.float32(0.0))
    a = np.abs(vals).astype(np.float32)[..., None]            # exact: a power of two times a bf16 value (or below every code)
    passed = np.where(_E2M1_TIE_UP, a >= _E2M1_MIDPOINTS, a > _E2M1_MIDPOINTS)
    code = passed.sum(axis=-1).astype(np.uint8)               # the midpoints passed: 0..7, nothing above 6.0 = code 7
    code |= np.where((code != 0) & np.signbit(vals), 8, 0).astype(np.uint8)
    code = code.reshape(n, dim)
    codes[:] = code[:, 0::2] | (code[:, 1::2] << 4)
    return codes, scales


def mxfp4_dequantize(codes, scales) -> np.ndarray:
    """code * 2^(scale byte - 127) as bf16 bits uint16 [n, dim]: exact (2 significant bits, the exponent in range)."""
    c = np.ascontiguousarray(codes, dtype=np.uint8)
    s = np.ascontiguousarray(scales, dtype=np.uint8)
    n, half = c.shape
    dim = 2 * half
    assert s.shape == (n, dim // MXFP4_BLOCK)
    nib = np.empty((n, dim), dtype=np.uint8)
    nib[:, 0::2], nib[:, 1::2] = c & 15, c >> 4
    mags = _E2M1_MAGNITUDES[nib & 7]
    vals = np.where(nib & 8, -mags, mags).astype(np.float32)
    two_e = np.ldexp(np.float32(1.0), s.astype(np.int32) - 127).astype(np.float32)
    out = (vals.reshape(n, dim // MXFP4_BLOCK, MXFP4_BLOCK) * two_e[:, :, None]).astype(np.float32).reshape(n, dim)
    bits32 = np.ascontiguousarray(out).view(np.uint32)
    assert not np.any(bits32 & 0xFFFF), "code * 2^E is not exact in bf16"
    return (bits32 >> 16).astype(np.uint16)


class MultiVectorStore:
    """Device-resident CSR of the per-token vectors of every chunk; document i is collection row i.
    format "bf16": 2 x dim bytes per stored token, 100 k passages of 120 tokens at 1024-d take 24.6 GB.
    format "fp8":  e4m3fn codes and one power-of-two scale per vector (fp8_quantize_reference), dim + 4 bytes per token,
                   12.3 GB for the same; dim % 128 == 0.  Appends take the same bf16 vectors and quantise on the device;
                   MaxSim over it equals, bit for bit, MaxSim over a bf16 store of `export()`.
    format "mxfp4": OCP microscaling FP4, e2m1 codes with one e8m0 scale per 32 components (mxfp4_quantize_reference),
                   dim / 2 + dim / 32 bytes per token (544 at 1024-d), 6.5 GB for the same; dim % 128 == 0.  Appends and the
                   MaxSim identity as for fp8."""

    def __init__(self, dim: int, max_doc_vectors: int = 511, device: int = 0, format: str = "bf16", _handle: Optional[int] = None):
        self.dim, self.max_doc_vectors, self.device = int(dim), int(max_doc_vectors), int(device)
        if format not in FORMATS:
            raise ValueError(f"format={format!r}: expected 'bf16', 'fp8' or 'mxfp4'")
        self.format = format
        if _handle is None:
            h = ctypes.c_uint64()
            if format == "bf16":
                nat.call("hipmv_create", self.dim, self.max_doc_vectors, self.device, ctypes.byref(h))
            else:
                nat.call("hipmv_create_ex", self.dim, self.max_doc_vectors, self.device, FORMATS[format], ctypes.byref(h))
            _handle = h.value
        self._h = _handle

    @classmethod
    def load(cls, path: str, device: int = 0) -> "MultiVectorStore":
        """hipmv_load: a HIPMV001 (bf16), HIPMVQ81 (fp8) or HIPMVQ41 (mxfp4) file, validated before a store exists; the kind is the file's."""
        h = ctypes.c_uint64()
        nat.call("hipmv_load", str(path).encode(), int(device), ctypes.byref(h))
        out, info = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
        nat.call("hipmv_sizes", h.value, out.ctypes.data)
        nat.call("hipmv_format_info", h.value, info.ctypes.data)
        with open(path, "rb") as f:
            cap = int(np.frombuffer(f.read(20)[16:20], dtype=np.int32)[0])
        return cls(int(out[2]), cap, device, format=FORMAT_NAMES[int(info[0])], _handle=h.value)

    def to_fp8(self) -> "MultiVectorStore":
        """hipmv_to_fp8: a new fp8 store of this bf16 store's vectors, byte for byte a fresh fp8 store given them; this one
        stays as it is."""
        h = ctypes.c_uint64()
        nat.call("hipmv_to_fp8", self._h, ctypes.byref(h))
        return MultiVectorStore(self.dim, self.max_doc_vectors, self.device, format="fp8", _handle=h.value)

    def to_mxfp4(self) -> "MultiVectorStore":
        """hipmv_to_mxfp4: a new MXFP4 store of this bf16 store's vectors, byte for byte a fresh one given them; this one
        stays as it is."""
        h = ctypes.c_uint64()
        nat.call("hipmv_to_mxfp4", self._h, ctypes.byref(h))
        return MultiVectorStore(self.dim, self.max_doc_vectors, self.device, format="mxfp4", _handle=h.value)

    def format_info(self) -> Tuple[str, int, int]:
        """(format, bytes per stored vector, vectors stored as zero by the domain guard of fp8 and mxfp4 since creation)"""
        out = np.zeros(4, dtype=np.int64)
        nat.call("hipmv_format_info", self._h, out.ctypes.data)
        return FORMAT_NAMES[int(out[0])], int(out[1]), int(out[2])

    def export_fp8(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(offsets int64 [n + 1], codes uint8 [stored, dim], scales float32 [stored]) of an fp8 store: a test hook."""
        n, nv, _, _ = self.sizes()
        offsets = np.zeros(n + 1, dtype=np.int64)
        codes, scales = np.zeros((max(nv, 1), self.dim), dtype=np.uint8), np.zeros(max(nv, 1), dtype=np.float32)
        nat.call("hipmv_export_fp8", self._h, offsets.ctypes.data, codes.ctypes.data, scales.ctypes.data)
        return offsets, codes[:nv], scales[:nv]

    def export_mxfp4(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(offsets int64 [n + 1], codes uint8 [stored, dim / 2], scales uint8 [stored, dim / 32]) of an MXFP4 store: a test hook."""
        n, nv, _, _ = self.sizes()
        offsets = np.zeros(n + 1, dtype=np.int64)
        codes = np.zeros((max(nv, 1), self.dim // 2), dtype=np.uint8)
        scales = np.zeros((max(nv, 1), self.dim // MXFP4_BLOCK), dtype=np.uint8)
        nat.call("hipmv_export_mxfp4", self._h, offsets.ctypes.data, codes.ctypes.data, scales.ctypes.data)
        return offsets, codes[:nv], scales[:nv]

    def save(self, path: str) -> None:
        nat.call("hipmv_save", self._h, str(path).encode())

    def close(self) -> None:
        if getattr(self, "_h", None):
            try:
                nat.call("hipmv_destroy", self._h)
            finally:
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, vecs, offsets=None) -> None:
        """append(list of uint16 arrays [len_i, dim]) or append(vecs uint16 [total, dim], offsets int64 [n + 1]): bf16 bits."""
        if offsets is None:
            docs = [np.asarray(v, dtype=np.uint16).reshape(-1, self.dim) for v in vecs]
            offsets = np.zeros(len(docs) + 1, dtype=np.int64)
            if docs:
                offsets[1:] = np.cumsum([len(v) for v in docs])
            vecs = np.concatenate(docs) if docs else np.zeros((0, self.dim), np.uint16)
        vecs = np.ascontiguousarray(vecs, dtype=np.uint16)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        keep = vecs if vecs.size else np.zeros(1, np.uint16)        # an empty batch still passes a pointer
        nat.call("hipmv_append", self._h, keep.ctypes.data, offsets.ctypes.data, len(offsets) - 1)

    def append_device(self, vecs, counts) -> None:
        """hipmv_append_dev: vecs a bfloat16 CUDA tensor [n, row_stride, dim] (what encode_colbert returns), counts int32 [n]
        on the host.  The call waits for torch's current stream and returns with the store usable."""
        import torch
        from .index import _stream_ptr
        if vecs.dtype != torch.bfloat16 or vecs.dim() != 3 or not vecs.is_cuda or vecs.shape[2] != self.dim:
            raise ValueError("vecs must be a bfloat16 CUDA tensor [n, row_stride, dim]")
        vecs = vecs.contiguous()
        cnt = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        if len(cnt) != vecs.shape[0]:
            raise ValueError("one count per document")
        nat.call("hipmv_append_dev", self._h, vecs.data_ptr(), int(vecs.shape[1]), cnt.ctypes.data if len(cnt) else None, len(cnt),
                 _stream_ptr())

    def remove_ranges(self, ranges) -> None:
        r = np.ascontiguousarray(ranges, dtype=np.int64).reshape(-1, 2)
        nat.call("hipmv_remove_ranges", self._h, r.ctypes.data if len(r) else None, len(r))

    def sizes(self) -> Tuple[int, int, int, int]:
        """(documents, stored vectors, dim, longest stored document)"""
        out = np.zeros(4, dtype=np.int64)
        nat.call("hipmv_sizes", self._h, out.ctypes.data)
        return tuple(int(v) for v in out)

    def __len__(self) -> int:
        return self.sizes()[0]

    def export(self) -> Tuple[np.ndarray, np.ndarray]:
        """(offsets int64 [n + 1], vecs uint16 [stored, dim] of bf16 bits): a test hook.  Of an fp8 or MXFP4 store: the dequantised bits."""
        n, nv, _, _ = self.sizes()
        offsets, vecs = np.zeros(n + 1, dtype=np.int64), np.zeros((max(nv, 1), self.dim), dtype=np.uint16)
        nat.call("hipmv_export", self._h, offsets.ctypes.data, vecs.ctypes.data)
        return offsets, vecs[:nv]

    def maxsim_info(self) -> Tuple[int, int, int, int]:
        """(valid pairs, padding candidates, document vectors read, 0) of the last MaxSim call on this store; synchronises."""
        out = np.zeros(4, dtype=np.int64)
        nat.call("hipmaxsim_info", self._h, out.ctypes.data)
        return tuple(int(v) for v in out)

    def search_info(self) -> dict:
        """hipmaxsim_search_info (synchronises), of the last maxsim_search* on this store: valid and padding (query,
        document) pairs, document vectors its work items read, its chunks and work items; and three properties of the build
        and this store's dim: R = query rows per pass, G = queries per work item, documents per slice."""
        v = np.zeros(8, dtype=np.int64)
        nat.call("hipmaxsim_search_info", self._h, v.ctypes.data)
        names = ("valid_pairs", "padding_pairs", "doc_vectors_read", "pass_rows", "group_queries", "slice_docs", "chunks", "work_items")
        return {n: int(x) for n, x in zip(names, v)}


    # ---- centroid codes (csrc/maxsim_codes.hip) -----------------------------------------------------------------------
    def attach_centroids(self, centroids) -> None:
        """hipmv_attach_centroids: centroids uint16 [ncent, dim] (bf16 bits), ncent a multiple of 32 in 32..65536.  Every stored
        vector gets its code, the LOWEST c maximising the MaxSim kernels' product with centroid c; later appends are coded as
        they arrive.  Attaching again replaces the table."""
        c = np.ascontiguousarray(centroids, dtype=np.uint16)
        if c.ndim != 2 or c.shape[1] != self.dim:
            raise ValueError(f"centroids must be uint16 [ncent, {self.dim}] (bf16 bits)")
        nat.call("hipmv_attach_centroids", self._h, c.ctypes.data, int(c.shape[0]))

    def detach_centroids(self) -> None:
        nat.call("hipmv_detach_centroids", self._h)

    def centroid_info(self) -> Tuple[int, int, int]:
        """(ncent, or 0 for a store without centroids; coded vectors; bytes of codes)"""
        out = np.zeros(4, dtype=np.int64)
        nat.call("hipmv_centroid_info", self._h, out.ctypes.data)
        return int(out[0]), int(out[1]), int(out[2])

    def centroids(self) -> np.ndarray:
        """the attached table, uint16 [ncent, dim] of bf16 bits"""
        out = np.zeros((max(self.centroid_info()[0], 1), self.dim), dtype=np.uint16)
        nat.call("hipmv_export_centroids", self._h, out.ctypes.data)
        return out

    def codes(self) -> np.ndarray:
        """int32 [stored vectors], the code of every stored vector in store order"""
        nv = self.sizes()[1]
        out = np.zeros(max(nv, 1), dtype=np.int32)
        nat.call("hipmv_export_codes", self._h, out.ctypes.data)
        return out[:nv]

    def gather_f32(self, idx):
        """hipmv_gather_f32_dev: the stored vectors idx (global vector indices, store order) dequantised and widened ->
        float32 CUDA tensor [len(idx), dim]."""
        import torch
        ix = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        out = torch.empty((len(ix), self.dim), dtype=torch.float32, device=f"cuda:{self.device}")
        nat.call("hipmv_gather_f32_dev", self._h, ix.ctypes.data if len(ix) else None, len(ix), out.data_ptr() if len(ix) else None)
        return out

    def pruned_info(self) -> dict:
        """hipmaxsim_pruned_info (synchronises), of the last maxsim_search_pruned* on this store."""
        v = np.zeros(8, dtype=np.int64)
        nat.call("hipmaxsim_pruned_info", self._h, v.ctypes.data)
        names = ("valid_pairs", "padding_pairs", "codes_read", "table_bytes", "chunks", "work_items", "exact_pairs", "slice_docs")
        return {n: int(x) for n, x in zip(names, v)}


def centroid_codes_reference(vectors, centroids) -> np.ndarray:
    """The specification of a code in float64: vectors [n, dim] and centroids [ncent, dim] (values) -> int32 [n], the LOWEST
    index of the largest dot product."""
    v = np.asarray(vectors, dtype=np.float64).reshape(-1, np.asarray(centroids).shape[1])
    c = np.asarray(centroids, dtype=np.float64)
    if len(v) == 0:
        return np.zeros(0, dtype=np.int32)
    return np.argmax(v @ c.T, axis=1).astype(np.int32)      # numpy's argmax returns the first of equal maxima


def centroid_interaction_reference(q, codes_of_docs, centroids) -> np.ndarray:
    """The interaction stage of the pruned search in float64: q [Lq, dim] (values), codes_of_docs a list of int arrays (one
    per document), centroids [ncent, dim] -> float64 [documents], mean_i max_j q_i . centroid[code_j]; a document without
    codes gets -inf (it is never a candidate)."""
    qv = np.asarray(q, dtype=np.float64)
    table = qv @ np.asarray(centroids, dtype=np.float64).T           # [Lq, ncent]
    out = np.full(len(codes_of_docs), -np.inf, dtype=np.float64)
    for d, codes in enumerate(codes_of_docs):
        codes = np.asarray(codes, dtype=np.int64).reshape(-1)
        if len(codes) and len(qv):
            out[d] = table[:, codes].max(axis=1).sum() / len(qv)
    return out


def default_ncent(stored_vectors: int) -> int:
    """ColBERTv2's rule: the power of two nearest 16 sqrt(stored vectors), clamped to 32..65536."""
    target = 16.0 * float(max(int(stored_vectors), 1)) ** 0.5
    lo = 2 ** int(np.floor(np.log2(target)))
    best = lo if target - lo <= 2 * lo - target else 2 * lo
    return int(min(max(best, 32), 65536))


def train_token_centroids(store: MultiVectorStore, ncent: int = 0, iters: int = 6, seed: int = 0,
                          max_points_per_centroid: int = 256) -> np.ndarray:
    """Centroids for store.attach_centroids: a strided sample of at most ncent x max_points_per_centroid stored vectors
    (gather_f32: the stored values, dequantised), spherical k-means on the device (HipIVFIndex.build with the inner-product
    metric, whose centroids are normalised in fp64), rounded to bf16.  ncent = 0: default_ncent(stored vectors), cut down to
    the multiple of 32 the sample can fill.  -> uint16 [ncent, dim] of bf16 bits."""
    from .ivf import HipIVFIndex
    nv = store.sizes()[1]
    if ncent == 0:
        ncent = default_ncent(nv)
        while ncent > 32 and ncent > nv:
            ncent //= 2
    ncent = int(ncent)
    if ncent % 32 or not 32 <= ncent <= 65536:
        raise ValueError(f"ncent must be a multiple of 32 in 32..65536 (got {ncent})")
    if nv < ncent:
        raise ValueError(f"the store holds {nv} vectors: fewer than ncent = {ncent}")
    n_sample = min(nv, ncent * int(max_points_per_centroid))
    idx = (np.arange(n_sample, dtype=np.int64) * nv) // n_sample      # strided over the store: ascending, distinct
    ivf = HipIVFIndex(store.dim, ncent, "ip", device=store.device)
    try:
        ivf.build(store.gather_f32(idx), iters=iters, seed=seed)
        return bf16_bits(ivf.centroids())
    finally:
        ivf.close()


def _pruned_outputs(nq, k, ncand):
    return max(int(k), 1), max(int(ncand), 1)


def maxsim_search_pruned(store: MultiVectorStore, q_vecs, q_counts, scopes, scope_of_query, k: int, ncand: int, id_base: int = 0,
                         want_candidates: bool = False):
    """hipmaxsim_search_pruned: maxsim_search's arguments and result, the exact stage seeing only the best `ncand` documents
    of the scope by centroid interaction (1 <= k <= ncand <= 256; the store has centroids attached).  With want_candidates,
    -> (scores, ids, cand_ids int64 [nq, ncand], cand_scores float32 [nq, ncand])."""
    from .index import pack_scopes
    qv = np.ascontiguousarray(q_vecs, dtype=np.uint16)
    qc = np.ascontiguousarray(q_counts, dtype=np.int32).reshape(-1)
    if qv.ndim != 3 or qv.shape[2] != store.dim or len(qc) != qv.shape[0]:
        raise ValueError("q_vecs must be [nq, q_stride, dim] and q_counts [nq]")
    nq = qv.shape[0]
    ranges, offsets, soq = pack_scopes(scopes, scope_of_query, nq)
    kk, cc = _pruned_outputs(nq, k, ncand)
    scores, ids = np.zeros((nq, kk), np.float32), np.zeros((nq, kk), np.int64)
    cids, csc = np.zeros((nq, cc), np.int64), np.zeros((nq, cc), np.float32)
    nat.call("hipmaxsim_search_pruned", store._h, qv.ctypes.data, qc.ctypes.data, int(qv.shape[1]), nq, int(k), int(ncand),
             ranges.ctypes.data, offsets.ctypes.data, len(offsets) - 1, soq.ctypes.data, int(id_base), scores.ctypes.data, ids.ctypes.data,
             cids.ctypes.data if want_candidates else None, csc.ctypes.data if want_candidates else None)
    return (scores, ids, cids, csc) if want_candidates else (scores, ids)


def maxsim_search_pruned_device(store: MultiVectorStore, q_vecs, q_counts, scopes, scope_of_query, k: int, ncand: int, id_base: int = 0,
                                want_candidates: bool = False):
    """hipmaxsim_search_pruned_dev on torch's current stream: maxsim_search_device's arguments and `ncand`.  -> CUDA tensors
    (scores, ids) or, with want_candidates, (scores, ids, cand_ids, cand_scores); nothing is synchronised."""
    import torch
    from .index import _stream_ptr, pack_scopes
    if q_vecs.dtype != torch.bfloat16 or q_vecs.dim() != 3 or not q_vecs.is_cuda or q_vecs.shape[2] != store.dim:
        raise ValueError("q_vecs must be a bfloat16 CUDA tensor [nq, q_stride, dim]")
    if q_counts.dtype != torch.int32 or not q_counts.is_cuda or q_counts.numel() != q_vecs.shape[0]:
        raise ValueError("q_counts must be an int32 CUDA tensor [nq]")
    qv, qc = q_vecs.contiguous(), q_counts.contiguous()
    nq = qv.shape[0]
    ranges, offsets, soq = pack_scopes(scopes, scope_of_query, nq)
    kk, cc = _pruned_outputs(nq, k, ncand)
    scores = torch.empty((nq, kk), dtype=torch.float32, device=qv.device)
    ids = torch.empty((nq, kk), dtype=torch.int64, device=qv.device)
    cids = torch.empty((nq, cc), dtype=torch.int64, device=qv.device) if want_candidates else None
    csc = torch.empty((nq, cc), dtype=torch.float32, device=qv.device) if want_candidates else None
    nat.call("hipmaxsim_search_pruned_dev", store._h, qv.data_ptr(), qc.data_ptr(), int(qv.shape[1]), nq, int(k), int(ncand),
             ranges.ctypes.data, offsets.ctypes.data, len(offsets) - 1, soq.ctypes.data, int(id_base), scores.data_ptr(), ids.data_ptr(),
             cids.data_ptr() if want_candidates else None, csc.data_ptr() if want_candidates else None, _stream_ptr())
    return (scores, ids, cids, csc) if want_candidates else (scores, ids)


def maxsim(store: MultiVectorStore, q_vecs, q_counts, cand_ids, k: int, id_base: int = 0):
    """hipmaxsim_host: q_vecs uint16 [nq, q_stride, dim] (bf16 bits), q_counts int32 [nq], cand_ids int64 [nq, depth], all on
    the host.  -> (scores float32 [nq, k], ids int64 [nq, k], positions int32 [nq, k], pair scores float32 [nq, depth])."""
    qv = np.ascontiguousarray(q_vecs, dtype=np.uint16)
    qc = np.ascontiguousarray(q_counts, dtype=np.int32).reshape(-1)
    cand = np.ascontiguousarray(cand_ids, dtype=np.int64)
    if qv.ndim != 3 or qv.shape[2] != store.dim or cand.ndim != 2 or cand.shape[0] != qv.shape[0] or len(qc) != qv.shape[0]:
        raise ValueError("q_vecs must be [nq, q_stride, dim], q_counts [nq] and cand_ids [nq, depth]")
    nq, depth = cand.shape
    kk = max(int(k), 1)
    scores, ids = np.zeros((nq, kk), np.float32), np.zeros((nq, kk), np.int64)
    pos, pairs = np.zeros((nq, kk), np.int32), np.zeros((nq, max(depth, 1)), np.float32)
    nat.call("hipmaxsim_host", store._h, qv.ctypes.data, qc.ctypes.data, int(qv.shape[1]), nq, cand.ctypes.data, depth, int(id_base),
             int(k), pairs.ctypes.data, scores.ctypes.data, ids.ctypes.data, pos.ctypes.data)
    return scores, ids, pos, pairs


def maxsim_device(store: MultiVectorStore, q_vecs, q_counts, cand_ids, k: int, id_base: int = 0, want_pairs: bool = True):
    """hipmaxsim_dev on torch's current stream: q_vecs bfloat16 [nq, q_stride, dim] and q_counts int32 [nq] (the outputs of
    encode_colbert), cand_ids int64 [nq, depth] (what hybrid_search*_device returned), all CUDA tensors.  -> CUDA tensors
    (scores [nq, k], ids [nq, k], positions [nq, k], pair scores [nq, depth] or None); nothing is synchronised."""
    import torch
    from .index import _stream_ptr
    if q_vecs.dtype != torch.bfloat16 or q_vecs.dim() != 3 or not q_vecs.is_cuda or q_vecs.shape[2] != store.dim:
        raise ValueError("q_vecs must be a bfloat16 CUDA tensor [nq, q_stride, dim]")
    if q_counts.dtype != torch.int32 or not q_counts.is_cuda or q_counts.numel() != q_vecs.shape[0]:
        raise ValueError("q_counts must be an int32 CUDA tensor [nq]")
    if cand_ids.dtype != torch.int64 or cand_ids.dim() != 2 or not cand_ids.is_cuda or cand_ids.shape[0] != q_vecs.shape[0]:
        raise ValueError("cand_ids must be an int64 CUDA tensor [nq, depth]")
    qv, qc, cand = q_vecs.contiguous(), q_counts.contiguous(), cand_ids.contiguous()
    nq, depth = cand.shape
    kk = max(int(k), 1)
    dev = cand.device
    scores = torch.empty((nq, kk), dtype=torch.float32, device=dev)
    ids = torch.empty((nq, kk), dtype=torch.int64, device=dev)
    pos = torch.empty((nq, kk), dtype=torch.int32, device=dev)
    pairs = torch.empty((nq, depth), dtype=torch.float32, device=dev) if want_pairs else None
    nat.call("hipmaxsim_dev", store._h, qv.data_ptr(), qc.data_ptr(), int(qv.shape[1]), nq, cand.data_ptr(), depth, int(id_base), int(k),
             pairs.data_ptr() if want_pairs else None, scores.data_ptr(), ids.data_ptr(), pos.data_ptr(), _stream_ptr())
    return scores, ids, pos, pairs


def maxsim_search(store: MultiVectorStore, q_vecs, q_counts, scopes, scope_of_query, k: int, id_base: int = 0):
    """hipmaxsim_search_scoped: the exact MaxSim top k over EVERY document of each query's scope.  q_vecs uint16
    [nq, q_stride, dim] (bf16 bits) and q_counts int32 [nq] on the host; `scopes` / `scope_of_query` as in
    HipFlatIndex.search_scoped, the ranges over the store's documents.  -> (scores float32 [nq, k], ids int64 [nq, k]): the
    documents of the scope that hold a vector by (score descending, id ascending), id = document + id_base; padding
    (-FLT_MAX, -1).  A pair's score is the bits `maxsim` gives it."""
    from .index import pack_scopes
    qv = np.ascontiguousarray(q_vecs, dtype=np.uint16)
    qc = np.ascontiguousarray(q_counts, dtype=np.int32).reshape(-1)
    if qv.ndim != 3 or qv.shape[2] != store.dim or len(qc) != qv.shape[0]:
        raise ValueError("q_vecs must be [nq, q_stride, dim] and q_counts [nq]")
    nq = qv.shape[0]
    ranges, offsets, soq = pack_scopes(scopes, scope_of_query, nq)
    kk = max(int(k), 1)
    scores, ids = np.zeros((nq, kk), np.float32), np.zeros((nq, kk), np.int64)
    nat.call("hipmaxsim_search_scoped", store._h, qv.ctypes.data, qc.ctypes.data, int(qv.shape[1]), nq, int(k), ranges.ctypes.data,
             offsets.ctypes.data, len(offsets) - 1, soq.ctypes.data, int(id_base), scores.ctypes.data, ids.ctypes.data)
    return scores, ids


def maxsim_search_device(store: MultiVectorStore, q_vecs, q_counts, scopes, scope_of_query, k: int, id_base: int = 0, out=None):
    """hipmaxsim_search_scoped_dev on torch's current stream: q_vecs bfloat16 [nq, q_stride, dim] and q_counts int32 [nq] CUDA
    tensors (the outputs of encode_colbert); the scope tables are host data, copied before the call returns.  -> CUDA tensors
    (scores float32 [nq, k], ids int64 [nq, k]); nothing is synchronised."""
    import torch
    from .index import _stream_ptr, pack_scopes
    if q_vecs.dtype != torch.bfloat16 or q_vecs.dim() != 3 or not q_vecs.is_cuda or q_vecs.shape[2] != store.dim:
        raise ValueError("q_vecs must be a bfloat16 CUDA tensor [nq, q_stride, dim]")
    if q_counts.dtype != torch.int32 or not q_counts.is_cuda or q_counts.numel() != q_vecs.shape[0]:
        raise ValueError("q_counts must be an int32 CUDA tensor [nq]")
    qv, qc = q_vecs.contiguous(), q_counts.contiguous()
    nq = qv.shape[0]
    ranges, offsets, soq = pack_scopes(scopes, scope_of_query, nq)
    kk = max(int(k), 1)
    if out is None:
        out = (torch.empty((nq, kk), dtype=torch.float32, device=qv.device), torch.empty((nq, kk), dtype=torch.int64, device=qv.device))
    scores, ids = out
    nat.call("hipmaxsim_search_scoped_dev", store._h, qv.data_ptr(), qc.data_ptr(), int(qv.shape[1]), nq, int(k), ranges.ctypes.data,
             offsets.ctypes.data, len(offsets) - 1, soq.ctypes.data, int(id_base), scores.data_ptr(), ids.data_ptr(), _stream_ptr())
    return scores, ids


def maxsim_search_reference(pair_scores, valid, ranges, scope_offsets, scope_of_query, k: int, id_base: int = 0):
    """The selection of hipmaxsim_search_scoped restated in numpy: the specification of its order and padding (pair scores
    are hipmaxsim's by definition).  pair_scores float32 [nq, n_docs] and valid bool [nq, n_docs] (query i has a vector and
    document d holds one); ranges int64 [n_ranges, 2] half-open, scope_offsets [n_scopes + 1], scope_of_query [nq].  Query i
    ranks the valid documents inside the ranges of ITS scope by (score descending, id ascending); id = document + id_base;
    ranks past them get (-FLT_MAX, -1).  -> (scores float32 [nq, k], ids int64 [nq, k])."""
    ps = np.asarray(pair_scores, dtype=np.float32)
    ok = np.asarray(valid, dtype=bool)
    rg = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    off = np.asarray(scope_offsets, dtype=np.int64).reshape(-1)
    soq = np.asarray(scope_of_query, dtype=np.int64).reshape(-1)
    nq = ps.shape[0]
    scores = np.full((nq, k), NEG_MAX, dtype=np.float32)
    ids = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        s = int(soq[i])
        docs = [d for lo, hi in rg[off[s]:off[s + 1]] for d in range(int(lo), int(hi)) if ok[i, d]]
        docs.sort(key=lambda d: (-float(ps[i, d]), d))
        for r, d in enumerate(docs[:k]):
            scores[i, r], ids[i, r] = ps[i, d], d + int(id_base)
    return scores, ids
