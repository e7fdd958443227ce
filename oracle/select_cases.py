"""
oracle/select_cases.py -- designed inputs for every selection kernel behind csrc/topk_device.h: the canonical merge
(hiprag_merge_topk_dev), reciprocal-rank fusion (hiprrf_fuse / hiprrf_fuse_dev) and the BM25 selectors, shared by the GPU
tests (tests/test_selection_gpu.py) and by the CPU tests that prove the cases can tell a right kernel from a subtly wrong
one (tests/test_select_cases_cpu.py).

TEST INFRASTRUCTURE ONLY (see oracle/hybrid_oracle.py header).  numpy only: importable without torch and without the
library.  Every generator is deterministic (seeded from the case's own parameters); a *_cases() function returns light
specs whose .name is the report line, build_*() turns a spec into arrays.

NaN scores are excluded on purpose: the kernels order by an integer image of the score bits, in which a NaN lands above
+inf or below -inf depending on its sign bit, while a numeric sort has no order for it at all.  The order of a NaN is
unspecified (include/hiprag.h says so) and nothing here pins it.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import hybrid_oracle as ho

DBL_MAX = float(np.finfo(np.float64).max)
FLT_MAX = np.finfo(np.float32).max
F32_DENORM = np.float32(2.0 ** -149)        # smallest positive fp32 denormal


def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode())


# ======================================================================================================================
# Merge
# ======================================================================================================================
MERGE_NQ = 5
MERGE_TILE = 4096            # kTile of topk_device.h
MERGE_PATTERNS = ("distinct", "plateau", "levels", "pad", "dup", "extremes", "zeros")
GAP_ID_BASE = 10 ** 15       # ids of the gap elements: valid-looking, never a legitimate answer


def merge_kernel_shape(n_parts: int, k_in: int, k_out: int) -> str:
    """The dispatch rule of hiprag_merge_topk_dev, restated: 'wave/NPL<n>' or 'stream/<tiles>' (tiles wg_stream_topk runs)."""
    M = n_parts * k_in
    if k_out <= 64 and M <= 64 * 8:
        npl = (M + 63) // 64
        return "wave/NPL%d" % (1 if npl <= 1 else 2 if npl <= 2 else 4 if npl <= 4 else 8)
    if M <= MERGE_TILE:
        return "stream/1"
    fresh = MERGE_TILE - k_out                      # every later tile carries k_out winners
    return "stream/%d" % (1 + (M - MERGE_TILE + fresh - 1) // fresh)


# (n_parts, k_in, k_out, gap, the kernel shape it must select)
def _merge_shapes() -> List[Tuple[int, int, int, int, str]]:
    out = []
    wave = [(1, 1, 1), (1, 63, 1), (63, 1, 1), (8, 8, 1), (64, 1, 1), (1, 64, 1), (5, 13, 2), (2, 64, 2), (3, 43, 4),
            (4, 64, 4), (257, 1, 8), (7, 73, 8), (8, 64, 8), (512, 1, 8), (1, 512, 8)]
    for n_parts, k_in, npl in wave:
        for k_out in (1, 10, 64):
            out.append((n_parts, k_in, k_out, 0 if k_out == 10 else 7, "wave/NPL%d" % npl))
    out += [
        (27, 19, 10, 7, "stream/1"),          # M = 513: one past the wave kernel
        (8, 8, 65, 0, "stream/1"),            # M = 64, k_out one past the wave kernel
        (5, 8, 100, 3, "stream/1"),           # M = 40 < k_out: more ranks than candidates
        (65, 63, 10, 0, "stream/1"),          # M = 4095
        (16, 256, 100, 5, "stream/1"),        # M = 4096: the tile exactly full
        (17, 241, 10, 0, "stream/2"),         # M = 4097: one entry in the second tile
        (7937, 1, 256, 1, "stream/3"),        # M = 2 * 4096 - 256 + 1: the third tile holds exactly one entry
        (48, 256, 256, 0, "stream/4"),        # M = 3 * 4096: the scoped path's largest (48 parts x 256); 3840 fresh per tile
        (4, 1025, 4095, 2, "stream/5"),       # M = 4100 at the largest legal k_out: four tiles of ONE fresh entry each
        (9, 1000, 4095, 2, "stream/4905"),    # M = 9000 at the largest legal k_out: one fresh entry per tile (see below)
    ]
    return out


# wg_stream_topk runs k_out selection rounds per tile and a later tile brings in 4096 - k_out fresh candidates, so a call
# costs about tiles * k_out rounds of ~2 us on an MI355X.  M = 9000 at k_out = 4095 is 4905 tiles * 4095 rounds: measured
# ~40 s per launch, whatever the number of queries (one workgroup each).  The GPU test therefore runs the cases of that
# shape TOGETHER (merge_batched_gpu_cases: all patterns stacked along the query axis, one launch per metric and call, the
# launches side by side on streams of their own) and every other case on its own (merge_gpu_cases); (4, 1025, 4095) puts the
# same property -- the largest legal k_out, every winner carried through tiles of one fresh entry -- into a 0.1 s case too.
MERGE_GPU_MAX_ROUNDS = 100_000


def merge_rounds(spec: "MergeSpec") -> int:
    kernel = merge_kernel_shape(spec.n_parts, spec.k_in, spec.k_out)
    return int(kernel.split("/")[1]) * spec.k_out if kernel.startswith("stream/") else spec.k_out


def merge_gpu_cases() -> List["MergeSpec"]:
    return [s for s in merge_cases() if merge_rounds(s) <= MERGE_GPU_MAX_ROUNDS]


def merge_batched_gpu_cases() -> List["MergeSpec"]:
    return [s for s in merge_cases() if merge_rounds(s) > MERGE_GPU_MAX_ROUNDS]


def stack_merge_cases(cases: List["MergeCase"]) -> Tuple[np.ndarray, np.ndarray, int]:
    """Cases of one shape, gap and metric as ONE input of len(cases) * nq queries: scores / ids [n_parts, part_stride] with
    part p = the cases' parts p one after the other, then the gap elements of the first case; returns them and part_stride."""
    sp = cases[0].spec
    assert all((c.spec.n_parts, c.spec.nq, c.spec.k_in, c.spec.k_out, c.spec.gap, c.spec.metric) ==
               (sp.n_parts, sp.nq, sp.k_in, sp.k_out, sp.gap, sp.metric) for c in cases)
    n = sp.nq * sp.k_in
    scores = np.concatenate([c.scores[:, :n] for c in cases] + [cases[0].scores[:, n:]], axis=1)
    ids = np.concatenate([c.ids[:, :n] for c in cases] + [cases[0].ids[:, n:]], axis=1)
    return np.ascontiguousarray(scores), np.ascontiguousarray(ids), len(cases) * n + sp.gap


MERGE_SHAPES = _merge_shapes()


@dataclass(frozen=True)
class MergeSpec:
    n_parts: int
    nq: int
    k_in: int
    k_out: int
    gap: int
    metric: int
    pattern: str
    kernel: str          # expected kernel shape

    @property
    def M(self) -> int:
        return self.n_parts * self.k_in

    @property
    def part_stride(self) -> int:
        return self.nq * self.k_in + self.gap

    @property
    def name(self) -> str:
        return "%s-%dx%d-k%d-gap%d-%s" % (self.pattern, self.n_parts, self.k_in, self.k_out, self.gap,
                                          "ip" if self.metric == ho.METRIC_IP else "l2")


def merge_pattern_fits(pattern: str, n_parts: int, k_in: int, k_out: int) -> bool:
    M = n_parts * k_in
    if pattern == "levels":
        return M > k_out and M >= 2          # rank k_out must fall inside a plateau with members on both sides
    if pattern == "dup":
        return n_parts >= 2                  # the same (score, id) in two parts
    return True


def merge_cases() -> List[MergeSpec]:
    out = []
    for n_parts, k_in, k_out, gap, kernel in MERGE_SHAPES:
        for metric in (ho.METRIC_IP, ho.METRIC_L2):
            for pattern in MERGE_PATTERNS:
                if merge_pattern_fits(pattern, n_parts, k_in, k_out):
                    out.append(MergeSpec(n_parts, MERGE_NQ, k_in, k_out, gap, metric, pattern, kernel))
    return out


@dataclass
class MergeCase:
    spec: MergeSpec
    scores: np.ndarray   # float64 [n_parts, part_stride]: part p = scores[p, :nq * k_in] as [nq, k_in], then `gap` elements
    ids: np.ndarray      # int64, same layout

    def parts(self):
        """The parts as the oracle takes them: two lists of n_parts arrays [nq, k_in]."""
        s, n = self.spec, self.spec.nq * self.spec.k_in
        return ([self.scores[p, :n].reshape(s.nq, s.k_in) for p in range(s.n_parts)],
                [self.ids[p, :n].reshape(s.nq, s.k_in) for p in range(s.n_parts)])

    def flat(self):
        """Per query, all candidates in the kernel's input order (part-major): scores [nq, M], ids [nq, M]."""
        ps, pi = self.parts()
        return np.concatenate(ps, axis=1), np.concatenate(pi, axis=1)

    def oracle(self):
        ps, pi = self.parts()
        return ho.merge_partial_topk(ps, pi, self.spec.k_out, self.spec.metric)


_EXTREME_POOL = np.array([DBL_MAX, -DBL_MAX, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, 1e-40, -1e-40, 1.0,
                          np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), -1.0, np.nextafter(-1.0, -2.0), 3.0e38, 3.5e38,
                          np.nextafter(DBL_MAX, 0.0)], dtype=np.float64)


def _spread_order(rng, n_parts: int, k_in: int) -> np.ndarray:
    """All M positions, ordered so that every prefix is spread over the parts as evenly as it can be."""
    cols = np.stack([rng.permutation(k_in) for _ in range(n_parts)])        # [n_parts, k_in]
    order = []
    for r in range(k_in):
        for p in rng.permutation(n_parts):
            order.append(p * k_in + cols[p, r])
    return np.asarray(order, dtype=np.int64)


def build_merge_case(spec: MergeSpec) -> MergeCase:
    """Scores are designed as GOODNESS g (larger is better) and stored as g for inner product, -g for L2 (exact), except
    `zeros`, which is designed on the stored scores themselves."""
    rng = np.random.default_rng(_seed("merge", spec.n_parts, spec.k_in, spec.k_out, spec.gap, spec.metric, spec.pattern))
    n_parts, nq, k_in, k_out, M = spec.n_parts, spec.nq, spec.k_in, spec.k_out, spec.M
    sign = 1.0 if spec.metric == ho.METRIC_IP else -1.0
    g = np.empty((nq, M), dtype=np.float64)
    ids = np.empty((nq, M), dtype=np.int64)
    for q in range(nq):
        # a random permutation: the lowest ids sit in late parts and late positions as often as in early ones
        ids[q] = rng.permutation(M) * 3 + 1000 + (q % 2) * (1 << 40)
        g[q] = rng.standard_normal(M) * 10.0
    pat = spec.pattern
    if pat == "distinct":
        g[0] = -np.sort(-g[0])      # best first: every winner sits in the first tile and must survive every carry
        g[1] = np.sort(g[1])        # best last: every winner sits in the last tile (or the last lanes)
    if pat == "plateau":
        for q in range(nq):
            g[q] = (0.5, -3.25, 1e300, 7.0, -1e-300)[q % 5]
    elif pat == "levels":
        n_hi = k_out // 2
        n_mid = min(M - n_hi, k_out - n_hi + max(1, (M - k_out) // 2))
        assert n_hi < k_out < n_hi + n_mid and n_hi + n_mid <= M
        for q in range(nq):
            order = _spread_order(rng, n_parts, k_in)
            g[q] = -2.5
            g[q, order[:n_mid]] = 0.75                       # the plateau that holds rank k_out, over all parts
            g[q, order[n_mid:n_mid + n_hi]] = 4.0
    elif pat == "pad":
        hole = rng.random((nq, M)) < 1.0 / 3.0
        if n_parts >= 2:
            p = n_parts // 2
            hole[:, p * k_in:(p + 1) * k_in] = True          # one whole part is padding
        hole[0, :] = True                                    # query 0 has nothing at all
        ids[hole] = -1
        g[hole] = DBL_MAX                                    # a score that would win if padding were ranked
    elif pat == "dup":
        nd = min(3, k_in)
        for q in range(nq):
            for j in range(nd):
                a, b = j, (n_parts - 1) * k_in + (k_in - 1 - j)
                g[q, a] = 100.0 + j                          # near the top, so both copies reach the output
                g[q, b], ids[q, b] = g[q, a], ids[q, a]
    elif pat == "extremes":
        for q in range(nq):
            g[q] = rng.choice(_EXTREME_POOL, size=M)
    elif pat == "zeros":
        for q in range(nq):
            n_pos = min(k_out // 2, M // 4)
            n_neg = M // 4
            order = rng.permutation(M)
            g[q] = 0.0
            g[q, order[:n_pos]] = rng.integers(1, 4, size=n_pos).astype(np.float64)
            g[q, order[n_pos:n_pos + n_neg]] = -rng.integers(1, 4, size=n_neg).astype(np.float64)
            zpos = order[n_pos + n_neg:]
            zpos = zpos[np.argsort(ids[q, zpos])]            # zero entries by ascending id, in four blocks - + - +
            blk = (np.arange(len(zpos)) * 4) // max(len(zpos), 1)
            g[q, zpos[blk % 2 == 0]] = -0.0                  # the lowest ids hold -0.0
        g = g * sign                                         # undo the flip below: this pattern is laid out on the scores
    s = g * sign
    scores = np.empty((n_parts, spec.part_stride), dtype=np.float64)
    idbuf = np.empty((n_parts, spec.part_stride), dtype=np.int64)
    n = nq * k_in
    for p in range(n_parts):
        scores[p, :n] = s[:, p * k_in:(p + 1) * k_in].reshape(-1)
        idbuf[p, :n] = ids[:, p * k_in:(p + 1) * k_in].reshape(-1)
    if spec.gap:
        scores[:, n:] = sign * 1e308                         # would win
        idbuf[:, n:] = GAP_ID_BASE + np.arange(n_parts * spec.gap).reshape(n_parts, spec.gap)
    return MergeCase(spec, scores, idbuf)


# ======================================================================================================================
# RRF
# ======================================================================================================================
RRF_DEPTHS = ((0, 7), (7, 0), (1, 1), (63, 65), (64, 64), (50, 7))
# the last one: a document of both lists scores -0.0 + -0.0 = -0.0, one of a single list -0.0 + 0.0 = +0.0; they tie
RRF_WEIGHTS = ((60.0, 1.0, 1.0), (60.0, 0.7, 0.3), (0.0, 1.0, 1.0), (-0.5, 1.0, 1.0), (60.0, 1.0, 0.0), (60.0, 0.0, 0.0),
               (60.0, 1.0, -1.0), (60.0, -0.0, -0.0))
RRF_NQ = 4


@dataclass(frozen=True)
class RrfSpec:
    depth_a: int
    depth_b: int
    nq: int
    k: int
    c: float
    w_a: float
    w_b: float

    @property
    def name(self) -> str:
        return "rrf-%d+%d-nq%d-k%d-c%g-w%g,%g" % (self.depth_a, self.depth_b, self.nq, self.k, self.c, self.w_a, self.w_b)


def rrf_cases() -> List[RrfSpec]:
    out = []
    for da, db in RRF_DEPTHS:
        for k in (1, 10, da + db + 5):
            for c, wa, wb in RRF_WEIGHTS:
                out.append(RrfSpec(da, db, RRF_NQ, k, c, wa, wb))
    out.append(RrfSpec(2048, 2048, 2, 2048 + 2048 + 5, 60.0, 0.7, 0.3))      # the depth limit, once
    return out


def build_rrf_case(spec: RrfSpec) -> Tuple[np.ndarray, np.ndarray]:
    """ids_a [nq, depth_a], ids_b [nq, depth_b], int64.  Ids come from a universe smaller than the two lists together, so
    an id repeats inside a list (its first occurrence defines the rank) and sits in both lists at different ranks; about
    one entry in seven is a -1 hole, in the middle of the list; odd queries use ids just below 2^62."""
    rng = np.random.default_rng(_seed("rrf", spec.depth_a, spec.depth_b, spec.nq))     # one content per depth pair
    da, db, nq = spec.depth_a, spec.depth_b, spec.nq
    uni = max(2, (da + db) * 2 // 3)
    a = np.empty((nq, da), dtype=np.int64)
    b = np.empty((nq, db), dtype=np.int64)
    for q in range(nq):
        for lst, depth in ((a, da), (b, db)):
            u = rng.integers(0, uni, size=depth)
            v = (1 << 62) - 1 - u * 5 if q % 2 else 17 + u * 3
            if depth >= 3:
                v[1:-1][rng.random(depth - 2) < 1.0 / 7.0] = -1
            lst[q] = v
    if da == 1 and db == 1:            # the four possible one-entry pairs
        a[:, 0] = (5, 5, -1, -1)
        b[:, 0] = (5, 9, 4, -1)
    return a, b


# ======================================================================================================================
# BM25 selectors, driven through one-term postings: the accumulator array IS the designed array
# ======================================================================================================================
BM25_NDOCS = (1, 3, 4095, 4096, 4097, 9215, 9216, 9217, 2 * 9216 + 5, 16386)
BM25_K_WAVE = (1, 33, 50, 64)         # tiled path by default, select_wave_kernel under HIPBM25_GLOBAL_ACC=1
BM25_K_F32 = (65, 200)                # select_f32_kernel + bm25_finish_kernel
BM25_PATTERNS = ("exactly_k", "k_minus_1", "all_equal", "descending", "ascending", "plateau_share", "plateau_tile",
                 "plateau_quarter", "tail", "winner_per_share", "denormal", "flt_max", "crowd")
BM25_SHARE = 4096                     # kSelPerWave: one wave's share in select_wave_kernel, one chunk in select_f32_kernel
BM25_TILE = 9216                      # kTileDocs of the tiled path; a wave of it filters a quarter, 2304 documents


@dataclass(frozen=True)
class Bm25Spec:
    n_docs: int
    k: int
    pattern: str

    @property
    def paths(self) -> Tuple[str, ...]:
        return ("tiled", "global") if self.k <= 64 else ("f32",)

    @property
    def name(self) -> str:
        return "%s-n%d-k%d" % (self.pattern, self.n_docs, self.k)


def bm25_plateau_boundary(pattern: str, n_docs: int) -> Optional[int]:
    """The document id the rank-k plateau of a plateau_* case straddles, or None if n_docs has no such boundary."""
    unit = {"plateau_share": BM25_SHARE, "plateau_tile": BM25_TILE, "plateau_quarter": BM25_TILE // 4}[pattern]
    if pattern == "plateau_quarter":
        b = 3 * unit if n_docs > 3 * unit else unit          # 6912 is a quarter boundary that is no multiple of 4096
    else:
        b = (n_docs - 1) // unit * unit                      # the last multiple with at least one document behind it
    return b if 0 < b < n_docs else None


def bm25_pattern_fits(pattern: str, n_docs: int, k: int) -> bool:
    if pattern.startswith("plateau_"):
        return bm25_plateau_boundary(pattern, n_docs) is not None
    if pattern == "tail":
        return n_docs % 4 != 0 and n_docs > 4
    if pattern == "winner_per_share":
        return n_docs > BM25_SHARE
    return True


def bm25_select_cases() -> List[Bm25Spec]:
    return [Bm25Spec(n, k, pat) for n in BM25_NDOCS for pat in BM25_PATTERNS for k in BM25_K_WAVE + BM25_K_F32
            if bm25_pattern_fits(pat, n, k)]


def bm25_accumulators(spec: Bm25Spec) -> np.ndarray:
    """The designed fp32 accumulator array [n_docs]; 0 = the document is not in the posting list."""
    rng = np.random.default_rng(_seed("bm25", spec.n_docs, spec.k, spec.pattern))
    n, k, pat = spec.n_docs, spec.k, spec.pattern
    low = lambda size: (rng.random(size) * 0.4 + 0.05).astype(np.float32)      # background scores, all below 0.5
    acc = np.zeros(n, dtype=np.float32)
    if pat in ("exactly_k", "k_minus_1"):
        m = min(n, k if pat == "exactly_k" else k - 1)
        acc[rng.choice(n, size=m, replace=False)] = (rng.random(m) + 0.5).astype(np.float32)
    elif pat == "all_equal":
        acc[:] = 1.5
    elif pat == "descending":
        acc[:] = np.arange(n, 0, -1, dtype=np.float32)
    elif pat == "ascending":
        acc[:] = np.arange(1, n + 1, dtype=np.float32)
    elif pat.startswith("plateau_"):
        b = bm25_plateau_boundary(pat, n)
        lo, hi = max(0, b - k), min(n, b + k)                 # up to k members on each side of the boundary
        acc[:] = low(n)
        acc[lo:hi] = 0.75
        rest = np.concatenate([np.arange(0, lo), np.arange(hi, n)])
        n_hi = min(k // 2, len(rest))                         # fewer than k above the plateau: rank k lies inside it
        acc[rng.choice(rest, size=n_hi, replace=False)] = (rng.random(n_hi) + 1.0).astype(np.float32)
    elif pat == "tail":
        t = n % 4
        acc[:] = low(n)
        acc[n - t:] = (np.arange(t, 0, -1) + 1.0).astype(np.float32)       # the best documents: the scalar tail of the float4 load
    elif pat == "winner_per_share":
        acc[:] = low(n)
        for s0 in range(0, n, BM25_SHARE):
            acc[s0 + int(rng.integers(0, min(BM25_SHARE, n - s0)))] = np.float32(1.0 + rng.random())
    elif pat == "denormal":
        acc[:] = rng.integers(0, 8, size=n).astype(np.float32) * F32_DENORM     # 0 .. 7 units of 2^-149: ties everywhere
    elif pat == "flt_max":
        acc[:] = rng.choice(np.array([FLT_MAX, np.nextafter(FLT_MAX, np.float32(0)), 1.0, 0.0], dtype=np.float32), size=n)
    elif pat == "crowd":
        acc[:] = low(n)
        order = rng.permutation(n)
        n_hi = min(k // 2, n)
        n_tie = min(n - n_hi, max(2, (n * 2) // 5))           # ~40 % of all documents tied at the score of rank k
        acc[order[:n_hi]] = (rng.random(n_hi) + 1.0).astype(np.float32)
        acc[order[n_hi:n_hi + n_tie]] = 0.75
    else:
        raise ValueError(pat)
    return acc


def bm25_postings(acc: np.ndarray) -> ho.Postings:
    """One term whose list holds the documents with a positive designed value, as impacts: querying the term makes the
    accumulators equal `acc`."""
    docs = np.flatnonzero(acc > 0).astype(np.uint32)
    n = acc.shape[0]
    return ho.Postings(n, 1, np.asarray([0, docs.size], dtype=np.uint64), docs, acc[docs].astype(np.float32),
                       np.ones(docs.size, dtype=np.uint32), np.ones(n, dtype=np.int64))


BM25_QUERY = [np.asarray([0], dtype=np.uint32)]
