"""
oracle/width_cases.py -- the case table and the designed data of the WIDTH tests: every vector path of the dense, scoped and
IVF kernels at widths d off the 4-float (vector load) and 128-float (d_pad) grids, shared by the GPU tests
(tests/test_widths_gpu.py) and by the CPU tests that prove the data can tell a right kernel from a subtly wrong one
(tests/test_width_cases_cpu.py).

TEST INFRASTRUCTURE ONLY (see oracle/hybrid_oracle.py header).  numpy only: importable without torch and without the
library.  Every generator is deterministic (seeded from its own parameters).

Three parts:
  * the dispatch rules of the scan, restated from csrc/dense_plan.h, the library's one home for them (pieces: create_dense;
    ring, scan_waves, filter_on, passes: plan_scan), and SCAN_CELLS, the table of launches that reaches every kernel shape
    the rules can select.  The restatement is kept on purpose: tests/test_scan_plan_cpu.py and tests/test_widths_gpu.py
    compare it with what the library itself answers (hiprag_scan_plan, plan_label), so a drift of either shows;
  * tail_heavy / tail_heavy_queries: rows and queries whose LAST columns (behind the last multiple of 4, 8 and 16) and whose
    last 8-column piece carry a large, row-dependent share of the norm, and whose first 16 columns flip sign from one row to
    the next -- a kernel that drops, misplaces or over-reads a tail reorders the top k; MUTANTS are the numpy models of such
    kernels;
  * planted: k rows per query whose exact scores are separated from each other and from every other row by a margin
    computed from scan_eps_ref, the float64 restatement of the certificate's slack -- on such data a correct scan MUST be
    certified (no exhaustive path), so a test may assert which path answered.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Callable, List, Optional, Tuple

import numpy as np

from . import hybrid_oracle as ho

MODES = ("bf16", "q64")
K_TAG_SLACK = 2.0 ** -21          # kTagSlack
U32 = 2.0 ** -24                  # fp32 unit roundoff
PASS_Q = 64                       # kPassQ: queries per pass over the index
NO_FILTER_GROUPS = 1024           # kNoFilterGroups
MAX_D = 1024                      # kMaxDPad


def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode())


# ======================================================================================================================
# The dispatch rules, restated
# ======================================================================================================================
def pieces(d: int) -> int:
    """P: 1 KiB fp32 pieces per 32-row block = d_pad / 8, d_pad = d rounded up to 128 (create_dense)."""
    return 16 * ((d + 127) // 128)


def d_pad(d: int) -> int:
    return 8 * pieces(d)


def nblocks(n: int) -> int:
    return (n + 31) // 32


def scan_waves(d: int, nblk: int, scan_cus: int, mode: str) -> int:
    """DenseIndex::scan_waves: waves per scan workgroup."""
    return 4 if (mode == "bf16" and pieces(d) % 32 == 0 and nblk < scan_cus * 72) else 8


def ring(d: int, mode: str = "bf16") -> int:
    """scan_pass: depth of the load ring.  q64 always runs 16; the bf16 kernel runs 16 where that divides the P / 2 pieces of a
    block of the filter copy, else 8 (the 4-wave form exists with 16 only: scan_waves gives 4 for P % 32 == 0 alone)."""
    if mode == "q64":
        return 16
    return 16 if (pieces(d) // 2) % 16 == 0 else 8


def filter_on(nblk: int) -> bool:
    """scan_pass / finish_pass: the in-scan bound is used only above kNoFilterGroups groups (two per block)."""
    return 2 * nblk > NO_FILTER_GROUPS


def passes(nq: int) -> str:
    return "one" if nq <= PASS_Q else "multi"


def vec_paths(d: int) -> str:
    """Which load form the width selects: 'vec' -- every 16-byte load form (retile_bf16_kernel's two float4 per lane, the
    query staging's float4 loads, the IVF kernels' vec = 1 forms); 'vec+tail8' -- d % 4 == 0 but the last 8-column group of
    the filter copy is cut (col + 8 > d: scalar form for that lane, float4 for the rest); 'scalar' -- d % 4 != 0: the scalar
    forms everywhere."""
    if d % 4:
        return "scalar"
    return "vec" if d % 8 == 0 else "vec+tail8"


def scan_label(d: int, n: int, nq: int, scan_cus: int, mode: str) -> str:
    """The kernel shape a launch selects, e.g. 'bf16/P128/ring16/w4/one'."""
    return "%s/P%d/ring%d/w%d/%s" % (mode, pieces(d), ring(d, mode), scan_waves(d, nblocks(n), scan_cus, mode), passes(nq))


def plan_label(shape, plan) -> str:
    """The same label from what the LIBRARY says: a hipidx_scan_shape_t and the hipidx_scan_plan_t hiprag_scan_plan gives for
    it (any objects with those fields).  A wide launch reads 'bf16/P128/wide/w8/multi'."""
    return "%s/P%d/%s/w%d/%s" % ({3: "bf16", 2: "q64"}[shape.mode], shape.P, "wide" if plan.wide else "ring%d" % plan.ring,
                                plan.waves, "multi" if plan.multi_pass else "one")


EDGE_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 17, 31, 33, 63, 65, 127, 128, 129, 130, 131, 255, 257, 383, 385, 513, 639, 640,
               641, 769, 895, 896, 897, 1001, 1022, 1023, 1024)

# widths of the scan-shape cells: the issue's seven, plus 513 (P = 80) and 769 (P = 112), the two members of the ring-8
# family {16, 48, 80, 112} no other test reaches
SCAN_WIDTHS = (1023, 897, 769, 641, 513, 385, 257, 129, 7)
SCAN_CUS = 4                  # workgroups the cells leave the scan (set_spare_cus(n_cu - 4)): 8 waves need nblocks >= 4 * 72
SCAN_N_SMALL = 3000           # 94 blocks < 288: 4 waves where P % 32 == 0; several blocks per wave, a ragged last block
SCAN_N_LARGE = 9250           # 290 blocks >= 288: 8 waves with ring 16
SCAN_NQ = (3, 65)             # one pass; two passes, the second with one query
SCAN_K = 10


@dataclass(frozen=True)
class ScanCell:
    d: int
    n: int
    nq: int
    mode: str
    metric: int
    label: str                # the kernel shape the cell must select (with SCAN_CUS workgroups)

    @property
    def name(self) -> str:
        return "d%d-n%d-nq%d-%s-%s" % (self.d, self.n, self.nq, self.mode, "ip" if self.metric == ho.METRIC_IP else "l2")


def scan_cells() -> List[ScanCell]:
    """Every reachable cell of {ring 8, ring 16} x {4, 8 waves} x {one pass, multi pass} x {ip, l2} x {bf16, q64}: ring 8 runs
    with 8 waves only and q64 with (ring 16, 8 waves) only -- the rules above allow nothing else."""
    out = []
    for d in SCAN_WIDTHS:
        P = pieces(d)
        for metric in (ho.METRIC_IP, ho.METRIC_L2):
            for nq in SCAN_NQ:
                ps = passes(nq)
                if P % 32 == 0:
                    out.append(ScanCell(d, SCAN_N_SMALL, nq, "bf16", metric, "bf16/P%d/ring16/w4/%s" % (P, ps)))
                    out.append(ScanCell(d, SCAN_N_LARGE, nq, "bf16", metric, "bf16/P%d/ring16/w8/%s" % (P, ps)))
                else:
                    out.append(ScanCell(d, SCAN_N_SMALL, nq, "bf16", metric, "bf16/P%d/ring8/w8/%s" % (P, ps)))
                out.append(ScanCell(d, SCAN_N_SMALL, nq, "q64", metric, "q64/P%d/ring16/w8/%s" % (P, ps)))
    return out


# ======================================================================================================================
# bf16, the certificate's slack and the row bounds, restated in float64
# ======================================================================================================================
def bf16_round(a: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 (ties to even), as float32: what (__bf16)f and v_cvt_pk_bf16_f32 give for finite values."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u >> 16) & 1) + 0x7FFF
    return ((u + r) & 0xFFFF0000).astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _f32_round_up(v: np.ndarray) -> np.ndarray:
    """float64 -> the smallest float32 >= v (row_stats_kernel: f = (float)acc; if (f < acc) f = nextafterf(f, inf))."""
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    low = f.astype(np.float64) < v
    return np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def row_bounds_ref(x: np.ndarray) -> Tuple[np.float32, np.float32]:
    """(max |x|^2, max |x - bf16(x)|^2) over the rows, each row's fp64 sum rounded UP to float32: hipidx_row_bounds.  (The
    kernel sums a row in another order; its fp64 sum differs from numpy's by ~1e-16 relative, which moves the float32 image
    only where the sum sits on a rounding boundary.)"""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    if x64.shape[0] == 0:
        return np.float32(0), np.float32(0)
    dx = x64 - bf16_round(x).astype(np.float64)
    return (_f32_round_up((x64 * x64).sum(axis=1)).max(), _f32_round_up((dx * dx).sum(axis=1)).max())


def row_bounds_interval(x: np.ndarray):
    """(lo, hi), each a pair like row_bounds_ref: the float32 images the two maxima can take when a row's fp64 sum of d
    squares is formed in ANY order -- such sums differ from numpy's by at most d * 2^-53 relative.  lo == hi == row_bounds_ref
    unless a row's sum lies within that distance of a float32 value."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    if x64.shape[0] == 0:
        z = (np.float32(0), np.float32(0))
        return z, z
    dx = x64 - bf16_round(x).astype(np.float64)
    r = x64.shape[1] * 2.0 ** -53
    n2, d2 = (x64 * x64).sum(axis=1), (dx * dx).sum(axis=1)
    return ((_f32_round_up(n2 * (1 - r)).max(), _f32_round_up(d2 * (1 - r)).max()),
            (_f32_round_up(n2 * (1 + r)).max(), _f32_round_up(d2 * (1 + r)).max()))


def _scan_eps(dpad: int, mode: str, metric: int, qn2, xn2: float, dq2, dx2: float):
    """scan_eps of dense_finish.h, term for term."""
    xn, qn = math.sqrt(xn2), np.sqrt(qn2)
    eps = 1.05 * (dpad + 80) * U32 * qn * xn
    if mode == "q64":
        eps = eps + 7.62939453125e-06 * 1.01 * qn * xn + 1.0001 * np.sqrt(dq2) * xn
    else:
        eps = eps + 1.0001 * (np.sqrt(dq2) * xn + math.sqrt(dx2) * (qn + np.sqrt(dq2)))
    if metric == ho.METRIC_IP:
        return eps + K_TAG_SLACK * (qn * xn + eps)
    eps = 2.0 * eps + 4.0 * U32 * (xn * xn + qn * xn) + 4.0 * U32 * qn2
    return eps + K_TAG_SLACK * (2.0 * qn * xn + xn * xn + eps)


def scan_eps_ref(d: int, mode: str, metric: int, x: np.ndarray, q: np.ndarray) -> np.ndarray:
    """The certificate's slack per query [nq], float64, from the data alone: |scan value - exact score| <= eps on the scale
    the scan selects by (inner product: <x, q>; L2: 2 <x, q> - |x|^2)."""
    q64 = np.atleast_2d(np.asarray(q, dtype=np.float32)).astype(np.float64)
    dq = q64 - bf16_round(np.atleast_2d(np.asarray(q, dtype=np.float32))).astype(np.float64)
    xn2, dx2 = row_bounds_ref(x)
    return _scan_eps(d_pad(d), mode, metric, (q64 * q64).sum(axis=1), float(xn2), (dq * dq).sum(axis=1), float(dx2))


def scan_scale_scores(x: np.ndarray, q: np.ndarray, metric: int) -> np.ndarray:
    """Exact scores [nq, n] on the scan's scale, float64."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    q64 = np.atleast_2d(np.asarray(q, dtype=np.float32)).astype(np.float64)
    s = q64 @ x64.T
    return s if metric == ho.METRIC_IP else 2.0 * s - (x64 * x64).sum(axis=1)[None, :]


def score_error_bound(d: int, x: np.ndarray, q: np.ndarray, ids: np.ndarray, metric: int) -> np.ndarray:
    """Bound [nq, k] of |s - ref64| for the float64 scores of the fp64 re-score: (d_pad + 16) * 2^-53 * sum_i |t_i| over the
    summed terms t_i (x_i q_i for inner product, (x_i - q_i)^2 for L2) of row ids[q, j]; 0 where ids < 0.  d_pad products and
    sums in the lane, four butterfly steps, each within 2^-53 relative; the rest is slack."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    q64 = np.atleast_2d(np.asarray(q, dtype=np.float32)).astype(np.float64)
    out = np.zeros(ids.shape, dtype=np.float64)
    for b in range(ids.shape[0]):
        ok = ids[b] >= 0
        rows = x64[ids[b][ok]]
        t = np.abs(rows * q64[b][None, :]) if metric == ho.METRIC_IP else (rows - q64[b][None, :]) ** 2
        out[b, ok] = (d_pad(d) + 16) * 2.0 ** -53 * t.sum(axis=1)
    return out


# ======================================================================================================================
# tail_heavy
# ======================================================================================================================
def tail_bounds(d: int) -> List[int]:
    """Column boundaries of the TAIL SEGMENTS: from the first tail column on, every boundary a kernel's tail handling can sit
    at -- 16 * (d // 16), 8 * (d // 8), 4 * (d // 4), d - 8 (the last 8-column piece of a d that fills its d_pad to less than
    8) -- up to d.  A d on the 16 grid has no ragged tail; its last two 8-column groups stand in (d - 16, d - 8)."""
    first = 16 * (d // 16) if d % 16 else max(0, d - 16)
    b = {first, 8 * (d // 8), 4 * (d // 4), d - 8, d}
    return sorted(v for v in b if first <= v <= d)


def _tail_heavy(n: int, d: int, rng, rows: bool) -> np.ndarray:
    x = rng.standard_normal((n, d))
    tb = tail_bounds(d)
    ts = tb[0]
    hd = min(16, d)
    if rows:   # first 16 columns: one sign per row, flipping from each row to its successor
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        x[:, :hd] = sign[:, None] * (0.5 + np.abs(x[:, :hd]))
    x[:, max(ts, hd):] += 0.6      # tail columns have a mean: a centroid that loses them moves

    def put(lo, hi, share):
        if hi > lo:
            nn = np.sqrt((x[:, lo:hi] ** 2).sum(axis=1))
            nn[nn == 0] = 1.0
            x[:, lo:hi] *= (np.sqrt(share) / nn)[:, None]

    w_tail = rng.uniform(0.45, 0.8, size=n)                      # the tail's share of |x|^2, row by row
    segs = [(lo, hi) for lo, hi in zip(tb[:-1], tb[1:]) if hi > lo]
    cut = rng.uniform(0.5, 1.5, size=(n, len(segs)))
    cut /= cut.sum(axis=1, keepdims=True)                        # ... split over the segments, row by row
    if ts >= hd:
        w_head = 0.3 * (1.0 - w_tail)
        put(0, hd, w_head)
        put(hd, ts, 1.0 - w_tail - w_head)
    for j, (lo, hi) in enumerate(segs):
        put(lo, hi, w_tail * cut[:, j])
    x /= np.sqrt((x ** 2).sum(axis=1, keepdims=True))
    return x


def tail_heavy(n: int, d: int, seed: int = 0, scaled: bool = False) -> np.ndarray:
    """float32 [n, d] rows, unit norm (scaled: times a per-row factor in 0.1 .. 30): 45-80 % of every row's squared norm
    sits in the tail segments (tail_bounds), split between them row by row; the first 16 columns hold one sign per row that
    flips from row to row (so what lies behind a row's end is far from the zero padding a kernel should see); rows n // 2 ..
    n // 2 + 2 and n - 2 are exact copies of row 1, row n // 3 is zero."""
    rng = np.random.default_rng(_seed("tail_heavy", n, d, seed, scaled))
    x = _tail_heavy(n, d, rng, rows=True)
    if scaled:
        x *= rng.uniform(0.1, 30.0, size=(n, 1))
    x = x.astype(np.float32)
    if n >= 16:
        x[n // 2:n // 2 + 3] = x[1]
        x[n - 2] = x[1]
        x[n // 3] = 0
    return x


def tail_heavy_queries(nq: int, d: int, seed: int = 0, scaled: bool = False) -> np.ndarray:
    """Queries with the same tail structure (no sign pattern, no copies): the tails of rows and queries meet in the score."""
    rng = np.random.default_rng(_seed("tail_heavy_queries", nq, d, seed, scaled))
    q = _tail_heavy(nq, d, rng, rows=False)
    if scaled:
        q *= rng.uniform(0.2, 7.0, size=(nq, 1))
    return q.astype(np.float32)


# ======================================================================================================================
# Mutants: numpy models of subtly wrong kernels.  A mutant maps (x, q, metric) to the (x', q', metric') a WRONG kernel would
# effectively score; .applies(d) says whether it differs from the right kernel at that width at all.
# ======================================================================================================================
def _zero_cols(a: np.ndarray, keep: np.ndarray) -> np.ndarray:
    out = a.copy()
    out[:, ~keep] = 0
    return out


def _drop_from(c0: Callable[[int], int]):
    def f(x, q, metric):
        d = x.shape[1]
        keep = np.arange(d) < c0(d)
        return _zero_cols(x, keep), _zero_cols(q, keep), metric
    return f


def _restride(a: np.ndarray, stride: int, width: int) -> np.ndarray:
    """Row r = the `width` floats at r * stride of the row-major buffer (zeros behind its end)."""
    n, d = a.shape
    flat = np.concatenate([a.reshape(-1), np.zeros(n * max(stride, width) + width, dtype=a.dtype)])
    idx = (np.arange(n) * stride)[:, None] + np.arange(width)[None, :]
    return flat[idx]


def _m_stride4(x, q, metric):
    d = x.shape[1]
    return _restride(x, 4 * ((d + 3) // 4), d), q, metric


def _over_read(a: np.ndarray) -> np.ndarray:
    """Every row with its padding up to the next multiple of 8 read from what follows it in memory."""
    d = a.shape[1]
    return _restride(a, d, 8 * ((d + 7) // 8))


def _pad8(a: np.ndarray) -> np.ndarray:
    d = a.shape[1]
    return np.concatenate([a, np.zeros((a.shape[0], 8 * ((d + 7) // 8) - d), dtype=a.dtype)], axis=1)


def _m_next_row(x, q, metric):
    # Under inner product a misread row tail meets the zero padding of the query and is invisible BY CONSTRUCTION; the
    # squared distance sees it.  So this mutant is judged under L2 whatever the case's metric (every GPU case runs both).
    return _over_read(x), _pad8(q), ho.METRIC_L2


def _m_next_query(x, q, metric):
    # a misread query tail alone shifts every distance of a query by one constant and no inner product at all: it can
    # reorder nothing.  It matters where the row's tail is misread too, which is the kernel that pads neither operand.
    return _over_read(x), _over_read(q), metric


def _piece_cols(d: int, skipped: Callable[[int, int], bool]) -> np.ndarray:
    P = pieces(d)
    p = np.arange(d) // 8
    return np.array([not skipped(int(pi), P) for pi in p], dtype=bool)


def _m_last_piece(x, q, metric):
    keep = _piece_cols(x.shape[1], lambda p, P: p == P - 1)
    return _zero_cols(x, keep), q, metric


def _m_second_batch(x, q, metric):
    # rescore4: lane pq owns pieces pq + 8 i; i = 8 .. 15 is the second load batch
    keep = _piece_cols(x.shape[1], lambda p, P: p >= 64 and (p % 8) >= P % 8)
    return _zero_cols(x, keep), q, metric


@dataclass(frozen=True)
class Mutant:
    name: str
    apply: Callable
    applies: Callable[[int], bool]
    rows_only: bool = True       # acts on the rows alone in a way a centroid (a mean of rows) can see


MUTANTS = (
    Mutant("drop_mod4", _drop_from(lambda d: 4 * (d // 4)), lambda d: d % 4 != 0),
    Mutant("drop_mod8", _drop_from(lambda d: 8 * (d // 8)), lambda d: d % 8 != 0),
    Mutant("drop_mod16", _drop_from(lambda d: 16 * (d // 16)), lambda d: d % 16 != 0),
    Mutant("stride4", _m_stride4, lambda d: d % 4 != 0),
    Mutant("tail_from_next_row", _m_next_row, lambda d: d % 8 != 0, rows_only=False),
    Mutant("query_tail_from_next_query", _m_next_query, lambda d: d % 8 != 0, rows_only=False),
    Mutant("skip_last_piece", _m_last_piece, lambda d: d > 8 * (pieces(d) - 1)),
    Mutant("skip_second_batch", _m_second_batch, lambda d: d > 512),
)


def mutant_search(m: Mutant, x: np.ndarray, q: np.ndarray, k: int, metric: int):
    """(ids of the right kernel, ids of the mutant), both by ho.flat_search."""
    xm, qm, mm = m.apply(x, q, metric)
    return ho.flat_search(x, q, k, mm)[1], ho.flat_search(xm, qm, k, mm)[1]


def centroid_update(x: np.ndarray) -> np.ndarray:
    """One round of the k-means update with ONE list: the mean of all rows, float64."""
    return np.asarray(x, dtype=np.float32).astype(np.float64).mean(axis=0)


# ======================================================================================================================
# planted
# ======================================================================================================================
FILLER_SCALE = 0.125
MARGIN_FACTOR = 4.0     # the guaranteed margin, in units of scan_eps_ref (see planted)


@dataclass
class Planted:
    x: np.ndarray        # float32 [n, d]
    q: np.ndarray        # float32 [d]: THE query (a test repeats it nq times: every query slot of a pass gets real work)
    rows: np.ndarray     # int64 [k]: the planted rows, best first
    metric: int

    def queries(self, nq: int) -> np.ndarray:
        return np.ascontiguousarray(np.repeat(self.q[None, :], nq, axis=0))


@lru_cache(maxsize=8)
def planted(n: int, d: int, k: int, metric: int, seed: int = 0) -> Planted:
    """Fillers 0.125 * tail_heavy(n, d); one unit tail-heavy query; k planted rows at scattered positions (the first row, both
    sides of a block boundary and the last row -- in a ragged block -- among them) whose exact scores on the scan's scale are
    1 - j * M, j = 0 .. k - 1, every filler below 0.25.  M is settled on the built float32 data: the smallest step with
    M >= 4.3 * scan_eps_ref (the larger of the two modes; eps depends on the planted rows' own norms, hence the loop).  What
    makes planted row j win lives in ONE tail segment (tail_bounds), segment j mod #segments:
      inner product   the row is a multiple of the query's part in that segment, plus a small filler: a scan that loses the
                      segment scores the row like a filler and never lists it;
      L2              the row is the query with that segment scaled by 1 - u_j.
    tests/test_width_cases_cpu.py checks on the data that the gaps between the k planted scores, and from the k-th to the
    best other row, are >= MARGIN_FACTOR * scan_eps_ref for both modes."""
    rng = np.random.default_rng(_seed("planted", n, d, k, metric, seed))
    fill = (FILLER_SCALE * tail_heavy(n, d, seed=seed + 7).astype(np.float64))
    q = tail_heavy_queries(1, d, seed=seed + 11)[0].astype(np.float64)
    tb = tail_bounds(d)
    segs = [(lo, hi) for lo, hi in zip(tb[:-1], tb[1:]) if hi > lo]
    share = lambda s: float((q[s[0]:s[1]] ** 2).sum())
    segs = [s for s in segs if share(s) >= 0.2] or [max(segs, key=share)]    # a thin segment would need a long row
    seg_n2 = [share(s) for s in segs]
    forced = [0, 31, 32, n - 1]
    others = [int(r) for r in rng.permutation(n) if r not in forced][:max(0, k - len(forced))]
    rows = np.asarray((forced + others)[:k], dtype=np.int64)
    rows = rows[rng.permutation(k)]

    def build(M: float) -> np.ndarray:
        x = fill.copy()
        for j, r in enumerate(rows):
            lo, hi = segs[j % len(segs)]
            if metric == ho.METRIC_IP:
                row = 0.2 * fill[r]                                  # a small filler, so that the row is no bare multiple
                row[lo:hi] = 0
                row[lo:hi] = q[lo:hi] * ((1.0 - j * M - float(row @ q)) / seg_n2[j % len(segs)])
            else:
                u = math.sqrt(j * M / seg_n2[j % len(segs)])         # score = |q|^2 - dist = 1 - u^2 |q_seg|^2
                row = q.copy()
                row[lo:hi] *= 1.0 - u
            x[r] = row
        return x.astype(np.float32)

    M = 0.01
    for _ in range(8):
        x = build(M)
        eps = max(float(scan_eps_ref(d, mode, metric, x, q.astype(np.float32))[0]) for mode in MODES)
        if M >= 4.3 * eps:
            break
        M = 4.6 * eps
    else:
        raise AssertionError("planted: the margin did not settle")
    filler_top = FILLER_SCALE if metric == ho.METRIC_IP else 2 * FILLER_SCALE
    assert 1.0 - (k - 1) * M > filler_top + M, "planted: no room for the planted scores"
    others = np.delete(scan_scale_scores(x, q.astype(np.float32), metric)[0], rows)
    assert others.max() <= filler_top * (1 + 1e-6), "planted: a filler above its ceiling"
    return Planted(x, q.astype(np.float32), rows, metric)


def planted_margins(p: Planted, d: int, k: int, mode: str) -> Tuple[float, float]:
    """(smallest gap among the k + 1 best exact scores of the query on the scan's scale, scan_eps_ref of the query)."""
    s = scan_scale_scores(p.x, p.q, p.metric)[0]
    top = np.sort(s)[::-1][:k + 1]
    return float(np.min(top[:-1] - top[1:])), float(scan_eps_ref(d, mode, p.metric, p.x, p.q)[0])
