"""
tests/maxsim_width_cases.py -- the widths, the small document and query sets and the numpy statements of one-line slips for
the MaxSim kernels (csrc/maxsim.hip, csrc/maxsim_search.hip, csrc/maxsim_docs.h) and the fp8 quantiser (csrc/multivec.hip),
shared by the CPU test (which proves that every case can fail) and the GPU tests.  colbert_cases.py and fp8_cases.py hold the
references and the bounds; nothing here is fitted to what the GPU gives, and no tolerance is introduced: integer data are
compared bit for bit, unit vectors within the bound maxsim_expected returns.

THE WIDTHS   what the kernels decide by dim: the 64-value chunks of a bf16 row (dim / 64), the 128-value lines of an fp8 row
  (dim / 128), and the query tiles T per pass of the search kernel (tiles_of below restates the driver's rule: 4 up to 576-d,
  3 from 640-d to 768-d, 2 from 832-d on).
      bf16   64 one chunk | 192 an odd chunk count, rows of 384 bytes | 576, 640 the T = 4 / 3 edge | 768, 832 the T = 3 / 2 edge
      fp8    256 two lines | 512 T = 4 | 640, 768 T = 3 (five and six lines) | 896, 1024 T = 2 (seven and eight lines)

THE MODEL    group_scores restates what one work item of maxsim_scope_kernel computes for its group of queries: the clamped
  counts, their prefix, the packed rows of a pass of R = 32 T rows, the maxima per packed row and document, the sums per member.
  Without a mutant it is maxsim_expected pair by pair (the CPU test holds it to that); its mutants are slips of the kernel:
      last_chunk_dropped        k >= dim - 64 takes no part in a dot product
      second_line_reads_first   fp8: the query side of line l > 0 is that of line 0 (k and k mod 128 share a query value)
      tile_reads_tile0          a pass's packed rows >= 32 are scored with its rows 0 .. 31
      count_not_clamped_low     a negative count is not raised to 0: the prefix runs backwards under the members behind it
      count_not_clamped_high    a count above q_stride is not cut to it: the member runs on into the rows of the next query
  stale_sum_table is the slip between work items (a workgroup's sums start from those of the item it took before), on the
  documented numbering of work_items; chunk_lost is the slip between chunks of queries (chunk 2 judged with chunk 1's counts,
  or with chunk 1's scopes).
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence

import numpy as np

import fp8_cases as fc
from colbert_cases import FILL16, NEG_MAX, maxsim_vectors
from oracle.linear_cases import bf16_bits, bf16_values

BF16_WIDTHS = (64, 192, 576, 640, 768, 832)
FP8_WIDTHS = (256, 512, 640, 768, 896, 1024)
SETS = [(d, "bf16") for d in BF16_WIDTHS] + [(d, "fp8") for d in FP8_WIDTHS]
REGIMES = ("exact", "random")                                   # integers in [-4, 4] | unit vectors

QTILE, GROUP, SLICE, MAX_TILES = 32, 8, 16, 4                   # kQTile, kSearchG, kSliceDocs, kMaxTiles
CHUNK_QUERIES = 16384                                           # kSearchMaxChunk
MAX_Q_STRIDE = 512


def tiles_of(dim: int) -> int:
    """T of maxsim_search.hip: the 32-row query tiles that fit in 160 KB less 4 KB of LDS, rows padded by 16 bytes, at most 4."""
    return min(MAX_TILES, (160 * 1024 - 4096) // (QTILE * (2 * dim + 16)))


# ---- set A: documents, queries, scopes -----------------------------------------------------------------------------------
N_DOCS = 42
LENGTHS = (0, 1, 31, 32, 33, 65)                                # stored lengths, cycled
CAP = 80
COPIES = tuple((i, 24 + i) for i in range(1, 6))                # documents 25..29 are copies of 1..5: equal scores, id order
COUNTS = (0, 1, 8, 8, 33, 70, 5, 12, 32, 2)                     # the first group of 8 packs 137 rows: two passes at T = 4
Q_STRIDE = 72
SCOPES = ([(0, 42)], [(3, 3)], [(5, 21), (21, 30), (33, 41)], [(0, 1), (6, 7), (36, 37)], [(17, 18)])   # [3]: empty documents only
EMPTY_SCOPES = (1, 3)
KS = (1, 10, 256)


def doc_vectors(regime: str, dim: int) -> List[np.ndarray]:
    docs = [maxsim_vectors(regime, LENGTHS[i % len(LENGTHS)], dim, 300 + i) for i in range(N_DOCS)]
    for src, dst in COPIES:
        docs[dst] = docs[src].copy()
    return docs


def query_vectors(regime: str, dim: int) -> List[np.ndarray]:
    return [maxsim_vectors(regime, n, dim, 700 + i) for i, n in enumerate(COUNTS)]


def query_block(queries: Sequence[np.ndarray], q_stride: int, dim: int):
    """(uint16 [nq, q_stride, dim] with poison behind every count, int32 counts)"""
    qv = np.full((len(queries), q_stride, dim), FILL16, dtype=np.uint16)
    for i, q in enumerate(queries):
        qv[i, :len(q)] = bf16_bits(q)
    return qv, np.asarray([len(q) for q in queries], np.int32)


def stored_values(docs: Sequence[np.ndarray], fmt: str) -> List[np.ndarray]:
    """What a store of `fmt` holds of the documents, as float64: the vectors, or their fp8 codes times the scales."""
    if fmt == "bf16":
        return [np.asarray(d, np.float64) for d in docs]
    return [fc.dequantized(*fc.quantize(bf16_bits(d))) if len(d) else np.asarray(d, np.float64) for d in docs]


def batch_of_every_query_under_every_scope(nq: int = len(COUNTS), ns: int = len(SCOPES)):
    """(query of row, scope of row): the rows of a scope ascend by query, so its first group is queries 0 .. 7."""
    return np.repeat(np.arange(nq), ns), np.tile(np.arange(ns), nq).astype(np.int32)


# ---- the model of one work item ------------------------------------------------------------------------------------------
WIDTH_MUTANTS = ("last_chunk_dropped", "second_line_reads_first", "tile_reads_tile0")
COUNT_MUTANTS = ("count_not_clamped_low", "count_not_clamped_high")


def applies(mutant: str, dim: int, fmt: str) -> bool:
    return fmt == "fp8" if mutant == "second_line_reads_first" else True


def csr(docs: Sequence[np.ndarray], dim: int):
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(d) for d in docs])
    flat = np.concatenate([np.asarray(d, np.float64).reshape(-1, dim) for d in docs]) if len(docs) else np.zeros((0, dim))
    return off, flat


def dots(q: np.ndarray, d: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    dim = q.shape[1]
    if mutant == "last_chunk_dropped":
        return q[:, :dim - 64] @ d[:, :dim - 64].T
    if mutant == "second_line_reads_first":
        return np.tile(q[:, :128], (1, dim // 128)) @ d.T
    return q @ d.T


def doc_max(s: np.ndarray, off: np.ndarray) -> np.ndarray:
    """s [rows, stored] -> [rows, docs]: the maximum over every document's columns, -inf for a document without vectors."""
    out = np.full((s.shape[0], len(off) - 1), -np.inf)
    full = np.flatnonzero(off[1:] > off[:-1])
    if len(full) and s.shape[0]:
        out[:, full] = np.maximum.reduceat(s, off[:-1][full], axis=1)
    return out


def clamped(counts, q_stride: int, mutant: Optional[str] = None) -> np.ndarray:
    c = np.asarray(counts, dtype=np.int64)
    if mutant != "count_not_clamped_low":
        c = np.maximum(c, 0)
    if mutant != "count_not_clamped_high":
        c = np.minimum(c, q_stride)
    return c


def group_scores(qflat: np.ndarray, q_stride: int, members: Sequence[int], counts, off: np.ndarray, flat: np.ndarray, tiles: int,
                 mutant: Optional[str] = None):
    """One group of at most 8 queries against every document: (sums float64 [members, docs], clamped counts).  qflat float64
    [nq * q_stride, dim] is the query block row after row; `counts` are the members' RAW counts.  The score of (member g,
    document d) is sums[g, d] / counts[g] where counts[g] > 0 and d holds a vector.  An unclamped count that runs past the
    block stops at its end (the model of a kernel that would read on)."""
    assert 1 <= len(members) <= GROUP
    mc = np.minimum(clamped(counts, q_stride, mutant), len(qflat))
    mpre = np.concatenate([[0], np.cumsum(mc)])
    rows_total, R, dim = int(mpre[-1]), tiles * QTILE, qflat.shape[1]
    sums = np.zeros((len(members), len(off) - 1))
    for row0 in range(0, max(rows_total, 0), R):
        nrows = min(R, rows_total - row0)
        lds = np.zeros((R, dim))
        for p in range(nrows):
            g = 0
            while mpre[g + 1] <= row0 + p:
                g += 1
            lds[p] = qflat[(members[g] * q_stride + row0 + p - mpre[g]) % len(qflat)]
        if mutant == "tile_reads_tile0":
            lds = lds[np.arange(R) % QTILE]
        m = doc_max(dots(lds, flat, mutant), off)
        for g in range(len(members)):
            lo, hi = max(int(mpre[g]) - row0, 0), min(int(mpre[g + 1]) - row0, nrows)
            if hi > lo:
                sums[g] += m[lo:hi].sum(axis=0)
    return sums, mc


def score_table(qv_bits: np.ndarray, counts, row_query: Sequence[int], stored: Sequence[np.ndarray], tiles: int,
                mutant: Optional[str] = None, group: int = GROUP):
    """The float32 pair scores of rows `row_query` of a batch that names ONE scope in this order (groups of 8 as the kernel
    forms them), and which of them are ranked: [rows, docs] each."""
    nq, q_stride, dim = qv_bits.shape
    qflat = bf16_values(qv_bits).astype(np.float64).reshape(nq * q_stride, dim)
    off, flat = csr(stored, dim)
    has = off[1:] > off[:-1]
    scores = np.full((len(row_query), len(stored)), NEG_MAX, dtype=np.float32)
    valid = np.zeros((len(row_query), len(stored)), dtype=bool)
    for g0 in range(0, len(row_query), group):
        members = [int(v) for v in row_query[g0:g0 + group]]
        sums, mc = group_scores(qflat, q_stride, members, [counts[m] for m in members], off, flat, tiles, mutant)
        for g in range(len(members)):
            if mc[g] > 0:
                valid[g0 + g] = has
                with np.errstate(invalid="ignore"):
                    scores[g0 + g, has] = (sums[g, has] / float(mc[g])).astype(np.float32)
    return scores, valid


# ---- the selection, vectorised ---------------------------------------------------------------------------------------------
def scope_docs(scope) -> np.ndarray:
    return np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in scope] + [np.zeros(0, np.int64)])


def rank_rows(scores: np.ndarray, valid: np.ndarray, scopes, soq, k: int):
    """maxsim_search_reference without its Python loops over documents: scores float32 [rows, docs], valid bool [rows, docs]
    -> (float32 [rows, k], int64 [rows, k]) by (score descending, id ascending) over the valid documents of the row's scope."""
    soq = np.asarray(soq)
    out_s = np.full((len(soq), k), NEG_MAX, dtype=np.float32)
    out_i = np.full((len(soq), k), -1, dtype=np.int64)
    for s, scope in enumerate(scopes):
        rows, ids = np.flatnonzero(soq == s), scope_docs(scope)
        if not len(rows) or not len(ids):
            continue
        sc, ok = scores[np.ix_(rows, ids)].astype(np.float64), valid[np.ix_(rows, ids)]
        order = np.argsort(np.where(ok, -sc, np.inf), axis=1, kind="stable")[:, :k]      # the ids ascend: ties keep id order
        take = np.take_along_axis(ok, order, axis=1)
        n = order.shape[1]
        out_s[rows, :n] = np.where(take, np.take_along_axis(sc, order, axis=1), NEG_MAX).astype(np.float32)
        out_i[rows, :n] = np.where(take, ids[order], -1)
    return out_s, out_i


# ---- work items ---------------------------------------------------------------------------------------------------------------
def work_items(scopes, soq):
    """The work items of a chunk in their documented numbering: the scopes in index order; of a scope with rows, item
    `within` = slice * ngroups + group, the slices being the 16-document blocks (cut on absolute boundaries) of its ranges
    in order.  -> list of (scope, slice of the scope, base document, p_lo, p_hi, member rows)."""
    soq = np.asarray(soq)
    items = []
    for s, scope in enumerate(scopes):
        rows = np.flatnonzero(soq == s)
        ngroups = -(-len(rows) // GROUP)
        blocks = [(b * SLICE, max(lo, b * SLICE) - b * SLICE, min(hi, (b + 1) * SLICE) - b * SLICE)
                  for lo, hi in scope if hi > lo for b in range(lo // SLICE, (hi - 1) // SLICE + 1)]
        for sl, (base, p_lo, p_hi) in enumerate(blocks):
            for g in range(ngroups):
                items.append((s, sl, base, p_lo, p_hi, rows[g * GROUP:(g + 1) * GROUP]))
    return items


def grid_of(n_items: int, cus: int) -> int:
    return max(1, min(n_items, 4 * cus))


def stale_sum_table(sums: np.ndarray, counts, doc_len, scopes, soq, cus: int) -> np.ndarray:
    """sums float64 [rows, docs] (row i against every document, before the division) -> the table a kernel gives whose
    sums[member slot][document slot] are zeroed on a workgroup's first item only: item i starts from what item i - grid left."""
    items = work_items(scopes, soq)
    grid = grid_of(len(items), cus)
    counts, doc_len = np.asarray(counts), np.asarray(doc_len)
    out = sums.copy()
    left = [None] * len(items)
    for i, (_, _, base, p_lo, p_hi, rows) in enumerate(items):
        lds = left[i - grid].copy() if i >= grid else np.zeros((GROUP, SLICE))
        for g, row in enumerate(rows):
            for p in range(p_lo, p_hi):
                if doc_len[base + p] > 0 and counts[row] > 0:
                    lds[g, p] += sums[row, base + p]
                    out[row, base + p] = lds[g, p]
        left[i] = lds
        if i >= grid:
            left[i - grid] = None
    return out


def consecutive_items_differ(scopes, soq, counts, cus: int) -> bool:
    """Some workgroup takes, one after the other, two items whose groups differ in members AND in packed rows."""
    items = work_items(scopes, soq)
    grid = grid_of(len(items), cus)
    c = np.asarray(counts)
    for i in range(grid, len(items)):
        a, b = items[i - grid][5], items[i][5]
        if len(a) != len(b) and int(c[a].sum()) != int(c[b].sum()):
            return True
    return False


def many_items_queries(cus: int) -> int:
    """The query count of the many-items case: at least 20, a last group that is not full, and a group count that does not
    divide the grid's stride 4 x CUs, so that a workgroup's consecutive items belong to different groups."""
    nq = 20
    while nq % GROUP == 0 or (4 * cus) % (-(-nq // GROUP)) == 0:
        nq += 4
    return nq


MANY_COUNTS = (3, 1, 0, 2, 5, 4, 1, 7, 2, 2, 6, 1, 0, 3, 9, 4, 1, 1, 2, 5)      # cycled; q_stride 9


def many_items_case(cus: int, dim: int, seed: int = 41):
    """16 x (4 x CUs + 300) documents of 0 .. 3 integer vectors each, nq queries of mixed counts, every query under two
    scopes (the whole store, an off-boundary sub-range): (doc lens, vecs float64, queries float64 list, scopes, rows)."""
    n_docs = SLICE * (4 * cus + 300)
    rng = np.random.default_rng(seed + dim)
    lens = rng.integers(0, 4, size=n_docs)
    vecs = rng.integers(-4, 5, size=(int(lens.sum()), dim)).astype(np.float64)
    nq = many_items_queries(cus)
    queries = [rng.integers(-4, 5, size=(MANY_COUNTS[i % len(MANY_COUNTS)], dim)).astype(np.float64) for i in range(nq)]
    scopes = [[(0, n_docs)], [(5, 40), (57, n_docs - 23)]]
    b_q, b_s = batch_of_every_query_under_every_scope(nq, 2)
    return lens, vecs, queries, scopes, b_q, b_s


def sum_table(queries: Sequence[np.ndarray], lens, vecs: np.ndarray) -> np.ndarray:
    """float64 [nq, docs]: sum_i max_j q_i . d_j, one matmul per query (0 where either side is empty)."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out = np.zeros((len(queries), len(lens)))
    has = off[1:] > off[:-1]
    for i, q in enumerate(queries):
        if len(q):
            out[i, has] = doc_max(q @ vecs.T, off)[:, has].sum(axis=0)
    return out


def scores_of_sums(sums: np.ndarray, counts, lens):
    """(float32 scores, valid) of a sum table: one division in fp64 and one rounding to fp32, as the kernel does."""
    c = np.asarray(counts, np.float64)[:, None]
    valid = (c > 0) & (np.asarray(lens)[None, :] > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(valid, sums / c, NEG_MAX).astype(np.float32), valid


# ---- two chunks of queries -------------------------------------------------------------------------------------------------
TWO_CHUNK_NQ = CHUNK_QUERIES + 5
TWO_CHUNK_SCOPES = ([(0, 13)], [(9, 30)], [(2, 5), (25, 40)])


def two_chunk_case(dim: int = 64, seed: int = 77):
    """40 documents of 0 .. 3 integer vectors, 16389 queries of 0 .. 2 vectors (q_stride 2) over three scopes; the counts and
    the scopes of queries i and i + 16384 differ."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 4, size=40)
    lens[[0, 12, 29]] = (2, 0, 3)
    vecs = rng.integers(-4, 5, size=(int(lens.sum()), dim)).astype(np.float64)
    counts = rng.integers(0, 3, size=TWO_CHUNK_NQ).astype(np.int32)
    soq = rng.integers(0, 3, size=TWO_CHUNK_NQ).astype(np.int32)
    tail = np.arange(CHUNK_QUERIES, TWO_CHUNK_NQ)
    counts[tail - CHUNK_QUERIES] = (1, 2, 1, 2, 2)
    counts[tail] = (2, 1, 2, 1, 1)
    soq[tail] = (soq[tail - CHUNK_QUERIES] + 1) % 3
    q = rng.integers(-4, 5, size=(TWO_CHUNK_NQ, 2, dim)).astype(np.float64)
    return lens, vecs, q, counts, soq


def two_chunk_scores(lens, vecs, q, counts):
    """Vectorised: (float32 [nq, docs], valid) for queries of at most two vectors."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nq, _, dim = q.shape
    m = doc_max(q.reshape(nq * 2, dim) @ vecs.T, off).reshape(nq, 2, len(lens))
    has = np.asarray(lens) > 0
    c = np.asarray(counts)
    sums = np.where(has[None, :], m[:, 0], 0.0) + np.where(has[None, :] & (c[:, None] == 2), m[:, 1], 0.0)
    return scores_of_sums(sums, c, lens)


def chunk_lost(values: np.ndarray) -> np.ndarray:
    """The queries of chunk 2 given what stands at the same place of chunk 1 (an offset `+ o` dropped)."""
    out = np.asarray(values).copy()
    out[CHUNK_QUERIES:] = out[:len(out) - CHUNK_QUERIES]
    return out


# ---- the count cases -----------------------------------------------------------------------------------------------------------
COUNT_STRIDE = 40
RAW_COUNTS = (7, -3, 33, 0, COUNT_STRIDE + 5, 12, 2 ** 31 - 1, COUNT_STRIDE)      # one group of eight
ORDINARY = (0, 2, 5, 7)                                                           # its members with a count in 1 .. q_stride


def count_case(dim: int, regime: str = "exact"):
    """Eight queries of COUNT_STRIDE real vectors each (a clamped count never reaches poison) and the raw counts."""
    queries = [maxsim_vectors(regime, COUNT_STRIDE, dim, 900 + i) for i in range(len(RAW_COUNTS))]
    qv, _ = query_block(queries, COUNT_STRIDE, dim)
    return qv, np.asarray(RAW_COUNTS, np.int32)


# ---- the quantiser: one vector per lane ---------------------------------------------------------------------------------------
def lane_sweep_vectors(dim: int, seed: int = 5) -> np.ndarray:
    """bf16 bits [dim / 16, dim]: vector l holds its largest magnitude alone in value 16 l, the first of lane l's sixteen;
    every other value is at most an eighth of it (and not zero), so a reduction of amax that loses lane l picks a scale at
    least 8 times smaller and every code changes."""
    rng = np.random.default_rng(seed * 4099 + dim)
    n = dim // 16
    binade = rng.integers(-3, 4, size=n)
    top = np.ldexp(1.0 + rng.integers(0, 8, size=n) / 8.0, binade)
    v = rng.uniform(1 / 64, 1 / 8, size=(n, dim)) * rng.choice([-1.0, 1.0], size=(n, dim)) * np.ldexp(1.0, binade)[:, None]
    v[np.arange(n), 16 * np.arange(n)] = top * rng.choice([-1.0, 1.0], size=n)
    bits = bf16_bits(v.astype(np.float32))
    mag = (bits & 0x7FFF).astype(np.int64)
    peak = mag[np.arange(n), 16 * np.arange(n)]
    rest = mag.copy()
    rest[np.arange(n), 16 * np.arange(n)] = 0
    assert np.all((rest.max(axis=1) >> 7) <= (peak >> 7) - 3) and np.all(rest.sum(axis=1) > 0)      # three binades below
    return bits


def store_vectors(dim: int) -> np.ndarray:
    """The vectors of the store tests at one width: unit, integer, special and the lane sweep.  (special_vectors needs 65
    components; the 64-d store, which is bf16 only and keeps bit patterns as they are, gets the first 64 of its 128-d set.)"""
    special = fc.special_vectors(dim) if dim >= 128 else fc.special_vectors(128)[:, :dim]
    return np.concatenate([fc.unit_vectors(24, dim, 3), fc.integer_vectors(12, dim, 4), special, lane_sweep_vectors(dim)])


# ---- set A on the GPU: one store and one pair table per (regime, dim, format), shared by the GPU tests ---------------------------
@functools.lru_cache(maxsize=None)
def gpu_setup(regime: str, dim: int, fmt: str):
    """The store of set A, the query block, hipmaxsim's pair scores of every (query, document) and what the store exports."""
    from hiprag import MultiVectorStore, maxsim
    docs, queries = doc_vectors(regime, dim), query_vectors(regime, dim)
    store = MultiVectorStore(dim, max_doc_vectors=CAP, format=fmt)
    store.append([bf16_bits(d) for d in docs])
    qv, qc = query_block(queries, Q_STRIDE, dim)
    cand = np.tile(np.arange(N_DOCS, dtype=np.int64), (len(COUNTS), 1))
    out = maxsim(store, qv, qc, cand, k=N_DOCS)
    info = store.maxsim_info()
    off, vecs = store.export()
    lens = np.asarray([len(d) for d in docs])
    valid = (qc[:, None] > 0) & (lens[None, :] > 0)
    return dict(store=store, docs=docs, queries=queries, qv=qv, qc=qc, cand=cand, out=out, pairs=out[3], info=info, off=off, vecs=vecs,
                lens=lens, valid=valid)
