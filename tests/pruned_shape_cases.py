"""
tests/pruned_shape_cases.py -- the data, the numpy model and the one-line slips of the centroid codes and the pruned
late-interaction search (csrc/maxsim_codes.hip) at the shapes pruned_cases.py does not reach: documents of up to 511 vectors,
scopes of three and more slices, every query-table shape, every width.  Shared by test_pruned_shape_cases_cpu.py (which shows
that every comparison of the GPU file can fail) and test_maxsim_pruned_shapes_gpu.py.  Nothing here is fitted to what the GPU
gives; the only tolerance is pruned_cases.product_tolerance.

TWO REGIMES
  exact    centroids, stored vectors and query vectors are integers in [-1, 1]: bf16 values, and MXFP4 values too (a block's
           maximum 1 gives E = -2 and the codes +-4 . 2^-2).  A dot product is an integer of magnitude <= dim, exact in fp32 in
           any order; a maximum is exact; a sum of at most 512 of them is an integer <= 512 dim, exact in fp64; one division and
           one rounding to float, which numpy does identically.  A query's scores are S / Lq with one Lq and integers |S| <=
           512 x 128 = 2^16: two different ones differ by at least 2^-16 of the larger, 256 float steps, so ranking the float64
           scores and ranking their float32 roundings agree.  The candidates are compared BIT FOR BIT, and since a score is a
           small integer over Lq, dozens of documents tie: only the id order resolves them.  Used on bf16 and mxfp4 stores (an
           fp8 vector's scale is amax / 448, no power of two, so fp8 does not keep integers).
  random   pruned_cases.random_centroids and clustered_docs: compared with pruned_cases.check_candidates at
           product_tolerance(dim), on all three formats.

SET L      600 documents = three slices of 256.  Lengths 0 .. 3, except the FIXED documents, which put a length of 63 / 64 / 65,
           two and three chunks of 64 codes, odd and even last chunks and the cap 511 at both ends of the store and on both
           sides of the slice boundaries 256 and 512.  Centroids 37 and 69 are copies of centroid 5: the same lane of the codes
           kernel (c mod 32), tile 1 of trip 0 and tile 0 of trip 1.  PAIRS of documents hold the same codes in reverse order,
           one pair inside slice 0, one across slices 0 and 1: exactly equal scores in either regime.
SET T      60 documents with the fixed lengths of set L, for the table shapes (ncent 32 .. 288).

THE MODEL  stored_codes, stage_scores and model_rank restate the stage: codes -> query table [ncent][P] -> per-document maximum
           -> fp64 mean -> the best of every slice -> merge.  Without a mutant it is centroid_interaction_reference +
           rank_candidates; MUTANTS lists its slips.
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence

import numpy as np

import pruned_cases as pc
from oracle.linear_cases import bf16_bits, bf16_values

POISON = 0x7FC5
REGIMES = ("exact", "random")
SLICE, GROUP, MAX_CAND, ROW_TILE, ROW_BLOCK = 256, 8, 256, 32, 128       # kCodeSlice, kPrunedG, kMaxCand, kRowTile, kRowBlock
CAP = 511

N_DOCS = 600
FIXED = {0: 511, 63: 63, 64: 64, 65: 65, 255: 129, 256: 128, 257: 127, 511: 200, 512: 65, 599: 511}
PAIRS = ((63, 100), (64, 300))                                           # (document, its reversed copy): inside slice 0 | across slices
COPIES_OF_5 = (37, 69)
DIM, NCENT = 128, 96

COUNTS = (1, 31, 32, 33, 64, 65, 130, 0, -3, None)                      # None: q_stride + 5
STRIDES = (1, 32, 33, 65, 136, 512)
SCOPES_L = ([(0, 600)], [(0, 66)], [(60, 70), (250, 260), (505, 520)], [(599, 600)])
NCANDS = (1, 16, 256)
EDGE_SCOPES = ([(0, 255)], [(0, 256)], [(0, 257)], [(255, 513)], [(256, 512)], [(1, 600)], [(511, 513)])
EDGE_NCANDS = (1, 255, 256)
TABLE_NCENTS = (32, 96, 160, 288)                                        # wave 0 only | three waves | a block + a wave | two blocks + a wave
TABLE_STRIDES = (33, 136)
N_DOCS_T = 60
SCOPES_T = ([(0, 60)], [(7, 19), (41, 42)])
WIDTH_LENGTHS = (1, 64, 64)                                              # 129 stored vectors: one block of 128 plus one


# ---- data --------------------------------------------------------------------------------------------------------------------
def copies(ncent: int):
    return tuple(c for c in COPIES_OF_5 if c < ncent)


def centroids(regime: str, ncent: int, dim: int, seed: int) -> np.ndarray:
    """bf16 bits uint16 [ncent, dim]; centroids 37 and 69 (where they exist) are copies of centroid 5."""
    if regime == "exact":
        cent = bf16_bits(np.random.default_rng(seed).integers(-1, 2, size=(ncent, dim)).astype(np.float32))
    else:
        cent = pc.random_centroids(ncent, dim, seed).copy()
    for c in copies(ncent):
        cent[c] = cent[5]
    return cent


def integer_vectors(n: int, dim: int, rng) -> np.ndarray:
    return bf16_bits(rng.integers(-1, 2, size=(int(n), dim)).astype(np.float32))


def integers_around(cent_bits: np.ndarray, which, rng, redrawn: int = 16) -> np.ndarray:
    """Integer vectors near centroid[which]: the centroid with `redrawn` of its components drawn again.  Its product with its
    own centroid is about 2/3 (dim - redrawn), with any other about +-sqrt(dim) 2/3: the copies of that centroid alone tie."""
    which = np.asarray(which, dtype=np.int64)
    v = bf16_values(cent_bits).astype(np.float64)[which]
    for row in v:
        at = rng.choice(v.shape[1], size=redrawn, replace=False)
        row[at] = rng.integers(-1, 2, size=redrawn)
    return bf16_bits(v.astype(np.float32))


def lengths_l(seed: int) -> List[int]:
    lens = np.random.default_rng(seed).integers(0, 4, size=N_DOCS)
    for d, n in FIXED.items():
        lens[d] = n
    for src, dst in PAIRS:
        lens[dst] = lens[src]
    return [int(n) for n in lens]


def lengths_t() -> List[int]:
    fixed = list(FIXED.values())
    return [fixed[i % len(fixed)] for i in range(N_DOCS_T)]


@functools.lru_cache(maxsize=None)
def documents(which: str, regime: str, dim: int = DIM, ncent: int = NCENT, seed: int = 7):
    """Set "L" or "T" -> (centroid bits, list of document bits, `drawn`).  drawn: random regime, the centroid every vector was
    drawn around (a copy of 5 counted as 5), one array per document; exact regime None (the vectors are random integers, and
    about one in seven ties for its maximum)."""
    cent = centroids(regime, ncent, dim, seed)
    lens = lengths_l(seed + 1) if which == "L" else lengths_t()
    if regime == "exact":
        rng = np.random.default_rng(seed + 2)
        docs, drawn = [integer_vectors(n, dim, rng) for n in lens], None
    else:
        docs, drawn = pc.clustered_docs(cent, lens, seed + 2)
        drawn = [np.where(np.isin(w, COPIES_OF_5), 5, w) for w in drawn]
    if which == "L":
        for src, dst in PAIRS:
            docs[dst] = docs[src][::-1].copy()
            if drawn is not None:
                drawn[dst] = drawn[src][::-1].copy()
    return cent, docs, drawn


def raw_counts(q_stride: int) -> np.ndarray:
    """COUNTS cut to what fits; the last is q_stride + 5"""
    return np.asarray([q_stride + 5 if c is None else min(c, q_stride) for c in COUNTS], dtype=np.int32)


def clamp(count: int, q_stride: int) -> int:
    return int(min(max(int(count), 0), q_stride))


@functools.lru_cache(maxsize=None)
def queries(regime: str, q_stride: int, dim: int = DIM, ncent: int = NCENT, seed: int = 7):
    """(uint16 [10, q_stride, dim] with poison behind every count, int32 raw counts).  The query of count q_stride + 5 holds
    q_stride vectors: what the clamped count reads."""
    cent = centroids(regime, ncent, dim, seed)
    rng = np.random.default_rng(seed + 3 + 1000 * q_stride)
    qc = raw_counts(q_stride)
    qv = np.full((len(qc), q_stride, dim), POISON, dtype=np.uint16)
    for i, c in enumerate(qc):
        n = clamp(c, q_stride)
        if regime == "exact":
            qv[i, :n] = integer_vectors(n, dim, rng)
        else:
            qv[i, :n] = pc.vectors_around(cent, rng.integers(0, ncent, size=n), rng, noise=0.5)
    return qv, qc


def batch(nq: int, ns: int):
    """every query under every scope: (query of row, scope of row).  A scope's rows ascend by query: with ten queries its
    groups are queries 0 .. 7 and 8, 9."""
    return np.repeat(np.arange(nq), ns), np.tile(np.arange(ns), nq).astype(np.int32)


def scope_docs(scope) -> List[int]:
    return [d for lo, hi in scope for d in range(lo, hi)]


def slices_of(scope):
    """The slices of a scope: every range cut on ABSOLUTE multiples of 256, in range order."""
    return [(max(lo, b * SLICE), min(hi, (b + 1) * SLICE)) for lo, hi in scope if hi > lo for b in range(lo // SLICE, (hi - 1) // SLICE + 1)]


def expected_items(scopes, soq) -> int:
    """work items of a call: over the scopes, slices x groups of 8 of the queries that name it"""
    soq = np.asarray(soq)
    return sum(len(slices_of(sc)) * (-(-int((soq == s).sum()) // GROUP)) for s, sc in enumerate(scopes))


def width_documents(regime: str, dim: int):
    """(centroid bits [96, dim], three documents of 1, 64 and 64 vectors, `drawn` as documents() gives it): random integer
    vectors | vectors around random centroids"""
    cent = centroids(regime, NCENT, dim, 31 + dim)
    if regime == "exact":
        rng = np.random.default_rng(32 + dim)
        return cent, [integer_vectors(n, dim, rng) for n in WIDTH_LENGTHS], None
    docs, drawn = pc.clustered_docs(cent, WIDTH_LENGTHS, 32 + dim)
    return cent, docs, [np.where(np.isin(w, COPIES_OF_5), 5, w) for w in drawn]


def width_queries(regime: str, cent: np.ndarray, dim: int):
    """two queries of 40 and 5 vectors, q_stride 40"""
    rng = np.random.default_rng(33 + dim)
    qc = np.asarray([40, 5], np.int32)
    qv = np.full((2, 40, dim), POISON, dtype=np.uint16)
    for i, n in enumerate(qc):
        qv[i, :n] = integer_vectors(n, dim, rng) if regime == "exact" else pc.vectors_around(cent, rng.integers(0, len(cent), size=n), rng, noise=0.5)
    return qv, qc


# ---- the reference, as the GPU file uses it -----------------------------------------------------------------------------------
def reference_scores(qv: np.ndarray, qc, codes, off, cent_bits) -> np.ndarray:
    """float64 [queries, documents]: centroid_interaction_reference of every query's clamped count of rows"""
    from hiprag.colbert import centroid_interaction_reference
    c = bf16_values(cent_bits).astype(np.float64)
    codes_of = [codes[off[d]:off[d + 1]] for d in range(len(off) - 1)]
    q_stride = qv.shape[1]
    return np.stack([centroid_interaction_reference(bf16_values(qv[i, :clamp(qc[i], q_stride)]), codes_of, c) for i in range(len(qc))])


def expected_candidates(ref_row: np.ndarray, count: int, scope, ncand: int, id_base: int = 0):
    """(ids int64 [ncand], scores float32 [ncand]) the float64 definition implies; a query without vectors: padding"""
    return pc.rank_candidates(ref_row, scope_docs(scope) if count > 0 else [], ncand, id_base=id_base)


def same_candidates(got_ids, got_scores, want_ids, want_scores) -> bool:
    """bit for bit"""
    return (np.asarray(got_ids, np.int64).tobytes() == np.asarray(want_ids, np.int64).tobytes()
            and np.asarray(got_scores, np.float32).tobytes() == np.asarray(want_scores, np.float32).tobytes())


def verdict(regime: str, got_ids, got_scores, ref_row, count: int, scope, ncand: int, dim: int, id_base: int = 0):
    """THE comparison of the GPU file: None, or what is wrong.  exact: bitwise; random: check_candidates."""
    if regime == "exact":
        want = expected_candidates(ref_row, count, scope, ncand, id_base)
        return None if same_candidates(got_ids, got_scores, *want) else "the candidates are not the float64 ranking's, bit for bit"
    return pc.check_candidates(got_ids, got_scores, ref_row, scope_docs(scope) if count > 0 else [], ncand, pc.product_tolerance(dim), id_base=id_base)


# ---- the model and its mutants ------------------------------------------------------------------------------------------------
CODE_MUTANTS = ("argmax_tie_to_higher_centroid",)
TABLE_MUTANTS = ("centroids_of_partial_block_zeroed", "rows_past_first_tile_zeroed")
SCORE_MUTANTS = ("codes_past_64_dropped", "second_code_chunk_rereads_first", "odd_last_code_dropped", "query_rows_past_64_dropped",
                 "count_not_clamped_low", "count_not_clamped_high")
RANK_MUTANTS = ("third_slice_lost", "tie_to_higher_document")
MUTANTS = SCORE_MUTANTS + RANK_MUTANTS + CODE_MUTANTS + TABLE_MUTANTS


def applies(mutant: str, regime: str, q_stride: int, ncent: int = NCENT) -> bool:
    """Whether the slip can show on set L (or T) at this stride through the GPU file's comparison."""
    if mutant == "query_rows_past_64_dropped":
        return q_stride >= 65                         # a query of more than 64 rows
    if mutant == "rows_past_first_tile_zeroed":
        return q_stride >= 33
    if mutant == "centroids_of_partial_block_zeroed":
        return ncent % ROW_BLOCK != 0
    if mutant == "argmax_tie_to_higher_centroid":
        return ncent > COPIES_OF_5[0]                 # shows in the CODES, which the GPU file compares; a copy's table row is the original's
    return True


def model_codes(values, cent_vals, mutant: Optional[str] = None) -> np.ndarray:
    """int32 [n]: the lowest centroid of the largest float64 product.  argmax_tie_to_higher_centroid: a lane of the codes kernel
    sees centroids r, r + 32, r + 64 .. in turn and replaces on >=, so among equal maxima of ONE lane the highest wins; the
    butterfly across lanes still prefers the lower centroid."""
    s = np.asarray(values, np.float64) @ np.asarray(cent_vals, np.float64).T
    if mutant != "argmax_tie_to_higher_centroid":
        return np.argmax(s, axis=1).astype(np.int32)
    out = np.zeros(len(s), np.int32)
    for v, row in enumerate(s):
        best = np.flatnonzero(row == row.max())
        out[v] = min(int(best[best % ROW_TILE == r].max()) for r in set((best % ROW_TILE).tolist()))
    return out


def model_table(q_vals: np.ndarray, cent_vals: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    """float64 [ncent, P] of one query: T[c][i] = q_i . centroid_c, P = q_stride rounded up to 32, rows behind q_stride zero
    (rows behind the query's count hold what the poison gives: NaN, which nothing may read)."""
    q_stride, ncent = len(q_vals), len(cent_vals)
    P = -(-q_stride // ROW_TILE) * ROW_TILE
    t = np.zeros((ncent, P))
    with np.errstate(invalid="ignore"):
        t[:, :q_stride] = np.asarray(cent_vals, np.float64) @ np.asarray(q_vals, np.float64).T
    if mutant == "centroids_of_partial_block_zeroed":
        t[ROW_BLOCK * (ncent // ROW_BLOCK):] = 0.0
    if mutant == "rows_past_first_tile_zeroed":
        t[:, ROW_TILE:] = 0.0
    return t


def _read_codes(codes: np.ndarray, lq: int, mutant: Optional[str]) -> np.ndarray:
    """the codes of one document as the interaction kernel takes them, 64 at a time"""
    if mutant == "codes_past_64_dropped":
        return codes[:64]
    out = []
    for j0 in range(0, len(codes), 64):
        n = min(64, len(codes) - j0)
        chunk = codes[:n] if mutant == "second_code_chunk_rereads_first" else codes[j0:j0 + n]
        if mutant == "odd_last_code_dropped" and 0 < lq <= 32 and n % 2:      # the lane halves take alternate codes
            chunk = chunk[:n - 1]
        out.append(chunk)
    return np.concatenate(out) if out else codes[:0]


def model_scores(table: np.ndarray, count: int, q_stride: int, codes: np.ndarray, off: np.ndarray, mutant: Optional[str] = None):
    """One query against every document -> (float32 [documents], ranked bool [documents]).
    count_not_clamped_high: the rows i >= q_stride are read where they would lie, T[c P + i], the zero rows up to P and then the
    next centroid's (the end of the table again behind it), and the sum is divided by the raw count.
    count_not_clamped_low: a negative count is taken for a query WITH vectors: no row is added, and 0 / count = -0 ranks every
    document of the scope."""
    n_docs = len(off) - 1
    lq = int(count)
    if mutant != "count_not_clamped_low":
        lq = max(lq, 0)
    if mutant != "count_not_clamped_high":
        lq = min(lq, q_stride)
    has = off[1:] > off[:-1]
    scores = np.full(n_docs, pc.NEG_MAX, dtype=np.float32)
    if lq == 0:
        return scores, np.zeros(n_docs, bool)
    if lq < 0:
        scores[has] = np.float32(0.0) / np.float32(lq)
        return scores, has.copy()
    ncent, P = table.shape
    flat = table.reshape(-1)
    rows = np.arange(lq)
    per_doc = [_read_codes(codes[off[d]:off[d + 1]], lq, mutant) for d in range(n_docs)]
    keep = np.asarray([len(c) > 0 for c in per_doc])
    sums = np.full(n_docs, -np.inf)
    if keep.any():
        allc = np.concatenate([c for c in per_doc if len(c)]).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum([len(c) for c in per_doc if len(c)])])[:-1]
        vals = flat[np.minimum(allc[:, None] * P + rows[None, :], len(flat) - 1)]       # [codes, lq]
        m = np.maximum.reduceat(vals, starts, axis=0)                                   # [documents with codes, lq]
        if mutant == "query_rows_past_64_dropped":
            m = m[:, :64]
        sums[keep] = m.sum(axis=1)
    with np.errstate(over="ignore"):
        scores[has] = (sums[has] / float(lq)).astype(np.float32)
    return scores, has.copy()


def model_rank(scores: np.ndarray, ranked: np.ndarray, scope, ncand: int, id_base: int = 0, mutant: Optional[str] = None):
    """The best min(ncand, 256) of every slice by (score descending, id ascending), then the merge of the slices' lists under
    the same order -> (ids int64 [ncand], scores float32 [ncand]), padding (-1, -FLT_MAX).
    third_slice_lost: the merge reads the first two lists only.  tie_to_higher_document: equal scores by id DESCENDING."""
    sign = -1 if mutant == "tie_to_higher_document" else 1
    key = lambda d: (-float(scores[d]), sign * d)
    lists = []
    for lo, hi in slices_of(scope):
        docs = sorted((d for d in range(lo, hi) if ranked[d]), key=key)
        lists.append(docs[:min(ncand, SLICE)])
    if mutant == "third_slice_lost":
        lists = lists[:2]
    merged = sorted((d for part in lists for d in part), key=key)[:ncand]
    ids = np.full(ncand, -1, dtype=np.int64)
    out = np.full(ncand, pc.NEG_MAX, dtype=np.float32)
    for r, d in enumerate(merged):
        ids[r], out[r] = d + id_base, scores[d]
    return ids, out


def stage_scores(qv: np.ndarray, qc, codes, off, cent_bits, mutant: Optional[str] = None):
    """the model's scores of every query: list of (float32 [documents], ranked)"""
    c = bf16_values(cent_bits).astype(np.float64)
    q_stride = qv.shape[1]
    out = []
    for i in range(len(qc)):
        table = model_table(bf16_values(qv[i]).astype(np.float64), c, mutant)
        out.append(model_scores(table, int(qc[i]), q_stride, np.asarray(codes), np.asarray(off), mutant))
    return out


def stored_codes(docs: Sequence[np.ndarray], cent_bits: np.ndarray, mutant: Optional[str] = None):
    """(codes int32 [stored], offsets int64) of documents held as they are (a bf16 store, or an MXFP4 store of integers)"""
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(d) for d in docs])
    vals = bf16_values(np.concatenate([d.reshape(-1, cent_bits.shape[1]) for d in docs]))
    return model_codes(vals, bf16_values(cent_bits), mutant), off
