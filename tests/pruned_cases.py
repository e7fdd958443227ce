"""
Data and comparison helpers of the centroid-code and pruned-search tests (test_maxsim_pruned_cpu.py, test_multivec_codes_gpu.py,
test_maxsim_pruned_gpu.py).  No GPU here: test_maxsim_pruned_cpu.py holds the helpers against mutants of the numpy references
and the data against the margins the GPU tests rely on.
"""
import numpy as np

from oracle.linear_cases import bf16_bits, bf16_values

NEG_MAX = -float(np.finfo(np.float32).max)
NOISE = 0.25                       # of a vector around its centroid
QUERY_NOISE = 0.1                  # of a planted query vector around a document vector


def unit(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def random_centroids(ncent, dim, seed):
    """bf16 bits uint16 [ncent, dim] of random unit vectors"""
    return bf16_bits(unit(np.random.default_rng(seed).standard_normal((ncent, dim))).astype(np.float32))


def vectors_around(cent_bits, which, rng, noise=NOISE):
    """bf16(unit(centroid[which] + noise * unit noise)) -> bits uint16 [len(which), dim]"""
    c = bf16_values(cent_bits).astype(np.float64)[np.asarray(which, dtype=np.int64)]
    if len(c) == 0:
        return np.zeros((0, cent_bits.shape[1]), np.uint16)
    return bf16_bits(unit(c + noise * unit(rng.standard_normal(c.shape))).astype(np.float32))


def clustered_docs(cent_bits, lengths, seed, noise=NOISE):
    """One document per length, every vector around a random centroid.  -> (list of bits arrays, list of the drawn centroids)"""
    rng = np.random.default_rng(seed)
    docs, drawn = [], []
    for n in lengths:
        which = rng.integers(0, len(cent_bits), size=int(n))
        drawn.append(which)
        docs.append(vectors_around(cent_bits, which, rng, noise))
    return docs, drawn


def top2_margin(values, centroids):
    """smallest gap between the best and the second-best fp64 dot product over the rows of `values`"""
    s = np.sort(np.asarray(values, np.float64) @ np.asarray(centroids, np.float64).T, axis=1)
    return float((s[:, -1] - s[:, -2]).min())


def product_tolerance(dim):
    """|fp32 MFMA accumulation - exact| of a dot product of two vectors of norm <= 1.01 (unit vectors rounded to bf16): the
    products are exact in fp32, dim additions each round by at most 2^-24 of a partial sum no larger than sum |a_k b_k| <=
    |a| |b|; a mean of such values and its rounding to float stay inside (dim + 2) steps."""
    return (dim + 2) * 2.0 ** -24 * 1.01 * 1.01


def rank_candidates(approx, in_scope, ncand, id_base=0, tie_order=None):
    """The candidate list a score per document implies: documents of `in_scope` (ascending local ids) whose score is finite,
    by (score descending, id ascending), first ncand, padded with (-1, -FLT_MAX).  tie_order: a MUTANT's tie-break -- a rank
    per document used in place of its id."""
    approx = np.asarray(approx, dtype=np.float64)
    docs = [d for d in in_scope if np.isfinite(approx[d])]
    docs.sort(key=lambda d: (-approx[d], d if tie_order is None else tie_order[d]))
    ids = np.full(ncand, -1, dtype=np.int64)
    scores = np.full(ncand, NEG_MAX, dtype=np.float32)
    for r, d in enumerate(docs[:ncand]):
        ids[r], scores[r] = d + id_base, np.float32(approx[d])
    return ids, scores


def check_candidates(got_ids, got_scores, ref, in_scope, ncand, tol, id_base=0):
    """One query's candidates against `ref`, the float64 interaction score of every document (-inf: holds no vector).
    Returns None, or a string that says what is wrong:
      the first min(ncand, valid documents of the scope) ranks are distinct valid documents of the scope, the rest padding;
      every score lies within tol of the reference's;
      scores do not ascend, and EQUAL scores come in ascending id order;
      no omitted document beats a returned one by more than 2 tol."""
    got_ids, got_scores = np.asarray(got_ids, np.int64), np.asarray(got_scores, np.float32)
    ref = np.asarray(ref, dtype=np.float64)
    valid = [d for d in in_scope if np.isfinite(ref[d])]
    n = min(ncand, len(valid))
    if len(got_ids) != ncand or len(got_scores) != ncand:
        return "wrong length"
    if np.any(got_ids[n:] != -1) or np.any(got_scores[n:] != np.float32(NEG_MAX)):
        return f"ranks past {n} are not padding"
    local = got_ids[:n] - id_base
    if len(set(local.tolist())) != n or any(int(d) not in set(valid) for d in local):
        return "a rank holds a document outside the scope, without vectors, or twice"
    for r in range(n):
        if abs(float(got_scores[r]) - ref[local[r]]) > tol:
            return f"rank {r}: score {float(got_scores[r])} of document {int(local[r])}, reference {ref[local[r]]}"
    for r in range(1, n):
        if got_scores[r] > got_scores[r - 1]:
            return f"scores ascend at rank {r}"
        if got_scores[r] == got_scores[r - 1] and got_ids[r] < got_ids[r - 1]:
            return f"equal scores at ranks {r - 1}, {r} are not in id order"
    if n:
        floor = min(ref[d] for d in local)
        for d in valid:
            if d not in set(local.tolist()) and ref[d] > floor + 2 * tol:
                return f"document {d} ({ref[d]}) is missing though it beats a returned one ({floor})"
    return None


# ---- the planted-document data of the usefulness test ---------------------------------------------------------------------
PLANT_DOCS, PLANT_CENT, PLANT_DIM, PLANT_QUERIES, PLANT_LQ, PLANT_NCAND = 400, 256, 128, 16, 8, 16


def planted(seed):
    """400 documents of 20..40 vectors around 256 random unit centroids at 128-d; 16 queries of 8 vectors, query i = the first
    8 vectors of document targets[i] plus 0.1 unit noise, renormalised.  -> (centroid bits, list of document bits, query bits
    [16, 8, dim], targets)"""
    rng = np.random.default_rng(1000 + seed)
    cent = random_centroids(PLANT_CENT, PLANT_DIM, 2000 + seed)
    docs, _ = clustered_docs(cent, rng.integers(20, 41, size=PLANT_DOCS), 3000 + seed)
    targets = rng.choice(PLANT_DOCS, size=PLANT_QUERIES, replace=False)
    q = np.zeros((PLANT_QUERIES, PLANT_LQ, PLANT_DIM), np.uint16)
    for i, t in enumerate(targets):
        v = bf16_values(docs[t][:PLANT_LQ]).astype(np.float64)
        q[i] = bf16_bits(unit(v + QUERY_NOISE * unit(rng.standard_normal(v.shape))).astype(np.float32))
    return cent, docs, q, targets
