"""
The rerank kernel (hipmaxsim_*, maxsim_kernel<Docs> and its dot_tile) at every width of tests/maxsim_width_cases.py: one
64-value chunk, an odd chunk count off the 128 grid, the widths between 128 and 1024 in bf16; two to eight lines in fp8.  The
pair scores of every (query, document) of set A against colbert_cases.maxsim_expected over what the store exports: bit for
bit on integer data, within the bound maxsim_expected returns on unit vectors.  An fp8 store against the bf16 store of its
dequantised vectors byte for byte, the counters against their closed form, and the same bytes from run to run.
The search tests (test_maxsim_search_paths_gpu.py) rest their expectations on the pair table checked here.
"""
import numpy as np
import pytest

import fp8_cases as fc
import maxsim_width_cases as wc
from colbert_cases import NEG_MAX, maxsim_expected, score_ratio, select_expected
from oracle.linear_cases import bf16_bits, bf16_values

pytestmark = pytest.mark.gpu


def _equal(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("regime", wc.REGIMES)
@pytest.mark.parametrize("dim,fmt", wc.SETS)
def test_pair_scores_of_set_a_at_every_width(gpu, dim, fmt, regime):
    from hiprag import maxsim
    s = wc.gpu_setup(regime, dim, fmt)
    off, stored = s["off"], bf16_values(s["vecs"]).astype(np.float64)
    assert np.array_equal(np.diff(off), s["lens"])
    if fmt == "fp8":                                      # what the store exports is the format's statement of the documents
        for j in (1, 5):
            assert np.array_equal(stored[off[j]:off[j + 1]], wc.stored_values(s["docs"][j:j + 1], "fp8")[0])
    scores, ids, pos, pairs = s["out"]
    worst = 0.0
    for i, q in enumerate(s["queries"]):
        for j in range(wc.N_DOCS):
            if not s["valid"][i, j]:
                assert pairs[i, j] == np.float32(NEG_MAX), (i, j)
                continue
            want, bound = maxsim_expected(q, stored[off[j]:off[j + 1]], regime)
            r = score_ratio(pairs[i, j], want, bound)
            worst = max(worst, r)
            assert r <= 1.0, (regime, dim, fmt, wc.COUNTS[i], int(s["lens"][j]), float(pairs[i, j]), want, bound)
    print(f"maxsim widths {regime} {dim} {fmt}: worst |got - ref| / bound = {worst:.3g} over {int(s['valid'].sum())} pairs (exact: 0 = bits)")
    # the selection over the pair scores, the copies in position order
    for i in range(len(wc.COUNTS)):
        sc, ii, pp = select_expected(pairs[i], s["cand"][i], s["valid"][i], wc.N_DOCS)
        assert np.array_equal(ids[i], ii) and np.array_equal(pos[i], pp) and sc.tobytes() == scores[i].tobytes()
        if wc.COUNTS[i]:
            for src, dst in wc.COPIES:
                assert pairs[i, src].tobytes() == pairs[i, dst].tobytes() and list(ids[i]).index(src) < list(ids[i]).index(dst)
    # the counters' closed form: a document's vectors are read once per 32-row tile of the query
    n_valid = int(s["valid"].sum())
    reads = sum(int(s["lens"][j]) * -(-wc.COUNTS[i] // 32) for i in range(len(wc.COUNTS)) for j in range(wc.N_DOCS) if s["valid"][i, j])
    assert s["info"] == (n_valid, s["valid"].size - n_valid, reads, 0), s["info"]
    again = maxsim(s["store"], s["qv"], s["qc"], s["cand"], k=wc.N_DOCS)             # the same bytes from run to run
    _equal(again, s["out"])
    assert s["store"].maxsim_info() == s["info"]


@pytest.mark.parametrize("regime", wc.REGIMES)
@pytest.mark.parametrize("dim", wc.FP8_WIDTHS)
def test_fp8_equals_its_bf16_twin_at_every_width(gpu, dim, regime):
    from hiprag import MultiVectorStore, maxsim
    s = wc.gpu_setup(regime, dim, "fp8")
    twin = MultiVectorStore(dim, max_doc_vectors=wc.CAP)                             # bf16, holding the dequantised vectors
    twin.append(s["vecs"], s["off"])
    _equal(maxsim(twin, s["qv"], s["qc"], s["cand"], k=wc.N_DOCS), s["out"])
    assert twin.maxsim_info() == s["info"]
    if regime == "exact":                                                            # integers are lossless: the bf16 store's bits
        if dim in wc.BF16_WIDTHS:
            _equal(wc.gpu_setup("exact", dim, "bf16")["out"], s["out"])
    else:                                                                            # and the format moved the vectors
        _, codes, scales = s["store"].export_fp8()
        c, sc = fc.quantize(np.concatenate([bf16_bits(d) for d in s["docs"] if len(d)]))
        assert codes.tobytes() == c.tobytes() and scales.tobytes() == sc.tobytes()
        assert not np.array_equal(bf16_values(s["vecs"]).astype(np.float64), np.concatenate([d for d in s["docs"] if len(d)]))
