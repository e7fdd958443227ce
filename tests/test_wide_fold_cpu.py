"""
The fold schedule of the wide scan kernel (wide_fold of csrc/dense_plan.h, the function scan_wide_kernel itself asks when
it parks a tile) through the library, without a GPU: hiprag_wide_fold says for which pair numbers of its walk a wave
recomputes the bound of its 64-query unit.  Compared with a brute-force restatement for N in {1, 2, 4, 8, 16, 64} and
grids of 32, 56, 208, 224 and 256 workgroups: N = 1 always folds, the first pairs always fold, from there every wave folds
exactly once in any N consecutive pairs, and at every pair number the folds for one query pair are spread evenly over the
(workgroup, row half)s.
"""
import ctypes

import numpy as np
import pytest

EVERY = (1, 2, 4, 8, 16, 64)
GRIDS = (32, 56, 208, 224, 256)
PAIRS = 3 * 64 + 7   # pair numbers looked at: the first pairs, then three periods of the longest schedule and a bit


def _restated(p, wg, wave, every, first):
    """one wave, one pair, in words: the first pairs always; then when pair number + 2 wg + row half + query pair is a
    multiple of N"""
    row_half, query_pair = wave % 2, wave // 2
    return p < first or (p + 2 * wg + row_half + query_pair) % every == 0


@pytest.fixture(scope="module")
def first():
    from hiprag.index import wide_fold_constants
    f, default = wide_fold_constants()
    assert f >= 4, "the bound forms in a launch's first tiles: they all fold"
    assert default in (1, 2, 4, 8, 16, 32, 64)
    return f


def _table(cus, every):
    """fold[wg, wave, p] from the library"""
    from hiprag.index import wide_fold
    return np.stack([np.stack([wide_fold(0, PAIRS, wg, wave, every) for wave in range(8)]) for wg in range(cus)])


@pytest.mark.parametrize("cus", GRIDS)
@pytest.mark.parametrize("every", EVERY)
def test_the_schedule_against_its_restatement(first, cus, every):
    got = _table(cus, every)
    want = np.array([[[_restated(p, wg, wave, every, first) for p in range(PAIRS)] for wave in range(8)] for wg in range(cus)])
    assert np.array_equal(got, want)
    what = f"cus {cus} every {every}"
    if every == 1:
        assert got.all(), what
    assert got[:, :, :first].all(), what
    # from there every (workgroup, wave) folds exactly once in any N consecutive pair numbers
    later = got[:, :, first:].astype(np.int64)
    windows = np.lib.stride_tricks.sliding_window_view(later, every, axis=2).sum(axis=3)
    assert windows.shape[2] == PAIRS - first - every + 1 and (windows == 1).all(), what
    # for every pair number and every query pair: floor or ceil(2 G / N) of the 2 G (workgroup, row half) fold
    lo, hi = (2 * cus) // every, -(-(2 * cus) // every)
    for qp in range(4):
        n = later[:, 2 * qp:2 * qp + 2, :].sum(axis=(0, 1))
        assert ((n == lo) | (n == hi)).all(), f"{what} query pair {qp}"


def test_a_window_anywhere_in_the_walk(first):
    """p0 > 0: the entry answers for pairs p0 .. p0 + n - 1"""
    from hiprag.index import wide_fold
    whole = wide_fold(0, 300, 17, 5, 8)
    assert np.array_equal(wide_fold(123, 100, 17, 5, 8), whole[123:223])
    assert wide_fold(0, 0, 0, 0, 1).shape == (0,)


def test_bad_arguments_are_errors():
    from hiprag import _native as nat
    out = (ctypes.c_uint8 * 8)()
    for p0, n, wg, wave, every in ((-1, 1, 0, 0, 4), (0, -1, 0, 0, 4), (0, 1, -1, 0, 4), (0, 1, 0, 8, 4), (0, 1, 0, -1, 4),
                                   (0, 1, 0, 0, 0), (0, 1, 0, 0, 3), (0, 1, 0, 0, 128), (0, 1, 0, 0, -4), (1 << 31, 1, 0, 0, 4),
                                   (0, 1, 1 << 28, 0, 4)):
        with pytest.raises(nat.HipRagError):
            nat.call("hiprag_wide_fold", p0, n, wg, wave, every, out, None, None)
    with pytest.raises(nat.HipRagError):
        nat.call("hiprag_wide_fold", 0, 4, 0, 0, 4, None, None, None)
