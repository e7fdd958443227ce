"""
The walk of the wide scan kernel (wide_walk / wide_walk_pair of csrc/dense_plan.h, the function scan_wide_kernel itself
calls) asked through the library, without a GPU: hiprag_wide_walk gives the (row tile, column) pairs of one workgroup in
its order.  Compared with a restatement in numpy over every nrt in 1..400 and the four bench shapes, ncol 1..4 and seven
grids: every pair exactly once, the full rounds as the walk by row tile had them, the longest sequence the best that
whole pairs allow.
"""
import ctypes

import numpy as np
import pytest

NRTS = list(range(1, 401)) + [489, 977, 1954, 3907]
NCOLS = (1, 2, 3, 4)
GRIDS = (32, 33, 56, 100, 208, 224, 256)


def _ceil(a, b):
    return -(-a // b)


def _library_walk(fn, nrt, ncol, cus, rts, cols, counts):
    """all workgroups of one (nrt, ncol, cus): the sequences one after another in rts / cols, their lengths in counts"""
    cap = len(rts)
    at = 0
    for w in range(cus):
        rc = fn(nrt, ncol, cus, w, cap - at, ctypes.byref(rts, 8 * at), ctypes.byref(cols, 4 * at), ctypes.byref(counts, 8 * w))
        assert rc == 0
        assert counts[w] <= cap - at, "a workgroup's sequence is longer than every pair of the launch"
        at += counts[w]
    n = np.frombuffer(counts, np.int64, cus).copy()
    return np.frombuffer(rts, np.int64, at).copy(), np.frombuffer(cols, np.int32, at).copy(), n


def _restated_walk(nrt, ncol, cus):
    """The same, by brute force: a table of who computes which pair at which position.  Full rounds: workgroup w walks row
    tiles w, w + cus, ... and all columns of each; the left-over pairs, numbered row tile first, go round the workgroups."""
    F, L = divmod(nrt, cus)
    seqs = [[] for _ in range(cus)]
    if F == 0:
        for w in range(nrt):
            seqs[w] = [(w, c) for c in range(ncol)]
        return seqs
    for w in range(cus):
        seqs[w] = [(w + i * cus, c) for i in range(F) for c in range(ncol)]
    for t in range(L * ncol):
        seqs[t % cus].append((F * cus + t // ncol, t % ncol))
    return seqs


@pytest.fixture(scope="module")
def walk_fn():
    from hiprag import _native as nat
    nat.load()
    fn = getattr(ctypes.CDLL(nat.LIB_PATH), "hiprag_wide_walk")
    fn.restype = ctypes.c_int32
    fn.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p]
    return fn


@pytest.mark.parametrize("cus", GRIDS)
def test_the_walk_against_its_restatement(walk_fn, cus):
    rts = (ctypes.c_int64 * (max(NRTS) * max(NCOLS)))()
    cols = (ctypes.c_int32 * (max(NRTS) * max(NCOLS)))()
    counts = (ctypes.c_int64 * cus)()
    for nrt in NRTS:
        F, L = divmod(nrt, cus)
        for ncol in NCOLS:
            rt, col, n = _library_walk(walk_fn, nrt, ncol, cus, rts, cols, counts)
            what = f"nrt {nrt} ncol {ncol} cus {cus}"
            # (a) every pair exactly once
            assert len(rt) == nrt * ncol, what
            assert np.array_equal(np.sort(rt * ncol + col), np.arange(nrt * ncol)), what
            assert col.min() >= 0 and col.max() < ncol and rt.min() >= 0 and rt.max() < nrt, what
            # the whole walk, pair by pair and in order, is the restatement's
            want = _restated_walk(nrt, ncol, cus)
            assert n.tolist() == [len(s) for s in want], what
            flat = np.array([p for s in want for p in s], dtype=np.int64).reshape(-1, 2)
            assert np.array_equal(rt, flat[:, 0]) and np.array_equal(col, flat[:, 1]), what
            # (b) the first F ncol pairs of every workgroup are the walk by row tile (F == 0: the whole sequence is)
            wg = np.repeat(np.arange(cus), n)                               # the workgroup of every pair
            pos = np.arange(len(rt)) - np.repeat(np.cumsum(n) - n, n)       # and its position in that workgroup's sequence
            head = pos < F * ncol if F else np.ones(len(rt), bool)
            assert (n >= F * ncol).all(), what
            assert np.array_equal(rt[head], (wg + (pos // ncol) * cus)[head]), what
            assert np.array_equal(col[head], (pos % ncol)[head]), what
            if F == 0:
                assert np.array_equal(n, np.where(np.arange(cus) < nrt, ncol, 0)), what
            # (c) the longest sequence
            if F:
                assert n.max() == F * ncol + _ceil(L * ncol, cus) == _ceil(nrt * ncol, cus), what
            assert n.max() <= _ceil(nrt, cus) * ncol, what


@pytest.mark.parametrize("rows,nq,cus,nrt,left,before,after", [
    (1_000_000, 512, 224, 3907, 99, 36, 35),
    (500_000, 1024, 224, 1954, 162, 36, 35),
    (250_000, 1024, 208, 977, 145, 20, 19),
    (125_000, 1024, 208, 489, 73, 12, 10),
])
def test_the_bench_shapes(walk_fn, rows, nq, cus, nrt, left, before, after):
    """(d) pair-times of a launch at the four bench shapes, by row tile and with the last round split by column"""
    from hiprag.index import wide_walk
    ncol = _ceil(nq, 256)
    assert _ceil(rows, 256) == nrt and nrt % cus == left
    assert _ceil(nrt, cus) * ncol == before
    longest = max(len(wide_walk(nrt, ncol, cus, w)[0]) for w in range(cus))
    assert longest == after == _ceil(nrt * ncol, cus)


def test_bad_arguments_are_errors(walk_fn):
    from hiprag import _native as nat
    n = ctypes.c_int64()
    for args in ((0, 1, 32, 0), (10, 0, 32, 0), (10, 5, 32, 0), (10, 1, 0, 0), (10, 1, 32, 32), (10, 1, 32, -1), (1 << 28, 1, 32, 0)):
        with pytest.raises(nat.HipRagError):
            nat.call("hiprag_wide_walk", *args, 0, None, None, ctypes.byref(n))
    with pytest.raises(nat.HipRagError):
        nat.call("hiprag_wide_walk", 10, 1, 32, 0, 4, None, None, ctypes.byref(n))
