"""
The removal plan of a document CSR (csrc/compaction_plan.h) asked through the library itself: hiprag_compaction_plan is host
arithmetic over stored lengths and a range table, needs no device and no handle, and is the code hiptok_remove_ranges and
hipmv_remove_ranges carry out.  Against hand-worked values and against a brute-force plan in numpy that marks every item
with its document, drops the removed ones and reads the runs off the survivors.
"""
import ctypes

import numpy as np
import pytest

# the refused tables of tests/test_range_table_gpu.py, over 40 documents, and what their messages hold
N_REFUSED = 40
REFUSED = [([(3, 2)], "is not within"), ([(-1, 2)], "is not within"), ([(0, 41)], "is not within"),
           ([(4, 6), (5, 7)], "ascend and do not overlap"), ([(6, 8), (1, 2)], "ascend and do not overlap")]


def plan(lens, ranges, n_ranges=None, null_ranges=False):
    """(out6, runs [n_runs][3]) of hiprag_compaction_plan"""
    from hiprag import _native as nat
    lens = np.ascontiguousarray(lens, np.int32)
    tab = np.ascontiguousarray(ranges, np.int64).reshape(-1, 2)
    n_ranges = len(tab) if n_ranges is None else n_ranges
    out6 = np.full(6, -7, np.int64)
    runs = np.full((max(n_ranges, 0) + 1, 3), -7, np.int64)
    nat.call("hiprag_compaction_plan", lens.ctypes.data if len(lens) else None, len(lens),
             None if null_ranges or not len(tab) else tab.ctypes.data, n_ranges, out6.ctypes.data, runs.ctypes.data)
    assert np.all(runs[out6[5]:] == -7), "rows behind n_runs were written"
    return out6.tolist(), runs[:out6[5]].tolist()


def brute_force(lens, ranges):
    """The same from the items: every item carries its document and its position; the survivors behind the first removed
    document land densely from that document's offset on, and a run is what survives between two removed stretches."""
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    removed = np.zeros(n, bool)
    for lo, hi in ranges:
        removed[lo:hi] = True
    total, longest = int(lens.sum()), int(lens.max(initial=0))
    if not removed.any():
        return [n, total, n, total, longest, 0], []
    starts = removed & ~np.concatenate(([False], removed[:-1]))     # a removed stretch begins here
    stretch = np.cumsum(starts)                                      # removed stretches at or before a document
    first = int(np.argmax(removed))
    item_first = int(lens[:first].sum())
    item_doc = np.repeat(np.arange(n), lens)
    src = np.flatnonzero(~removed[item_doc] & (stretch[item_doc] >= 1))
    dst = item_first + np.arange(len(src))
    runs = []
    for g in np.unique(stretch[item_doc[src]]):
        m = stretch[item_doc[src]] == g
        assert np.array_equal(src[m] - src[m][0], dst[m] - dst[m][0])     # a run is contiguous on both sides
        runs.append([int(src[m][0]), int(dst[m][0]), int(m.sum())])
    kept = lens[~removed]
    return [first, item_first, len(kept), int(kept.sum()), int(kept.max(initial=0)), len(runs)], runs


HAND = [
    # lens, table, out6 = {first, its offset, docs after, items after, longest after, n_runs}, runs {src, dst, len}
    ("tail only", [2, 0, 3, 1], [(2, 4)], [2, 2, 2, 2, 2, 0], []),
    ("everything", [1, 2], [(0, 2)], [0, 0, 0, 0, 0, 0], []),
    ("the first document", [3, 1, 0, 2], [(0, 1)], [0, 0, 3, 3, 2, 1], [[3, 0, 3]]),
    ("only empty documents", [2, 0, 3, 0, 1], [(1, 2), (3, 4)], [1, 2, 3, 6, 3, 2], [[2, 2, 3], [5, 5, 1]]),
    ("empty and touching ranges", [1, 2, 3, 4, 5], [(0, 0), (1, 2), (2, 3), (4, 4)], [1, 1, 3, 10, 5, 1], [[6, 1, 9]]),
    ("an empty run between two ranges", [1, 2, 0, 0, 3, 4], [(1, 2), (4, 5)], [1, 1, 4, 5, 4, 1], [[6, 1, 4]]),
    ("nothing removed", [2, 3], [(1, 1)], [2, 5, 2, 5, 3, 0], []),
    ("no table", [2, 3], [], [2, 5, 2, 5, 3, 0], []),
    ("no documents", [], [(0, 0)], [0, 0, 0, 0, 0, 0], []),
    ("no documents, no table", [], [], [0, 0, 0, 0, 0, 0], []),
]


@pytest.mark.parametrize("name,lens,ranges,out6,runs", HAND, ids=[h[0] for h in HAND])
def test_hand_worked_plans(name, lens, ranges, out6, runs):
    assert plan(lens, ranges) == (out6, runs)
    assert brute_force(lens, ranges) == (out6, runs)


def test_random_tables_against_the_brute_force_plan():
    rng = np.random.default_rng(20240611)
    for case in range(400):
        n = int(rng.integers(0, 65))
        lens = rng.integers(0, 6, n) * (rng.random(n) < 0.6)          # lengths 0..5, zeros frequent
        cuts = np.sort(rng.integers(0, n + 1, 2 * int(rng.integers(0, 9))))      # ascending ends: empty and touching ranges occur
        ranges = [(int(a), int(b)) for a, b in cuts.reshape(-1, 2)]
        assert plan(lens, ranges) == brute_force(lens, ranges), (case, lens.tolist(), ranges)


def test_refused_tables_name_the_document_count():
    from hiprag import _native as nat
    lens = np.arange(N_REFUSED) % 4
    for ranges, text in REFUSED:
        with pytest.raises(nat.HipRagError) as e:
            plan(lens, ranges)
        assert e.value.code == -1 and text in str(e.value), (ranges, str(e.value))
    with pytest.raises(nat.HipRagError) as e:
        plan(lens, [(3, 2)])
    assert "n_docs = 40" in str(e.value)
    with pytest.raises(nat.HipRagError) as e:
        plan(lens, [], n_ranges=2, null_ranges=True)
    assert e.value.code == -1 and "ranges is null" in str(e.value)
    with pytest.raises(nat.HipRagError) as e:
        plan(lens, [], n_ranges=-1)
    assert e.value.code == -1 and "must not be negative" in str(e.value)
