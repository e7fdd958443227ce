"""
The work items of the three sliced scoped searches (csrc/slice_items.h) asked through the library itself: hiprag_slice_items
is host arithmetic, needs no device and no handle, and runs the decode scoped_kernel, maxsim_scope_kernel and
interaction_kernel run, over tables formed as the counting sort and group_item_scan_kernel form them.  Against a brute force
in numpy that marks every entry with the range of its scope that holds it: for every scope and every query group of it the
windows of its items are disjoint and cover exactly the scope's entries, on absolute slice boundaries; items come in (scope,
slice, group) order; the groups of a slice hold the queries that name the scope, once each; there are as many items as
hiprag_scope_plan's bound says.  Integer equality throughout.
"""
import ctypes

import numpy as np
import pytest

E_INVALID = -1
SENTINEL = -7
SHAPES = [(256, 16), (16, 8), (256, 8)]      # (slice_rows, group): flat scoped, exact MaxSim, pruned MaxSim
WORDS = 8                                    # scope, slice, group, members, first, base, p_lo, p_hi


def slice_items(ranges, offsets, soq, n, slice_rows, group, *, cap=None, count_only=False):
    """[items][8] of hiprag_slice_items; on refusal raises after checking that nothing was written"""
    from hiprag import _native as nat
    r = np.ascontiguousarray(ranges, np.int64).reshape(-1, 2)
    o = np.ascontiguousarray(offsets, np.int32)
    q = np.ascontiguousarray(soq, np.int32)
    args = (r.ctypes.data if len(r) else None, o.ctypes.data, len(o) - 1, q.ctypes.data, len(q), n, slice_rows, group)
    count = ctypes.c_int64(SENTINEL)
    if cap is None:
        nat.call("hiprag_slice_items", *args, None, 0, ctypes.byref(count))
        cap = count.value
        if count_only:
            return cap
    out = np.full((cap + 1) * WORDS, SENTINEL, np.int64)
    count = ctypes.c_int64(SENTINEL)
    try:
        nat.call("hiprag_slice_items", *args, out.ctypes.data, cap, ctypes.byref(count))
    except nat.HipRagError:
        assert count.value == SENTINEL and np.all(out == SENTINEL), "a refused call wrote to its outputs"
        raise
    assert np.all(out[count.value * WORDS:] == SENTINEL), "words behind the items were written"
    return out[:count.value * WORDS].reshape(-1, WORDS)


def plan_bound(ranges, offsets, soq, n, slice_rows, group):
    from hiprag import _native as nat
    r = np.ascontiguousarray(ranges, np.int64).reshape(-1, 2)
    o = np.ascontiguousarray(offsets, np.int32)
    q = np.ascontiguousarray(soq, np.int32)
    out8 = np.zeros(8, np.int64)
    nat.call("hiprag_scope_plan", r.ctypes.data if len(r) else None, o.ctypes.data, len(o) - 1, q.ctypes.data, len(q), n, slice_rows, group,
             out8.ctypes.data, None, 0)
    return int(out8[2])


def check(ranges, offsets, soq, n, S, G):
    """every property of the module docstring, from the entries"""
    items = slice_items(ranges, offsets, soq, n, S, G)
    r = np.asarray(ranges, np.int64).reshape(-1, 2)
    soq = np.asarray(soq, np.int64)
    n_scopes = len(offsets) - 1
    named = np.bincount(soq, minlength=n_scopes)
    pair_offs = np.concatenate([[0], np.cumsum(named)])      # a stable sort by scope: scope s holds places pair_offs[s] ..
    assert len(items) == plan_bound(ranges, offsets, soq, n, S, G) == slice_items(ranges, offsets, soq, n, S, G, count_only=True)
    keys = [tuple(int(v) for v in it[:3]) for it in items]
    assert keys == sorted(set(keys)), "items are not in strict (scope, slice, group) order"
    assert {k[0] for k in keys} == {s for s in range(n_scopes) if named[s] and np.any(r[offsets[s]:offsets[s + 1], 1] > r[offsets[s]:offsets[s + 1], 0])}
    for s in range(n_scopes):
        mine = items[items[:, 0] == s]
        if not named[s]:
            assert len(mine) == 0, "a scope no query names has items"
            continue
        owner = np.full(n, -1, np.int64)
        for j in range(offsets[s], offsets[s + 1]):
            owner[r[j, 0]:r[j, 1]] = j
        groups = -(-int(named[s]) // G)
        n_slices = len({(int(owner[i]), int(i) // S) for i in np.flatnonzero(owner >= 0)})
        assert sorted(set(mine[:, 1].tolist())) == list(range(n_slices)), "the slices of a scope are not 0 .. slices - 1"
        for sl in range(n_slices):
            of_slice = mine[mine[:, 1] == sl]
            assert of_slice[:, 2].tolist() == list(range(groups))
            assert of_slice[:, 3].sum() == named[s], "the members of a slice's groups are not the queries that name the scope"
            for g, it in enumerate(of_slice):
                assert it[3] == min(G, named[s] - g * G) and it[4] == pair_offs[s] + g * G
                assert len({tuple(v) for v in of_slice[:, 5:].tolist()}) == 1, "the groups of a slice differ in their window"
        for g in range(groups):
            seen = np.zeros(n, np.int64)
            for _, _, _, _, _, base, p_lo, p_hi in mine[mine[:, 2] == g].tolist():
                assert base % S == 0 and 0 <= p_lo < p_hi <= S
                assert len(set(owner[base + p_lo:base + p_hi].tolist())) == 1, "a window crosses the end of a range"
                seen[base + p_lo:base + p_hi] += 1
            assert np.array_equal(seen, (owner >= 0).astype(np.int64)), "the windows of a group are not exactly the scope's entries, once each"
    return items


def designed_table(S, G):
    """Every case at once, laid on the boundaries of slices of S entries and groups of G queries."""
    scopes = [
        ([], 1),                                                        # a scope without ranges
        ([(S + 3, S + 3), (S + 7, S + 8)], G),                          # an empty range; a one-entry range
        ([(S, 2 * S),                                                   # starts on and ends on a boundary
          (3 * S - 1, 4 * S + 1),                                       # starts one before, ends one after: three slices
          (5 * S + 1, 6 * S - 1),                                       # starts one after, ends one before
          (7 * S - 1, 7 * S)], G + 1),                                  # one entry, the last of its slice
        ([(8 * S + 2, 8 * S + 5), (8 * S + 9, 8 * S + 12)], 2 * G + 1), # two ranges inside one slice
        ([(0, 13 * S)], 0),                                             # the whole structure, named by no query
        ([(9 * S, 12 * S), (12 * S, 12 * S + 1)], 1),                   # exactly three slices, then a touching entry
    ]
    ranges, offsets, per_scope = [], [0], []
    for rs, n_queries in scopes:
        ranges += rs
        offsets.append(len(ranges))
        per_scope.append(n_queries)
    soq = []                                                            # queries of different scopes interleaved: round robin
    left = list(per_scope)
    while any(left):
        for s in range(len(left)):
            if left[s]:
                soq.append(s)
                left[s] -= 1
    return ranges, offsets, soq, 13 * S


@pytest.mark.parametrize("S,G", SHAPES)
def test_designed_table(S, G):
    ranges, offsets, soq, n = designed_table(S, G)
    items = check(ranges, offsets, soq, n, S, G)
    # hand-worked: the range [3S - 1, 4S + 1) of scope 2 is slices 1..3 of it, windows [S - 1, S), [0, S), [0, 1)
    got = [tuple(it[[1, 5, 6, 7]].tolist()) for it in items if it[0] == 2 and it[2] == 0 and 1 <= it[1] <= 3]
    assert got == [(1, 2 * S, S - 1, S), (2, 3 * S, 0, S), (3, 4 * S, 0, 1)]
    # the two ranges inside one slice of scope 3: two slices of the scope on one base
    got = [tuple(it[[1, 5, 6, 7]].tolist()) for it in items if it[0] == 3 and it[2] == 2]
    assert got == [(0, 8 * S, 2, 5), (1, 8 * S, 9, 12)]
    assert items[items[:, 0] == 3][:, 3].tolist() == [G, G, 1] * 2


def test_random_tables():
    rng = np.random.default_rng(20261021)
    for case in range(24):
        n = int(rng.integers(1, 1500))
        n_scopes = int(rng.integers(1, 6))
        ranges, offsets = [], [0]
        for _ in range(n_scopes):
            m = int(rng.integers(0, 4))
            ends = np.sort(rng.integers(0, n + 1, 2 * m))
            if m and rng.random() < 0.5:
                ends = np.minimum((ends + int(rng.integers(-1, 2))).clip(0) // 16 * 16, n)
                ends = np.sort(ends)
            ranges += [(int(a), int(b)) for a, b in ends.reshape(-1, 2)]
            offsets.append(len(ranges))
        soq = rng.integers(0, n_scopes, int(rng.integers(1, 40))).tolist()
        for S, G in SHAPES:
            check(ranges, offsets, soq, n, S, G)


def refused(ranges=((0, 10), (20, 30)), offsets=(0, 1, 2), soq=(0, 1, 1), n=1000, S=256, G=16, **kw):
    from hiprag import _native as nat
    with pytest.raises(nat.HipRagError) as e:
        slice_items(ranges, offsets, soq, n, S, G, **kw)
    assert e.value.code == E_INVALID
    return str(e.value)


def test_refusals_write_nothing():
    for S, G in [(16, 16), (256, 1), (0, 8), (32, 8), (16, 0)]:
        assert "no sliced search" in refused(S=S, G=G, cap=4)
    assert "items_cap" in refused(cap=1)                   # the table has 2 items: one slice and one group in either scope
    assert len(slice_items(((0, 10), (20, 30)), (0, 1, 2), (0, 1, 1), 1000, 256, 16, cap=2)) == 2
    assert "ranges[1]" in refused(ranges=((0, 10), (20, 1001)), cap=4)
    assert "scope_of_query[1]" in refused(soq=(0, 2, 1), cap=4)
    assert "n must not be negative" in refused(n=-1, cap=4)
