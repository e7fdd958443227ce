"""
The scope tables of the scoped searches (csrc/scope_plan.h) asked through the library itself: hiprag_scope_plan is host
arithmetic over the tables, needs no device and no handle, and is the code hipidx_search_scoped_dev, hipivf_search_scoped_dev,
hipbm25_search_scoped_dev and hipmaxsim_search_scoped_dev run.  The image against hand-worked values and against a brute
force in numpy that marks every entry with the range of every scope that holds it and counts rows and slices from the marks;
the refused tables of tests/test_scoped_gpu.py with the words their messages must hold.
"""
import numpy as np
import pytest

E_INVALID = -1
SENTINEL = -7
SHAPES = [(16, 8), (16, 16), (256, 8), (256, 16), (0, 8), (0, 16)]      # (slice_rows, group)


def scope_plan(ranges, offsets, soq, n, slice_rows, group, *, n_scopes=None, nq=None, null=(), cap=None, sizes_only=False):
    """(out8, image) of hiprag_scope_plan; on refusal raises after checking that nothing was written"""
    from hiprag import _native as nat
    r = np.ascontiguousarray(ranges, np.int64).reshape(-1, 2)
    o = np.ascontiguousarray(offsets, np.int32)
    q = np.ascontiguousarray(soq, np.int32)
    n_scopes = len(o) - 1 if n_scopes is None else n_scopes
    nq = len(q) if nq is None else nq
    full = 3 * len(r) + 1 + 3 * max(n_scopes, 0) + 1 + max(nq, 0)      # the six sections
    cap = full if cap is None else cap
    out8 = np.full(8, SENTINEL, np.int64)
    img = np.full(max(cap, 1) + 3, SENTINEL, np.int64)
    try:
        nat.call("hiprag_scope_plan", None if "ranges" in null or not len(r) else r.ctypes.data,
                 None if "scope_offsets" in null else o.ctypes.data, n_scopes, None if "scope_of_query" in null else q.ctypes.data, nq, n,
                 slice_rows, group, None if "out8" in null else out8.ctypes.data, None if sizes_only else img.ctypes.data,
                 0 if sizes_only else cap)
    except nat.HipRagError:
        assert np.all(out8 == SENTINEL) and np.all(img == SENTINEL), "a refused call wrote to its outputs"
        raise
    words = int(out8[0])
    if sizes_only:
        assert np.all(img == SENTINEL)
        return out8.tolist(), None
    assert np.all(img[words:] == SENTINEL), "words behind the image were written"
    return out8.tolist(), img[:words].tolist()


def brute_force(ranges, offsets, soq, n, slice_rows, group):
    """The same from the entries: owner[s][i] = the range of scope s that holds entry i, or -1.  A scope's rows are its
    marked entries, its slices the distinct (range, i // slice_rows) among them."""
    r = np.asarray(ranges, np.int64).reshape(-1, 2)
    n_scopes, n_ranges, nq = len(offsets) - 1, len(r), len(soq)
    lean = [int(v) for v in r.reshape(-1)] + [int(v) for v in offsets] + [int(v) for v in soq]
    if slice_rows == 0:
        o_off, o_soq = 2 * n_ranges, 2 * n_ranges + n_scopes + 1
        return [len(lean), 0, 0, o_off, o_off, o_soq, o_soq, o_soq], lean
    per_range = np.zeros(n_ranges, np.int64)
    rows, slices = [], []
    for s in range(n_scopes):
        owner = np.full(n, -1, np.int64)
        for j in range(offsets[s], offsets[s + 1]):
            assert np.all(owner[r[j, 0]:r[j, 1]] == -1)
            owner[r[j, 0]:r[j, 1]] = j
        marked = np.flatnonzero(owner >= 0)
        pairs = {(int(owner[i]), int(i) // slice_rows) for i in marked}
        for j, _ in pairs:
            per_range[j] += 1
        rows.append(len(marked))
        slices.append(len(pairs))
    named = np.bincount(np.asarray(soq, np.int64), minlength=n_scopes)
    bound = sum(-(-int(named[s]) // group) * slices[s] for s in range(n_scopes))
    slice_start = [0] + [int(v) for v in np.cumsum(per_range)]
    img = [int(v) for v in r.reshape(-1)] + slice_start + [int(v) for v in offsets] + rows + slices + [int(v) for v in soq]
    o_slice = 2 * n_ranges
    o_off = o_slice + n_ranges + 1
    o_rows = o_off + n_scopes + 1
    o_sl = o_rows + n_scopes
    o_soq = o_sl + n_scopes
    return [len(img), max(slices, default=0), bound, o_slice, o_off, o_rows, o_sl, o_soq], img


# One table with every feature the rules allow: scope 0 = two touching ranges; scope 1 has no range; scope 2 = a range that
# ends on a boundary of both slice sizes (256), one that starts on it, and an empty one; scope 3 lies behind scope 4
# (descending order across scopes); scope 4 overlaps scope 0 and is named by no query, as is scope 1.
HAND_N = 1000
HAND_RANGES = [(0, 10), (10, 30), (100, 256), (256, 300), (300, 300), (500, 600), (20, 40)]
HAND_OFFSETS = [0, 2, 2, 5, 6, 7]
HAND_SOQ = [0] * 9 + [2, 3]
HAND_FLAT = [v for r in HAND_RANGES for v in r]
HAND = {
    # (slice_rows, group): out8 = {words, smax, bound, o_slice, o_off, o_rows, o_sl, o_soq}, slice_start, rows, slices
    (16, 8): ([49, 13, 26, 14, 22, 28, 33, 38], [0, 1, 3, 13, 16, 16, 23, 25], [30, 0, 200, 100, 20], [3, 0, 13, 7, 2]),
    (256, 16): ([49, 2, 6, 14, 22, 28, 33, 38], [0, 1, 2, 3, 4, 4, 6, 7], [30, 0, 200, 100, 20], [2, 0, 2, 2, 1]),
}


@pytest.mark.parametrize("shape", sorted(HAND))
def test_hand_worked_image(shape):
    out8, slice_start, rows, slices = HAND[shape]
    want = HAND_FLAT + slice_start + HAND_OFFSETS + rows + slices + HAND_SOQ
    assert scope_plan(HAND_RANGES, HAND_OFFSETS, HAND_SOQ, HAND_N, *shape) == (out8, want)
    assert brute_force(HAND_RANGES, HAND_OFFSETS, HAND_SOQ, HAND_N, *shape) == (out8, want)
    assert scope_plan(HAND_RANGES, HAND_OFFSETS, HAND_SOQ, HAND_N, *shape, sizes_only=True) == (out8, None)


def test_hand_worked_lean_image():
    want = HAND_FLAT + HAND_OFFSETS + HAND_SOQ
    assert scope_plan(HAND_RANGES, HAND_OFFSETS, HAND_SOQ, HAND_N, 0, 16) == ([31, 0, 0, 14, 14, 20, 20, 20], want)


CASES = [
    ("every feature at once", HAND_RANGES, HAND_OFFSETS, HAND_SOQ),
    ("one scope, the whole structure", [(0, 777)], [0, 1], [0, 0, 0]),
    ("no range at all", [], [0, 0, 0], [1, 0]),
    ("only empty ranges", [(0, 0), (5, 5), (777, 777)], [0, 2, 3], [0, 1, 1]),
    ("touching ranges across a slice boundary", [(250, 256), (256, 262), (262, 512), (512, 513)], [0, 4], [0] * 17),
    ("ends on and starts on a slice boundary", [(3, 16), (16, 19), (32, 512)], [0, 1, 2, 3], [2, 1, 0, 0]),
    ("overlapping ranges in different scopes, descending", [(600, 700), (0, 650), (10, 20)], [0, 1, 2, 3], [2, 2, 1, 0] * 5),
    ("the last entry alone", [(776, 777)], [0, 1], [0]),
]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name,ranges,offsets,soq", CASES, ids=[c[0] for c in CASES])
def test_listed_tables_against_the_brute_force(name, ranges, offsets, soq, shape):
    assert scope_plan(ranges, offsets, soq, 777, *shape) == brute_force(ranges, offsets, soq, 777, *shape)


def random_table(rng):
    n = int(rng.integers(0, 2001))
    n_scopes = int(rng.integers(1, 7))
    ranges, offsets = [], [0]
    for _ in range(n_scopes):
        m = int(rng.integers(0, 5))
        ends = np.sort(rng.integers(0, n + 1, 2 * m))           # ascending ends: empty and touching ranges occur
        if m and rng.random() < 0.5:
            ends = np.minimum(ends // 16 * 16, n) if rng.random() < 0.5 else np.minimum(ends // 256 * 256, n)   # on slice boundaries
        ranges += [(int(a), int(b)) for a, b in ends.reshape(-1, 2)]
        offsets.append(len(ranges))
    soq = rng.integers(0, n_scopes, int(rng.integers(1, 40))).tolist()
    return ranges, offsets, soq, n


def test_random_tables_against_the_brute_force():
    rng = np.random.default_rng(20261020)
    for case in range(48):
        ranges, offsets, soq, n = random_table(rng)
        for shape in SHAPES:
            assert scope_plan(ranges, offsets, soq, n, *shape) == brute_force(ranges, offsets, soq, n, *shape), (case, shape, ranges, offsets, soq)


# ---- the refused tables of tests/test_scoped_gpu.py (n = 1000, two scopes, three queries) and the words of their messages
GOOD = dict(ranges=((0, 10), (20, 30)), offsets=(0, 1, 2), soq=(0, 1, 1))
REFUSED = [
    (dict(null=("ranges",)), "ranges is null"),
    (dict(null=("scope_offsets",)), "scope_offsets is null"),
    (dict(null=("scope_of_query",)), "scope_of_query is null"),
    (dict(offsets=(1, 1, 2)), "scope_offsets must start at 0"),
    (dict(offsets=(0, 2, 1)), "scope_offsets descends"),
    (dict(ranges=((-1, 10), (20, 30))), "ranges[0]"),
    (dict(ranges=((0, 10), (30, 20))), "ranges[1]"),
    (dict(ranges=((0, 10), (20, 1001))), "ranges[1]"),
    (dict(ranges=((0, 10), (9, 30)), offsets=(0, 2, 2)), "ranges[1]"),       # overlap inside one scope
    (dict(soq=(0, 2, 1)), "scope_of_query[1]"),
    (dict(soq=(0, 1, -1)), "scope_of_query[2]"),
]


def refused(slice_rows=256, group=16, n=1000, **kw):
    from hiprag import _native as nat
    a = dict(GOOD)
    extra = {k: kw.pop(k) for k in list(kw) if k not in a}
    a.update(kw)
    with pytest.raises(nat.HipRagError) as e:
        scope_plan(a["ranges"], a["offsets"], a["soq"], n, slice_rows, group, **extra)
    assert e.value.code == E_INVALID
    return str(e.value)


@pytest.mark.parametrize("kwargs,word", REFUSED, ids=[w for _, w in REFUSED[:5]] + [f"{w} #{i}" for i, (_, w) in enumerate(REFUSED[5:])])
def test_refused_tables_and_their_words(kwargs, word):
    for slice_rows in (256, 0):
        assert word in refused(slice_rows=slice_rows, **kwargs)


def test_messages_name_the_count_and_the_rule():
    assert "is not within 0 <= lo <= hi <= n = 1000" in refused(ranges=((0, 10), (20, 1001)))
    assert "of scope 1 is not within" in refused(ranges=((0, 10), (30, 20)))
    assert "the ranges of a scope ascend and do not overlap" in refused(ranges=((0, 10), (9, 30)), offsets=(0, 2, 2))
    assert "is not a scope in 0..1" in refused(soq=(0, 2, 1))
    # the tables the rules allow: overlap in different scopes, touching ranges, descending order across scopes
    for kw in (dict(ranges=((0, 10), (5, 30))), dict(ranges=((0, 10), (10, 30)), offsets=(0, 2, 2)), dict(ranges=((500, 600), (0, 10)))):
        a = dict(GOOD, **kw)
        assert scope_plan(a["ranges"], a["offsets"], a["soq"], 1000, 256, 16) == brute_force(a["ranges"], a["offsets"], a["soq"], 1000, 256, 16)


def test_the_entry_checks_its_own_arguments():
    assert "nq" in refused(nq=0)
    assert "n_scopes" in refused(n_scopes=0)
    assert "n must not be negative" in refused(n=-1)
    assert "slice_rows" in refused(slice_rows=-1)
    assert "group" in refused(group=0)
    assert "out8" in refused(null=("out8",))
    assert "image_cap" in refused(cap=9)          # the image of GOOD has 4 + 3 + 3 + 2 + 2 + 3 = 17 words
    assert "image_cap" in refused(cap=16)
    assert "image_cap" in refused(slice_rows=0, cap=9)     # the lean one 4 + 3 + 3 = 10
    assert scope_plan(GOOD["ranges"], GOOD["offsets"], GOOD["soq"], 1000, 0, 16, cap=10)[0][0] == 10


def test_the_first_broken_rule_is_reported():
    # in the order of include/hiprag.h: null tables, offsets, null ranges, the ranges scope by scope, scope_of_query
    assert "scope_offsets is null" in refused(null=("scope_offsets", "scope_of_query", "ranges"))
    assert "scope_of_query is null" in refused(null=("scope_of_query",), offsets=(1, 1, 2))
    assert "must start at 0" in refused(offsets=(1, 0, 2), soq=(0, 5, 1))
    assert "descends" in refused(offsets=(0, 2, 1), null=("ranges",))
    assert "ranges is null" in refused(null=("ranges",), soq=(0, 5, 1))
    assert "ranges[0]" in refused(ranges=((0, 1001), (30, 20)))
    assert "is not within" in refused(ranges=((0, 10), (12, 9)), offsets=(0, 2, 2))      # bounds before overlap in one range
    assert "ranges[1]" in refused(ranges=((0, 10), (9, 30), (40, 35)), offsets=(0, 2, 3))
    assert "ranges[1]" in refused(ranges=((0, 10), (30, 20)), soq=(7, 1, 1))
    assert "scope_of_query[0]" in refused(soq=(2, 2, -1))
    assert "n_scopes" in refused(n_scopes=0, null=("scope_offsets",))                    # the entry's own checks come first
