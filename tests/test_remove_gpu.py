"""
hipidx_remove_ranges: after a removal the index is indistinguishable from its FRESH-BUILD TWIN -- an index of the same d,
metric, scan mode and id_base built by one add of np.delete(X, rows, 0): ntotal, the bytes save writes, reconstruct, the three
outputs of search_dev (scan path and exhaustive path) and of search_scoped_dev, row_bounds, launch_queries, and what a later
add sees.  Ids are also those of the CPU oracle over the survivors.
"""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu

METRICS = {"ip": ho.METRIC_IP, "l2": ho.METRIC_L2}
STAGING_LIMIT = 256 << 20


def _rows_of(ranges):
    return np.concatenate([np.arange(lo, hi) for lo, hi in ranges] + [np.zeros(0, np.int64)]).astype(np.int64)


def _build(x, d, metric, id_base=0):
    from hiprag import HipFlatIndex
    ix = HipFlatIndex(d, metric)
    if id_base:
        ix.set_id_base(id_base)
    if len(x):
        ix.add(x)
    return ix


def _file(ix, path):
    ix.save(str(path))
    return open(path, "rb").read()


def _same_searches(ix, twin, x, metric, id_base, tag, oracle=True):
    """search_dev (nq 1 and 70; k 10, 50 on the scan path, 200 on the exhaustive path) and search_scoped_dev over two scopes:
    all three outputs bit-equal to the twin's; ids equal to the oracle's over the surviving rows x"""
    import torch
    n, d = x.shape
    q70 = ho.synthetic_queries(70, d, seed=77)
    for nq in (1, 70):
        q = torch.from_numpy(q70[:nq]).cuda()
        for k in (10, 50, 200):
            a = [t.cpu().numpy() for t in ix.search_device(q, k)]
            b = [t.cpu().numpy() for t in twin.search_device(q, k)]
            for u, v, name in zip(a, b, ("scores64", "scores32", "ids")):
                assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (tag, "search_dev", name, nq, k)
            if oracle and k == 50:
                _, want = ho.flat_search(x, q70[:nq], k, METRICS[metric], id_base=id_base)
                assert np.array_equal(a[2], want), (tag, "oracle ids", nq, k)
    # two scopes: a range that straddles a block boundary near the front, and two ranges up to the last row
    scopes = [[(1, min(n, 45))], [(n // 3, n // 3 + (n - n // 3) // 2), (n - max(1, n // 7), n)]]
    q = torch.from_numpy(q70[:6]).cuda()
    soq = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    a = [t.cpu().numpy() for t in ix.search_scoped_device(q, 10, scopes, soq)]
    b = [t.cpu().numpy() for t in twin.search_scoped_device(q, 10, scopes, soq)]
    for u, v, name in zip(a, b, ("scores64", "scores32", "ids")):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (tag, "search_scoped_dev", name)


def _same_index(ix, twin, x, metric, id_base, tmp_path, tag, oracle=True):
    n, d = x.shape
    assert ix.ntotal == twin.ntotal == n, tag
    assert _file(ix, tmp_path / "a.index") == _file(twin, tmp_path / "b.index"), (tag, "save")
    for r in sorted({0, n // 2, n - 1, min(31, n - 1), min(32, n - 1)} if n else ()):
        assert np.array_equal(ix.reconstruct(r).view(np.uint32), x[r].view(np.uint32)), (tag, "reconstruct", r)
    a, b = ix.row_bounds(), twin.row_bounds()
    assert (a[0].view(np.uint32), a[1].view(np.uint32)) == (b[0].view(np.uint32), b[1].view(np.uint32)), (tag, "row_bounds", a, b)
    assert ix.launch_queries == twin.launch_queries, tag
    if n:
        _same_searches(ix, twin, x, metric, id_base, tag, oracle)


def _remove_and_compare(x, d, metric, ranges, tmp_path, tag, id_base=0, oracle=True):
    """remove `ranges` from an index of x, compare with the twin, add 1 000 rows to both, compare again; returns remove_info"""
    ix = _build(x, d, metric, id_base)
    rows = _rows_of(ranges)
    assert ix.remove_ranges(ranges) == len(rows), tag
    info = ix.remove_info()
    assert info["rows_removed"] == len(rows) and info["staging_bytes"] <= STAGING_LIMIT, (tag, info)
    survivors = np.delete(x, rows, axis=0)
    first = int(rows.min()) if len(rows) else len(x)
    assert info["rows_moved"] == len(survivors) - first, (tag, info)
    twin = _build(survivors, d, metric, id_base)
    _same_index(ix, twin, survivors, metric, id_base, tmp_path, tag, oracle)
    more = ho.synthetic_vectors(1000, d, seed=5150)          # the rows behind the new ntotal must be zero again
    ix.add(more)
    twin.add(more)
    _same_index(ix, twin, np.concatenate([survivors, more]), metric, id_base, tmp_path, tag + " +1000", oracle)
    ix.close()
    twin.close()
    return info


def _small_tables(n):
    """range tables over n >= 900 rows"""
    return {
        "single row": [(n // 2, n // 2 + 1)],
        "row 0": [(0, 1)],
        "last row": [(n - 1, n)],
        "whole tail": [(n - n // 3, n)],
        "inside one block": [(65, 77)],
        "crossing blocks and 256": [(29, 35), (250, 263), (509, 771)],
        "touching and empty": [(10, 10), (10, 20), (20, 33), (40, 40), (50, 61), (n, n)],
    }


@pytest.mark.parametrize("mode", ["bf16", "q64"])
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("d", [1024, 100, 8])
def test_small_range_tables_match_the_fresh_build(gpu, tmp_path, monkeypatch, d, metric, mode):
    monkeypatch.setenv("HIPRAG_SCAN_MODE", mode)          # read when a handle is created
    n = 937
    x = ho.synthetic_vectors(n, d, seed=11 + d)
    for name, ranges in _small_tables(n).items():
        info = _remove_and_compare(x, d, metric, ranges, tmp_path, f"{name} d={d} {metric} {mode}")
        if name in ("last row", "whole tail"):
            assert info["rows_moved"] == 0 and info["chunks"] == 0 and info["staging_bytes"] == 0, (name, info)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("d", [1024, 100, 8])
def test_everything_then_add(gpu, tmp_path, d, metric):
    n = 300
    x = ho.synthetic_vectors(n, d, seed=3)
    info = _remove_and_compare(x, d, metric, [(0, n)], tmp_path, f"everything d={d} {metric}")
    assert info["rows_moved"] == 0
    ix = _build(x, d, metric)
    assert ix.remove_ranges([(0, 100), (100, n)]) == n and ix.ntotal == 0
    assert ix.remove_ranges([]) == 0 and ix.remove_ranges([(0, 0)]) == 0 and ix.ntotal == 0


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("d", [1024, 100, 8])
def test_many_small_ranges(gpu, tmp_path, d, metric):
    n = 6011
    x = ho.synthetic_vectors(n, d, seed=21)
    rng = np.random.default_rng(5)
    starts = 3 + 11 * np.arange(520)
    ranges = [(int(s), int(s + rng.integers(1, 8))) for s in starts]       # 520 ranges of 1..7 rows, 11 apart
    info = _remove_and_compare(x, d, metric, ranges, tmp_path, f"many d={d} {metric}")
    assert info["chunks"] == 1


@pytest.mark.parametrize("metric,mode", [("ip", "bf16"), ("l2", "q64")])
def test_large_index_moves_in_several_chunks(gpu, tmp_path, monkeypatch, metric, mode):
    """70 000 x 1024: the 4-wave scan partition, and more rows behind the first removed one than one 256 MiB chunk of staging
    holds (a block of 32 rows is 192.1 KiB of fp32 rows, filter copy and norms: 1 364 blocks = 43 648 rows per chunk)"""
    monkeypatch.setenv("HIPRAG_SCAN_MODE", mode)
    n, d = 70000, 1024
    x = ho.synthetic_vectors(n, d, seed=8)
    ranges = [(5, 6), (1000, 1033), (31999, 32001), (40000, 40007), (69990, 69995)]
    info = _remove_and_compare(x, d, metric, ranges, tmp_path, f"large {metric} {mode}")
    assert info["chunks"] >= 2 and info["rows_moved"] == n - 48 - 5


def test_removed_outlier_brings_the_bounds_back(gpu, tmp_path):
    n, d = 2000, 100
    x = ho.synthetic_vectors(n, d, seed=4)
    x[777] *= 10.0                                           # 100 x the squared norm of every other row
    ix = _build(x, d, "ip")
    before = ix.row_bounds()
    assert before[0] >= 99.0
    assert ix.remove_ranges([(777, 778)]) == 1
    survivors = np.delete(x, [777], axis=0)
    twin = _build(survivors, d, "ip")
    after, want = ix.row_bounds(), twin.row_bounds()
    assert after[0] < 1.01 and after[0] < before[0] and after[1] < before[1], (before, after)    # the bounds fell ...
    assert (after[0].view(np.uint32), after[1].view(np.uint32)) == (want[0].view(np.uint32), want[1].view(np.uint32))   # ... to the twin's
    _same_index(ix, twin, survivors, "ip", 0, tmp_path, "outlier")


def test_remove_info_counts_the_rows_behind_the_first_removed_one(gpu):
    n, d = 5000, 100
    x = ho.synthetic_vectors(n, d, seed=6)
    for r, m in ((0, 1), (1, 40), (2500, 3), (4967, 1), (4000, 1000)):
        ix = _build(x, d, "l2")
        assert ix.remove_ranges([(r, r + m)]) == m
        info = ix.remove_info()
        assert info == {"rows_removed": m, "rows_moved": ix.ntotal - r, "chunks": 1 if ix.ntotal > r else 0,
                        "staging_bytes": info["staging_bytes"]}
        assert info["staging_bytes"] <= STAGING_LIMIT and (info["staging_bytes"] > 0) == (ix.ntotal > r)
        ix.close()


def test_two_removals_equal_the_removal_of_their_union(gpu, tmp_path):
    n, d = 3000, 1024
    x = ho.synthetic_vectors(n, d, seed=9)
    one, two = _build(x, d, "l2"), _build(x, d, "l2")
    # union, in the original numbering: [100, 130) and [2000, 2100) first, then [50, 60) and [1500, 1600)
    one.remove_ranges([(50, 60), (100, 130), (1500, 1600), (2000, 2100)])
    two.remove_ranges([(100, 130), (2000, 2100)])
    two.remove_ranges([(50, 60), (1470, 1570)])              # 1500 - 30 rows already gone before it
    survivors = np.delete(x, _rows_of([(50, 60), (100, 130), (1500, 1600), (2000, 2100)]), axis=0)
    _same_index(two, one, survivors, "l2", 0, tmp_path, "two removals")


def test_bad_tables_are_refused_and_leave_the_index_as_it_was(gpu, tmp_path):
    from hiprag import HipRagError
    n, d = 500, 100
    x = ho.synthetic_vectors(n, d, seed=12)
    ix = _build(x, d, "ip")
    before = _file(ix, tmp_path / "before.index")
    bounds = ix.row_bounds()
    for bad in ([(100, 200), (50, 60)],            # descending
                [(100, 200), (150, 250)],          # overlapping
                [(400, 501)],                      # hi > ntotal
                [(-1, 5)],                         # negative lo
                [(30, 20)],                        # hi < lo
                None):                             # a null table with n > 0
        with pytest.raises(HipRagError):
            ix.remove_ranges(bad)
        assert ix.ntotal == n and _file(ix, tmp_path / "after.index") == before, bad
        assert ix.row_bounds() == bounds
    assert ix.remove_ranges([(100, 200)]) == 100                          # and it still works


def test_an_index_under_a_live_ivf_view_is_refused(gpu, tmp_path):
    from hiprag import HipFlatIndex, HipRagError
    from hiprag.ivf import HipIVFIndex
    d = 64
    x = ho.synthetic_vectors(64, d, seed=2)
    rows, cents = _build(x, d, "ip"), _build(x[[0, 32]], d, "ip")
    before = _file(rows, tmp_path / "rows.index")
    ivf = HipIVFIndex.from_parts(rows, cents, [0, 32, 64], np.arange(64))
    for held in (rows, cents):
        with pytest.raises(HipRagError, match="IVF"):
            held.remove_ranges([(0, 1)])
    assert rows.ntotal == 64 and _file(rows, tmp_path / "rows2.index") == before
    ivf.close()
    assert rows.remove_ranges([(3, 9)]) == 6 and rows.ntotal == 58
    twin = HipFlatIndex(d, "ip")
    twin.add(np.delete(x, np.arange(3, 9), axis=0))
    assert _file(rows, tmp_path / "rows3.index") == _file(twin, tmp_path / "twin.index")


def test_ranges_are_local_and_ids_carry_the_base(gpu, tmp_path):
    n, d, base = 1500, 100, 1_000_000
    x = ho.synthetic_vectors(n, d, seed=14)
    _remove_and_compare(x, d, "l2", [(0, 3), (700, 733)], tmp_path, "id_base", id_base=base)
    ix = _build(x, d, "ip", id_base=base)
    ix.remove_ranges([(10, 20)])
    _, ids = ix.search(x[25:26], 1)
    assert ids[0, 0] == base + 15                              # row 25 is row 15 now, and the base is added
