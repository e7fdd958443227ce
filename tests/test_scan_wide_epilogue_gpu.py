"""
The epilogue of the wide scan kernel (csrc/scan_wide.h): a tile's bound, test and appends run in phases under the k-steps
of the NEXT tile, so a wave carries a pending tile across tile, column and row-tile boundaries and drains it where the
next tile has fewer k-steps than there are phases, and a lane takes one list position per query and tile for up to four
entries.  A lost pending tile only shows if it held a top-k row, so the cases that target draining PLANT their queries:
query j is row r_j plus 5 % noise, renormalised, and ids[:, 0] must be r.  Every case: ids bit-exact against the CPU
oracle, scores within 1e-4, every launch a wide one, nobody on the exhaustive path.
"""
import functools

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu
TOL = 1e-4
K = 10

# list entries per query of the PARENT commit's wide kernel at the shape of test_lists_do_not_get_longer, three runs on
# one MI355X; the bound is their largest, with no margin: a later test against a bound that only rises
# cannot lengthen a list
PARENT_LIST_ENTRIES_PER_QUERY = (357.740234375, 412.705078125, 424.314453125)


@functools.lru_cache(maxsize=None)
def _rows(n, d, seed):
    x = ho.synthetic_vectors(n, d, seed=seed)
    x.setflags(write=False)
    return x


def _planted(x, r, seed):
    """row r_j plus 5 % noise, renormalised (the construction of test_every_wave_position_is_home_of_a_best_row)"""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((len(r), x.shape[1]))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    q = x[r].astype(np.float64) + 0.05 * noise
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _index(monkeypatch, x, metric, wide="1", spare=0):
    from hiprag import HipFlatIndex
    monkeypatch.setenv("HIPRAG_SCAN_WIDE", wide)
    ix = HipFlatIndex(x.shape[1], metric)
    ix.add(x)
    ix.set_spare_cus(spare)
    return ix


def _check(ix, x, q, metric, r=None, rows=None):
    es, ei = ho.flat_search(x, q, K, metric)
    s, i = ix.search(q, K)
    if r is not None:
        rows = slice(None) if rows is None else rows
        assert np.array_equal(i[rows, 0], r), f"planted rows lost: first bad queries {np.argwhere(i[rows, 0] != r)[:5].ravel()}"
    assert np.array_equal(i, ei), f"ids differ: first bad queries {np.argwhere((i != ei).any(1))[:5].ravel()}"
    assert np.allclose(s, es, rtol=0, atol=TOL)
    st = ix.stats()
    assert st["wide_launches"] == st["launches"] and st["launches"] >= 1
    assert st["fallback_queries"] == 0
    return st


@pytest.mark.parametrize("d,metric", [(64, ho.METRIC_IP), (64, ho.METRIC_L2), (256, ho.METRIC_IP), (512, ho.METRIC_IP),
                                      (1024, ho.METRIC_IP)])
def test_every_number_of_k_steps(gpu, monkeypatch, d, metric):
    """d = 64 / 256 / 512 / 1024 -> 2 / 4 / 8 / 16 k-steps per tile.  20,011 rows = 79 row tiles, one per workgroup, and 256
    queries = one column: a workgroup's only tile is drained after the loop, and with two k-steps every phase runs there.
    Planted rows in the first tile, a middle tile and the last full tile, every (block, query tile) position."""
    n, nq = 20011, 256
    x = _rows(n, d, 401)
    j = np.arange(nq)
    t = np.array([0, 39, n // 256 - 1])[(j // 8) % 3]
    r = 32 * (8 * t + j % 8) + (7 * j) % 32
    ix = _index(monkeypatch, x, metric)
    st = _check(ix, x, _planted(x, r, 402), metric, r)
    assert st["launches"] == 1


@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
def test_pending_tile_of_a_wave_that_goes_dead(gpu, monkeypatch, metric):
    """16,385 rows, d = 100, 257 queries: the second column has one live unit, so the waves of units 1..3 carry the pending
    tile of column 0 into a column they do not compute.  Queries 64..255 (units 1..3) are planted, tile by tile, in the one
    row tile each workgroup owns; the others are ordinary."""
    n, d, nq = 16385, 100, 257
    x = _rows(n, d, 411)
    q = ho.synthetic_queries(nq, d, seed=412).copy()
    j = np.arange(64, 256)
    r = 256 * (j % 64) + 32 * ((j // 64 + j) % 8) + (7 * j) % 32      # all 64 full row tiles, every block of a tile
    q[64:256] = _planted(x, r, 413)
    ix = _index(monkeypatch, x, metric)
    st = _check(ix, x, q, metric, r, slice(64, 256))
    assert st["launches"] == 1 and st["passes"] == 5


@pytest.mark.parametrize("nq", [300, 1024])
def test_pending_across_row_tiles_and_the_last_tile(gpu, monkeypatch, nq):
    """70,001 rows, d = 200 (four k-steps, so every tile change drains two phases at once), 200 spare CUs: every workgroup
    walks four or five row tiles.  Planted rows in a workgroup's first tile, a tile of its second round, the last full
    tile and the partial last tile (row 70,000, the index's last)."""
    n, d = 70001, 200
    x = _rows(n, d, 421)
    import torch
    g = torch.cuda.get_device_properties(0).multi_processor_count - 200      # scan workgroups
    assert 32 <= g and 4 * g <= (n + 255) // 256
    j = np.arange(nq)
    kind = (j // 8) % 4
    t = np.array([3, g + 7, n // 256 - 1, 0])[kind]
    r = np.where(kind == 3, n - 1, 32 * (8 * t + j % 8) + (7 * j) % 32)
    ix = _index(monkeypatch, x, ho.METRIC_IP, spare=200)
    st = _check(ix, x, _planted(x, r, 422 + nq), ho.METRIC_IP, r)
    assert st["launches"] == 1


@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
def test_fused_counts(gpu, monkeypatch, metric):
    """40 copies of one row inside one 256-row tile, five in each of its 8 blocks, and a query equal to that row: all four
    blocks of a lane pass at once, so a lane takes four list positions with one atomic.  search_device returns the same
    bits whichever kernel nominated the candidates; the duplicate query may take the exhaustive path, in both or in none."""
    import torch
    n, d, nq = 20011, 128, 200
    x = _rows(n, d, 431).copy()
    q = ho.synthetic_queries(nq, d, seed=432).copy()
    tile = 17
    dup = (256 * tile + 32 * np.arange(8)[:, None] + np.array([0, 7, 13, 22, 31])[None, :]).ravel()
    x[dup] = x[5]
    q[3] = x[5]
    qd = torch.from_numpy(q).cuda()
    outs, fallbacks = [], []
    for wide in ("0", "1"):
        ix = _index(monkeypatch, x, metric, wide)
        s64, s32, ids = ix.search_device(qd, K)
        torch.cuda.synchronize()
        st = ix.stats()
        assert st["wide_launches"] == (st["launches"] if wide == "1" else 0) and st["launches"] == 1
        assert st["list_entries"] / st["queries"] <= 2048
        fallbacks.append(st["fallback_queries"])
        outs.append((s64.clone(), s32.clone(), ids.clone()))
        ix.close()
    assert fallbacks[0] == fallbacks[1]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2])
    es, ei = ho.flat_search(x, q, K, metric)
    assert np.array_equal(outs[1][2].cpu().numpy(), ei)
    assert np.allclose(outs[1][1].cpu().numpy(), es, rtol=0, atol=TOL)


def test_lists_do_not_get_longer(gpu, monkeypatch):
    """The shape of test_the_filter_filters (70,001 rows, d = 256, 512 queries, wide): the lists are no longer than the
    parent commit's, whose three measured values stand above."""
    n, d, nq = 70001, 256, 512
    x = _rows(n, d, 351)
    q = ho.synthetic_queries(1024, d, seed=352)[:nq]
    ix = _index(monkeypatch, x, ho.METRIC_IP)
    st = _check(ix, x, q, ho.METRIC_IP)
    per_query = st["list_entries"] / st["queries"]
    print(f"list entries per query {per_query:.2f} (parent: {PARENT_LIST_ENTRIES_PER_QUERY})")
    assert per_query <= max(PARENT_LIST_ENTRIES_PER_QUERY)
