"""
The last round of the wide scan's walk (wide_walk, csrc/dense_plan.h; csrc/scan_wide.h follows it): the row tiles left
over by the full rounds are split by COLUMN over all the workgroups, so a workgroup's tail pairs are tiles of different
row tiles, a row tile's columns run on different workgroups at once, and a pending tile of the full rounds finishes under a
tail pair.  Small indexes on a grid of 56 workgroups (set_spare_cus(n_cu - 56), wide forced): two full rounds and a tail
of L row tiles, with a partial last tile.  A pair that the walk skipped loses a planted row; a pair computed twice puts
duplicate keys on a list, which the finish's ranking by counting turns into a fallback query.
"""
import functools

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu
TOL = 1e-4
K = 10
G = 56            # workgroups of the scan
ROUNDS = 2        # full rounds
NQ_MAX = 1024


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _rows(d):
    """the largest index of the file; a case takes its first n rows"""
    x = ho.synthetic_vectors((ROUNDS * G + 55) * 256 - 5, d, seed=611 + d)
    x.setflags(write=False)
    return x


def _planted_rows(left):
    """Query j of column c = j // 256, jj = j % 256: group jj // 8 chooses the row tile, jj % 8 the block, 7 j % 32 the row.
    Row tiles: one of the first round, the last of the full rounds, the first, a middle and the last of the tail -- at
    ncol columns the pair (tail tile i, column c) is number i ncol + c of the tail, a workgroup's first tail pair below 56
    and its second from 56 on, so with the first and the last tail tile both positions are home of a planted row wherever
    the walk has both -- and the very last row of the partial last tile.  The same in every column."""
    nrt = ROUNDS * G + left
    n = nrt * 256 - 5
    j = np.arange(NQ_MAX)
    jj = j % 256
    tiles = np.array([3, ROUNDS * G - 1, ROUNDS * G, ROUNDS * G + left // 2, nrt - 1, nrt - 1])
    kind = (jj // 8) % len(tiles)
    r = 256 * tiles[kind] + 32 * (jj % 8) + (7 * j) % 32
    return n, np.where(kind == len(tiles) - 1, n - 1, np.minimum(r, n - 1))


def _planted(x, r, seed):
    """row r_j plus 5 % noise, renormalised: a pair that the walk skipped loses the planted row"""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((len(r), x.shape[1]))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    q = x[r].astype(np.float64) + 0.05 * noise
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _queries(left, d):
    """rows and the 1024 planted queries, once per (L, d); a launch of nq queries takes the first nq"""
    n, r = _planted_rows(left)
    x = _rows(d)[:n]
    q = _planted(x, r, 1000 * left + d)
    q.setflags(write=False)
    return x, r, q


@functools.lru_cache(maxsize=None)
def _truth(left, d, metric, col):
    """the oracle's answer for the 256 queries of one column, once: a case of more columns adds only what no case before it
    has asked for (the oracle is one CPU thread, a few seconds per column at d = 416)"""
    x, r, q = _queries(left, d)
    lo = 256 * col
    es, ei = ho.flat_search(x, q[lo:lo + 256], K, metric)
    assert np.array_equal(ei[:, 0], r[lo:lo + 256]), "the oracle itself does not find every planted row: the case is badly built"
    return es, ei


def _case(left, d, metric, nq):
    x, r, q = _queries(left, d)
    cols = [_truth(left, d, metric, c) for c in range((nq + 255) // 256)]
    return x, r[:nq], q[:nq], np.concatenate([c[0] for c in cols])[:nq], np.concatenate([c[1] for c in cols])[:nq]


@pytest.mark.parametrize("metric", [ho.METRIC_IP, ho.METRIC_L2])
@pytest.mark.parametrize("d", [128, 416])       # 4 k-steps per tile: every tile ends in a drain; 16: the phases run under the next pair
@pytest.mark.parametrize("nq", [256, 512, 600, 1024])   # 1, 2, 3 (a short last one) and 4 columns
@pytest.mark.parametrize("left", [1, 28, 29, 55])
def test_the_tail_is_split_by_column(gpu, monkeypatch, left, nq, d, metric):
    """nrt = 2 x 56 + L row tiles, rows = 256 nrt - 5.  L = 28 at two columns fills the tail exactly, L = 29 gives one
    workgroup two tail pairs, L = 1 spreads one row tile over ncol workgroups.  Ids are the oracle's and no planted row is
    lost on the grid of 56; ids and scores are the same arrays on the grids of n_cu, n_cu - 32 and n_cu - 48 workgroups;
    every launch is a wide one and no query takes the exhaustive path."""
    from hiprag import HipFlatIndex
    n_cu = _n_cu()
    assert n_cu - G >= 0
    x, r, q, es, ei = _case(left, d, metric, nq)
    assert (len(x) + 255) // 256 == ROUNDS * G + left and len(x) % 256 == 251
    monkeypatch.setenv("HIPRAG_SCAN_WIDE", "1")
    ix = HipFlatIndex(d, metric)
    ix.add(x)
    outs = []
    spares = (n_cu - G, 0, 32, 48)
    for spare in spares:
        ix.set_spare_cus(spare)
        s, i = ix.search(q, K)
        assert np.array_equal(i[:, 0], r), f"spare {spare}: planted rows lost, first bad queries {np.argwhere(i[:, 0] != r)[:5].ravel()}"
        assert np.array_equal(i, ei), f"spare {spare}: ids differ, first bad queries {np.argwhere((i != ei).any(1))[:5].ravel()}"
        assert np.allclose(s, es, rtol=0, atol=TOL)
        outs.append((s, i))
    for s, i in outs[1:]:
        assert np.array_equal(i, outs[0][1]) and np.array_equal(s, outs[0][0])
    st = ix.stats()
    assert st["wide_launches"] == st["launches"] == len(spares)
    assert st["fallback_queries"] == 0
    ix.close()


def test_list_entries_at_the_shape_of_the_list_bound(gpu, monkeypatch):
    """70,001 x 256, 512 queries, wide, every CU (274 row tiles: one full round and 18 left over, split over 36
    workgroups): reports the list entries per query.  test_lists_do_not_get_longer (test_scan_wide_epilogue_gpu.py) holds the
    bound; this case only shows the figure."""
    from hiprag import HipFlatIndex
    n, d, nq = 70001, 256, 512
    x = ho.synthetic_vectors(n, d, seed=351)
    q = ho.synthetic_queries(1024, d, seed=352)[:nq]
    monkeypatch.setenv("HIPRAG_SCAN_WIDE", "1")
    ix = HipFlatIndex(d, ho.METRIC_IP)
    ix.add(x)
    ix.search(q, K)
    st = ix.stats()
    print(f"list entries per query {st['list_entries'] / st['queries']:.2f}")
    assert st["wide_launches"] == st["launches"] == 1 and st["fallback_queries"] == 0
    ix.close()
