"""
The tile loop of the wide scan kernel (csrc/scan_wide.h): a tile's first and last k-step are written out (the first takes
a zero C operand, the last parks the tile), phases run in the even steps, and what a step needs at its head -- the
staging streams, the ring slots, the fragment addresses, the walk's next pair -- is computed one step ahead, behind the
staging of the step before it, by live and dead waves alike.  A step that staged from a stale cursor, computed from the wrong slot or started
a tile on the accumulators of the one before it only shows if the tile held a top-k row, so the queries are PLANTED as in
test_scan_wide_fold_gpu.py: query j is row r_j plus 5 % noise, renormalised, and ids[:, 0] must be r.  Planted rows lie in
a workgroup's first tile, in the tile entered right behind a column change (the same row tile, the queries of the next
column: both columns ask for every planted tile), in a tile entered right behind a row-tile change, in the last full row
tile and at the index's last row (the partial last tile, which has only its first row half).
Every case: ids bit-exact against the CPU oracle, scores within 1e-4, every launch a wide one, nobody on the exhaustive
path (a tile tested wrongly but rescued there must not pass), and search_device's three outputs equal to those of the
narrow kernels (HIPRAG_SCAN_WIDE=0) over the same data.
"""
import functools

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu
TOL = 1e-4
K = 10
N = 70001          # 274 row tiles, the last one partial: 113 rows, its second row half does not exist


def _grid(spare):
    import torch
    g = torch.cuda.get_device_properties(0).multi_processor_count - spare      # scan workgroups
    assert g >= 32
    return g


@functools.lru_cache(maxsize=None)
def _rows(n, d):
    x = ho.synthetic_vectors(n, d, seed=731 + d)
    x.setflags(write=False)
    return x


def _planted(x, r, seed):
    """row r_j plus 5 % noise, renormalised (the construction of test_scan_wide_fold_gpu.py)"""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((len(r), x.shape[1]))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    q = x[r].astype(np.float64) + 0.05 * noise
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(n, d, nq, metric, g):
    """rows, planted queries, their rows and the oracle's answer, once per shape; a launch of fewer queries takes the first.
    Groups of 8 queries go round five kinds of row tile, in every column: tile 3 (pair 0 of workgroup 3's walk in column 0,
    its pair 1 -- right behind the column change -- in column 1), tiles g + 7 and 3 g + 5 (entered behind a row-tile
    change; taken modulo the full row tiles on a small index), the last full row tile, and the index's last row."""
    nrt, full = (n + 255) // 256, n // 256
    x = _rows(n, d)
    j = np.arange(nq)
    kind = (j // 8) % 5
    t = np.array([3, (g + 7) % full, (3 * g + 5) % full, full - 1, 0])[kind]
    r = np.where(kind == 4, n - 1, 32 * (8 * t + j % 8) + (7 * j) % 32)
    assert nrt == full + 1 and r.max() == n - 1
    q = _planted(x, r, 900 + nq + d)
    q.setflags(write=False)
    es, ei = ho.flat_search(x, q, K, metric)
    assert np.array_equal(ei[:, 0], r), "the oracle itself does not find every planted row: the case is badly built"
    return x, q, r, es, ei


def _index(monkeypatch, x, metric, spare, wide="1", every=None):
    from hiprag import HipFlatIndex
    monkeypatch.setenv("HIPRAG_SCAN_WIDE", wide)
    if every is None:
        monkeypatch.delenv("HIPRAG_WIDE_FOLD_EVERY", raising=False)
    else:
        monkeypatch.setenv("HIPRAG_WIDE_FOLD_EVERY", str(every))
    ix = HipFlatIndex(x.shape[1], metric)
    ix.add(x)
    ix.set_spare_cus(spare)
    return ix


def _check(monkeypatch, case, metric, spare, nq=None, every=None):
    """the four assertions of every case (the module's docstring); returns the wide index's statistics"""
    import torch
    x, q, r, es, ei = case
    if nq is not None:
        q, r, es, ei = q[:nq], r[:nq], es[:nq], ei[:nq]
    ix = _index(monkeypatch, x, metric, spare, every=every)
    s, i = ix.search(q, K)
    assert np.array_equal(i[:, 0], r), f"planted rows lost: first bad queries {np.argwhere(i[:, 0] != r)[:5].ravel()}"
    assert np.array_equal(i, ei), f"ids differ: first bad queries {np.argwhere((i != ei).any(1))[:5].ravel()}"
    assert np.allclose(s, es, rtol=0, atol=TOL)
    qd = torch.from_numpy(q.copy()).cuda()
    wide = [t.clone() for t in ix.search_device(qd, K)]
    torch.cuda.synchronize()
    st = ix.stats()
    assert st["wide_launches"] == st["launches"] == 2
    assert st["fallback_queries"] == 0
    ix.close()
    nx = _index(monkeypatch, x, metric, spare, wide="0", every=every)
    narrow = [t.clone() for t in nx.search_device(qd, K)]
    torch.cuda.synchronize()
    assert nx.stats()["wide_launches"] == 0
    nx.close()
    assert len(wide) == len(narrow) == 3 and all(torch.equal(a, b) for a, b in zip(wide, narrow)), \
        "search_device differs between the wide and the narrow kernels"
    return st


@pytest.mark.parametrize("d,metric", [(100, ho.METRIC_IP), (200, ho.METRIC_IP), (384, ho.METRIC_IP), (512, ho.METRIC_IP),
                                      (1024, ho.METRIC_IP), (100, ho.METRIC_L2), (512, ho.METRIC_L2)])
def test_every_tile_length(gpu, monkeypatch, d, metric):
    """KS = 4, 8, 12, 16, 32 k-steps per tile.  4: the first and the last step are two apart and every phase runs in the
    drain; 12: the phases fit exactly; 200 spare CUs: the tail pairs of a walk change row tile from pair to pair."""
    assert (d + 127) // 128 * 4 in (4, 8, 12, 16, 32)
    _check(monkeypatch, _case(N, d, 512, metric, _grid(200)), metric, 200)


@pytest.mark.parametrize("every", [1, 8])
@pytest.mark.parametrize("d", [200, 512])
def test_fold_schedules(gpu, monkeypatch, d, every):
    _check(monkeypatch, _case(N, d, 512, ho.METRIC_IP, _grid(200)), ho.METRIC_IP, 200, every=every)


@pytest.mark.parametrize("nq", [300, 65])
def test_dead_units_keep_the_books(gpu, monkeypatch, nq):
    """300 queries: the second column has one live unit; 65: the only column has two.  The waves of the other units run no
    MFMA and must stage, advance and count exactly as the live ones do."""
    _check(monkeypatch, _case(N, 200, 512, ho.METRIC_IP, _grid(200)), ho.METRIC_IP, 200, nq=nq)


def test_four_columns(gpu, monkeypatch):
    _check(monkeypatch, _case(N, 100, 1024, ho.METRIC_IP, _grid(200)), ho.METRIC_IP, 200)


@pytest.mark.parametrize("spare", [32, 200])
def test_fewer_row_tiles_than_workgroups(gpu, monkeypatch, spare):
    """20,011 rows are 79 row tiles.  32 spare CUs: a walk is the two pairs of one row tile and most workgroups own nothing;
    200: one full round and a tail of 23 row tiles."""
    g = _grid(spare)
    assert (79 < g) == (spare == 32)
    _check(monkeypatch, _case(20011, 200, 512, ho.METRIC_IP, g), ho.METRIC_IP, spare)


def _expected_folds(n, nq, g, every):
    """the sum of hiprag_wide_fold over every wave's walk: the tiles a wave parks (its unit has a query, its row half a
    block) and folds -- the closed form of test_scan_wide_fold_gpu.py's test_the_counter_counts_fold_tiles"""
    from hiprag.index import wide_fold, wide_walk
    nrt, ncol, nunits, nblocks = (n + 255) // 256, (nq + 255) // 256, (nq + 63) // 64, (n + 31) // 32
    total = pairs = 0
    for wg in range(g):
        rts, cols = wide_walk(nrt, ncol, g, wg)
        pairs += len(rts)
        for wave in range(8):
            parked = (4 * cols + wave // 2 < nunits) & (8 * rts + 4 * (wave % 2) < nblocks)
            total += int((parked & wide_fold(0, len(rts), wg, wave, every)).sum())
    return total, pairs


def test_the_counter(gpu, monkeypatch):
    """70,144 rows = 274 full row tiles, 512 queries, one fold tile in four behind the first pairs: wide_theta_folds is the
    schedule's sum over the tiles the waves parked, once per launch (two launches: search and search_device)."""
    n, nq, g, every = 70144, 512, _grid(200), 4
    nrt = n // 256
    x = _rows(n, 512)
    j = np.arange(nq)
    r = 32 * (8 * np.array([3, g + 7, 3 * g + 5, nrt - 1, nrt - 2])[(j // 8) % 5] + j % 8) + (7 * j) % 32
    q = _planted(x, r, 977)
    es, ei = ho.flat_search(x, q, K, ho.METRIC_IP)
    st = _check(monkeypatch, (x, q, r, es, ei), ho.METRIC_IP, 200, every=every)
    want, pairs = _expected_folds(n, nq, g, every)
    assert pairs == 274 * 2 and want < 8 * pairs
    assert st["wide_theta_folds"] == 2 * want
