"""
The fold schedule of the wide scan kernel (csrc/scan_wide.h, wide_fold of csrc/dense_plan.h): behind the first pairs of
its walk a wave recomputes the bound of its unit only in one tile out of HIPRAG_WIDE_FOLD_EVERY and otherwise tests a
tile against what thetac holds.  A tile tested against a wrong bound only shows if it held a top-k row, so the queries are
PLANTED as in test_scan_wide_epilogue_gpu.py: query j is row r_j plus 5 % noise, renormalised, and ids[:, 0] must be r.
Every case: ids bit-exact against the CPU oracle, scores within 1e-4, every launch a wide one, nobody on the exhaustive
path.  200 spare CUs leave 56 workgroups, so a workgroup walks nine or ten (row tile, column) pairs of the 274 row tiles
and two columns, and the pairs behind the first kWideFoldFirst are no-fold tiles for most waves.
"""
import functools

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu
TOL = 1e-4
K = 10
SPARE = 200


@functools.lru_cache(maxsize=None)
def _rows(n, d, seed):
    x = ho.synthetic_vectors(n, d, seed=seed)
    x.setflags(write=False)
    return x


def _planted(x, r, seed):
    """row r_j plus 5 % noise, renormalised (the construction of test_scan_wide_epilogue_gpu.py)"""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((len(r), x.shape[1]))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    q = x[r].astype(np.float64) + 0.05 * noise
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _grid():
    import torch
    g = torch.cuda.get_device_properties(0).multi_processor_count - SPARE      # scan workgroups
    assert g >= 32
    return g


@functools.lru_cache(maxsize=None)
def _case(n, d, nq, metric, g):
    """rows, planted queries, their rows and the oracle's answer, once per shape.  Planted rows: a workgroup's first tile
    (pair 0 or 1 of its walk), tiles of its third and fourth round (pairs 4..7: beyond kWideFoldFirst), the last full row
    tile and the partial last one (the index's last row) -- both in the tail, the last pairs of a walk."""
    from hiprag.index import wide_fold_constants
    nrt = (n + 255) // 256
    assert 2 * 2 >= wide_fold_constants()[0] and 4 * g <= nrt, "rounds three and four must lie beyond the first pairs, and exist"
    x = _rows(n, d, 521)
    j = np.arange(nq)
    kind = (j // 8) % 5
    t = np.array([3, 2 * g + 7, 3 * g + 5, n // 256 - 1, 0])[kind]
    r = np.where(kind == 4, n - 1, 32 * (8 * t + j % 8) + (7 * j) % 32)
    q = _planted(x, r, 522 + nq)
    q.setflags(write=False)
    es, ei = ho.flat_search(x, q, K, metric)
    return x, q, r, es, ei


def _index(monkeypatch, x, metric, every, spare=SPARE):
    from hiprag import HipFlatIndex
    monkeypatch.setenv("HIPRAG_SCAN_WIDE", "1")
    monkeypatch.setenv("HIPRAG_WIDE_FOLD_EVERY", str(every))
    ix = HipFlatIndex(x.shape[1], metric)
    ix.add(x)
    ix.set_spare_cus(spare)
    return ix


def _check(ix, case):
    x, q, r, es, ei = case
    s, i = ix.search(q, K)
    assert np.array_equal(i[:, 0], r), f"planted rows lost: first bad queries {np.argwhere(i[:, 0] != r)[:5].ravel()}"
    assert np.array_equal(i, ei), f"ids differ: first bad queries {np.argwhere((i != ei).any(1))[:5].ravel()}"
    assert np.allclose(s, es, rtol=0, atol=TOL)
    st = ix.stats()
    assert st["wide_launches"] == st["launches"] == 1
    assert st["fallback_queries"] == 0
    return st


def _expected_folds(n, nq, g, every):
    """the sum of hiprag_wide_fold over every wave's walk: the tiles a wave parks (its unit has a query, its row half a
    block) and folds"""
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


@pytest.mark.parametrize("every", [1, 4, 64])
@pytest.mark.parametrize("d,metric", [(512, ho.METRIC_IP), (200, ho.METRIC_IP), (512, ho.METRIC_L2)])
def test_phases_in_the_loop_and_in_the_drain(gpu, monkeypatch, d, metric, every):
    """70,001 rows, 512 queries.  d = 512: 16 k-steps per tile, so a no-fold tile waits for k-step 8 of the next tile and
    runs T and A inside the loop; d = 200: 8 k-steps, T and A of every tile run in the drain, with or without B0..B3 ahead
    of them in the loop."""
    case = _case(70001, d, 512, metric, _grid())
    _check(_index(monkeypatch, case[0], metric, every), case)


def test_short_second_column(gpu, monkeypatch):
    """300 queries: the second column has one live unit, the waves of the others carry a pending tile -- a no-fold one
    for most of them -- through a tile they do not compute."""
    x, q, r, es, ei = _case(70001, 512, 512, ho.METRIC_IP, _grid())   # the first 300 queries of the shared case
    _check(_index(monkeypatch, x, ho.METRIC_IP, 4), (x, q[:300], r[:300], es[:300], ei[:300]))


def test_same_outputs_as_folding_in_every_tile(gpu, monkeypatch):
    """search_device returns the same bits whether every tile folds or one in four: the schedule only changes which
    candidates beyond the answer are listed."""
    import torch
    x, q, r, es, ei = _case(70001, 512, 512, ho.METRIC_IP, _grid())
    qd = torch.from_numpy(q.copy()).cuda()
    outs = []
    for every in (1, 4):
        ix = _index(monkeypatch, x, ho.METRIC_IP, every)
        s64, s32, ids = ix.search_device(qd, K)
        torch.cuda.synchronize()
        st = ix.stats()
        assert st["wide_launches"] == st["launches"] == 1 and st["fallback_queries"] == 0
        outs.append((s64.clone(), s32.clone(), ids.clone()))
        ix.close()
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert np.array_equal(outs[1][2].cpu().numpy(), ei)


@pytest.mark.parametrize("every", [1, 4])
def test_the_counter_counts_fold_tiles(gpu, monkeypatch, every):
    """70,144 rows = 274 full row tiles, 512 queries: every wave parks every tile of its walk.  wide_theta_folds counts the
    tiles a wave parked as fold tiles -- exactly the schedule's, whatever a bounded wait of phase T recomputed on the way
    (wide_theta_fresh is not a fold tile)."""
    n, nq, g = 70144, 512, _grid()
    case = _case(n, 512, nq, ho.METRIC_IP, g)
    ix = _index(monkeypatch, case[0], ho.METRIC_IP, every)
    assert ix.stats()["wide_theta_folds"] == 0
    st = _check(ix, case)
    want, pairs = _expected_folds(n, nq, g, every)
    assert pairs == 274 * 2
    if every == 1:
        assert want == 8 * pairs
    else:
        assert want < 8 * pairs
    assert st["wide_theta_folds"] == want


@pytest.mark.parametrize("value", ["0", "3", "128", "-4", "4x", ""])
def test_a_bad_setting_is_an_error(gpu, monkeypatch, value):
    from hiprag import HipFlatIndex
    from hiprag._native import HipRagError
    monkeypatch.setenv("HIPRAG_WIDE_FOLD_EVERY", value)
    with pytest.raises(HipRagError):
        HipFlatIndex(64, ho.METRIC_IP)
