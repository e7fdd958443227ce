"""
How many CUs a pipelined scan leaves to the finish of the launch before it (hipidx_pipe_spare_cus, DenseIndex::pipe_spare_cus):
48, or 32 where a full launch takes the wide scan and the larger grid saves it a round of row tiles.  The choice moves the
scan's partition and nothing else: results are the same arrays whatever the number of spare CUs, the library's own
pipeline (a search_device call of several launches) and ShardedFlatIndex both take the library's choice, and
hipidx_set_spare_cus keeps its meaning.
"""
import functools

import numpy as np
import pytest

from oracle import hybrid_oracle as ho

pytestmark = pytest.mark.gpu
TOL = 1e-4
K = 10


@functools.lru_cache(maxsize=None)
def _rows(n, d, seed):
    x = ho.synthetic_vectors(n, d, seed=seed)
    x.setflags(write=False)
    return x


def _planted(x, r, seed):
    """row r_j plus 5 % noise, renormalised: a fragment read from a buffer that had not landed, or a tile that a
    re-partitioned grid skipped, loses the planted row"""
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((len(r), x.shape[1]))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    q = x[r].astype(np.float64) + 0.05 * noise
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _expected_spare(n_rows, n_cu):
    """the rule, restated: both grids must have a row tile per workgroup (the wide scan's condition), and 32 must save a round"""
    nrt = (n_rows + 255) // 256
    g48, g32 = n_cu - 48, n_cu - 32
    if nrt < g32 or g48 < 32 or n_rows <= 64 * 256:
        return 48
    return 32 if -(-nrt // g32) < -(-nrt // g48) else 48


def test_results_do_not_depend_on_the_spare_cus(gpu, monkeypatch):
    """70,001 rows x 200, 512 planted queries (two columns), wide forced; spare = 0, both values the rule can choose, and 200
    (every workgroup walks four or five row tiles).  Planted rows in a workgroup's first tile, a later round, the last full
    tile and the partial last tile (row 70,000), at every (block, query tile) position of a wave.  Ids and scores are the
    same arrays across the four, ids are the oracle's, no planted row is lost."""
    from hiprag import HipFlatIndex
    n, d, nq = 70001, 200, 512
    x = _rows(n, d, 521)
    g = _n_cu() - 200
    assert 32 <= g and 4 * g <= (n + 255) // 256
    j = np.arange(nq)
    kind = (j // 8) % 4
    t = np.array([3, g + 7, n // 256 - 1, 0])[kind]
    r = np.where(kind == 3, n - 1, 32 * (8 * t + j % 8) + (7 * j) % 32)
    q = _planted(x, r, 522)
    es, ei = ho.flat_search(x, q, K, ho.METRIC_IP)
    assert np.array_equal(ei[:, 0], r), "the oracle itself does not find every planted row: the case is badly built"
    monkeypatch.setenv("HIPRAG_SCAN_WIDE", "1")
    ix = HipFlatIndex(d, ho.METRIC_IP)
    ix.add(x)
    outs = []
    for spare in (0, 32, 48, 200):
        ix.set_spare_cus(spare)
        assert ix.spare_cus == spare
        s, i = ix.search(q, K)
        assert np.array_equal(i[:, 0], r), f"spare {spare}: planted rows lost, first bad queries {np.argwhere(i[:, 0] != r)[:5].ravel()}"
        assert np.array_equal(i, ei), f"spare {spare}: ids differ, first bad queries {np.argwhere((i != ei).any(1))[:5].ravel()}"
        assert np.allclose(s, es, rtol=0, atol=TOL)
        outs.append((s, i))
    for s, i in outs[1:]:
        assert np.array_equal(i, outs[0][1]) and np.array_equal(s, outs[0][0])
    st = ix.stats()
    assert st["wide_launches"] == st["launches"] == 4 and st["fallback_queries"] == 0


def test_a_pipelined_search_leaves_the_spare_cus_alone(gpu):
    """70,001 x 200 with set_spare_cus(s): a search_device call of more queries than a launch takes runs the library's own
    pipeline on a smaller grid.  The caller's setting still reads s afterwards, the call's three outputs are the same bytes
    as those of the same call on a fresh index, and the ids of the first 64 queries are the oracle's."""
    import torch
    from hiprag import HipFlatIndex
    n, d, s = 70001, 200, 100
    x = _rows(n, d, 521)

    def run():
        ix = HipFlatIndex(d, ho.METRIC_IP)
        ix.add(x)
        ix.set_spare_cus(s)
        nq = ix.launch_queries + 76
        q = ho.synthetic_queries(nq, d, seed=541)
        out = [t.cpu().numpy() for t in ix.search_device(torch.from_numpy(q).cuda(), K)]
        return ix, q, out

    ix, q, a = run()
    assert ix.spare_cus == s
    st = ix.stats()
    assert st["launches"] == 2 and st["queries"] == len(q) and st["fallback_queries"] == 0
    _, _, b = run()
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    assert np.array_equal(a[2][:64], ho.flat_search(x, q[:64], K, ho.METRIC_IP)[1])
    # the pipeline's grid is no member of the index: a plain launch afterwards still runs on n_cu - s workgroups
    s2, i2 = ix.search(q[:64], K)
    assert np.array_equal(i2, a[2][:64]) and ix.spare_cus == s


@pytest.mark.parametrize("n", [20011,            # fewer row tiles than workgroups: narrow scan
                               416 * 256,        # 2 rounds on 208 workgroups and on 224
                               430 * 256 - 5])   # 3 rounds on 208, 2 on 224 (a partial last tile)
def test_the_choice_follows_the_rounds(gpu, n):
    """d = 64, launches of 1024 queries.  The library's choice is the rule's; asking for it sets nothing; ShardedFlatIndex
    takes it; a search_device call of two launches (the library's own pipeline) returns the oracle's ids and leaves the
    caller's setting as it was."""
    import torch
    from hiprag import HipFlatIndex
    from hiprag.sharded import ShardedFlatIndex
    d, nq = 64, 2048
    x = _rows(n, d, 531)
    ix = HipFlatIndex(d, ho.METRIC_IP)
    ix.add(x)
    assert ix.launch_queries == 1024
    want = _expected_spare(n, _n_cu())
    if _n_cu() == 256:
        assert want == {20011: 48, 416 * 256: 48, 430 * 256 - 5: 32}[n]
    assert ix.pipe_spare_cus == want
    assert ix.spare_cus == 0
    q = ho.synthetic_queries(nq, d, seed=532)
    es, ei = ho.flat_search(x, q, K, ho.METRIC_IP)
    s64, s32, ids = ix.search_device(torch.from_numpy(q).cuda(), K)
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy(), ei)
    assert np.allclose(s32.cpu().numpy(), es, rtol=0, atol=TOL)
    st = ix.stats()
    assert st["launches"] == 2 and st["fallback_queries"] == 0
    assert st["wide_launches"] == (2 if n > 64 * 256 and (n + 255) // 256 >= _n_cu() - want else 0)
    assert ix.spare_cus == 0
    sh = ShardedFlatIndex(ix, 0)
    assert ix.spare_cus == want
    _, _, sid = sh.search_device(torch.from_numpy(q[:1024]).cuda(), K)
    torch.cuda.synchronize()
    assert np.array_equal(sid.cpu().numpy(), ei[:1024])
