"""
Every vector path of the dense, scoped and IVF kernels at widths d off the 4-float and 128-float grids (oracle/width_cases.py;
tests/test_width_cases_cpu.py proves on the CPU that the data tell a kernel that drops, misplaces or over-reads a tail from a
right one).  Every comparison is against oracle.hybrid_oracle.flat_search (fp64) or a numpy restatement.

Bars: ids exact; fp32 scores within 1e-4 on unit-norm data; float64 scores within score_error_bound (the re-score sums
d_pad products in fp64: (d_pad + 16) * 2^-53 * sum |terms|, from the reference alone); the fp32 score is the float64 one
rounded.

Why the scan-shape cells may assert `fallback_queries == 0`: the planted data guarantee, on the scan's scale, a margin of at
least 4 x scan_eps_ref between the k-th and the (k + 1)-th exact score (checked on the CPU).  A correct scan value deviates
from the exact score by at most eps, so the best group the finish does NOT re-score has a scan value <= (k + 1)-th score +
eps, while the certificate needs k-th score > that value + eps: 2 x eps are necessary, the other 2 are slack for the quad
tag and the rounding of the bound.  A fallback on these data therefore means the scan mis-scored a row.
"""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho
from oracle import width_cases as wc

pytestmark = pytest.mark.gpu
TOL = 1e-4
K = 10
METRICS = (ho.METRIC_IP, ho.METRIC_L2)
E_UNSUPPORTED = -6   # include/hiprag.h


def mname(metric):
    return "ip" if metric == ho.METRIC_IP else "l2"


def check_device(ix, x, q, k, metric, tag, unit):
    """search_device against the fp64 oracle: ids, float64 scores within the bound, fp32 = rounded float64 (and within 1e-4
    of the oracle on unit-norm data).  Returns the worst float64 error over its bound."""
    import torch
    s64, s32, ids = [t.cpu().numpy() for t in ix.search_device(torch.from_numpy(q).cuda(), k)]
    es, ei, es64 = ho.flat_search(x, q, k, metric, return_f64=True)
    assert np.array_equal(ids, ei), (tag, "ids", np.argwhere((ids != ei).any(axis=1))[:4].ravel())
    ok = ei >= 0
    bound = wc.score_error_bound(x.shape[1], x, q, ei, metric)
    err = np.abs(s64 - es64)
    worst = float(np.max(np.where(ok, err / np.maximum(bound, 1e-300), 0.0))) if ok.any() else 0.0
    print("%s: worst |s64 - ref64| = %.3g (%.2f of its bound)" % (tag, float(err[ok].max()) if ok.any() else 0.0, worst))
    assert np.all(err[ok] <= bound[ok]), (tag, "float64 scores", worst)
    assert np.array_equal(s32[ok], s64[ok].astype(np.float32)), (tag, "fp32 scores are not the rounded float64 ones")
    if unit:
        assert np.allclose(s32[ok], es[ok], rtol=0, atol=TOL), (tag, "fp32 scores")
    return worst


def check_row_bounds(ix, x, tag):
    """row_bounds() == the numpy maxima rounded up.  The kernel sums a row's squares in fp64 in another order than numpy;
    the two sums differ by at most d * 2^-53 relative, so the float32 image is pinned to [lo, hi] of row_bounds_interval --
    one value, except where a row's sum sits within that distance of a float32."""
    got = ix.row_bounds()
    lo, hi = wc.row_bounds_interval(x)
    assert lo[0] <= got[0] <= hi[0] and lo[1] <= got[1] <= hi[1], (tag, got, lo, hi)


def sweep_data(d, scaled=False):
    return wc.tail_heavy(500, d, seed=d, scaled=scaled), wc.tail_heavy_queries(65, d, seed=d, scaled=scaled)


# ---- flat sweep --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", wc.MODES)
@pytest.mark.parametrize("d", wc.EDGE_WIDTHS)
def test_flat_sweep(gpu, monkeypatch, d, mode):
    """500 rows in two unequal adds, the second starting mid-block; nq = 1 (the scan stages its own tile) and 65 (qtile_kernel
    in bf16 mode, two passes); both metrics; then reconstruct and row_bounds."""
    from hiprag import HipFlatIndex
    monkeypatch.setenv("HIPRAG_SCAN_MODE", mode)
    for scaled in (False, True) if d in (3, 129, 513, 769, 1023) else (False,):
        x, q = sweep_data(d, scaled)
        for metric in METRICS:
            ix = HipFlatIndex(d, metric)
            ix.add(x[:173])
            ix.add(x[173:])
            for nq in (1, 65):
                check_device(ix, x, q[:nq], K, metric, "flat d=%d %s %s nq=%d%s" % (d, mode, mname(metric), nq,
                                                                                     " scaled" if scaled else ""), not scaled)
            for r in (0, 250, 499):
                assert np.array_equal(ix.reconstruct(r).view(np.uint32), x[r].view(np.uint32)), (d, r)
            check_row_bounds(ix, x, d)
            ix.close()


@pytest.mark.parametrize("d", [3, 129, 1023])
def test_save_load_round_trip(gpu, tmp_path, d):
    import torch
    from hiprag import HipFlatIndex
    x, q = sweep_data(d)
    for metric in METRICS:
        ix = HipFlatIndex(d, metric)
        ix.add(x[:173])
        ix.add(x[173:])
        check_device(ix, x, q, K, metric, "save/load d=%d %s before" % (d, mname(metric)), True)
        ix.save(str(tmp_path / "w.hipidx"))
        back = HipFlatIndex.load(str(tmp_path / "w.hipidx"))
        assert (back.ntotal, back.d, back.metric) == (500, d, metric)
        qd = torch.from_numpy(q).cuda()
        a = [t.cpu().numpy() for t in ix.search_device(qd, K)]
        b = [t.cpu().numpy() for t in back.search_device(qd, K)]
        for u, v in zip(a, b):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (d, metric)
        assert np.array_equal(back.reconstruct(499).view(np.uint32), x[499].view(np.uint32))
        assert back.row_bounds() == ix.row_bounds()


def test_save_and_reconstruct_a_ragged_last_block(gpu, tmp_path):
    """n = 33, d = 7: one full block and a block of one row, a width off the 4-float grid; save, load and reconstruct all
    read rows through the one untile path."""
    from hiprag import HipFlatIndex
    x = wc.tail_heavy(33, 7, seed=5)
    ix = HipFlatIndex(7, ho.METRIC_L2)
    ix.add(x)
    ix.save(str(tmp_path / "r.hipidx"))
    back = HipFlatIndex.load(str(tmp_path / "r.hipidx"))
    assert (back.ntotal, back.d) == (33, 7)
    for h in (ix, back):
        for r in (0, 31, 32):
            assert np.array_equal(h.reconstruct(r).view(np.uint32), x[r].view(np.uint32)), r


# ---- scan shapes -------------------------------------------------------------------------------------------------------
def _cells_of(d, metric):
    return [c for c in wc.scan_cells() if c.d == d and c.metric == metric]


@pytest.mark.parametrize("metric", METRICS, ids=mname)
@pytest.mark.parametrize("d", wc.SCAN_WIDTHS)
def test_scan_shapes_answer_on_the_fast_path(gpu, monkeypatch, d, metric):
    """The table's cells at the smallest n that selects them, on planted data (derivation of the margin: module docstring)."""
    import torch
    from hiprag import HipFlatIndex
    from hiprag.index import scan_plan
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cu > wc.SCAN_CUS
    for c in _cells_of(d, metric):
        monkeypatch.setenv("HIPRAG_SCAN_MODE", c.mode)
        p = wc.planted(c.n, d, wc.SCAN_K, metric)
        ix = HipFlatIndex(d, metric)
        ix.add(p.x)
        ix.set_spare_cus(n_cu - wc.SCAN_CUS)
        scan_cus = n_cu - ix.spare_cus
        assert wc.scan_label(d, c.n, c.nq, scan_cus, c.mode) == c.label, c.name
        # ... and the library's own dispatch, for the handle as it stands: the cell reaches the kernel shape it is named for
        shape = ix.scan_shape()
        assert (shape.nblocks, shape.P, shape.n_cu) == (wc.nblocks(c.n), wc.pieces(d), n_cu), c.name
        assert wc.plan_label(shape, scan_plan(shape, c.nq, wc.SCAN_K, scan_cus)) == c.label, c.name
        q = p.queries(c.nq)
        check_device(ix, p.x, q, wc.SCAN_K, metric, "scan %s %s" % (c.label, c.name), False)
        _, ids = ix.search(q, wc.SCAN_K)
        assert np.array_equal(ids, np.repeat(p.rows[None, :], c.nq, axis=0)), c.name
        st = ix.stats()
        assert st["queries"] == 2 * c.nq and st["fallback_queries"] == 0, (c.name, c.label, st)
        ix.close()


@pytest.mark.parametrize("d", [7, 129])
def test_scan_with_the_filter_on(gpu, monkeypatch, d):
    """More than kNoFilterGroups groups: the scan keeps its own bound and lists only what reaches it."""
    from hiprag import HipFlatIndex
    n = 16500
    assert wc.filter_on(wc.nblocks(n)) and not wc.filter_on(wc.nblocks(wc.SCAN_N_LARGE))
    for mode in wc.MODES:
        monkeypatch.setenv("HIPRAG_SCAN_MODE", mode)
        for metric in METRICS:
            p = wc.planted(n, d, wc.SCAN_K, metric)
            for mode_ in wc.MODES:
                gap, eps = wc.planted_margins(p, d, wc.SCAN_K, mode_)
                assert gap >= wc.MARGIN_FACTOR * eps
            ix = HipFlatIndex(d, metric)
            ix.add(p.x)
            check_device(ix, p.x, p.queries(65), wc.SCAN_K, metric, "filter d=%d %s %s" % (d, mode, mname(metric)), False)
            assert ix.stats()["fallback_queries"] == 0
            ix.close()


# ---- exhaustive and extension paths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", wc.MODES)
@pytest.mark.parametrize("d", [5, 131, 1023])
def test_exhaustive_and_extension_paths(gpu, monkeypatch, d, mode):
    """A zero query ties every row; 300 exact copies of one row, each in a group of its own, tie for the top 50 of the query
    that equals them: the certificate must refuse, and the extension or the exhaustive path answers -- exactly."""
    from hiprag import HipFlatIndex
    monkeypatch.setenv("HIPRAG_SCAN_MODE", mode)
    n = 9000
    x = wc.tail_heavy(n, d, seed=3)
    copies = 100 + 29 * np.arange(300)
    x[copies] = x[7]
    q = wc.tail_heavy_queries(4, d, seed=4)
    q[1] = x[7]
    q[2] = 0
    for metric in METRICS:
        ix = HipFlatIndex(d, metric)
        ix.add(x)
        for k in (10, 50):
            check_device(ix, x, q, k, metric, "exhaustive d=%d %s %s k=%d" % (d, mode, mname(metric), k), True)
        _, ids = ix.search(q, 50)
        assert list(ids[1]) == [7] + list(copies[:49])
        st = ix.stats()
        assert st["fallback_queries"] + st["roundb_queries"] >= 1, st
        ix.close()


# ---- scoped flat search ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [7, 130, 897, 1023])
def test_scoped_search(gpu, d):
    """Scopes that start and end mid-quad (rows 4j + 1 .. 4j' + 2), one of them inside one quad, one up to the last row."""
    from test_scoped_gpu import oracle_scoped
    from hiprag import HipFlatIndex
    n = 3000
    x = wc.tail_heavy(n, d, seed=21)
    scopes = [[(1, 2)], [(5, 7), (33, 34)], [(4 * 100 + 1, 4 * 300 + 2)], [(2, 4 * 8 + 3), (4 * 500 + 3, n)],
              [(4 * 700 + 1, 4 * 700 + 2), (4 * 720 + 2, 4 * 740 + 1)]]
    for metric in METRICS:
        ix = HipFlatIndex(d, metric)
        ix.add(x)
        for nq in (1, 17):
            q = wc.tail_heavy_queries(nq, d, seed=22)
            soq = (np.arange(nq, dtype=np.int32) * 3 + 2) % len(scopes)
            s, i = ix.search_scoped(q, K, scopes, soq)
            es, ei = oracle_scoped(x, q, K, metric, scopes, soq)
            assert np.array_equal(i, ei), (d, metric, nq)
            assert np.allclose(s, es, rtol=0, atol=TOL), (d, metric, nq)
        ix.close()


# ---- removal -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", wc.MODES)
@pytest.mark.parametrize("d", [7, 130, 1023])
def test_removal_matches_the_fresh_build(gpu, tmp_path, monkeypatch, d, mode):
    """The twin check of tests/test_remove_gpu.py (searches against the twin AND the oracle over the survivors, reconstruct
    against the input, row_bounds) on tail-heavy rows."""
    from test_remove_gpu import _remove_and_compare
    monkeypatch.setenv("HIPRAG_SCAN_MODE", mode)
    x = wc.tail_heavy(937, d, seed=31)
    for metric in ("ip", "l2"):
        _remove_and_compare(x, d, metric, [(29, 35), (250, 263), (509, 771)], tmp_path, "d=%d %s %s" % (d, metric, mode))
        survivors = np.delete(x, np.r_[29:35, 250:263, 509:771], axis=0)
        from hiprag import HipFlatIndex
        ix = HipFlatIndex(d, metric)
        ix.add(x)
        ix.remove_ranges([(29, 35), (250, 263), (509, 771)])
        check_row_bounds(ix, survivors, d)
        ix.close()


# ---- IVF ---------------------------------------------------------------------------------------------------------------
IVF_SHAPES = [(3000, 7, 5), (6000, 130, 16), (6000, 1023, 16), (4000, 897, 8)]
SHAPE_IDS = dict(ids=lambda s: "x".join(map(str, s)))


def ivf_rows(n, d):
    x = wc.tail_heavy(n, d, seed=41)
    x[40:60] = x[3]
    return x


@pytest.mark.parametrize("metric", METRICS, ids=mname)
@pytest.mark.parametrize("shape", IVF_SHAPES, **SHAPE_IDS)
def test_ivf_rounds_are_oracle_rounds_and_host_equals_device(gpu, metric, shape):
    """The loop of test_every_round_is_one_oracle_round (iters 0 .. 3: the initial centroids and three updates, each against
    the oracle's): ivf_gather_kernel, assignment, the sums of the update (ivf_chunk_sum_kernel, ivf_update_kernel), the final
    layout; then the device entry; then the training sample (the gather without an index table), as test_training_sample."""
    import torch
    from test_ivf_build_gpu import build, init_rows, list_of_rows, oracle_assign, oracle_update, train_rows
    n, d, nlist = shape
    x = ivf_rows(n, d)
    init = init_rows(n, nlist, 0)
    prev = None
    for t in range(4):
        ix = build(x, nlist, metric, t)
        c = ix.centroids()
        if t == 0:
            assert np.array_equal(c, x[init])
        else:
            assert np.allclose(c, prev, rtol=0, atol=1e-6), f"round {t}: centroids differ from the oracle's update"
        offs, orig = ix.lists()
        assign = oracle_assign(c, x, metric)
        assert np.array_equal(list_of_rows(offs, orig, n), assign), f"round {t}: lists differ from the exact assignment"
        prev = oracle_update(x, assign, c, metric)
    dev = build(torch.from_numpy(x).cuda(), nlist, metric, 3)
    assert np.array_equal(dev.centroids().view(np.uint32), ix.centroids().view(np.uint32))
    for u, v in zip(dev.lists(), ix.lists()):
        assert np.array_equal(u, v)
    m = 701
    xt = x[train_rows(n, m)]
    c0 = build(x, nlist, metric, 0, seed=3, max_train_rows=m).centroids()
    assert np.array_equal(c0.view(np.uint32), xt[init_rows(m, nlist, 3)].view(np.uint32))
    ix = build(x, nlist, metric, 1, seed=3, max_train_rows=m)
    assert np.allclose(ix.centroids(), oracle_update(xt, oracle_assign(c0, xt, metric), c0, metric), rtol=0, atol=1e-6)
    offs, orig = ix.lists()
    assert np.array_equal(np.sort(orig[orig >= 0]), np.arange(n))


@pytest.mark.parametrize("shape", IVF_SHAPES, **SHAPE_IDS)
def test_ivf_layout_file_and_searches(gpu, tmp_path, shape):
    """File contents as test_layout_and_file_contents; full probe == the flat oracle; search_batch == the one-query path bit
    for bit and == the CPU IVF restatement at nprobe = 3."""
    import torch
    from test_ivf_build_gpu import build, cpu_ivf_search, read_ivf_file
    n, d, nlist = shape
    x = ivf_rows(n, d)
    q = wc.tail_heavy_queries(65, d, seed=42)
    for metric in METRICS:
        ix = build(x, nlist, metric, 3)
        offs, orig = ix.lists()
        assert offs[0] == 0 and np.all(offs % 32 == 0) and offs[-1] == len(orig)
        assert np.array_equal(np.sort(orig[orig >= 0]), np.arange(n))
        ix.save(str(tmp_path / "a.ivf"))
        f = read_ivf_file(tmp_path / "a.ivf")
        assert (f["version"], f["d"], f["metric"], f["nlist"], f["n"], f["stored"]) == (1, d, metric, nlist, n, len(orig))
        assert np.array_equal(f["cents"], ix.centroids()) and np.array_equal(f["offs"], offs) and np.array_equal(f["orig"], orig)
        assert np.array_equal(f["rows"][orig >= 0].view(np.uint32), x[orig[orig >= 0]].view(np.uint32))
        assert not np.any(f["rows"][orig < 0])
        es, ei = ho.flat_search(x, q, K, metric)
        for fn in (ix.search, ix.search_batch):
            s, i = fn(q, K, nprobe=nlist)
            assert np.array_equal(i, ei) and np.allclose(s, es, rtol=0, atol=TOL), (shape, metric, fn.__name__)
        qd = torch.from_numpy(q).cuda()
        want = cpu_ivf_search(x, ix.centroids(), offs, orig, q, K, 3, metric)
        one = [t.cpu().numpy() for t in ix.search_device(qd, K, 3)]
        bat = [t.cpu().numpy() for t in ix.search_batch_device(qd, K, 3)]
        assert np.array_equal(one[2], want) and np.array_equal(bat[2], want), (shape, metric)
        for u, v in zip(one, bat):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (shape, metric)


@pytest.mark.parametrize("metric", METRICS, ids=mname)
@pytest.mark.parametrize("d", [7, 130, 897, 1023])
def test_ivf_add_and_remove_against_the_model(gpu, tmp_path, metric, d):
    """One short script of tests/test_ivf_update_gpu.py's steps against IvfModel: state and file bytes after every step,
    then the full probe against the flat oracle."""
    from test_ivf_update_cpu import separated_centroids
    from test_ivf_update_gpu import NLIST, check_state, edge_script, fresh
    cents = separated_centroids(NLIST, d, seed=9)
    ix, m = fresh(cents, metric)
    script = edge_script(cents, seed=41)
    for name, step in [script[j] for j in (0, 1, 2, 3, 4, 8, 9, 10, 11, 15)]:
        info, batch_bytes = step(ix, m)
        m.check()
        check_state(ix, m, tmp_path / "s.ivf", "d=%d %s" % (d, name), info, batch_bytes)
    q = np.concatenate([m.x[::37], wc.tail_heavy_queries(5, d, seed=43)])
    es, ei = ho.flat_search(m.x, q, K, metric)
    for fn in (ix.search, ix.search_batch):
        s, i = fn(q, K, nprobe=NLIST)
        assert np.array_equal(i, ei) and np.allclose(s, es, rtol=0, atol=TOL), (d, metric, fn.__name__)


def _scoped_reference(x, q, k, metric, cand_rows):
    """the exact top k of every query among ITS candidate rows: ids and float64 scores (0 where the id is -1)"""
    ids = np.full((len(q), k), -1, dtype=np.int64)
    s64 = np.zeros((len(q), k), dtype=np.float64)
    for j, rows in enumerate(cand_rows):
        if len(rows):
            _, local, sc = ho.flat_search(x[rows], q[j:j + 1], k, metric, return_f64=True)
            ids[j] = np.where(local[0] >= 0, rows[np.maximum(local[0], 0)], -1)
            s64[j] = sc[0]
    return ids, s64


@pytest.mark.parametrize("metric", METRICS, ids=mname)
@pytest.mark.parametrize("shape", IVF_SHAPES, **SHAPE_IDS)
def test_ivf_search_scoped(gpu, metric, shape):
    """search_scoped in both probe modes against numpy: probe-any is cpu_ivf_scoped of tests/test_ivf_scoped_gpu.py (the top
    nprobe lists whatever the scope, then the in-scope rows); scope-aware probing is the restatement of
    tests/test_ivf_scope_probe_gpu.py (the first min(nprobe, members) MEMBER lists of the coarse order, then their in-scope
    rows), here with the top k from the fp64 oracle too.  Scopes start and end mid-quad; one is a single row, one is empty."""
    import torch
    from test_ivf_build_gpu import build
    from test_ivf_scoped_gpu import cpu_ivf_scoped
    from test_ivf_scope_probe_gpu import members_of
    n, d, nlist = shape
    x = ivf_rows(n, d)
    ix = build(x, nlist, metric, 3)
    cents = ix.centroids()
    offs, orig = ix.lists()
    scopes = [[(1, 2)], [(5, 7), (4 * 100 + 1, 4 * 300 + 2)], [(2, 4 * 8 + 3), (n - 4 * 200 + 3, n)], [],
              [(4 * 350 + 1, 4 * 350 + 2), (4 * 360 + 2, 4 * 420 + 1)], [(0, n)]]
    msets = [set(members_of(offs, orig, s)) for s in scopes]
    for nq in (1, 17):
        q = wc.tail_heavy_queries(nq, d, seed=44)
        soq = ((np.arange(nq, dtype=np.int32) * 5 + 1) % len(scopes)).astype(np.int32)
        qd = torch.from_numpy(q).cuda()
        order = ho.flat_search(cents, q, nlist, metric)[1]
        for nprobe in (1, 3, nlist):
            tag = "ivf scoped %s %s nq=%d nprobe=%d" % ("x".join(map(str, shape)), mname(metric), nq, nprobe)
            want_any = cpu_ivf_scoped(x, cents, offs, orig, q, K, nprobe, metric, scopes, soq)
            cand = []
            for j in range(nq):
                probes = [int(l) for l in order[j] if int(l) in msets[soq[j]]][:nprobe]
                seg = np.concatenate([orig[offs[l]:offs[l + 1]] for l in probes] + [np.zeros(0, np.int64)])
                keep = np.zeros(len(seg), dtype=bool)
                for lo, hi in scopes[soq[j]]:
                    keep |= (seg >= lo) & (seg < hi)
                cand.append(np.sort(seg[keep]))
            want_scope = _scoped_reference(x, q, K, metric, cand)
            for probe, (e_ids, e_s64) in (("any", want_any), ("scope", want_scope)):
                s64, s32, ids = [t.cpu().numpy() for t in ix.search_scoped_device(qd, K, scopes, soq, nprobe=nprobe, probe=probe)]
                assert np.array_equal(ids, e_ids), (tag, probe)
                ok = e_ids >= 0
                bound = wc.score_error_bound(d, x, q, e_ids, metric)
                err = np.abs(s64 - e_s64)
                if ok.any():
                    print("%s %s: worst |s64 - ref64| = %.3g (%.2f of its bound)"
                          % (tag, probe, float(err[ok].max()), float((err[ok] / np.maximum(bound[ok], 1e-300)).max())))
                assert np.all(err[ok] <= bound[ok]), (tag, probe)
                assert np.array_equal(s32[ok], s64[ok].astype(np.float32)), (tag, probe)
                assert np.allclose(s32[ok], e_s64[ok], rtol=0, atol=TOL), (tag, probe)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_width_1025_is_refused_as_unsupported(gpu):
    """Every entry that creates an index answers d = 1025 with HIPRAG_E_UNSUPPORTED and leaves no handle behind.  (That the
    refusal precedes every launch is read off the source -- create_dense and hipivf_build return before their first HIP call
    -- not something a test can observe: there is no index whose counters could be read.)"""
    import torch
    from hiprag import HipFlatIndex, HipIVFIndex, HipRagError
    x = np.zeros((64, 1025), dtype=np.float32)

    def refused(fn):
        with pytest.raises(HipRagError) as e:
            fn()
        assert e.value.code == E_UNSUPPORTED, e.value

    refused(lambda: HipFlatIndex(1025, "ip"))
    refused(lambda: HipIVFIndex(1025, 4, "l2").build(x, iters=1))
    refused(lambda: HipIVFIndex(1025, 4, "l2").build(torch.from_numpy(x).cuda(), iters=1))
    refused(lambda: HipIVFIndex.from_centroids(x[:4], "ip"))
    torch.cuda.synchronize()                                   # the device is as usable as before
    ix = HipFlatIndex(1024, "ip")                              # ... and the limit itself is accepted
    ix.add(wc.tail_heavy(64, 1024, seed=1))
    assert ix.ntotal == 64
