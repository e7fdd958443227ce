"""
The width cases (oracle/width_cases.py) judged on the CPU: the case table reaches every kernel shape the restated dispatch
rules can select, the tail-heavy data tell numpy models of subtly wrong kernels (MUTANTS) from the right one, and the
planted data carry the margin that lets a GPU test assert that the scan's fast path answered.  No GPU, no library.
"""
import numpy as np
import pytest

from oracle import hybrid_oracle as ho
from oracle import width_cases as wc

N, NQ, K = 500, 20, 10            # the flat sweep's index and depth; 20 queries for the shares
MIN_SHARE = 0.2                   # the bar: a mutant changes the ids of at least one query in five
METRICS = (ho.METRIC_IP, ho.METRIC_L2)


# ---- the rules, against hand-worked values from the source ------------------------------------------------------------
def test_restated_rules_on_hand_worked_values():
    assert [wc.pieces(d) for d in (1, 128, 129, 512, 513, 640, 641, 768, 769, 896, 897, 1024)] == \
        [16, 16, 32, 64, 80, 80, 96, 96, 112, 112, 128, 128]
    # ring: 16 where it divides P / 2 -- P / 2 = 8, 24, 40, 56 (P = 16, 48, 80, 112) run 8
    assert [wc.ring(d) for d in (7, 129, 257, 385, 513, 641, 769, 897)] == [8, 16, 8, 16, 8, 16, 8, 16]
    assert all(wc.ring(d, "q64") == 16 for d in wc.EDGE_WIDTHS)
    # waves: 4 only for bf16, P % 32 == 0 and fewer than 72 blocks per workgroup
    assert wc.scan_waves(1023, 287, 4, "bf16") == 4 and wc.scan_waves(1023, 288, 4, "bf16") == 8
    assert wc.scan_waves(1023, 18431, 256, "bf16") == 4 and wc.scan_waves(1023, 18432, 256, "bf16") == 8
    assert wc.scan_waves(257, 1, 256, "bf16") == 8 and wc.scan_waves(1023, 1, 256, "q64") == 8
    assert not wc.filter_on(512) and wc.filter_on(513)
    assert [wc.vec_paths(d) for d in (3, 4, 8, 12, 130, 1023, 1024)] == \
        ["scalar", "vec+tail8", "vec", "vec+tail8", "scalar", "scalar", "vec"]
    assert wc.d_pad(1) == 128 and wc.d_pad(1023) == 1024


def test_edge_widths_hold_the_issue_list_and_both_sides_of_every_predicate():
    must = {1, 2, 3, 4, 5, 7, 8, 9, 15, 17, 31, 33, 63, 65, 127, 129, 130, 131, 255, 257, 383, 385, 513, 639, 640, 641, 769,
            895, 896, 897, 1001, 1022, 1023, 128, 1024}
    assert must <= set(wc.EDGE_WIDTHS) and max(wc.EDGE_WIDTHS) <= wc.MAX_D
    assert {wc.pieces(d) for d in wc.EDGE_WIDTHS} == set(range(16, 129, 16))          # every P in 16 .. 128
    assert {wc.vec_paths(d) for d in wc.EDGE_WIDTHS} == {"scalar", "vec+tail8", "vec"}
    assert any(d < 4 for d in wc.EDGE_WIDTHS)                                          # vec_ok needs d >= 4 as well
    for m in wc.MUTANTS:                                                               # every mutant bites somewhere, and
        assert any(m.applies(d) for d in wc.EDGE_WIDTHS), m.name                       # none everywhere: controls exist
        assert not all(m.applies(d) for d in wc.EDGE_WIDTHS), m.name
    # rescore4 / rescore_load8: a lane owns P / 8 pieces; 10 (P = 80) and 14 (P = 112) are the splits past the first batch
    # of 8 that do not fill the second
    assert {wc.pieces(d) // 8 for d in wc.EDGE_WIDTHS} >= {10, 14}


def test_scan_cells_reach_every_selectable_kernel_shape():
    cells = wc.scan_cells()
    for c in cells:                                  # each label against the restated rule
        assert wc.scan_label(c.d, c.n, c.nq, wc.SCAN_CUS, c.mode) == c.label, c.name
        assert not wc.filter_on(wc.nblocks(c.n))     # (the filter has a case of its own in the GPU file)
        assert c.n % 32 != 0                         # a ragged last block
    got = {(c.mode, wc.ring(c.d, c.mode), wc.scan_waves(c.d, wc.nblocks(c.n), wc.SCAN_CUS, c.mode), wc.passes(c.nq), c.metric)
           for c in cells}
    want = set()
    for ps in ("one", "multi"):
        for metric in METRICS:
            want |= {("bf16", 16, 4, ps, metric), ("bf16", 16, 8, ps, metric), ("bf16", 8, 8, ps, metric),
                     ("q64", 16, 8, ps, metric)}     # ring 8 x 4 waves and q64 x anything else do not exist
    assert got == want
    assert {wc.pieces(c.d) for c in cells} == {16, 32, 48, 64, 80, 96, 112, 128}
    assert {wc.pieces(c.d) for c in cells if wc.ring(c.d) == 8} == {16, 48, 80, 112}
    assert {1023, 897, 641, 385, 257, 129, 7} <= {c.d for c in cells}
    assert all(c.d % 4 for c in cells)


def test_bf16_rounding_is_round_to_nearest_even():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415927, 0.0, 1e-40],
                 dtype=np.float32)
    r = wc.bf16_round(a)
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == np.float32(1.0 + 2.0 ** -6) and r[3] == np.float32(1.0 + 2.0 ** -7)
    assert abs(r[4] - a[4]) <= 2.0 ** -8 * abs(a[4]) and r[5] == 0.0
    assert np.all(wc.bf16_round(r) == r)


# ---- the data ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True])
def test_tail_heavy_has_the_designed_structure(scaled):
    for d in wc.EDGE_WIDTHS:
        x = wc.tail_heavy(N, d, seed=d, scaled=scaled).astype(np.float64)
        q = wc.tail_heavy_queries(NQ, d, seed=d, scaled=scaled).astype(np.float64)
        live = np.ones(N, dtype=bool)
        live[N // 3] = False
        assert not x[N // 3].any()
        for r in (N // 2, N // 2 + 1, N // 2 + 2, N - 2):
            assert np.array_equal(x[r], x[1])
        n2 = (x ** 2).sum(axis=1)
        if not scaled:
            assert np.allclose(n2[live], 1.0, atol=1e-5)
        else:
            assert n2[live].max() / n2[live].min() > 100.0
        tb = wc.tail_bounds(d)
        for a in (x[live], q):                         # every tail segment holds a real, row-dependent share of the norm
            for lo, hi in zip(tb[:-1], tb[1:]):
                if hi > lo and (lo, hi) != (0, d):          # (one segment that is the whole vector: share 1)
                    sh = (a[:, lo:hi] ** 2).sum(axis=1) / (a ** 2).sum(axis=1)
                    assert sh.min() > 0.04 and sh.max() - sh.min() > 0.1, (d, lo, hi, sh.min(), sh.max())
        # a row's successor starts with the opposite sign in every one of the first 16 columns, at a size that matters
        hd = min(16, d)
        copies = {N // 2, N // 2 + 1, N // 2 + 2, N - 2, N // 3}
        rows = np.array([r for r in range(N - 1) if r not in copies and r + 1 not in copies])
        assert np.all(x[rows, :hd] * x[rows + 1, :hd] < 0)
        if d >= 32:
            assert (np.abs(x[rows + 1, :hd]).sum(axis=1) / np.sqrt(n2[rows + 1])).min() > 0.5


def _shares(d, scaled, metric):
    x = wc.tail_heavy(N, d, seed=d, scaled=scaled)
    q = wc.tail_heavy_queries(NQ, d, seed=d, scaled=scaled)
    out = {}
    for m in wc.MUTANTS:
        if m.applies(d):
            right, wrong = wc.mutant_search(m, x, q, K, metric)
            out[m.name] = float((right != wrong).any(axis=1).mean())
    return out, x


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("metric", METRICS)
def test_every_mutant_changes_the_ids(metric, scaled):
    """The bar is one query in five; the data are chosen to clear it by a factor, and the shares are printed."""
    worst = {}
    for d in wc.EDGE_WIDTHS:
        shares, _ = _shares(d, scaled, metric)
        for name, s in shares.items():
            if s < worst.get(name, (2.0, 0))[0]:
                worst[name] = (s, d)
            assert s >= MIN_SHARE, (name, d, s)
    tag = "%s %s" % ("ip" if metric == ho.METRIC_IP else "l2", "scaled" if scaled else "unit")
    for name, (s, d) in sorted(worst.items()):
        print("mutant share [%s] %-28s worst %.2f at d=%d" % (tag, name, s, d))
    assert set(worst) == {m.name for m in wc.MUTANTS}
    assert min(s for s, _ in worst.values()) >= 2 * MIN_SHARE           # "by a clear factor"


@pytest.mark.parametrize("scaled", [False, True])
def test_every_row_mutant_moves_the_one_list_centroid(scaled):
    for d in wc.EDGE_WIDTHS:
        x = wc.tail_heavy(N, d, seed=d, scaled=scaled)
        q = wc.tail_heavy_queries(1, d, seed=d, scaled=scaled)
        want = wc.centroid_update(x)
        for m in wc.MUTANTS:
            if m.applies(d) and m.rows_only:
                xm = m.apply(x, q, ho.METRIC_IP)[0]
                assert not np.allclose(wc.centroid_update(xm), want, atol=1e-6), (m.name, d)


def test_controls_are_untouched_by_mutants_that_do_not_apply():
    for d in (128, 1024, 8):
        x = wc.tail_heavy(64, d, seed=d)
        q = wc.tail_heavy_queries(3, d, seed=d)
        for m in wc.MUTANTS:
            if not m.applies(d):
                right, wrong = wc.mutant_search(m, x, q, K, ho.METRIC_L2)
                assert np.array_equal(right, wrong), (m.name, d)


# ---- planted -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", wc.SCAN_WIDTHS)
def test_planted_rows_win_by_four_eps_in_both_modes(d):
    """The margin the GPU test's `fallback_queries == 0` rests on: between the k planted scores, and from the k-th to the
    best other row, at least MARGIN_FACTOR x scan_eps_ref on the scan's scale, for both operand modes."""
    for metric in METRICS:
        for n in sorted({c.n for c in wc.scan_cells() if c.d == d and c.metric == metric}):      # every n a cell runs
            p = wc.planted(n, d, wc.SCAN_K, metric)
            _, ids = ho.flat_search(p.x, p.q, wc.SCAN_K, metric)
            assert np.array_equal(ids[0], p.rows), (d, metric)
            assert {0, 31, 32, n - 1} <= set(p.rows.tolist())
            s = wc.scan_scale_scores(p.x, p.q, metric)[0]
            ceiling = wc.FILLER_SCALE * (1 if metric == ho.METRIC_IP else 2)
            assert np.delete(s, p.rows).max() <= ceiling * (1 + 1e-6) < s[p.rows].min()    # the fillers stay under their ceiling
            for mode in wc.MODES:
                gap, eps = wc.planted_margins(p, d, wc.SCAN_K, mode)
                print("planted d=%d n=%d %s %s: gap %.4g = %.1f eps" % (d, n, "ip" if metric == ho.METRIC_IP else "l2", mode,
                                                                         gap, gap / eps))
                assert gap >= wc.MARGIN_FACTOR * eps, (d, metric, mode, gap, eps)


def test_planted_rows_depend_on_their_tail_segment():
    """Inner product: a scan that loses one tail segment scores the planted rows of that segment below fillers."""
    for d in (1023, 129, 7):
        p = wc.planted(wc.SCAN_N_SMALL, d, wc.SCAN_K, ho.METRIC_IP)
        tb = wc.tail_bounds(d)
        hit = 0
        for lo, hi in zip(tb[:-1], tb[1:]):
            keep = np.ones(d, dtype=bool)
            keep[lo:hi] = False
            s = wc.scan_scale_scores(p.x[:, keep], p.q[keep], ho.METRIC_IP)[0]
            kth_other = np.sort(np.delete(s, p.rows))[::-1][40]
            hit += int((s[p.rows] < kth_other).sum())
        assert hit >= wc.SCAN_K // 2, (d, hit)


def test_scan_eps_ref_follows_the_formula_on_a_hand_case():
    # bf16-exact unit vectors: both truncation terms vanish, eps = 1.05 (d_pad + 80) 2^-24 |q||x| (1 + 2^-21) + 2^-21 |q||x|
    x = np.zeros((2, 130), dtype=np.float32)
    x[0, 129] = 1.0
    x[1, 0] = 0.5
    q = np.zeros((1, 130), dtype=np.float32)
    q[0, 129] = 2.0
    a = 1.05 * (256 + 80) * 2.0 ** -24 * 2.0
    for mode in wc.MODES:
        extra = 7.62939453125e-06 * 1.01 * 2.0 if mode == "q64" else 0.0
        got = wc.scan_eps_ref(130, mode, ho.METRIC_IP, x, q)[0]
        assert got == pytest.approx((a + extra) * (1 + 2.0 ** -21) + 2.0 ** -21 * 2.0, rel=1e-12)
    assert wc.row_bounds_ref(x) == (np.float32(1.0), np.float32(0.0))
    for data in (x, wc.tail_heavy(200, 131, seed=1, scaled=True)):
        lo, hi = wc.row_bounds_interval(data)
        ref = wc.row_bounds_ref(data)
        assert lo[0] <= ref[0] <= hi[0] <= np.nextafter(lo[0], np.float32(np.inf))
        assert lo[1] <= ref[1] <= hi[1] <= np.nextafter(lo[1], np.float32(np.inf))
    y = np.full((1, 3), 1.0 + 2.0 ** -10, dtype=np.float32)                     # |y|^2 is not a float32: rounded UP
    n2 = wc.row_bounds_ref(y)[0]
    assert float(n2) >= 3.0 * (1.0 + 2.0 ** -10) ** 2 > float(np.nextafter(n2, np.float32(0)))
