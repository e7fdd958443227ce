"""
The scan's launch policy (csrc/dense_plan.h) asked through the library itself: hiprag_scan_plan is arithmetic over a shape,
needs no device and no handle, so these run on a machine without a GPU.  Against hand-worked values, against the rules as
oracle/width_cases.py and tests/test_pipe_spare_cus_gpu.py restate them, and against the formulas the host code used before
the policy had one home (written out below).
"""
import pytest

from oracle import hybrid_oracle as ho
from oracle import width_cases as wc
from test_pipe_spare_cus_gpu import _expected_spare

BF16, Q64 = 3, 2
MODE = {"bf16": BF16, "q64": Q64}


def shape(nblocks, P, mode=BF16, wide_env=-1, n_cu=256, launch_env=0):
    from hiprag import _native as nat
    return nat.HipIdxScanShape(nblocks, P, mode, wide_env, n_cu, launch_env)


def plan(s, nq, k=10, cus=256):
    from hiprag.index import scan_plan
    return scan_plan(s, nq, k, cus)


def test_hand_worked_values():
    # waves: 4 only for bf16, P % 32 == 0 and fewer than 72 blocks per workgroup
    assert plan(shape(287, 128), 3, cus=4).waves == 4 and plan(shape(288, 128), 3, cus=4).waves == 8
    assert plan(shape(18431, 128), 3, cus=256).waves == 4 and plan(shape(18432, 128), 3, cus=256).waves == 8
    assert plan(shape(1, 48), 3).waves == 8 and plan(shape(1, 128, Q64), 3).waves == 8
    # ring: 16 where it divides P / 2 -- P = 16, 48, 80, 112 run 8; q64 always 16
    for P in range(16, 129, 16):
        assert plan(shape(94, P), 3, cus=4).ring == (8 if P in (16, 48, 80, 112) else 16), P
        assert plan(shape(94, P, Q64), 3, cus=4).ring == 16, P
    # the filter: off at 512 blocks (1024 groups), on at 513
    assert plan(shape(512, 64), 3).filter == 0 and plan(shape(513, 64), 3).filter == 1
    # passes; the bf16 kernels alone copy query-tile images, and only in multi-pass launches
    assert plan(shape(94, 64), 64).multi_pass == 0 and plan(shape(94, 64), 65).multi_pass == 1
    assert [plan(shape(94, 64, m), nq).qtile_image for m in (BF16, Q64) for nq in (64, 65)] == [0, 1, 0, 0]
    # no scan without rows or beyond the finish's depth; the filter is reported either way
    assert plan(shape(0, 64), 3).run == 0 and plan(shape(94, 64), 3, k=128).run == 1
    p = plan(shape(600, 64), 3, k=129)
    assert p.run == 0 and p.filter == 1


def test_every_scan_cell_gets_the_kernel_shape_it_is_named_for():
    for c in wc.scan_cells():
        s = shape(wc.nblocks(c.n), wc.pieces(c.d), MODE[c.mode])
        p = plan(s, c.nq, wc.SCAN_K, wc.SCAN_CUS)
        assert p.run == 1 and wc.plan_label(s, p) == c.label, (c.name, wc.plan_label(s, p))


def test_the_wide_rule_on_both_sides_of_every_term():
    big = 300 * 8            # 300 row tiles: the filter on, a row tile for each of 256 workgroups
    wide = lambda s, nq, cus=256: plan(s, nq, cus=cus).wide
    for nq in (65, 256, 1024):
        assert wide(shape(big, 128, Q64), nq) == 0 and wide(shape(big, 128, Q64, wide_env=1), nq) == 0
        assert wide(shape(big, 128, wide_env=0), nq) == 0
    # forced: from 65 queries
    assert wide(shape(big, 128, wide_env=1), 64) == 0 and wide(shape(big, 128, wide_env=1), 65) == 1
    # default: at least 256 queries ...
    assert wide(shape(big, 128), 255) == 0 and wide(shape(big, 128), 256) == 1
    # ... and at least `cus` row tiles of 8 blocks
    assert wide(shape(8 * 255, 128), 1024) == 0 and wide(shape(8 * 255 + 1, 128), 1024) == 1
    assert wide(shape(8 * 255, 128), 1024, cus=255) == 1 and wide(shape(8 * 207 + 1, 128), 256, cus=208) == 1
    # below 32 workgroups never
    for env in (-1, 1):
        assert wide(shape(big, 128, wide_env=env), 1024, cus=31) == 0 and wide(shape(big, 128, wide_env=env), 1024, cus=32) == 1
    # at 512 blocks (the filter off) never
    for env in (-1, 1):
        assert wide(shape(512, 128, wide_env=env), 1024, cus=32) == 0 and wide(shape(513, 128, wide_env=env), 1024, cus=32) == 1
    # a wide launch: 8 waves, 128 KiB of LDS, images
    p = plan(shape(big, 128), 512)
    assert (p.waves, p.ring, p.multi_pass, p.qtile_image, p.lds_bytes) == (8, 0, 1, 1, 131072)
    assert wc.plan_label(shape(big, 128), p) == "bf16/P128/wide/w8/multi"


ROWS = (1, 16384, 16385, 20011, 207 * 256, 208 * 256, 223 * 256 + 1, 224 * 256, 416 * 256, 417 * 256, 430 * 256 - 5, 125000,
        448 * 256 + 1, 250000, 500000, 1000000, 2000000)


def test_pipe_spare_cus_is_the_rule_as_the_gpu_test_states_it():
    for n_cu in (64, 80, 96, 128, 256, 304):
        for d in (64, 1024):
            for n in ROWS:
                p = plan(shape(wc.nblocks(n), wc.pieces(d), n_cu=n_cu), 3)
                assert p.pipe_spare_cus == _expected_spare(n, n_cu), (n_cu, d, n)
    assert {plan(shape(wc.nblocks(n), 128), 3).pipe_spare_cus for n in ROWS} == {32, 48}
    # the two recorded cases: a width-1024 bf16 index at 256 CUs
    p = plan(shape(wc.nblocks(1000000), 128), 3)
    assert (p.pipe_spare_cus, p.launch_queries) == (32, 512)
    p = plan(shape(wc.nblocks(125000), 128), 3)
    assert (p.pipe_spare_cus, p.launch_queries) == (48, 1024)
    # 430 * 256 - 5 rows x 64: 3 rounds on 208 workgroups, 2 on 224
    assert plan(shape(wc.nblocks(430 * 256 - 5), 16), 3).pipe_spare_cus == 32
    # q64, or the wide kernel switched off: the narrow scan's 48
    assert plan(shape(wc.nblocks(1000000), 128, Q64), 3).pipe_spare_cus == 48
    assert plan(shape(wc.nblocks(1000000), 128, wide_env=0), 3).pipe_spare_cus == 48
    # HIPRAG_LAUNCH_QUERIES: rounded down to whole passes, within 64 .. 1024
    assert [plan(shape(94, 64, launch_env=e), 3).launch_queries for e in (1, 64, 200, 5000)] == [64, 64, 192, 1024]
    assert [plan(shape(nb, 128), 3).launch_queries for nb in (0, 1, 31250, 62500)] == [1024, 1024, 512, 256]


def _former(nb, P, mode, nq, cus, waves, wide):
    """lds_bytes, ncls, bytes_per_pass (ip, l2) as scan_pass and hipidx_get_stats computed them inline"""
    lds = 2 * (8 + 8) * 4 * 64 * 16 if wide else P * 1024 + 2 * 896 * 16 + 64 + 8 * 64 * 4
    bpw = -(-nb // (cus * waves))
    ncls = max(1, min(64, -(-nb // bpw)))
    stream = nb * P * (512 if mode == BF16 else 1024)
    return lds, ncls, stream // (4 if wide else 1), (stream + nb * 32 * 4) // (4 if wide else 1)


def test_fields_equal_the_former_inline_formulas():
    seen = set()
    for c in wc.scan_cells():
        key = (wc.nblocks(c.n), wc.pieces(c.d), MODE[c.mode], c.nq)
        if key in seen:
            continue
        seen.add(key)
        nb, P, mode, nq = key
        for cus in (wc.SCAN_CUS, 256):
            p = plan(shape(nb, P, mode), nq, wc.SCAN_K, cus)
            assert p.wide == 0
            assert (p.lds_bytes, p.ncls, p.bytes_per_pass_ip, p.bytes_per_pass_l2) == _former(nb, P, mode, nq, cus, p.waves, False), (key, cus)
    assert len(seen) >= 40
    # few blocks on a large grid: fewer classes than 64; many: all 64
    assert plan(shape(5, 16), 3, cus=256).ncls == 5 and plan(shape(94, 64), 3, cus=4).ncls == 16 and plan(shape(290, 64), 3, cus=4).ncls == 29
    assert plan(shape(31250, 128), 64).ncls == 64
    # one wide launch: 1M x 1024, 512 queries, 224 workgroups
    nb = wc.nblocks(1000000)
    p = plan(shape(nb, 128), 512, 10, 224)
    assert p.wide == 1
    assert (p.lds_bytes, p.ncls, p.bytes_per_pass_ip, p.bytes_per_pass_l2) == _former(nb, 128, BF16, 512, 224, 8, True)
    assert p.bytes_per_pass_ip == 31250 * 128 * 512 // 4


def test_bad_arguments_are_refused():
    from hiprag import _native as nat
    for s, nq, k, cus in ((shape(10, 0), 1, 1, 1), (shape(10, 24), 1, 1, 1), (shape(-1, 16), 1, 1, 1), (shape(10, 16, 4), 1, 1, 1),
                          (shape(10, 16), 0, 1, 1), (shape(10, 16), 1, 0, 1), (shape(10, 16), 1, 1, 0), (shape(10, 16, n_cu=0), 1, 1, 1)):
        with pytest.raises(nat.HipRagError):
            plan(s, nq, k, cus)
