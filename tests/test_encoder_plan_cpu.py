"""
The encoder's forward policy (csrc/encoder_plan.h) asked through the library itself: hipenc_forward_plan is arithmetic over a
shape, needs no device and no handle, so these run on a machine without a GPU.  Against hand-worked values on both sides of
every term, and against the rules as oracle/encoder_cases.py (forward_path) and oracle/linear_cases.py (tile_split, skinny_ok)
restate them: the restatements stay the independent statement of the rule, and this is where they meet the library.
"""
import itertools

import pytest

from oracle import encoder_cases as ec
from oracle import linear_cases as lc

SMALL, BIG, TILED = 0, 1, 2


def shape(H=1024, F=4096, n_cu=256, small_rows=384, use256=1):
    from hiprag import _native as nat
    return nat.HipEncShape(H, F, n_cu, small_rows, use256)


def plan(s, T, S=64):
    from hiprag.encoder import forward_plan
    assert T % S == 0
    return forward_plan(s, T // S, S)


def label(p):
    """forward_path's name of a plan"""
    return {SMALL: "small", BIG: "big"}.get(p.path) or ("tiled_splitk" if max(p.osplit, p.dsplit) > 1 else "tiled")


def test_small_path_on_both_sides_of_every_term():
    # the row count: 384 rows are the last small batch, 448 the first that is not; 0 means never
    assert plan(shape(), 384).path == SMALL and plan(shape(), 448).path == TILED
    assert plan(shape(small_rows=0), 64).path == TILED and plan(shape(small_rows=64), 64).path == SMALL
    assert plan(shape(small_rows=2048), 2048).path == SMALL and plan(shape(small_rows=2048), 2112).path == TILED
    # H <= 1024
    assert plan(shape(H=1024, F=2048), 64).path == SMALL and plan(shape(H=1152, F=2048), 64).path == TILED
    # skinny_ok: K / ceil(K / 1024) a multiple of 128.  H = 1024: one range of 1024.  F = 1536: two ranges of 768 = 6 x 128, which
    # IS admissible; F = 1152: two ranges of 576 = 4.5 x 128, which is not.  (Every H <= 1024 is one range: always admissible.)
    assert plan(shape(H=1024, F=1536), 64).path == SMALL and plan(shape(H=384, F=1536), 64).path == SMALL
    assert plan(shape(H=1024, F=1152), 64).path == TILED and plan(shape(H=1024, F=1280), 64).path == SMALL
    assert lc.skinny_ok(1024) and lc.skinny_ok(1536) and not lc.skinny_ok(1152)
    # at most four partials: F = 4096 splits 4 ways, F = 5120 (admissible as a K: 5 x 1024) 5 ways
    assert plan(shape(F=4096), 64).path == SMALL and plan(shape(F=4096), 64).fsplit == 4
    assert lc.skinny_ok(5120) and plan(shape(F=5120), 64).path == TILED and plan(shape(F=5120), 64).fsplit == 5
    # small wins where the batch would also fill the 256-tile kernel
    p = plan(shape(small_rows=1 << 20), 16384)
    assert (p.path, p.M, p.osplit, p.dsplit, p.head_split) == (SMALL, 16384, 1, 1, 1)


def test_big_path_on_both_sides_of_every_term():
    # the narrowest product (N = H) gives every CU a tile: 63 row tiles x 4 = 252 < 256, 64 x 4 = 256
    assert plan(shape(), 16128).path == TILED and plan(shape(), 16384).path == BIG
    assert plan(shape(n_cu=64), 3840).path == TILED and plan(shape(n_cu=64), 4096).path == BIG
    # rows are padded to whole 256-tiles first: 16129 rows are 64 row tiles
    p = plan(shape(), 16192)
    assert (p.path, p.M) == (BIG, 16384)
    assert plan(shape(use256=0), 16384).path == TILED and plan(shape(use256=0), 131072).path == TILED
    assert plan(shape(H=1152, F=4608), 131072).path == TILED                         # H <= 1024
    # The three per-product tests.  (M, H, H) and (M, H, F) share N = H and the row count, and K % 128 holds for every width
    # hipenc_create admits, so neither can fail without the other: H = 384 (N = H is no multiple of 256) fails both while
    # (M, F, H) with F = 1536 passes
    assert plan(shape(H=384, F=1536), 131072).path == TILED and plan(shape(H=512, F=1536), 131072).path == BIG
    # (M, F, H) alone, by its shape: F = 4224 is no multiple of 256 (as K of the third product it is fine: 33 x 128)
    assert plan(shape(F=4224), 16384).path == TILED and plan(shape(F=4352), 16384).path == BIG
    # (M, F, H) alone, by its fill (at least n_cu / 2 tiles): F = 256 is one column tile: 64 row tiles < 128, 128 are enough
    assert plan(shape(F=256), 16384).path == TILED and plan(shape(F=256), 32768 - 256).path == TILED
    assert plan(shape(F=256), 32768).path == BIG


def test_tile_split_written_out():
    # (H, M, K) -> split: doubled while the launch stays under 512 workgroups, K divides and a split keeps >= 256 of K
    assert lc.tile_split(1024, 2560, 4096) == 4 and lc.tile_split(1024, 2560, 1024) == 4 and lc.tile_split(1024, 16384, 4096) == 1
    p = plan(shape(), 2560)
    assert (p.path, p.M, p.osplit, p.dsplit) == (TILED, 2560, 4, 4)
    p = plan(shape(use256=0), 16384)
    assert (p.path, p.M, p.osplit, p.dsplit) == (TILED, 16384, 1, 1)
    # the 512-workgroup term at H = 1024 (8 column tiles): 31 row tiles -> 248, 496 < 512 -> 4; 32 -> 256, 512 -> 2;
    # 63 -> 504 -> 2; 64 -> 512 -> 1
    assert [plan(shape(), T).osplit for T in (3968, 4096, 8064, 8192)] == [4, 2, 2, 1]
    # rows are padded to whole 128-tiles first: 3969..4032 rows are 32 row tiles
    assert (plan(shape(), 4032).M, plan(shape(), 4032).osplit) == (4096, 2)
    # a split keeps at least 256 of K: K = 384 none, K = 512 two, K = 768 two (192 < 256), K = 1024 four
    assert [plan(shape(H=H, F=4 * H, small_rows=0), 64).osplit for H in (384, 512, 768, 1024)] == [1, 2, 2, 4]
    # K a multiple of split x 128: K = 640 stops at two (640 / 256 leaves 128), K = 1280 goes to four (320 each)
    assert [plan(shape(H=128, F=F, small_rows=0), 64).dsplit for F in (640, 1280)] == [2, 4]


def test_head_split_and_workspace_for_one_case_per_path():
    p = plan(shape(), 384)             # small: the four partials of FFN-down size the workspace; the head's product is one
    assert (p.path, p.T, p.M, p.fsplit, p.head_split, p.pre_bytes) == (SMALL, 384, 384, 4, 1, 384 * 1024 * 4 * 4)
    p = plan(shape(), 16704)           # big (the rows of MODEL_CASES' big_h1024): 66 row tiles of 256, one set of rows
    assert (p.path, p.T, p.M, p.osplit, p.dsplit, p.head_split, p.pre_bytes) == (BIG, 16704, 16896, 1, 1, 1, 16896 * 1024 * 4)
    p = plan(shape(), 2560)            # tiled: the head takes the out-projection's split
    assert (p.path, p.head_split, p.pre_bytes) == (TILED, 4, 2560 * 1024 * 4 * 4)
    p = plan(shape(H=384, F=1536, small_rows=0), 1536)     # the splits differ: out-projection 1, FFN-down 4
    assert (p.path, p.osplit, p.dsplit, p.head_split, p.pre_bytes) == (TILED, 1, 4, 1, 1536 * 384 * 4 * 4)


GRID_H = (128, 256, 384, 1024, 2048)
GRID_T = (64, 128, 384, 448, 2560, 16384, 131072)


def test_the_library_and_the_restated_rules_agree():
    n = 0
    for H, T, small_rows, use256, n_cu in itertools.product(GRID_H, GRID_T, (0, 384, 1024), (0, 1), (64, 256)):
        F = 4 * H
        p = plan(shape(H, F, n_cu, small_rows, use256), T)
        what = (H, T, small_rows, use256, n_cu)
        assert label(p) == ec.forward_path(H, F, T, small_rows, bool(use256), n_cu), what
        assert p.T == T and p.fsplit == lc.skinny_split(F), what
        if p.path == SMALL:
            assert lc.skinny_ok(H) and lc.skinny_ok(F) and p.M == -(-T // 128) * 128, what
        if p.path == BIG:
            assert p.M == -(-T // 256) * 256, what
        if p.path == TILED:
            M = -(-T // 128) * 128
            assert (p.M, p.osplit, p.dsplit, p.head_split) == (M, lc.tile_split(H, M, H), lc.tile_split(H, M, F), lc.tile_split(H, M, H)), what
            assert p.pre_bytes == M * H * 4 * max(p.osplit, p.dsplit), what
        else:
            assert (p.osplit, p.dsplit, p.head_split) == (1, 1, 1), what
        n += 1
    assert n == 5 * 7 * 3 * 2 * 2


@pytest.mark.parametrize("name", list(ec.MODEL_CASES))
def test_every_model_case_gets_the_path_it_is_named_for(name):
    case = ec.MODEL_CASES[name]
    toks = ec.model_tokens(case)
    S = -(-max(len(t) for t in toks) // 64) * 64
    s = shape(case["cfg"]["hidden"], case["cfg"]["ffn"], 256, int(case["env"].get("HIPENC_SMALL_ROWS", 384)), 1)
    assert label(plan(s, len(toks) * S, S)) == case["path"], name


def test_bad_arguments_are_refused():
    from hiprag import _native as nat
    from hiprag.encoder import forward_plan
    for s, nseq, S in ((shape(H=0), 1, 64), (shape(H=192), 1, 64), (shape(H=2176), 1, 64), (shape(F=0), 1, 64), (shape(F=192), 1, 64),
                       (shape(n_cu=0), 1, 64), (shape(), 0, 64), (shape(), 1, 0), (shape(), 1, 96), (shape(), 1 << 20, 1 << 12)):
        with pytest.raises(nat.HipRagError):
            forward_plan(s, nseq, S)
    p = forward_plan(shape(small_rows=-5), 1, 64)            # a negative HIPENC_SMALL_ROWS reads as never
    assert p.path == TILED
