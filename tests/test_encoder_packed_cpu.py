"""
CPU: the layout of a packed encoder batch (hipenc_packed_layout, csrc/encoder_packed.h) against a few-line numpy restatement,
and the plans (hipenc_forward_plan(shape, 1, Tp)) the packed GPU cases of tests/test_encoder_packed_gpu.py mean to reach.
Both entries are arithmetic alone: no handle, no device.
"""
import numpy as np
import pytest

from oracle import encoder_cases as ec

N_CU = 256       # MI355X; the GPU test asks the handle itself
BIG_PACKED_LENS = (191, 129, 65, 64, 16, 1) * 24 + (192, 130, 2)      # the packed 256-tile case of the GPU test
LAYOUT_CASES = (ec.MIXED_LENS, (0, 5, 0), (64,), (1,) * 300)


def restated_layout(lens):
    R = [-(-n // 64) * 64 for n in lens]
    row_off = np.concatenate([[0], np.cumsum(R)]).astype(np.int32)
    gran_seq = np.repeat(np.arange(len(lens)), [r // 64 for r in R]).astype(np.int32)
    items = np.asarray([(i, j) for i, n in enumerate(lens) for j in range(-(-n // 128))], dtype=np.int32).reshape(-1, 2)
    return row_off, int(row_off[-1]), gran_seq, items


@pytest.mark.parametrize("lens", LAYOUT_CASES, ids=lambda l: f"n{len(l)}_first{l[0]}")
def test_packed_layout_equals_its_restatement(lens):
    from hiprag.encoder import packed_layout
    row_off, Tp, gran_seq, items = packed_layout(lens)
    w_off, w_Tp, w_gran, w_items = restated_layout(lens)
    assert Tp == w_Tp and Tp % 64 == 0
    assert np.array_equal(row_off, w_off) and np.array_equal(gran_seq, w_gran) and np.array_equal(items, w_items)
    # the owner of every granule holds it, and only real tiles are work: 128 j < len, none for an empty sequence
    for g, s in enumerate(gran_seq):
        assert row_off[s] <= 64 * g < row_off[s + 1]
    assert all(128 * j < lens[s] for s, j in items)
    assert len(items) == sum(-(-n // 128) for n in lens)
    assert not any(lens[s] == 0 for s, _ in items)


def test_packed_layout_of_the_mixed_lengths():
    from hiprag.encoder import packed_layout
    row_off, Tp, gran_seq, items = packed_layout(ec.MIXED_LENS)
    assert Tp == 768 and row_off.tolist() == [0, 256, 448, 576, 640, 704, 768]
    assert gran_seq.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 4, 5]
    assert items.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [2, 0], [3, 0], [4, 0], [5, 0]]


def test_packed_layout_edge_cases_and_checks():
    from hiprag import HipRagError
    from hiprag.encoder import packed_layout
    row_off, Tp, gran_seq, items = packed_layout(())
    assert Tp == 0 and row_off.tolist() == [0] and gran_seq.size == 0 and items.shape == (0, 2)
    row_off, Tp, gran_seq, items = packed_layout((0, 0))
    assert Tp == 0 and row_off.tolist() == [0, 0, 0] and items.shape == (0, 2)
    with pytest.raises(HipRagError):
        packed_layout((5, -1))
    with pytest.raises(HipRagError):
        packed_layout((2 ** 29, 2 ** 29))          # Tp would reach 2^30


def test_packed_batches_are_greedy_in_input_order():
    from hiprag.encoder import packed_batches
    lens = [200, 129, 65, 64, 16, 1, 0, 500]
    assert [list(r) for r in packed_batches(lens, None)] == [list(range(8))]
    assert [list(r) for r in packed_batches(lens, 448)] == [[0, 1], [2, 3, 4, 5, 6], [7]]     # 256 + 192 | 128 + 3 * 64 + 0 | 512 alone
    assert [list(r) for r in packed_batches(lens, 1)] == [[i] for i in range(8)]              # a batch holds at least one
    assert [list(r) for r in packed_batches([], 64)] == []


def _plan(hidden, ffn, small_rows, nseq, S):
    from hiprag import _native as nat
    from hiprag.encoder import forward_plan
    return forward_plan(nat.HipEncShape(hidden, ffn, N_CU, small_rows, 1), nseq, S)


def _name(p):
    return {0: "small", 1: "big"}.get(p.path) or ("tiled_splitk" if max(p.osplit, p.dsplit) > 1 else "tiled")


@pytest.mark.parametrize("name", list(ec.MODEL_CASES))
def test_plans_of_the_packed_model_cases(name):
    """The path every packed GPU case reaches on a 256-CU device, beside the padded one's."""
    from hiprag.encoder import packed_layout
    case = ec.MODEL_CASES[name]
    lens = case["lens"]
    S = -(-max(lens) // 64) * 64
    Tp = packed_layout(lens)[1]
    small_rows = int(case["env"].get("HIPENC_SMALL_ROWS", 384))
    hidden, ffn = case["cfg"]["hidden"], case["cfg"]["ffn"]
    p1, p2 = _plan(hidden, ffn, small_rows, len(lens), S), _plan(hidden, ffn, small_rows, 1, Tp)
    assert _name(p1) == case["path"] and p2.T == Tp
    agree = (p1.path, p1.osplit, p1.dsplit) == (p2.path, p2.osplit, p2.dsplit)
    if name in ("small_h256", "tiled_h256"):
        assert (len(lens) * S, Tp) == (1536, 768) and agree          # the bit-equality branch is reached
    if name == "big_h1024":
        assert Tp == 10304 and _name(p2) != "big"                    # packed, this batch falls off the 256-tile path
    assert _name(p2) == ec.forward_path(hidden, ffn, Tp, small_rows, True, N_CU)


def test_plan_of_the_packed_256_tile_case():
    from hiprag.encoder import packed_layout
    Tp = packed_layout(BIG_PACKED_LENS)[1]
    p = _plan(1024, 4096, 384, 1, Tp)
    assert Tp == 17344 and p.path == 1 and p.M == 17408 and Tp % 256 != 0      # the last 256-row tile is part padding
