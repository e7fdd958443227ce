"""
CPU: the checks of tests/test_encoder_linear_gpu.py can fail, and do not fail a correct kernel.

  * every exactness precondition holds at every shape the GPU tests run (the generators assert them; here they all run);
  * the restated dispatch (oracle/linear_cases.py) gives the branch each GPU case names;
  * every mutant -- a wrong version of the reference -- fails its case: other bits in the exact regime, >= 3 x the derived
    bound in the random and LayerNorm regimes (the factor is printed);
  * the correct computation in fp32 with a shuffled accumulation order passes: the bounds do not reject a correct kernel,
    and in the exact regime it reproduces the reference bit for bit, which is the regime's claim.
"""
import math

import numpy as np
import pytest

from oracle import linear_cases as lc

MUTANT_FACTOR = 3.0


def _gemm_shapes():
    shapes = set()
    for table in (lc.TILED_CASES, lc.TILED_PART_CASES, lc.G256_CASES, lc.SKINNY_CASES, lc.CHAIN_CASES):
        shapes |= {(c["M"], c["N"], c["K"]) for c in table}
    return sorted(shapes)


def test_exactness_preconditions_at_every_gpu_shape():
    for M, N, K in _gemm_shapes():
        d = lc.linear_data("exact", M, N, K)            # asserts inside
        worst = lc.exactness_precondition(d)
        assert worst < 2 ** 24 and K <= 4096
        # float64 holds the same sums exactly: the reference is exact
        assert np.array_equal(d["c"] * 64, np.round(d["c"] * 64))
    for c in lc.LN_CASES:
        for regime in lc.LN_REGIMES:
            d = lc.layernorm_data(regime, c["form"], c["M"], c["H"], c["nsplit"])    # asserts inside
            if c["form"] == 1:
                assert d["parts"].shape == (c["nsplit"], c["M"], c["H"])
            if regime == "constant":
                assert lc.layernorm_expected(d)["bound"] is None


def test_restated_dispatch_reaches_the_branch_each_case_names():
    for c in lc.TILED_CASES:
        lc.assert_reach(lc.tiled_plan(c["M"], c["N"], c["K"]), c["reach"], c)
    for c in lc.TILED_PART_CASES:
        lc.assert_reach(lc.tiled_plan(c["M"], c["N"], c["K"], c["ksplit"]), c["reach"], c)
    for c in lc.G256_CASES:
        for cap in lc.G256_CAPS:
            p = lc.g256_plan(c["M"], c["N"], c["K"], 256, cap)
            lc.assert_reach(p, c["reach"], c)
            assert (p["grid"], p["xcd_order"], p["max_owned"], p["min_owned"]) == lc.G256_WALKS[p["tiles"]][cap]
    for c in lc.SKINNY_CASES:
        lc.assert_reach(lc.skinny_plan(c["M"], c["N"], c["K"]), c["reach"], c)
    for c in lc.CHAIN_CASES:
        if c["impl"] == 3:
            assert lc.skinny_plan(c["M"], c["N"], c["K"])["split"] == c["ksplit"]
    # between them the cases reach every branch the kernels have
    plans = [lc.skinny_plan(c["M"], c["N"], c["K"]) for c in lc.SKINNY_CASES]
    assert {(p["NT"], p["FULL"]) for p in plans} == {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert {p["split"] for p in plans} == {1, 2, 4} and {p["steps"] for p in plans} >= {1, 3, 6, 8}
    assert any(p["mb_per_wg"] > 1 and p["last_group"] < p["mb_per_wg"] for p in plans)
    assert any(c["M"] == 64 for c in lc.SKINNY_CASES) and any(c["N"] % 32 == 16 and c["M"] >= 128 for c in lc.SKINNY_CASES)
    walks = [w for t in (9, 24) for w in lc.G256_WALKS[t].values()]
    assert any(g == 1 and mx > 1 for g, _, mx, _ in walks)                    # one workgroup walks every tile
    assert any(x == 0 and mx > mn for _, x, mx, mn in walks)                  # ragged walk, plain order
    assert any(x == 1 and mx > 1 for _, x, mx, _ in walks)                    # XCD order, more than one tile per workgroup
    # forward's real shapes use the same branches: F -> H of one query splits 4 ways, 131072 rows are 8 tiles per workgroup
    assert lc.skinny_plan(64, 1024, 4096)["split"] == 4 and lc.g256_plan(131072, 1024, 1024, 256)["max_owned"] == 8
    assert lc.tile_split(1024, 2560, 4096) == 4 and lc.tile_split(1024, 2560, 1024) == 4 and lc.tile_split(1024, 16384, 4096) == 1


# the case each mutant is shown on: small, with more than one tile, sequence and split
CARRIER = dict(M=256, N=384, K=256, heads=2, S=128, m_valid=192, ksplit=2)


def _expected(regime, epi, mutant=None):
    c = CARRIER
    d = lc.linear_data(regime, c["M"], c["N"], c["K"])
    return lc.linear_expected(d, epi, c["m_valid"], c["S"], c["heads"], c["ksplit"], mutant=mutant)


@pytest.mark.parametrize("mutant", lc.MUTANTS)
def test_every_gemm_mutant_fails(mutant):
    for epi in lc.MUTANT_EPIS[mutant]:
        for regime in lc.REGIMES:
            exp = _expected(regime, epi)
            bad = _expected(regime, epi, mutant)
            assert all(lc.worst_ratio(exp[n], lc.image_bits(exp[n])) <= 1.0 for n in exp)        # the unmutated image passes
            factor = max(lc.worst_ratio(exp[n], lc.image_bits(bad[n])) for n in exp)
            name = epi if isinstance(epi, str) else lc.EPI_NAMES[epi]
            print(f"[{mutant} / {name} / {regime}] worst |err| / bound {factor:.1f}")
            if regime == "exact" and epi != lc.EPI_GELU:
                assert factor == math.inf, (mutant, name)                # bits differ in at least one element
            else:
                assert factor >= MUTANT_FACTOR, (mutant, name, regime, factor)


@pytest.mark.parametrize("epi", [lc.EPI_QKV, lc.EPI_GELU, lc.EPI_RESID, lc.EPI_RESID16, lc.EPI_PART, "partsum"])
def test_shuffled_fp32_evaluation_passes(epi):
    c = CARRIER
    for M, N, K in ((c["M"], c["N"], c["K"]), (128, 384, 1024)):
        for regime in lc.REGIMES:
            d = lc.linear_data(regime, M, N, K)
            exp = lc.linear_expected(d, epi, None, c["S"], c["heads"], c["ksplit"])
            got = lc.shuffled_fp32_outputs(d, epi, c["S"], c["heads"], c["ksplit"], seed=3)
            worst = max(lc.worst_ratio(exp[n], got[n]) for n in exp)
            print(f"[shuffled fp32 / {epi} / {regime} / K={K}] worst |err| / bound {worst:.3f}")
            assert worst <= 1.0
            if regime == "exact" and epi != lc.EPI_GELU:
                assert worst == 0.0


def test_gelu_bound_holds_over_the_whole_range():
    x = np.linspace(-12.0, 12.0, 200001).astype(np.float32)
    err = np.abs(lc.gelu_fp32(x).astype(np.float64) - lc.gelu64(x.astype(np.float64)))
    ratio = float((err / lc.gelu_delta(x.astype(np.float64))).max())
    print(f"[gelu_exact in fp32 vs erf in fp64] worst |err| / delta {ratio:.3f}, worst |err| {err.max():.2e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("mutant,form,M,H", [("var_over_padded_lanes", 0, 5, 384), ("var_over_padded_lanes", 1, 5, 384),
                                             ("ln16_partner_stats", 2, 5, 640), ("ln16_partner_stats", 2, 18, 128)])
def test_every_layernorm_mutant_fails(mutant, form, M, H):
    for regime in ("random", "offset"):
        d = lc.layernorm_data(regime, form, M, H, 3 if form == 1 else 1)
        exp = lc.layernorm_expected(d)
        bad = lc.layernorm_expected(d, mutant)
        assert lc.worst_ratio(exp, lc.image_bits(exp)) <= 1.0
        factor = lc.worst_ratio(exp, lc.image_bits(bad))
        print(f"[{mutant} / form {form} M={M} H={H} / {regime}] worst |err| / bound {factor:.1f}")
        assert factor >= MUTANT_FACTOR


def test_shuffled_fp32_layernorm_passes_at_every_gpu_case():
    worst = {r: 0.0 for r in lc.LN_REGIMES}
    for c in lc.LN_CASES:
        for regime in lc.LN_REGIMES:
            d = lc.layernorm_data(regime, c["form"], c["M"], c["H"], c["nsplit"])
            r = lc.worst_ratio(lc.layernorm_expected(d), lc.layernorm_fp32_shuffled(d, seed=c["M"]))
            assert r <= 1.0, (c, regime, r)
            worst[regime] = max(worst[regime], r)
    print("[shuffled fp32 LayerNorm] worst |err| / bound: " + ", ".join(f"{r} {v:.3f}" for r, v in worst.items()))
    assert worst["constant"] == 0.0            # bf16(beta), bit for bit


def test_fill_and_mask_are_part_of_the_check():
    exp = _expected("exact", lc.EPI_RESID)["out"]
    img = lc.image_bits(exp)
    assert lc.worst_ratio(exp, img) == 0.0
    touched = img.copy()
    touched[CARRIER["m_valid"], 3] = 0                       # a padding row written
    assert lc.worst_ratio(exp, touched) == math.inf
    missed = img.copy()
    missed[0, 0] = lc.FILL32                                 # a real element never written
    assert lc.worst_ratio(exp, missed) == math.inf
