"""
GPU: the encoder's three GEMM kernels and three LayerNorm kernels, every output element against float64.

Through hipenc_linear_ex and hipenc_layernorm -- the launch helpers Encoder::forward uses -- at the smallest shapes that reach
each branch of the kernels and of their dispatch (oracle/linear_cases.py restates the dispatch; every case asserts the branch
it names).  Two data regimes per case: `exact` (small integers: fp32 accumulation is exact in any order, so fp32 outputs and
partials must match the reference bit for bit and bf16 outputs its ONE rounding) and `random` (Gaussian operands, an
element-wise bound derived from the reference alone).  Every output buffer starts as a NaN bit pattern: each element below
m_valid must be overwritten, each element at or above it must still hold the pattern.  Every launch runs twice for identical
bits.  tests/test_linear_cases_cpu.py shows on the CPU that wrong kernels (mutants) fail these same checks.
"""
import ctypes
import math

import numpy as np
import pytest

from oracle import linear_cases as lc

pytestmark = pytest.mark.gpu


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _filled(shape, f32):
    import torch
    return torch.full(shape, lc.FILL32 if f32 else lc.FILL16, dtype=torch.int32 if f32 else torch.int16, device="cuda:0")


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.int32 else np.uint16)


_DEV_CACHE = {}


def _operands(regime, M, N, K):
    key = (regime, M, N, K)
    if key not in _DEV_CACHE:
        _DEV_CACHE.clear()                       # one case's operands at a time
        _DEV_CACHE[key] = lc.as_torch(lc.linear_data(regime, M, N, K), "cuda:0")
    return _DEV_CACHE[key]


GUARD = 64          # rows of fill behind a partials buffer: a wrong split stride would land there


def _linear(regime, M, N, K, epi, impl, m_valid=None, S=64, heads=0, ksplit=0, cap=0, want_splits=None):
    """One launch -> {name: bit image on the host}.  Partials come back as [splits][m_valid][N] plus GUARD rows."""
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr as sp
    t = _operands(regime, M, N, K)
    m_valid = M if m_valid is None else m_valid
    splits = ctypes.c_int32(-1)
    if epi == lc.EPI_QKV:
        outs = dict(q=_filled((M // S, heads, S, 64), False), k=_filled((M // S, heads, S, 64), False),
                    vt=_filled((M // S, heads, 64, S), False))
        ptrs = (outs["q"].data_ptr(), outs["k"].data_ptr(), outs["vt"].data_ptr())
    elif epi == lc.EPI_PART:
        nsp = want_splits
        outs = dict(out=_filled((nsp * m_valid + GUARD, N), True))
        ptrs = (outs["out"].data_ptr(), None, None)
    else:
        outs = dict(out=_filled((M, N), epi == lc.EPI_RESID))
        ptrs = (outs["out"].data_ptr(), None, None)
    nat.call("hipenc_linear_ex", t["a"].data_ptr(), t["w"].data_ptr(), t["bias"].data_ptr(), M, N, K, epi,
             t["resid"].data_ptr() if epi in (lc.EPI_RESID, lc.EPI_RESID16) else None, ptrs[0], ptrs[1], ptrs[2], S, heads, impl,
             m_valid, ksplit, cap, ctypes.byref(splits), sp())
    torch.cuda.synchronize()
    got = {n: _bits(o) for n, o in outs.items()}
    if epi == lc.EPI_PART:
        assert splits.value == want_splits, (splits.value, want_splits)
        assert np.all(got["out"][want_splits * m_valid:] == lc.FILL32), "partials written beyond [splits][m_valid][N]"
        got["out"] = got["out"][:want_splits * m_valid].reshape(want_splits, m_valid, N)
    else:
        assert splits.value == 1
    return got


def _twice(*args, **kw):
    got = _linear(*args, **kw)
    again = _linear(*args, **kw)
    assert all(np.array_equal(got[n], again[n]) for n in got), "two launches, different bits"
    return got


def _check(regime, exp, got, what, bits_only=True):
    """-> worst |err| / bound over the outputs (0.0 where bits are compared).  The exact regime compares bits except for GELU."""
    worst = 0.0
    for n, e in exp.items():
        if regime == "exact" and bits_only:
            assert e["bound"] is None, (what, n)
        r = lc.worst_ratio(e, got[n])
        assert r <= 1.0, (what, n, r)
        worst = max(worst, r)
    return worst


def _partsum_bits(parts_bits, d, m_valid):
    """The partials summed in split order in fp32, + bias + residual -- the arithmetic of layernorm_kernel<true>'s front."""
    p = parts_bits.view(np.float32)
    t = p[0].copy()
    for s in range(1, p.shape[0]):
        t = t + p[s]
    full = np.full((d["M"], d["N"]), 0, dtype=np.uint32)
    full[:] = lc.FILL32
    full[:m_valid] = np.ascontiguousarray((t + d["bias"].astype(np.float32)) + d["resid"][:m_valid].astype(np.float32)).view(np.uint32)
    return full


def _id(c):
    s = f"{c['M']}x{c['N']}x{c['K']}"
    if "epi" in c:
        s += "-" + lc.EPI_NAMES[c["epi"]]
    if "ksplit" in c:
        s += f"-ks{c['ksplit']}"
    return s


# ---- 128 x 128 tiles (impl 1) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.TILED_CASES, ids=_id)
def test_tiled_kernel_every_element(gpu, case):
    M, N, K, epi = case["M"], case["N"], case["K"], case["epi"]
    lc.assert_reach(lc.tiled_plan(M, N, K), case["reach"], _id(case))
    worst = {}
    for regime in lc.REGIMES:
        d = lc.linear_data(regime, M, N, K)
        w = 0.0
        for m_valid in case["m_valids"]:
            for S in (case["S_list"] if epi == lc.EPI_QKV else (64,)):
                exp = lc.linear_expected(d, epi, m_valid, S, case["heads"])
                got = _twice(regime, M, N, K, epi, 1, m_valid, S, case["heads"])
                w = max(w, _check(regime, exp, got, (_id(case), regime, m_valid, S), bits_only=epi != lc.EPI_GELU))
        worst[regime] = w
    print(f"\n[impl 1 {_id(case)}] worst |err| / bound: " + ", ".join(f"{r} {v:.3f}" for r, v in worst.items()))


@pytest.mark.parametrize("case", lc.TILED_PART_CASES, ids=_id)
def test_tiled_split_k_partials_and_their_sum(gpu, case):
    M, N, K, ks = case["M"], case["N"], case["K"], case["ksplit"]
    lc.assert_reach(lc.tiled_plan(M, N, K, ks), case["reach"], _id(case))
    worst = {}
    for regime in lc.REGIMES:
        d = lc.linear_data(regime, M, N, K)
        w = 0.0
        for m_valid in case["m_valids"]:
            got = _twice(regime, M, N, K, lc.EPI_PART, 1, m_valid, ksplit=ks, want_splits=ks)
            w = max(w, _check(regime, lc.linear_expected(d, lc.EPI_PART, m_valid, ksplit=ks), got, (_id(case), regime, m_valid)))
            total = _partsum_bits(got["out"], d, m_valid)
            w = max(w, _check(regime, lc.linear_expected(d, "partsum", m_valid, ksplit=ks), {"out": total}, (_id(case), regime, "sum")))
            if regime == "exact":       # == the unsplit kernel's fp32 residual epilogue, bit for bit
                assert np.array_equal(total, _linear(regime, M, N, K, lc.EPI_RESID, 1, m_valid)["out"])
        worst[regime] = w
    print(f"\n[impl 1 partials {_id(case)}] worst |err| / bound: " + ", ".join(f"{r} {v:.3f}" for r, v in worst.items()))


# ---- persistent 256 x 256 tiles (impl 2) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.G256_CASES, ids=_id)
def test_persistent_kernel_every_walk_of_the_tiles(gpu, case):
    """max_workgroups 1: one workgroup walks every tile (staging stream, wave-private epilogue and re-stagger between all of
    them); 5: a ragged walk in the plain order; 8 and 16: the XCD order with workgroups owning more than one tile.  All of them
    must give the bits of the uncapped launch and of the 128-tile kernel."""
    M, N, K, epi = case["M"], case["N"], case["K"], case["epi"]
    tiles = case["reach"]["tiles"]
    n_cu = _n_cu()
    assert n_cu >= 24
    for cap in lc.G256_CAPS:
        p = lc.g256_plan(M, N, K, n_cu, cap)
        lc.assert_reach(p, case["reach"], _id(case))
        assert (p["grid"], p["xcd_order"], p["max_owned"], p["min_owned"]) == lc.G256_WALKS[tiles][cap], (cap, p)
    worst = {}
    for regime in lc.REGIMES:
        d = lc.linear_data(regime, M, N, K)
        w = 0.0
        for i, m_valid in enumerate(case["m_valids"]):
            S = case["S_list"][i % 3] if epi == lc.EPI_QKV else 64
            exp = lc.linear_expected(d, epi, m_valid, S, case["heads"])
            base = _twice(regime, M, N, K, epi, 2, m_valid, S, case["heads"], cap=0)
            w = max(w, _check(regime, exp, base, (_id(case), regime, m_valid, S), bits_only=epi != lc.EPI_GELU))
            if epi != lc.EPI_RESID16:
                small = _linear(regime, M, N, K, epi, 1, m_valid, S, case["heads"])
                assert all(np.array_equal(base[n], small[n]) for n in base), (_id(case), regime, m_valid, "impl 2 != impl 1")
            for cap in lc.G256_CAPS[1:]:
                got = _twice(regime, M, N, K, epi, 2, m_valid, S, case["heads"], cap=cap)
                assert all(np.array_equal(base[n], got[n]) for n in base), (_id(case), regime, m_valid, cap, "capped != uncapped")
        worst[regime] = w
    print(f"\n[impl 2 {_id(case)}, grids {[lc.G256_WALKS[tiles][c][0] for c in lc.G256_CAPS]}] worst |err| / bound: "
          + ", ".join(f"{r} {v:.3f}" for r, v in worst.items()))


# ---- small-batch kernel (impl 3) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.SKINNY_CASES, ids=_id)
def test_small_batch_kernel_every_element(gpu, case):
    M, N, K, epi = case["M"], case["N"], case["K"], case["epi"]
    plan = lc.skinny_plan(M, N, K)
    lc.assert_reach(plan, case["reach"], _id(case))
    sp = plan["split"]
    worst = {}
    for regime in lc.REGIMES:
        d = lc.linear_data(regime, M, N, K)
        if epi == lc.EPI_PART:
            got = _twice(regime, M, N, K, epi, 3, want_splits=sp)
            w = _check(regime, lc.linear_expected(d, epi, ksplit=sp), got, (_id(case), regime))
            total = _partsum_bits(got["out"], d, M)
            w = max(w, _check(regime, lc.linear_expected(d, "partsum", ksplit=sp), {"out": total}, (_id(case), regime, "sum")))
            if regime == "exact" and M % 128 == 0 and N % 128 == 0:
                assert np.array_equal(total, _linear(regime, M, N, K, lc.EPI_RESID, 1)["out"])
        else:
            S, heads = case.get("S", 64), case.get("heads", 0)
            got = _twice(regime, M, N, K, epi, 3, S=S, heads=heads)
            w = _check(regime, lc.linear_expected(d, epi, S=S, heads=heads), got, (_id(case), regime), bits_only=epi != lc.EPI_GELU)
        worst[regime] = w
    print(f"\n[impl 3 {_id(case)}: NT {plan['NT']}, FULL {plan['FULL']}, split {sp}, steps {plan['steps']}, "
          f"row blocks per workgroup {plan['mb_per_wg']}] worst |err| / bound: " + ", ".join(f"{r} {v:.3f}" for r, v in worst.items()))


def test_linear_ex_refuses_what_the_kernels_cannot_do(gpu):
    from hiprag import HipRagError
    ok = dict(regime="exact", M=256, N=768, K=128, epi=lc.EPI_GELU, impl=2)
    for bad in (dict(m_valid=100), dict(m_valid=320), dict(m_valid=0), dict(cap=-1), dict(impl=1, cap=4), dict(impl=4),
                dict(epi=lc.EPI_RESID, m_valid=192), dict(epi=lc.EPI_RESID16, m_valid=192), dict(impl=3, m_valid=192),
                dict(impl=3, epi=lc.EPI_RESID), dict(impl=2, epi=lc.EPI_PART, want_splits=1, ksplit=1),
                dict(impl=1, epi=lc.EPI_PART, want_splits=1, ksplit=5), dict(impl=1, epi=lc.EPI_PART, want_splits=1, ksplit=0),
                dict(impl=1, ksplit=2)):
        a = dict(ok, **bad)
        with pytest.raises(HipRagError):
            _linear(a.pop("regime"), a.pop("M"), a.pop("N"), a.pop("K"), a.pop("epi"), a.pop("impl"), **a)
    with pytest.raises(HipRagError):                      # K > 1024 splits over workgroups: partials only
        _linear("exact", 128, 128, 2048, lc.EPI_GELU, 3)
    with pytest.raises(HipRagError):                      # 1152 = 9 * 128: not a K the small-batch kernel takes
        _linear("exact", 128, 128, 1152, lc.EPI_PART, 3, want_splits=2)


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------
PAD_ROWS = 3


def _layernorm(d):
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr as sp
    dev = "cuda:0"
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    M, H, form = d["M"], d["H"], d["form"]
    gamma, beta = t(d["gamma"], torch.float32), t(d["beta"], torch.float32)
    y = _filled((M + PAD_ROWS, H), False)
    if form == 1:
        x, bias, resid = t(d["parts"], torch.float32), t(d["bias"], torch.float32), t(d["resid"], torch.bfloat16)
        nat.call("hipenc_layernorm", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), M, H, lc.LN_EPS, 1, d["nsplit"],
                 bias.data_ptr(), resid.data_ptr(), sp())
    else:
        x = t(d["x"], torch.float32 if form == 0 else torch.bfloat16)
        nat.call("hipenc_layernorm", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), M, H, lc.LN_EPS, form, 1, None,
                 None, sp())
    torch.cuda.synchronize()
    return _bits(y)


def _ln_padded(exp):
    M, H = exp["ref"].shape
    pad = lambda a, v: np.concatenate([a, np.full((PAD_ROWS, H), v, dtype=a.dtype)])
    return dict(kind="bf16", ref=pad(exp["ref"], 0.0), bound=None if exp["bound"] is None else pad(exp["bound"], 1.0),
                written=pad(exp["written"], False))


LN_GROUPS = sorted({(c["form"], c["H"]) for c in lc.LN_CASES})


@pytest.mark.parametrize("form,H", LN_GROUPS)
def test_layernorm_kernels_every_element(gpu, form, H):
    worst = {r: 0.0 for r in lc.LN_REGIMES}
    n = 0
    for c in lc.LN_CASES:
        if (c["form"], c["H"]) != (form, H):
            continue
        for regime in lc.LN_REGIMES:
            d = lc.layernorm_data(regime, form, c["M"], H, c["nsplit"])
            exp = _ln_padded(lc.layernorm_expected(d))
            assert (exp["bound"] is None) == (regime == "constant")          # constant rows: bf16(beta), bit for bit
            got = _layernorm(d)
            assert np.array_equal(got, _layernorm(d)), "two launches, different bits"
            r = lc.worst_ratio(exp, got)
            assert r <= 1.0, (form, H, c["M"], c["nsplit"], regime, r)
            worst[regime] = max(worst[regime], r)
            n += 1
    print(f"\n[layernorm form {form} H={H}: {n} cases] worst |err| / bound: " + ", ".join(f"{r} {v:.3f}" for r, v in worst.items()))


def test_layernorm_entry_validates_its_arguments(gpu):
    from hiprag import HipRagError
    base = lc.layernorm_data("random", 1, 5, 256, 2)
    for bad in (dict(H=192), dict(H=2176), dict(M=0), dict(form=3), dict(form=2, H=2048), dict(nsplit=5), dict(nsplit=0)):
        d = dict(base, **bad)
        if d["form"] != 1:
            d["x"] = np.zeros((max(d["M"], 1), 2048))
        with pytest.raises(HipRagError):
            _layernorm(d)


@pytest.mark.parametrize("case", lc.CHAIN_CASES, ids=lambda c: f"{c['M']}x{c['N']}x{c['K']}-impl{c['impl']}")
def test_partials_then_layernorm_equals_residual_then_layernorm(gpu, case):
    """The identity forward relies on when it splits K: partials summed inside layernorm_kernel<true> give the bits of the
    fp32 residual epilogue followed by layernorm_kernel<false>.  Exact regime: both see the same exact pre-LayerNorm row."""
    M, N, K, impl = case["M"], case["N"], case["K"], case["impl"]
    ks = case["ksplit"]
    if impl == 3:
        assert lc.skinny_plan(M, N, K)["split"] == ks
    d = lc.linear_data("exact", M, N, K)
    parts = _linear("exact", M, N, K, lc.EPI_PART, impl, ksplit=ks if impl == 1 else 0, want_splits=ks)["out"]
    pre = _linear("exact", M, N, K, lc.EPI_RESID, 1)["out"]
    rng = np.random.default_rng(5)
    gamma = (1.0 + 0.1 * rng.standard_normal(N)).astype(np.float32).astype(np.float64)
    beta = (0.1 * rng.standard_normal(N)).astype(np.float32).astype(np.float64)
    common = dict(M=M, H=N, gamma=gamma, beta=beta, regime="random")
    via_parts = _layernorm(dict(common, form=1, nsplit=ks, parts=parts.view(np.float32), bias=d["bias"], resid=d["resid"]))
    via_pre = _layernorm(dict(common, form=0, x=pre.view(np.float32)))
    assert np.array_equal(via_parts, via_pre)
    exp = _ln_padded(lc.layernorm_expected(dict(common, v=d["c"] + d["bias"] + d["resid"])))
    r = lc.worst_ratio(exp, via_parts)
    print(f"\n[chain {M}x{N}x{K} impl {impl}, {ks} partials] LayerNorm of the exact row: worst |err| / bound {r:.3f}")
    assert r <= 1.0
