"""
hipenc_forward_m3: dense, lexical and ColBERT outputs from ONE forward.  Every output is, bit for bit, what hipenc_forward,
hipenc_forward_lexical and hipenc_forward_colbert write for the same batch -- on one batch for every HIPENC_PATH_* that
hipenc_forward_plan reports reachable for the config (the two tiny configs of tests/test_colbert_head_gpu.py: hidden 128 and
256, 2 layers, synthetic weights), with ragged lengths that include 0, 1, 2 and max_len.  And the entry's checks.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_INVALID = -1
CONFIGS = {"h128": dict(hidden=128, heads=2, ffn=256, layers=2), "h256": dict(hidden=256, heads=4, ffn=512, layers=2)}
SEED = 23
VOCAB = 48
PATH_NAMES = {0: "small", 1: "big", 2: "tiled"}                  # HIPENC_PATH_*
# the batches the plan is asked about: padded lengths the model takes (max_pos 200) and 4 to 512 sequences
S_VALUES = (64, 128, 192)
NSEQ_VALUES = (4, 6, 8, 16, 64, 128, 256, 342, 384, 512)     # four at least: lengths 0, 1, 2 and max_len in every batch


@functools.lru_cache(maxsize=None)
def encoder(name):
    import torch
    from hiprag import EncoderConfig, HipEncoder, random_state
    cfg = EncoderConfig(vocab=VOCAB, max_pos=200, max_seq_len=192, **CONFIGS[name])
    enc = HipEncoder(cfg, random_state(cfg, seed=SEED))
    g = torch.Generator().manual_seed(SEED)
    H = cfg.hidden
    enc.set_lexical_head(torch.randn(H, generator=g) * 0.5, torch.randn(1, generator=g) * 0.1, (0, 1, 2, 3))
    enc.set_colbert_head(torch.randn(H, H, generator=g) * 0.05, torch.randn(H, generator=g) * 0.1)
    return enc, cfg


def reachable_batches(name):
    """{path: (nseq, S)}: for every path the plan gives some candidate batch of this config, the one with the fewest rows"""
    from hiprag.encoder import forward_plan
    enc, _ = encoder(name)
    shape = enc.shape()
    best = {}
    for S in S_VALUES:
        for nseq in NSEQ_VALUES:
            path = int(forward_plan(shape, nseq, S).path)
            if path not in best or nseq * S < best[path][0] * best[path][1]:
                best[path] = (nseq, S)
    return best


def batch(nseq, S):
    """ragged lengths around max_len = S - 2 (not a multiple of 64): 0, 1, 2 and max_len itself among them"""
    max_len = S - 2
    rng = np.random.default_rng(nseq * 1000 + S)
    pattern = [max_len, 0, 1, 2, 63, max_len - 1, 33, 5]
    lens = np.asarray([min(pattern[i % len(pattern)], max_len) for i in range(nseq)], dtype=np.int32)
    ids = np.zeros((nseq, max_len), dtype=np.int32)
    for i, n in enumerate(lens):
        if n >= 2:
            ids[i, :n] = [0] + rng.integers(3, VOCAB, size=n - 2).tolist() + [2]
    return ids, lens, max_len


def run_four(enc, H, ids, lens, max_len):
    """the four entries on the same batch, every output poisoned first -> dict of host arrays"""
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    n = len(lens)
    f32 = lambda *s: torch.full(s, 7.5, dtype=torch.float32, device="cuda")
    i32 = lambda *s: torch.full(s, -9, dtype=torch.int32, device="cuda")
    b16 = lambda *s: torch.full(s, 3.0, dtype=torch.bfloat16, device="cuda")
    o = dict(dense=f32(n, H), lex_dense=f32(n, H), col_dense=f32(n, H), m3_dense=f32(n, H),
             terms=i32(n, max_len), weights=f32(n, max_len), lcounts=i32(n), m3_terms=i32(n, max_len), m3_weights=f32(n, max_len),
             m3_lcounts=i32(n), vecs=b16(n, max_len - 1, H), ccounts=i32(n), m3_vecs=b16(n, max_len - 1, H), m3_ccounts=i32(n))
    p = {k: v.data_ptr() for k, v in o.items()}
    st = _stream_ptr()
    a = (enc._h, ids.ctypes.data, lens.ctypes.data, n, max_len)
    nat.call("hipenc_forward", *a, p["dense"], st)
    nat.call("hipenc_forward_lexical", *a, p["lex_dense"], p["terms"], p["weights"], p["lcounts"], st)
    nat.call("hipenc_forward_colbert", *a, p["col_dense"], p["vecs"], p["ccounts"], st)
    nat.call("hipenc_forward_m3", *a, p["m3_dense"], p["m3_terms"], p["m3_weights"], p["m3_lcounts"], p["m3_vecs"], p["m3_ccounts"], st)
    torch.cuda.synchronize()
    return {k: (v.view(torch.int16) if v.dtype == torch.bfloat16 else v).cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_all_six_outputs_on_every_reachable_path(gpu, name):
    enc, cfg = encoder(name)
    H = cfg.hidden
    batches = reachable_batches(name)
    print(f"{name}: " + ", ".join(f"{PATH_NAMES[p]} at {b[0]} x {b[1]}" for p, b in sorted(batches.items())))
    assert {0, 2} <= set(batches), "the small and the tiled path are reachable for every config"
    for path, (nseq, S) in sorted(batches.items()):
        ids, lens, max_len = batch(nseq, S)
        assert {0, 1, 2, max_len} <= set(lens.tolist())
        r = run_four(enc, H, ids, lens, max_len)
        tag = f"{name} {PATH_NAMES[path]}"
        for got, want in (("m3_dense", "dense"), ("m3_dense", "lex_dense"), ("m3_dense", "col_dense"), ("m3_terms", "terms"),
                          ("m3_weights", "weights"), ("m3_lcounts", "lcounts"), ("m3_vecs", "vecs"), ("m3_ccounts", "ccounts")):
            assert r[got].tobytes() == r[want].tobytes(), f"{tag}: {got} differs from {want}"
        # the outputs are real: counts as the heads define them, some weights and vectors non-zero, nothing left poisoned
        assert r["m3_ccounts"].tolist() == [max(0, int(n) - 1) for n in lens]
        assert (r["m3_lcounts"] >= 0).all() and (r["m3_lcounts"] <= np.maximum(lens - 2, 0)).all()
        if nseq >= 1 and lens[0] == max_len:
            assert r["m3_lcounts"][0] > 0 and (r["m3_weights"][0, :r["m3_lcounts"][0]] > 0).all()
            assert np.any(r["m3_vecs"][0, max_len - 2] != 0)
        assert not np.any(r["m3_dense"] == 7.5) and not np.any(r["m3_terms"] == -9) and not np.any(r["m3_weights"] == 7.5)


def test_null_dense_and_the_wrapper(gpu):
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    enc, cfg = encoder("h128")
    H = cfg.hidden
    ids, lens, max_len = batch(6, 64)
    r = run_four(enc, H, ids, lens, max_len)
    t = torch.full((6, max_len), -9, dtype=torch.int32, device="cuda")
    w = torch.full((6, max_len), 7.5, dtype=torch.float32, device="cuda")
    c = torch.full((6,), -9, dtype=torch.int32, device="cuda")
    v = torch.full((6, max_len - 1, H), 3.0, dtype=torch.bfloat16, device="cuda")
    vc = torch.full((6,), -9, dtype=torch.int32, device="cuda")
    nat.call("hipenc_forward_m3", enc._h, ids.ctypes.data, lens.ctypes.data, 6, max_len, None, t.data_ptr(), w.data_ptr(), c.data_ptr(),
             v.data_ptr(), vc.data_ptr(), _stream_ptr())                 # out_dense_dev = NULL: the heads alone, the same bits
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == r["terms"].tobytes() and w.cpu().numpy().tobytes() == r["weights"].tobytes()
    assert v.view(torch.int16).cpu().numpy().tobytes() == r["vecs"].tobytes() and vc.cpu().numpy().tobytes() == r["ccounts"].tobytes()
    # encode_m3 = encode_lexical + encode_colbert, input order restored over three length-sorted batches; a 1-token input
    rng = np.random.default_rng(5)
    toks = [([0] + rng.integers(3, VOCAB, size=max(n - 2, 0)).tolist() + [2])[:n] if n >= 2 else [0][:n] for n in (2, 130, 0, 63, 1, 65, 64)]
    d, tt, ww, cc, vv, vn = enc.encode_m3(toks, batch_size=3)
    ld, lt, lw, lc = enc.encode_lexical(toks, batch_size=3)
    cd, cv, cn = enc.encode_colbert(toks, batch_size=3)
    assert torch.equal(d, ld) and torch.equal(d, cd) and torch.equal(tt, lt) and torch.equal(ww, lw) and torch.equal(cc, lc)
    assert torch.equal(vv.view(torch.int16), cv.view(torch.int16)) and torch.equal(vn, cn)
    d1, t1, w1, c1, v1, n1 = enc.encode_m3([[0]], batch_size=3)
    assert tuple(t1.shape) == (1, 1) and tuple(v1.shape) == (1, 1, H) and int(n1[0]) == 0 and int(c1[0]) == 0


def test_the_checks_fire(gpu):
    import torch
    from hiprag import EncoderConfig, HipEncoder, random_state
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    cfg = EncoderConfig(vocab=VOCAB, max_pos=200, max_seq_len=192, **CONFIGS["h128"])
    H = cfg.hidden
    ids, lens = np.asarray([[0, 5, 2]], np.int32), np.asarray([3], np.int32)
    t = torch.full((1, 3), -9, dtype=torch.int32, device="cuda")
    w = torch.full((1, 3), 7.5, dtype=torch.float32, device="cuda")
    c = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    v = torch.full((1, 2, H), 3.0, dtype=torch.bfloat16, device="cuda")
    vc = torch.full((1,), -9, dtype=torch.int32, device="cuda")

    def forward(enc, max_len=3, lens_=lens, ids_=ids, **null):
        ptr = lambda name, x: None if name in null else x.data_ptr()
        nat.call("hipenc_forward_m3", enc._h, ids_.ctypes.data, lens_.ctypes.data, 1, max_len, None, ptr("terms", t), ptr("weights", w),
                 ptr("lcounts", c), ptr("vecs", v), ptr("ccounts", vc), _stream_ptr())

    g = torch.Generator().manual_seed(1)
    for missing in ("lexical", "colbert", "both"):                    # both heads must be set
        enc = HipEncoder(cfg, random_state(cfg, seed=SEED))
        if missing == "colbert":
            enc.set_lexical_head(torch.randn(H, generator=g), torch.randn(1, generator=g), (0, 1, 2, 3))
        if missing == "lexical":
            enc.set_colbert_head(torch.randn(H, H, generator=g) * 0.05, torch.randn(H, generator=g))
        with pytest.raises(nat.HipRagError) as e:
            forward(enc)
        assert e.value.code == E_INVALID and "head" in str(e.value), missing
        with pytest.raises(ValueError):
            enc.encode_m3([[0, 5, 2]])
        enc.close()
    enc, _ = encoder("h128")
    bad = [dict(max_len=1), dict(max_len=0), dict(terms=1), dict(weights=1), dict(lcounts=1), dict(vecs=1), dict(ccounts=1),
           dict(max_len=400), dict(lens_=np.asarray([4], np.int32)), dict(ids_=np.asarray([[0, VOCAB, 2]], np.int32))]
    for kw in bad:
        with pytest.raises(nat.HipRagError) as e:
            forward(enc, **kw)
        assert e.value.code == E_INVALID, kw
    torch.cuda.synchronize()
    assert int(c[0]) == -9 and int(vc[0]) == -9 and bool((t == -9).all()) and bool((w == 7.5).all()), "a refused call wrote its outputs"
    forward(enc)
    torch.cuda.synchronize()
    assert int(vc[0]) == 2 and int(c[0]) >= 0
