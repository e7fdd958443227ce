"""
The encoder's multi-vector (ColBERT) head: hipenc_colbert_rows (the head alone, on rows the test supplies, through the launches
the forward uses) in an exact and a random regime on the small-batch, the tiled and the split-K path; and
hipenc_forward_colbert on a tiny model -- the dense output is hipenc_forward's, the vectors are colbert_reference of the
hidden rows of the same batch, CLS skipped, EOS kept, input order restored.  Data, bounds: tests/colbert_cases.py.
"""
import functools

import numpy as np
import pytest

from colbert_cases import FILL16, head_data, head_expected, head_layout, layout_bound, layout_ratio
from oracle.linear_cases import bf16_bits, bf16_values, skinny_ok, tile_split

pytestmark = pytest.mark.gpu

E_INVALID = -1
ALL_LENS = (0, 1, 2, 63, 64, 65, 128)
# H, S, lengths, row_stride, the path the row count selects: "small" | ("tiled", K splits)
ROW_CASES = [
    dict(H=128, S=64, lens=(0, 1, 2, 63, 64), stride=63, path="small"),
    dict(H=1024, S=64, lens=(0, 1, 2, 63, 64), stride=63, path="small"),
    dict(H=1024, S=128, lens=(128, 65, 1), stride=127, path="small"),                      # 384 rows: the last small batch
    dict(H=1024, S=128, lens=(128, 65, 1, 0), stride=127, path=("tiled", 4)),              # 512 rows: the first tiled one
    dict(H=1024, S=128, lens=ALL_LENS, stride=127, path=("tiled", 4)),
    dict(H=128, S=128, lens=ALL_LENS, stride=127, path=("tiled", 1)),
    dict(H=128, S=128, lens=ALL_LENS, stride=40, path=("tiled", 1)),                       # a block narrower than the rows
]


def _path(T, H):
    if T <= 384 and H <= 1024 and skinny_ok(H):
        return "small"
    return ("tiled", tile_split(H, -(-T // 128) * 128, H))


def _library_path(nseq, S, H):
    """The same from the library's plan (hipenc_forward_plan) of a model of this width (F = 4 H) with the default switches: the
    path its forward takes at these rows, and the partials the head's product has there."""
    from hiprag import _native as nat
    from hiprag.encoder import forward_plan
    p = forward_plan(nat.HipEncShape(H, 4 * H, 256, 384, 1), nseq, S)
    assert p.path in (nat.ENC_PATH_SMALL, nat.ENC_PATH_TILED) and p.T == nseq * S
    return "small" if p.path == nat.ENC_PATH_SMALL else ("tiled", p.head_split)


def _run_rows(d, lens, S, stride):
    import torch
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    H, nseq = d["H"], len(lens)
    t16 = lambda a: torch.from_numpy(bf16_bits(a).view(np.int16).reshape(a.shape)).cuda().view(torch.bfloat16)
    x, w = t16(d["x"]), t16(d["w"])
    b = torch.from_numpy(d["b"].astype(np.float32)).cuda()
    ln = torch.from_numpy(np.asarray(lens, np.int32)).cuda()
    out = torch.from_numpy(np.full((nseq, stride, H), FILL16, np.uint16).view(np.int16)).cuda()       # poisoned
    cnt = torch.full((nseq,), -7, dtype=torch.int32, device="cuda")
    nat.call("hipenc_colbert_rows", x.data_ptr(), ln.data_ptr(), nseq, S, w.data_ptr(), b.data_ptr(), H, out.data_ptr(), cnt.data_ptr(),
             stride, _stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16), cnt.cpu().numpy()


@pytest.mark.parametrize("regime", ("exact", "random"))
@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: f"H{c['H']}-S{c['S']}-n{len(c['lens'])}-r{c['stride']}")
def test_rows_on_every_path(gpu, case, regime):
    from hiprag import colbert_reference
    H, S, lens, stride = case["H"], case["S"], case["lens"], case["stride"]
    T = len(lens) * S
    assert _path(T, H) == case["path"], "the row count no longer selects the path this case is for"
    assert _library_path(len(lens), S, H) == case["path"], "the library plans another path for these rows"
    d = head_data(regime, T, H)
    got, counts = _run_rows(d, lens, S, stride)
    y, bound = head_expected(d)
    want, want_counts = head_layout(y, lens, S, stride)
    assert np.array_equal(counts, want_counts) and np.array_equal(counts, [min(max(0, n - 1), stride) for n in lens])
    for i, c in enumerate(counts):
        assert np.all(got[i, c:] == 0), "rows at and behind the count are zero"
    if regime == "exact":
        # v and ss are exact whatever the order; sqrt, the division, the product and the bf16 rounding are the reference's
        splits = 1 if case["path"] == "small" else case["path"][1]
        ref = colbert_reference(d["x"], d["w"], d["b"], splits=splits)          # numpy fp32, operation for operation
        ref_out, _ = head_layout(ref.astype(np.float64), lens, S, stride)
        same = np.array_equal(got, bf16_bits(ref_out).reshape(got.shape))
        print(f"colbert rows exact H {H} S {S} stride {stride} {case['path']}: bits equal the reference: {same}")
        assert same
    else:
        r = layout_ratio(got, want, layout_bound(bound, lens, S, stride))
        print(f"colbert rows random H {H} S {S} stride {stride} {case['path']}: worst |got - ref| / bound = {r:.3g}")
        assert r <= 1.0
    again, counts2 = _run_rows(d, lens, S, stride)
    assert again.tobytes() == got.tobytes() and np.array_equal(counts, counts2)   # the same bits from run to run


def test_hook_refusals(gpu):
    import torch
    from hiprag import HipRagError
    from hiprag import _native as nat
    z = torch.zeros((64, 128), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((128, 128), dtype=torch.bfloat16, device="cuda")
    b = torch.zeros((128,), dtype=torch.float32, device="cuda")
    ln = torch.zeros((1,), dtype=torch.int32, device="cuda")
    out = torch.zeros((1, 63, 128), dtype=torch.bfloat16, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    ok = dict(x=z.data_ptr(), ln=ln.data_ptr(), nseq=1, S=64, w=w.data_ptr(), b=b.data_ptr(), H=128, out=out.data_ptr(), cnt=cnt.data_ptr(),
              stride=63)
    for kw in (dict(x=None), dict(ln=None), dict(w=None), dict(b=None), dict(out=None), dict(cnt=None), dict(nseq=0), dict(S=63), dict(S=0),
               dict(H=64), dict(H=2176), dict(stride=0), dict(stride=64)):
        a = dict(ok)
        a.update(kw)
        with pytest.raises(HipRagError) as e:
            nat.call("hipenc_colbert_rows", a["x"], a["ln"], a["nseq"], a["S"], a["w"], a["b"], a["H"], a["out"], a["cnt"], a["stride"], None)
        assert e.value.code == E_INVALID, kw


# ---- hipenc_forward_colbert on the tiny model of tests/test_lexical_gpu.py ---------------------------------------------------------
CONFIGS = {"h128": dict(hidden=128, heads=2, ffn=256, layers=2), "h256": dict(hidden=256, heads=4, ffn=512, layers=2)}
LENS = (2, 130, 0, 63, 1, 65, 64)          # not sorted: the batches are, and the results come back in this order
SEED = 11
BATCH = 3                                    # three length-sorted batches: 130 65 64 | 63 2 1 | 0


def _heads(H):
    """`perm`: one nonzero +-2^k per output -- c[n] = +-2^k x[pi(n)] is exact in fp32 whatever order the GEMM adds in, so the
    whole head is reproducible in numpy bit for bit on any hidden rows.  `dense`: a Gaussian head, compared within the bound."""
    rng = np.random.default_rng(SEED + H)
    perm = np.zeros((H, H))
    perm[np.arange(H), rng.permutation(H)] = rng.choice([-1.0, 1.0], size=H) * rng.choice([0.5, 1.0, 2.0], size=H)
    dense = bf16_values(bf16_bits(rng.standard_normal((H, H)) * 0.03))
    bias = (rng.standard_normal(H) * 0.1).astype(np.float32).astype(np.float64)
    return dict(perm=(perm, bias), dense=(dense, bias))


@functools.lru_cache(maxsize=None)
def setup(name):
    import torch
    from hiprag import EncoderConfig, HipEncoder, random_state
    cfg = EncoderConfig(vocab=48, max_pos=200, max_seq_len=192, **CONFIGS[name])
    rng = np.random.default_rng(SEED)
    toks = []
    for n in LENS:
        body = rng.integers(3, cfg.vocab, size=max(n - 2, 0)).tolist()
        toks.append(([0] + body + [2])[:n] if n >= 2 else [0][:n])
    enc = HipEncoder(cfg, random_state(cfg, seed=SEED))
    heads = _heads(cfg.hidden)
    outs = {}
    for kind, (w, b) in heads.items():
        enc.set_colbert_head(torch.from_numpy(w), torch.from_numpy(b))
        outs[kind] = tuple(t.cpu() for t in enc.encode_colbert(toks, batch_size=BATCH))
    hidden = enc.hidden_tokens(toks, batch_size=BATCH)
    return enc, cfg, toks, heads, outs, hidden


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_forward_vectors_equal_the_reference_of_the_hidden_rows(gpu, name):
    import torch
    from hiprag import colbert_reference
    enc, cfg, toks, heads, outs, hidden = setup(name)
    H = cfg.hidden
    w, b = heads["perm"]
    dense, vecs, counts = outs["perm"]
    assert tuple(vecs.shape) == (len(LENS), max(LENS) - 1, H) and vecs.dtype == torch.bfloat16 and counts.dtype == torch.int32
    assert counts.tolist() == [max(0, n - 1) for n in LENS]
    bits = vecs.view(torch.int16).numpy().view(np.uint16)
    for i, n in enumerate(LENS):
        c = max(0, n - 1)
        assert np.all(bits[i, c:] == 0)
        if c:
            ref = colbert_reference(hidden[i], w, b)                 # every position, CLS included
            assert np.array_equal(bits[i, :c], bf16_bits(ref[1:n])), f"sequence {i} (length {n}): CLS skipped, EOS kept, bit for bit"
            assert not np.array_equal(bits[i, :c], bf16_bits(ref[:n - 1])), "the test cannot tell CLS from the first token"
    # unit vectors: the norm of every stored row is 1 within bf16's rounding of H values
    rows = np.concatenate([bf16_values(bits[i, :max(0, n - 1)]) for i, n in enumerate(LENS)])
    assert np.all(np.abs(np.linalg.norm(rows, axis=1) - 1.0) < 2.0 ** -8)
    plain = enc.encode_tokens(toks, batch_size=BATCH).cpu().numpy()
    assert np.array_equal(dense.numpy().view(np.uint32), plain.view(np.uint32)) and np.all(dense.numpy()[2] == 0)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_forward_dense_head_within_the_bound(gpu, name):
    enc, cfg, toks, heads, outs, hidden = setup(name)
    w, b = heads["dense"]
    _, vecs, counts = outs["dense"]
    import torch
    bits = vecs.view(torch.int16).numpy().view(np.uint16)
    worst = 0.0
    for i, n in enumerate(LENS):
        if n < 2:
            continue
        d = dict(x=hidden[i].astype(np.float64), w=w, b=b, H=cfg.hidden, regime="random")
        y, bound = head_expected(d)
        got = bf16_values(bits[i, :n - 1])
        assert np.all(np.isfinite(got))
        worst = max(worst, float((np.abs(got - y[1:n]) / bound[1:n]).max()))
    print(f"forward_colbert {name} dense head: worst |got - ref| / bound = {worst:.3g}")
    assert worst <= 1.0


def test_encode_into_a_store_in_input_order(gpu):
    """encode_colbert_into takes the inputs a window at a time in input order: the store then holds, document for document, what
    encode_colbert gives for each window, and the dense rows come back in input order too."""
    import torch
    from hiprag import MultiVectorStore
    enc, cfg, toks, heads, _, _ = setup("h128")
    enc.set_colbert_head(torch.from_numpy(heads["perm"][0]), torch.from_numpy(heads["perm"][1]))
    store = MultiVectorStore(cfg.hidden, max_doc_vectors=100)             # 130 tokens: 129 vectors, cut to the cap
    dense = enc.encode_colbert_into(store, toks, batch_size=2, window=3).cpu().numpy()
    off, vecs = store.export()
    want_dense, want_rows, want_counts = [], [], []
    for o in range(0, len(toks), 3):
        d, v, c = enc.encode_colbert(toks[o:o + 3], batch_size=2)
        want_dense.append(d.cpu().numpy())
        bits = v.cpu().view(torch.int16).numpy().view(np.uint16)
        for i, n in enumerate(c.tolist()):
            want_counts.append(min(n, 100))
            want_rows.append(bits[i, :min(n, 100)])
    assert want_counts == [min(max(0, n - 1), 100) for n in LENS]
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(want_counts)]))
    assert np.array_equal(vecs, np.concatenate(want_rows))
    assert np.array_equal(dense.view(np.uint32), np.concatenate(want_dense).view(np.uint32))


def test_forward_refusals_and_null_dense(gpu):
    import torch
    from hiprag import EncoderConfig, HipEncoder, random_state
    from hiprag import _native as nat
    from hiprag.index import _stream_ptr
    cfg = EncoderConfig(vocab=48, max_pos=200, max_seq_len=192, **CONFIGS["h128"])
    enc = HipEncoder(cfg, random_state(cfg, seed=SEED))
    assert not enc.has_colbert
    ids, lens = np.asarray([[0, 5, 2]], np.int32), np.asarray([3], np.int32)
    pv = torch.from_numpy(np.full((1, 2, 128), FILL16, np.uint16).view(np.int16)).cuda()
    pc = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    pd = torch.full((1, 128), 7.0, device="cuda")

    def forward(max_len=3, vecs=pv, counts=pc, dense=None, lens_=lens, ids_=ids):
        nat.call("hipenc_forward_colbert", enc._h, ids_.ctypes.data, lens_.ctypes.data, 1, max_len, dense.data_ptr() if dense is not None else None,
                 vecs.data_ptr() if vecs is not None else None, counts.data_ptr() if counts is not None else None, _stream_ptr())

    with pytest.raises(nat.HipRagError) as e:     # no head set
        forward()
    assert e.value.code == E_INVALID
    with pytest.raises(ValueError):
        enc.encode_colbert([[0, 5, 2]])
    w, b = _heads(128)["perm"]
    with pytest.raises(nat.HipRagError):
        nat.call("hipenc_set_colbert_head", enc._h, None, None)
    with pytest.raises(ValueError):
        enc.set_colbert_head(torch.zeros(128, 64), torch.zeros(128))
    enc.set_colbert_head(torch.from_numpy(w), torch.from_numpy(b))
    assert enc.has_colbert
    bad = [dict(max_len=1), dict(max_len=0), dict(vecs=None), dict(counts=None), dict(max_len=400),                 # the position table
           dict(lens_=np.asarray([4], np.int32)), dict(ids_=np.asarray([[0, 48, 2]], np.int32))]                    # hipenc_forward's checks
    for kw in bad:
        with pytest.raises(nat.HipRagError) as e:
            forward(**kw)
        assert e.value.code == E_INVALID, kw
    torch.cuda.synchronize()
    assert bool((pv.view(torch.int16) == pv.view(torch.int16)[0, 0, 0]).all()) and int(pc[0]) == 7, "a refused call wrote its outputs"
    forward(dense=pd)
    torch.cuda.synchronize()
    with_dense = pv.clone()
    assert int(pc[0]) == 2 and not bool((pd == 7.0).any())
    forward()                                      # out_dense_dev = NULL: the vectors alone, the same bits
    torch.cuda.synchronize()
    assert torch.equal(pv, with_dense)
    enc.close()
