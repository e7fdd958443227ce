"""
Every selection kernel behind csrc/topk_device.h against the oracle, BIT FOR BIT, on inputs designed to sit on its
dispatch boundaries (oracle/select_cases.py; tests/test_select_cases_cpu.py shows that these cases tell a right kernel
from the listed subtly wrong ones):

  * hiprag_merge_topk_dev: the four wave forms (NPL 1, 2, 4, 8) and the streaming form at one, two, three, four, five
    and 4905 tiles, both metrics, with ties, k-th-place plateaus, padding that would win, duplicates, +-DBL_MAX / +-inf /
    denormals, signed zeros, and winning garbage in the gap between strided parts;
  * hiprrf_fuse / hiprrf_fuse_dev: empty lists (null pointers), repeated ids, holes, ids near 2^62, padding ranks, zero and
    negative weights;
  * the BM25 selectors (tile selector of taat_tile_kernel, select_wave_kernel, select_f32_kernel + bm25_finish_kernel and
    the packed merge behind the first two), driven with chosen fp32 accumulators through one-term postings.

The oracle is the specification; nothing here takes a tolerance.  Each test prints one line (pytest -s): case, size, kernel.
"""
import ctypes

import numpy as np
import pytest

from oracle import hybrid_oracle as ho
from oracle import select_cases as sc

pytestmark = pytest.mark.gpu

DBL_MAX = np.finfo(np.float64).max
FLT_MAX = np.finfo(np.float32).max


# ---------------------------------------------------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------------------------------------------------
def _merge_inputs(case):
    """The case's buffers on the GPU and the strided [n_parts, nq, k_in] views of them (the gap lies between the parts)."""
    import torch
    spec = case.spec
    sbuf = torch.from_numpy(case.scores).cuda()
    ibuf = torch.from_numpy(case.ids).cuda()
    shape, strides = (spec.n_parts, spec.nq, spec.k_in), (spec.part_stride, spec.k_in, 1)
    return sbuf, ibuf, torch.as_strided(sbuf, shape, strides), torch.as_strided(ibuf, shape, strides)


@pytest.mark.parametrize("spec", sc.merge_gpu_cases(), ids=lambda s: s.name)
def test_merge_every_dispatch_shape(gpu, spec):
    import torch
    from hiprag import merge_topk_device
    case = sc.build_merge_case(spec)
    es, ei = case.oracle()
    sbuf, ibuf, sv, iv = _merge_inputs(case)
    metric = "ip" if spec.metric == ho.METRIC_IP else "l2"
    print("merge %-36s M=%-5d k_out=%-4d kernel=%s" % (spec.name, spec.M, spec.k_out, spec.kernel))
    assert sc.merge_kernel_shape(spec.n_parts, spec.k_in, spec.k_out) == spec.kernel
    runs = []
    for _ in range(2):
        m64, m32, mids = merge_topk_device(sv, iv, spec.k_out, metric)
        torch.cuda.synchronize()
        runs.append((m64.cpu().numpy(), m32.cpu().numpy(), mids.cpu().numpy()))
    g64, g32, gi = runs[0]
    assert np.array_equal(gi, ei)
    assert np.array_equal(g64, es)
    pad = gi == -1
    with np.errstate(over="ignore"):
        assert np.array_equal(g32[~pad], g64[~pad].astype(np.float32))
    sgn = -1.0 if spec.metric == ho.METRIC_IP else 1.0
    assert (g64[pad] == sgn * DBL_MAX).all() and (g32[pad] == np.float32(sgn) * FLT_MAX).all()
    assert int(pad.sum()) == int((ei == -1).sum())
    # a second call gives the same bits (signed zeros and all)
    for a, b in zip(runs[0], runs[1]):
        assert a.tobytes() == b.tobytes()
    # the call reads, never writes, its inputs
    assert np.array_equal(sbuf.cpu().numpy(), case.scores) and np.array_equal(ibuf.cpu().numpy(), case.ids)


def test_merge_largest_k_out_over_9000_candidates(gpu):
    """M = 9000 at k_out = 4095: 4905 tiles of one fresh candidate each, 4095 selection rounds per tile -- about 40 s per
    launch on an MI355X however many queries it holds.  So all cases of the shape go into ONE launch per metric (the
    patterns stacked along the query axis, each block of nq queries checked against its own oracle), and the two calls of
    each metric run side by side on four streams: every check of test_merge_every_dispatch_shape, for every case, in the
    time of one launch."""
    import torch
    from hiprag import merge_topk_device
    specs = sc.merge_batched_gpu_cases()
    assert {(s.n_parts, s.k_in, s.k_out) for s in specs} == {(9, 1000, 4095)}
    jobs = []
    for metric in (ho.METRIC_IP, ho.METRIC_L2):
        cases = [sc.build_merge_case(s) for s in specs if s.metric == metric]
        sp = cases[0].spec
        scores, ids, stride = sc.stack_merge_cases(cases)
        sbuf, ibuf = torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda()
        shape, strides = (sp.n_parts, len(cases) * sp.nq, sp.k_in), (stride, sp.k_in, 1)
        sv, iv = torch.as_strided(sbuf, shape, strides), torch.as_strided(ibuf, shape, strides)
        jobs.append((metric, cases, scores, ids, sbuf, ibuf, sv, iv))
    torch.cuda.synchronize()
    outs = []
    for metric, cases, scores, ids, sbuf, ibuf, sv, iv in jobs:
        for _ in range(2):
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                outs.append(merge_topk_device(sv, iv, 4095, "ip" if metric == ho.METRIC_IP else "l2"))
    torch.cuda.synchronize()
    for j, (metric, cases, scores, ids, sbuf, ibuf, sv, iv) in enumerate(jobs):
        first, second = ([t.cpu().numpy() for t in outs[2 * j + c]] for c in (0, 1))
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()
        assert np.array_equal(sbuf.cpu().numpy(), scores) and np.array_equal(ibuf.cpu().numpy(), ids)
        sgn = -1.0 if metric == ho.METRIC_IP else 1.0
        for c, case in enumerate(cases):
            sp = case.spec
            print("merge %-36s M=%-5d k_out=%-4d kernel=%s" % (sp.name, sp.M, sp.k_out, sp.kernel))
            g64, g32, gi = (t[c * sp.nq:(c + 1) * sp.nq] for t in first)
            es, ei = case.oracle()
            assert np.array_equal(gi, ei), sp.name
            assert np.array_equal(g64, es), sp.name
            pad = gi == -1
            with np.errstate(over="ignore"):
                assert np.array_equal(g32[~pad], g64[~pad].astype(np.float32)), sp.name
            assert (g64[pad] == sgn * DBL_MAX).all() and (g32[pad] == np.float32(sgn) * FLT_MAX).all(), sp.name


@pytest.mark.parametrize("shape", [(3, 43, 10), (27, 19, 10)], ids=["wave", "stream"])
def test_merge_c_abi_optional_output_and_empty_batch(gpu, shape):
    """hiprag_merge_topk_dev itself: out_scores_dev may be null (the header allows it), and nq = 0 returns OK and writes
    nothing, on both kernel forms."""
    import torch
    from hiprag import _native
    n_parts, k_in, k_out = shape
    spec = sc.MergeSpec(n_parts, sc.MERGE_NQ, k_in, k_out, 7, ho.METRIC_L2, "levels", sc.merge_kernel_shape(*shape))
    case = sc.build_merge_case(spec)
    es, ei = case.oracle()
    sbuf, ibuf, sv, iv = _merge_inputs(case)
    o64 = torch.full((spec.nq, k_out), 123.0, dtype=torch.float64, device="cuda")
    oid = torch.full((spec.nq, k_out), 456, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.call("hiprag_merge_topk_dev", sv.data_ptr(), iv.data_ptr(), n_parts, 0, k_in, k_out, spec.part_stride,
                 _native.METRIC_L2, o64.data_ptr(), None, oid.data_ptr(), stream)
    torch.cuda.synchronize()
    assert (o64 == 123.0).all() and (oid == 456).all()
    _native.call("hiprag_merge_topk_dev", None, None, n_parts, 0, k_in, k_out, 0, _native.METRIC_L2, None, None, None, stream)
    _native.call("hiprag_merge_topk_dev", sv.data_ptr(), iv.data_ptr(), n_parts, spec.nq, k_in, k_out, spec.part_stride,
                 _native.METRIC_L2, o64.data_ptr(), None, oid.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(oid.cpu().numpy(), ei) and np.array_equal(o64.cpu().numpy(), es)


def test_merge_refuses_bad_shapes(gpu):
    import torch
    from hiprag import HipRagError, _native
    s = torch.zeros((2, 5, 8), dtype=torch.float64, device="cuda")
    i = torch.zeros((2, 5, 8), dtype=torch.int64, device="cuda")
    o64 = torch.zeros((5, 4096), dtype=torch.float64, device="cuda")
    oid = torch.zeros((5, 4096), dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(k_out=10, part_stride=40, metric=_native.METRIC_IP):
        _native.call("hiprag_merge_topk_dev", s.data_ptr(), i.data_ptr(), 2, 5, 8, k_out, part_stride, metric, o64.data_ptr(),
                     None, oid.data_ptr(), stream)

    call()
    call(k_out=4095)
    with pytest.raises(HipRagError):
        call(k_out=4096)
    with pytest.raises(HipRagError):
        call(part_stride=39)
    with pytest.raises(HipRagError):
        call(metric=2)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# RRF
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", sc.rrf_cases(), ids=lambda s: s.name)
def test_rrf_every_depth_shape(gpu, spec):
    import torch
    from hiprag import _native, rrf_fuse, rrf_fuse_device
    a, b = sc.build_rrf_case(spec)
    es, ei = ho.rrf_fuse(a, b, spec.k, spec.c, spec.w_a, spec.w_b)
    print("rrf   %-40s n=%-4d kernel=rrf_kernel" % (spec.name, spec.depth_a + spec.depth_b))
    hs, hi = rrf_fuse(a, b, spec.k, spec.c, spec.w_a, spec.w_b)
    assert np.array_equal(hi, ei) and np.array_equal(hs, es)
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ds, di = rrf_fuse_device(ad, bd, spec.k, spec.c, spec.w_a, spec.w_b)
    torch.cuda.synchronize()
    assert np.array_equal(di.cpu().numpy(), ei) and np.array_equal(ds.cpu().numpy(), es)
    if spec.depth_a == 0 or spec.depth_b == 0:      # the host entry point with a null pointer for the empty list
        s2 = np.empty((spec.nq, spec.k), dtype=np.float32)
        i2 = np.empty((spec.nq, spec.k), dtype=np.int64)
        _native.call("hiprrf_fuse", a.ctypes.data if spec.depth_a else None, b.ctypes.data if spec.depth_b else None, spec.nq,
                     spec.depth_a, spec.depth_b, spec.k, spec.c, spec.w_a, spec.w_b, s2.ctypes.data, i2.ctypes.data)
        assert np.array_equal(i2, ei) and np.array_equal(s2, es)
        ds.fill_(0), di.fill_(0)                    # and the device entry point
        _native.call("hiprrf_fuse_dev", ad.data_ptr() if spec.depth_a else None, bd.data_ptr() if spec.depth_b else None, spec.nq,
                     spec.depth_a, spec.depth_b, spec.k, spec.c, spec.w_a, spec.w_b, ds.data_ptr(), di.data_ptr(),
                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert np.array_equal(di.cpu().numpy(), ei) and np.array_equal(ds.cpu().numpy(), es)


def test_rrf_refuses_bad_shapes(gpu):
    from hiprag import HipRagError, rrf_fuse
    a = np.arange(2049, dtype=np.int64)[None]
    b = np.arange(2048, dtype=np.int64)[None]
    rrf_fuse(a[:, :2048], b, 5)
    with pytest.raises(HipRagError):
        rrf_fuse(a, b, 5)                       # depth sum 4097
    with pytest.raises(HipRagError):
        rrf_fuse(a[:, :7], b[:, :7], 5, c=-1.0)   # c + rank must stay positive


# ---------------------------------------------------------------------------------------------------------------------
# BM25 selectors
# ---------------------------------------------------------------------------------------------------------------------
_BM25_KERNELS = {"tiled": "taat_tile_kernel selector + merge_packed_kernel", "global": "select_wave_kernel + merge_packed_kernel",
                 "f32": "select_f32_kernel + bm25_finish_kernel"}


@pytest.mark.parametrize("spec,path", [(s, p) for s in sc.bm25_select_cases() for p in s.paths],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_bm25_selectors_on_designed_accumulators(gpu, monkeypatch, spec, path):
    import torch
    from hiprag import HipBM25, PostingsCSR
    acc = sc.bm25_accumulators(spec)
    p = sc.bm25_postings(acc)
    es, ei = ho.bm25_search(p, sc.BM25_QUERY, spec.k)
    print("bm25  %-32s n_docs=%-5d kernel=%s" % (spec.name, spec.n_docs, _BM25_KERNELS[path]))
    if path == "global":
        monkeypatch.setenv("HIPBM25_GLOBAL_ACC", "1")     # read when the index is created
    else:
        monkeypatch.delenv("HIPBM25_GLOBAL_ACC", raising=False)
    ix = HipBM25(PostingsCSR(p.n_docs, p.n_terms, p.offsets, p.doc_ids, p.impacts))
    try:
        s, i = ix.search(sc.BM25_QUERY, spec.k)
        assert np.array_equal(i, ei)
        assert np.array_equal(s, es)
        d64, d32, di = ix.search_device(sc.BM25_QUERY, spec.k)
        torch.cuda.synchronize()
        assert np.array_equal(di.cpu().numpy(), ei) and np.array_equal(d32.cpu().numpy(), es)
        e64 = np.where(ei >= 0, es.astype(np.float64), -DBL_MAX)
        assert np.array_equal(d64.cpu().numpy(), e64)
        ix.set_id_base(7)
        bs, bi = ho.topk_desc_id_asc(acc, spec.k, exclude_nonpositive=True, id_base=7)
        s7, i7 = ix.search(sc.BM25_QUERY, spec.k)
        assert np.array_equal(i7[0], bi) and np.array_equal(s7[0], bs)
    finally:
        ix.close()
