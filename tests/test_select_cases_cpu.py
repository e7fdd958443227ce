"""
The designed selection cases of oracle/select_cases.py can tell right from wrong -- checked without a GPU.

tests/test_selection_gpu.py compares every selection kernel bit for bit with the oracle on these cases.  That is only
worth something if a subtly wrong kernel would give a different answer on at least one of them, so here every listed
WRONG VARIANT of the merge, of RRF and of the BM25 selection is written out in a few lines of numpy, run on every case,
and must differ from the oracle somewhere; the cases that catch each variant are printed (pytest -s).  The structural
claims of the generators (which kernel shape a merge case selects, that a plateau really straddles its boundary) are
asserted too.
"""
import bisect
import functools
import math

import numpy as np
import pytest

from oracle import hybrid_oracle as ho
from oracle import select_cases as sc

F32_MIN_NORMAL = np.finfo(np.float32).tiny


def _report(title, caught):
    for variant, names in caught.items():
        print("%s / %-28s caught by %4d cases, e.g. %s" % (title, variant, len(names), ", ".join(names[:3])))
    missed = [v for v, names in caught.items() if not names]
    assert not missed, "no case catches: %s" % missed


# ---------------------------------------------------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _merge_case(spec):
    """Built once, shared by the tests below, never modified."""
    case = sc.build_merge_case(spec)
    return case, case.oracle()


def _pad(sel_s, sel_i, k, metric):
    out_s = np.full(k, -sc.DBL_MAX if metric == ho.METRIC_IP else sc.DBL_MAX)
    out_i = np.full(k, -1, dtype=np.int64)
    out_s[:len(sel_s)], out_i[:len(sel_i)] = sel_s, sel_i
    return out_s, out_i


def _canon(s, i, k, metric):
    order = np.lexsort((i, -s if metric == ho.METRIC_IP else s))[:k]
    return s[order], i[order]


def _merge_variant(case, variant):
    spec = case.spec
    k, metric, nq, k_in = spec.k_out, spec.metric, spec.nq, spec.k_in
    if variant == "part_stride_ignored":
        fs, fi = case.scores.reshape(-1), case.ids.reshape(-1)
        n = nq * k_in
        S = np.concatenate([fs[p * n:(p + 1) * n].reshape(nq, k_in) for p in range(spec.n_parts)], axis=1)
        I = np.concatenate([fi[p * n:(p + 1) * n].reshape(nq, k_in) for p in range(spec.n_parts)], axis=1)
    else:
        S, I = case.flat()
    out_s, out_i = np.empty((nq, k)), np.empty((nq, k), dtype=np.int64)
    for q in range(nq):
        s, i = S[q], I[q]
        if variant in ("truncated_512", "truncated_4096"):
            n = 512 if variant == "truncated_512" else 4096
            s, i = s[:n], i[:n]
        if variant != "padding_ranked":
            keep = i >= 0
            s, i = s[keep], i[keep]
        g = s if metric == ho.METRIC_IP else -s
        if variant == "tie_to_input_order":
            order = np.argsort(-g, kind="stable")[:k]
            rs, ri = s[order], i[order]
        elif variant == "negative_zero_below":
            order = np.lexsort((i, np.signbit(g), -g))[:k]     # the order of the integer image of g: +0.0 before -0.0
            rs, ri = s[order], i[order]
        elif variant == "carry_k_minus_1":
            # the streaming selection, tile by tile, with one winner too few carried into each next tile
            ent = sorted(zip((-g[:sc.MERGE_TILE]).tolist(), i[:sc.MERGE_TILE].tolist(), s[:sc.MERGE_TILE].tolist()))[:k]
            o = sc.MERGE_TILE
            while o < len(s):
                take = sc.MERGE_TILE - k
                del ent[k - 1:]
                for e in zip((-g[o:o + take]).tolist(), i[o:o + take].tolist(), s[o:o + take].tolist()):
                    bisect.insort(ent, e)
                del ent[k:]
                o += take
            rs, ri = np.asarray([e[2] for e in ent]), np.asarray([e[1] for e in ent], dtype=np.int64)
        elif variant == "duplicates_collapsed":
            _, first = np.unique(np.stack([g, i.astype(np.float64)]), axis=1, return_index=True)
            rs, ri = _canon(s[np.sort(first)], i[np.sort(first)], k, metric)
        else:
            rs, ri = _canon(s, i, k, metric)
        out_s[q], out_i[q] = _pad(rs, ri, k, metric)
    return out_s, out_i


MERGE_VARIANTS = ("tie_to_input_order", "negative_zero_below", "part_stride_ignored", "padding_ranked", "truncated_512",
                  "truncated_4096", "carry_k_minus_1", "duplicates_collapsed")


def test_merge_shapes_select_the_stated_kernels():
    """Every case names the kernel shape it was built for; the dispatch rule restated in merge_kernel_shape agrees, and the
    set covers all four wave forms, the one-tile form on both sides of its edges and the multi-tile carry."""
    seen = set()
    for n_parts, k_in, k_out, gap, kernel in sc.MERGE_SHAPES:
        M = n_parts * k_in
        assert sc.merge_kernel_shape(n_parts, k_in, k_out) == kernel, (n_parts, k_in, k_out)
        assert kernel.startswith("wave/") == (k_out <= 64 and M <= 512)
        assert 0 < k_out < sc.MERGE_TILE
        seen.add((kernel, M, k_out))
    kernels = {k for k, _, _ in seen}
    assert {"wave/NPL1", "wave/NPL2", "wave/NPL4", "wave/NPL8", "stream/1", "stream/2", "stream/3", "stream/4"} <= kernels
    wave_m = {M for k, M, _ in seen if k.startswith("wave/")}
    assert wave_m == {1, 63, 64, 65, 128, 129, 256, 257, 511, 512}
    for M in wave_m:
        assert {ko for k, m, ko in seen if m == M and k.startswith("wave/")} == {1, 10, 64}
    stream = {(M, ko) for k, M, ko in seen if k.startswith("stream/")}
    assert {(513, 10), (64, 65), (40, 100), (4095, 10), (4096, 100), (4097, 10), (2 * 4096 - 256 + 1, 256), (3 * 4096, 256),
            (9000, 4095), (4100, 4095)} <= stream
    # the GPU test runs every case: the one shape whose launch takes most of a minute batched, all others one by one
    assert sorted(s.name for s in sc.merge_gpu_cases() + sc.merge_batched_gpu_cases()) == sorted(s.name for s in sc.merge_cases())
    assert {(s.n_parts, s.k_in, s.k_out) for s in sc.merge_batched_gpu_cases()} == {(9, 1000, 4095)}
    # the third tile of the 7937-candidate shape holds exactly one entry
    assert (2 * 4096 - 256 + 1) - 4096 - (4096 - 256) == 1
    specs = sc.merge_cases()
    assert {s.metric for s in specs} == {ho.METRIC_IP, ho.METRIC_L2} and all(s.nq == 5 for s in specs)
    for shape in sc.MERGE_SHAPES:
        for metric in (ho.METRIC_IP, ho.METRIC_L2):
            pats = {s.pattern for s in specs if (s.n_parts, s.k_in, s.k_out, s.gap, s.kernel) == shape and s.metric == metric}
            assert pats == {p for p in sc.MERGE_PATTERNS if sc.merge_pattern_fits(p, *shape[:3])}
    print("merge: %d cases over %d shapes" % (len(specs), len(sc.MERGE_SHAPES)))


def test_merge_cases_are_what_they_claim():
    for spec in sc.merge_cases():
        case, (es, ei) = _merge_case(spec)
        S, I = case.flat()
        assert S.shape == (spec.nq, spec.M) and not np.isnan(case.scores).any()
        assert case.scores.shape == (spec.n_parts, spec.part_stride)
        if spec.gap:
            gs, gi = case.scores[:, spec.nq * spec.k_in:], case.ids[:, spec.nq * spec.k_in:]
            assert (gi >= sc.GAP_ID_BASE).all() and (np.abs(gs) == 1e308).all()
        assert (ei < sc.GAP_ID_BASE).all()
        if spec.pattern == "levels":      # rank k_out lies inside a plateau whose members are in and out, over the parts
            for q in range(spec.nq):
                kth = es[q, spec.k_out - 1]
                members = np.flatnonzero(S[q] == kth)
                assert len(members) > int((es[q] == kth).sum()) >= 1
                assert len(set(members // spec.k_in)) == min(spec.n_parts, len(members))
        if spec.pattern == "pad":
            assert (ei[0] == -1).all() and (I[0] == -1).all()
            assert (I == -1).mean() > 0.25
            if spec.n_parts >= 2:
                p = spec.n_parts // 2
                assert (I[:, p * spec.k_in:(p + 1) * spec.k_in] == -1).all()
        if spec.pattern == "dup":
            for q in range(spec.nq):
                pairs = list(zip(S[q].tolist(), I[q].tolist()))
                assert len(set(pairs)) < len(pairs)
        if spec.pattern == "zeros":
            for q in range(spec.nq):
                z = np.flatnonzero(S[q] == 0.0)
                if len(z) >= 2:
                    neg = np.signbit(S[q][z])
                    assert neg.any() and neg[np.argmin(I[q][z])]          # the lowest zero id holds -0.0
                if len(z) >= 4:
                    assert not neg.all()


def test_merge_wrong_variants_are_caught():
    caught = {v: [] for v in MERGE_VARIANTS}
    for spec in sc.merge_cases():
        case, (es, ei) = _merge_case(spec)
        vs, vi = _merge_variant(case, "none")
        assert np.array_equal(vi, ei) and np.array_equal(vs, es), spec.name      # the harness itself restates the oracle
        for v in MERGE_VARIANTS:
            vs, vi = _merge_variant(case, v)
            if not (np.array_equal(vi, ei) and np.array_equal(vs, es)):
                caught[v].append(spec.name)
    _report("merge", caught)
    # each boundary-sensitive slip is caught on the kernel shape it would live in
    names = lambda v: " ".join(caught[v])
    assert any("-zeros-" in n or n.startswith("zeros-") for n in caught["negative_zero_below"])
    by_kernel = {}
    for spec in sc.merge_cases():
        by_kernel.setdefault(spec.name, spec.kernel)
    for v in ("tie_to_input_order", "padding_ranked", "negative_zero_below"):
        kernels = {by_kernel[n] for n in caught[v]}
        assert {"wave/NPL1", "wave/NPL2", "wave/NPL4", "wave/NPL8", "stream/1", "stream/2", "stream/3", "stream/4"} <= kernels, (v, kernels)
    assert {by_kernel[n] for n in caught["carry_k_minus_1"]} >= {"stream/2", "stream/3", "stream/4"}, names("carry_k_minus_1")


# ---------------------------------------------------------------------------------------------------------------------
# RRF
# ---------------------------------------------------------------------------------------------------------------------
def _rrf_variant(a, b, spec, variant):
    f32 = np.float32
    k = spec.k
    out_s = np.full((a.shape[0], k), -np.finfo(np.float32).max, dtype=np.float32)
    out_i = np.full((a.shape[0], k), -1, dtype=np.int64)
    for q in range(a.shape[0]):
        ta, tb, pos = {}, {}, {}
        for lst, t, w, off in ((a[q], ta, spec.w_a, 0), (b[q], tb, spec.w_b, len(a[q]))):
            for r, d in enumerate(lst.tolist()):
                if d >= 0 and (variant == "last_occurrence" or d not in t):
                    t[d] = f32(w) / (f32(spec.c) + f32(r + 1))
                if d >= 0:
                    pos.setdefault(d, off + r)
        docs = sorted(set(ta) | set(tb))
        ent = [(f32(ta.get(d, f32(0))) + f32(tb.get(d, f32(0))), d) for d in docs]
        if variant == "both_lists_counted_twice":
            ent += [(f32(0) + tb[d], d) for d in docs if d in ta and d in tb]
        if variant == "zero_scores_dropped":
            ent = [e for e in ent if e[0] != 0]
        if variant == "tie_to_list_order":
            ent.sort(key=lambda e: (-float(e[0]), pos[e[1]]))
        elif variant == "negative_zero_below":
            ent.sort(key=lambda e: (-float(e[0]), bool(np.signbit(e[0])), e[1]))
        else:
            ent.sort(key=lambda e: (-float(e[0]), e[1]))
        ent = ent[:k]
        out_s[q, :len(ent)] = [e[0] for e in ent]
        out_i[q, :len(ent)] = [e[1] for e in ent]
    return out_s, out_i


RRF_VARIANTS = ("last_occurrence", "both_lists_counted_twice", "zero_scores_dropped", "tie_to_list_order", "negative_zero_below")


def test_rrf_cases_cover_the_stated_shapes_and_catch_the_wrong_variants():
    specs = sc.rrf_cases()
    assert {(s.depth_a, s.depth_b) for s in specs} == set(sc.RRF_DEPTHS) | {(2048, 2048)}
    assert sum(1 for s in specs if s.depth_a == 2048) == 1 and max(s.nq for s in specs) <= 5
    assert all(s.depth_a + s.depth_b <= 4096 and s.c + 1.0 > 0 for s in specs)
    for da, db in sc.RRF_DEPTHS:
        assert {s.k for s in specs if (s.depth_a, s.depth_b) == (da, db)} == {1, 10, da + db + 5}
        assert {(s.c, s.w_a, s.w_b) for s in specs if (s.depth_a, s.depth_b) == (da, db)} == set(sc.RRF_WEIGHTS)
    caught = {v: [] for v in RRF_VARIANTS}
    content = {"repeat": 0, "both": 0, "hole": 0, "big": 0, "padded_rank": 0, "zero_score_ranked": 0}
    for spec in specs:
        a, b = sc.build_rrf_case(spec)
        assert a.shape == (spec.nq, spec.depth_a) and b.shape == (spec.nq, spec.depth_b)
        for q in range(spec.nq):
            va, vb = a[q][a[q] >= 0], b[q][b[q] >= 0]
            content["repeat"] += len(set(va.tolist())) < len(va) or len(set(vb.tolist())) < len(vb)
            content["both"] += bool(set(va.tolist()) & set(vb.tolist()))
            content["hole"] += (a[q][1:-1] == -1).any() or (b[q][1:-1] == -1).any()
            content["big"] += max(va.max(initial=0), vb.max(initial=0)) > (1 << 62) - 10 ** 5
        es, ei = ho.rrf_fuse(a, b, spec.k, spec.c, spec.w_a, spec.w_b)
        content["padded_rank"] += bool((ei == -1).any())
        content["zero_score_ranked"] += bool(((es == 0) & (ei >= 0)).any())
        vs, vi = _rrf_variant(a, b, spec, "none")
        assert np.array_equal(vs, es) and np.array_equal(vi, ei), spec.name      # the harness itself restates the oracle
        for v in RRF_VARIANTS:
            vs, vi = _rrf_variant(a, b, spec, v)
            if not (np.array_equal(vi, ei) and np.array_equal(vs, es)):
                caught[v].append(spec.name)
    print("rrf: %d cases; content counts %s" % (len(specs), content))
    assert all(n > 0 for n in content.values()), content
    _report("rrf", caught)


# ---------------------------------------------------------------------------------------------------------------------
# BM25 selectors
# ---------------------------------------------------------------------------------------------------------------------
def _bm25_variant(acc, k, variant):
    acc = acc.copy()
    n = acc.shape[0]
    ids = np.arange(n, dtype=np.int64)
    if variant == "scalar_tail_dropped":
        acc[n - n % 4:] = 0
    if variant == "denormals_as_zero":
        acc[acc < F32_MIN_NORMAL] = 0
    keep = acc > 0
    s, i = acc[keep], ids[keep]
    if variant == "tie_to_higher_id":
        order = np.lexsort((-i, -s.astype(np.float64)))[:k]
    elif variant == "plateau_cut_at_share":
        # every 4096-document share keeps its k best BEFORE ties are resolved by id (here: ties to the higher id), then the
        # survivors are merged with the right comparator.  Any tie inside a share catches it; that the plateau_share cases
        # do -- ties laid across the share boundary -- is asserted by name below
        surv = []
        for s0 in range(0, n, sc.BM25_SHARE):
            m = (i >= s0) & (i < s0 + sc.BM25_SHARE)
            o = np.lexsort((-i[m], -s[m].astype(np.float64)))[:k]
            surv.append(np.flatnonzero(m)[o])
        surv = np.concatenate(surv) if surv else np.zeros(0, dtype=np.int64)
        order = surv[np.lexsort((i[surv], -s[surv].astype(np.float64)))[:k]]
    else:
        order = np.lexsort((i, -s.astype(np.float64)))[:k]
    out_s = np.full(k, -np.finfo(np.float32).max, dtype=np.float32)
    out_i = np.full(k, -1, dtype=np.int64)
    out_s[:len(order)], out_i[:len(order)] = s[order], i[order]
    return out_s[None], out_i[None]


BM25_VARIANTS = ("tie_to_higher_id", "scalar_tail_dropped", "plateau_cut_at_share", "denormals_as_zero")


def test_bm25_cases_are_what_they_claim_and_catch_the_wrong_variants():
    specs = sc.bm25_select_cases()
    assert {s.n_docs for s in specs} == {1, 3, 4095, 4096, 4097, 9215, 9216, 9217, 2 * 9216 + 5, 16386}
    assert {s.k for s in specs} == {1, 33, 50, 64, 65, 200} and max(s.n_docs for s in specs) <= 18437
    assert {s.pattern for s in specs} == set(sc.BM25_PATTERNS)
    caught = {v: [] for v in BM25_VARIANTS}
    straddled = {"plateau_share": set(), "plateau_tile": set(), "plateau_quarter": set()}
    for spec in specs:
        acc = sc.bm25_accumulators(spec)
        assert acc.dtype == np.float32 and acc.shape == (spec.n_docs,) and (acc >= 0).all() and np.isfinite(acc).all()
        p = sc.bm25_postings(acc)
        assert p.n_terms == 1 and np.array_equal(ho.bm25_scores_taat(p, [0]), acc)     # the accumulators ARE the design
        es, ei = ho.bm25_search(p, sc.BM25_QUERY, spec.k)
        n_pos, k = int((acc > 0).sum()), spec.k
        assert int((ei >= 0).sum()) == min(k, n_pos)
        if spec.pattern == "exactly_k":
            assert n_pos == min(k, spec.n_docs)
        if spec.pattern == "k_minus_1":
            assert n_pos == min(k - 1, spec.n_docs) and ei[0, -1] == -1
        if spec.pattern.startswith("plateau_"):
            b = sc.bm25_plateau_boundary(spec.pattern, spec.n_docs)
            unit = {"plateau_share": sc.BM25_SHARE, "plateau_tile": sc.BM25_TILE, "plateau_quarter": sc.BM25_TILE // 4}[spec.pattern]
            assert b % unit == 0 and 0 < b < spec.n_docs
            kth = es[0, k - 1]
            members = np.flatnonzero(acc == kth)
            assert members.min() < b <= members.max()                 # the plateau lies on both sides of the boundary
            assert np.array_equal(members, np.arange(members.min(), members.max() + 1))
            taken = int((es[0] == kth).sum())
            assert 1 <= taken < len(members)                          # rank k falls inside it
            assert (ei[0][es[0] == kth] < b).all()                    # and the winners are the members below the boundary
            straddled[spec.pattern].add(b)
        if spec.pattern == "tail":
            t = spec.n_docs % 4
            assert t and np.array_equal(ei[0, :min(k, t)], np.arange(spec.n_docs - t, spec.n_docs)[:min(k, t)])
        if spec.pattern == "winner_per_share":
            nshare = math.ceil(spec.n_docs / sc.BM25_SHARE)
            top = ei[0, :min(k, nshare)]
            assert len(set((top // sc.BM25_SHARE).tolist())) == len(top)
        if spec.pattern == "denormal":
            assert acc.max() < F32_MIN_NORMAL and (spec.n_docs < 8 or acc.max() > 0)
        if spec.pattern == "flt_max" and spec.n_docs >= 64:
            assert es[0, 0] == np.finfo(np.float32).max
        if spec.pattern == "crowd" and spec.n_docs >= 64:
            kth = es[0, k - 1]
            assert 0.35 <= (acc == kth).mean() <= 0.45 and (acc > kth).sum() < k
        vs, vi = _bm25_variant(acc, spec.k, "none")
        assert np.array_equal(vi, ei) and np.array_equal(vs, es), spec.name      # the harness itself restates the oracle
        for v in BM25_VARIANTS:
            vs, vi = _bm25_variant(acc, spec.k, v)
            if not (np.array_equal(vi, ei) and np.array_equal(vs, es)):
                caught[v].append(spec.name)
    assert {4096, 8192, 16384} <= straddled["plateau_share"] and {9216, 18432} <= straddled["plateau_tile"]
    assert {2304, 6912} <= straddled["plateau_quarter"]
    print("bm25: %d cases" % len(specs))
    _report("bm25", caught)
    assert any(n.startswith("plateau_share") for n in caught["plateau_cut_at_share"])
    assert any(n.startswith("tail") for n in caught["scalar_tail_dropped"])


def test_generators_are_deterministic():
    for spec in (sc.merge_cases()[3], sc.merge_cases()[-1]):
        a, b = sc.build_merge_case(spec), sc.build_merge_case(spec)
        assert a.scores.tobytes() == b.scores.tobytes() and a.ids.tobytes() == b.ids.tobytes()
    spec = sc.rrf_cases()[40]
    assert all(np.array_equal(x, y) for x, y in zip(sc.build_rrf_case(spec), sc.build_rrf_case(spec)))
    spec = sc.bm25_select_cases()[100]
    assert sc.bm25_accumulators(spec).tobytes() == sc.bm25_accumulators(spec).tobytes()
