"""
CPU: the references of the ColBERT head and of MaxSim (hiprag.colbert) against float64, and the proof that the GPU tests'
checks can fail -- every mutant of tests/colbert_cases.py differs in bits in the exact regime or misses the bound by at least
3 x in the random one.  No GPU, no native call.
"""
import numpy as np
import pytest

from colbert_cases import (HEAD_MUTANTS, MAXSIM_MUTANTS, head_data, head_expected, head_layout, layout_bound, layout_ratio,
                           maxsim_expected, maxsim_vectors, score_ratio, select_expected)
from oracle.linear_cases import bf16_bits, bf16_values, hulp16

LENS = (0, 1, 2, 63, 64)
S = 64


def test_maxsim_reference_on_hand_made_vectors():
    from hiprag.colbert import maxsim_reference
    q = np.asarray([[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]])
    d = np.asarray([[3.0, 0.0], [0.0, -1.0], [1.0, 1.0], [-5.0, -5.0]])
    # q0: max(3, 0, 1, -5) = 3; q1: max(0, -2, 2, -10) = 2; q2: max(3, -1, 2, -10) = 3
    assert maxsim_reference(q, d) == (3.0 + 2.0 + 3.0) / 3.0
    assert maxsim_reference(q[:1], d[1:2]) == 0.0
    assert maxsim_reference(q, d[3:]) == (-5.0 - 10.0 - 10.0) / 3.0          # a maximum may be negative: no clamp at zero
    with pytest.raises(AssertionError):
        maxsim_reference(q, d[:0])


@pytest.mark.parametrize("H", (128, 256))
def test_colbert_reference_against_float64(H):
    from hiprag.colbert import colbert_reference
    d = head_data("random", 64, H)
    y, bound = head_expected(d)
    for splits in (1, 2):
        got = colbert_reference(d["x"], d["w"], d["b"], splits=splits).astype(np.float64)
        r = float((np.abs(got - y) / bound).max())
        print(f"colbert_reference H {H} splits {splits}: worst |ref32 - ref64| / bound = {r:.3g}")
        assert r <= 1.0
        assert np.all(np.abs(np.linalg.norm(got, axis=1) - 1.0) < 2.0 ** -8)
    e = head_data("exact", 64, H)
    a = colbert_reference(e["x"], e["w"], e["b"], splits=1)
    assert np.array_equal(a, colbert_reference(e["x"], e["w"], e["b"], splits=2))     # exact sums: no order, no split
    y64, _ = head_expected(e)
    assert np.all(np.abs(a - y64) <= hulp16(np.abs(y64) + 1e-6) + 1e-6)               # and it is the same function
    # a zero row has no direction: 0 * (1 / 1e-12) = 0, no NaN
    z = colbert_reference(np.zeros((1, H)), e["w"], np.zeros(H))
    assert np.all(z == 0)


@pytest.mark.parametrize("mutant", HEAD_MUTANTS)
@pytest.mark.parametrize("regime", ("exact", "random"))
def test_head_mutants_fail(regime, mutant):
    d = head_data(regime, len(LENS) * S, 128)
    y, bound = head_expected(d)
    want, counts = head_layout(y, LENS, S, S - 1)
    lb = layout_bound(bound, LENS, S, S - 1)
    assert layout_ratio(bf16_bits(want).reshape(want.shape), want, lb) <= 1.0       # the correct image passes
    my, _ = head_expected(d, mutant if mutant == "no_normalisation" else None)
    mout, mcounts = head_layout(my, LENS, S, S - 1, mutant if mutant != "no_normalisation" else None)
    r = layout_ratio(bf16_bits(mout).reshape(want.shape), want, lb)
    print(f"head mutant {mutant} ({regime}): ratio {r:.3g}, counts {mcounts.tolist()} vs {counts.tolist()}")
    assert r >= 3.0
    if mutant != "no_normalisation":
        assert not np.array_equal(counts, mcounts)


@pytest.mark.parametrize("mutant", MAXSIM_MUTANTS)
@pytest.mark.parametrize("regime", ("exact", "random"))
def test_maxsim_mutants_fail(regime, mutant):
    from hiprag.colbert import maxsim_reference
    worst = np.inf
    for lq, ld in ((31, 33), (33, 127), (65, 5)):
        q, d = maxsim_vectors(regime, lq, 128, 1), maxsim_vectors(regime, ld, 128, 2)
        if mutant == "padding_in_max":
            q, d = np.abs(q), -np.abs(d)                   # zero rows change a maximum only where it is negative
        want, bound = maxsim_expected(q, d, regime)
        assert want == maxsim_reference(q, d)
        assert score_ratio(np.float32(want), want, bound) <= 1.0
        got, _ = maxsim_expected(q, d, regime, mutant, pad_rows=(-ld) % 32)
        worst = min(worst, score_ratio(np.float32(got), want, bound))
    print(f"maxsim mutant {mutant} ({regime}): smallest ratio {worst:.3g}")
    assert worst >= 3.0


def test_padding_rows_matter_only_for_negative_maxima():
    """The case the mutant `padding_in_max` needs: every q_i . d_j negative, so a zero row would win the maximum."""
    q = np.abs(maxsim_vectors("random", 5, 128, 3))
    d = -np.abs(maxsim_vectors("random", 33, 128, 4))
    want, bound = maxsim_expected(q, d, "random")
    got, _ = maxsim_expected(q, d, "random", "padding_in_max", pad_rows=31)
    assert want < 0 and got == 0.0 and score_ratio(np.float32(got), want, bound) >= 3.0


def test_selection_rule():
    from colbert_cases import NEG_MAX as NEG
    scores = np.asarray([0.5, 0.7, 0.5, NEG, 0.7, 0.1], dtype=np.float32)
    cand = np.asarray([10, 11, 10, -1, 12, 13], dtype=np.int64)
    valid = np.asarray([True, True, True, False, True, True])
    sc, ids, pos = select_expected(scores, cand, valid, 6)
    assert ids.tolist() == [11, 12, 10, 10, 13, -1] and pos.tolist() == [1, 4, 0, 2, 5, -1]
    assert sc[-1] == np.float32(NEG) and sc[0] == np.float32(0.7)
    sc, ids, pos = select_expected(scores, cand, valid, 1)
    assert ids.tolist() == [11] and pos.tolist() == [1]


def test_bf16_helpers_round_trip():
    from hiprag.colbert import bf16_bits as pb, bf16_values as pv
    x = np.asarray([0.0, 1.0, -2.5, 3.1415926, 1e-3, 65504.0], dtype=np.float32)
    assert np.array_equal(pb(x), bf16_bits(x)) and np.array_equal(pv(pb(x)).astype(np.float64), bf16_values(bf16_bits(x)))
    assert np.array_equal(pb(pv(pb(x))), pb(x))


# ---- the drop-in's bookkeeping and settings (no GPU) ----------------------------------------------------------------------------
def test_manifest_names_the_store_only_when_there_is_one(tmp_path):
    from rag.storage.hip_index.collection import CollectionManifest
    m = CollectionManifest(128, "ip")
    m.add_document("a", "red", 3)
    plain = m.to_json()
    assert "mv" not in plain                                    # a collection that never heard of the flag: byte for byte as before
    m.mv = {"dim": 128}
    m.save(tmp_path / "m.json")
    back = CollectionManifest.load(tmp_path / "m.json")
    assert back.mv == {"dim": 128} and back.rows == 3 and back.to_json() == dict(plain, mv={"dim": 128})
    assert CollectionManifest(128, "ip", plain["documents"]).mv is None


class _FakeStore:
    def __init__(self, n):
        self.n, self.dim = n, 128

    def __len__(self):
        return self.n


class _FakeIndex:
    ntotal, d, metric = 0, 128, 0


def test_a_collection_takes_token_vectors_for_every_document_or_for_none(tmp_path):
    from rag.storage.hip_index.collection import Collection, CollectionManifest
    some = (np.zeros((2, 3, 128)), np.zeros(2, np.int32))
    empty = Collection(tmp_path, CollectionManifest(128, "ip"), _FakeIndex())
    empty._check_colbert(None)
    empty._check_colbert(some)                                   # an empty collection may start a store
    held = CollectionManifest(128, "ip")
    held.add_document("a", "red", 3)
    plain = Collection(tmp_path, held, _FakeIndex())
    assert plain.manifest.mv is None
    plain._check_colbert(None)
    with pytest.raises(RuntimeError, match="without per-token vectors"):
        plain._check_colbert(some)
    late = Collection(tmp_path, held, _FakeIndex(), mv=_FakeStore(3))
    assert late.manifest.mv == {"dim": 128}
    late._check_colbert(some)
    with pytest.raises(RuntimeError, match="keeps per-token vectors"):
        late._check_colbert(None)
    with pytest.raises(RuntimeError, match="holds 2 documents"):
        Collection(tmp_path, held, _FakeIndex(), mv=_FakeStore(2))._check_colbert(some)


def test_config_combinations(monkeypatch):
    from rag.config import config
    for name in ("HIP_LATE_INTERACTION", "HIP_COLLECTION", "HIP_RERANK"):
        monkeypatch.delenv(name, raising=False)
    assert config.HIP_LATE_INTERACTION is False                  # off by default
    monkeypatch.setenv("HIP_RERANK", "true")
    assert config.HIP_LATE_INTERACTION is False                  # and then nothing is checked
    monkeypatch.setenv("HIP_LATE_INTERACTION", "true")
    with pytest.raises(ValueError, match="HIP_COLLECTION"):
        config.HIP_LATE_INTERACTION
    monkeypatch.setenv("HIP_COLLECTION", "true")
    with pytest.raises(ValueError, match="two second stages"):
        config.HIP_LATE_INTERACTION
    monkeypatch.setenv("HIP_RERANK", "false")
    assert config.HIP_LATE_INTERACTION is True                   # read at use
    import asyncio
    import rag.query.retriever as rt
    with pytest.raises(ValueError, match="two second stages"):
        rt.HybridRetriever(rerank=True)._late_interaction()
    assert rt.HybridRetriever(rerank=False)._late_interaction() is True

    class NoHead:
        pass
    with pytest.raises(RuntimeError, match="ColBERT head"):
        asyncio.run(rt._embed_query_colbert(NoHead(), "q"))
    with pytest.raises(RuntimeError, match="per-token vectors"):
        rt._multivec_of(None)
