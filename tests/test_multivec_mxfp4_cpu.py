"""
The MXFP4 format of the multi-vector store on the CPU: hiprag.colbert.mxfp4_quantize_reference (the specification) against its
integer restatement in tests/mxfp4_cases.py, the error bound, exactness of the dequantised values in bf16, the special vectors
-- and the proof that the cases can fail: every mutant of mxfp4_cases differs from the reference on at least one 128-d case
set.  The names of the format in Python and in the setting.  No GPU.
"""
import numpy as np
import pytest

import mxfp4_cases as mc
from oracle.linear_cases import bf16_bits, bf16_values


def _cases():
    return {
        "unit128": mc.unit_vectors(64, 128, 1),
        "unit1024": mc.unit_vectors(16, 1024, 2),
        "int128": mc.integer_vectors(32, 128, 3),
        "int1024": mc.integer_vectors(8, 1024, 4),
        "special128": mc.special_vectors(128),
        "special1024": mc.special_vectors(1024),
        "position128": mc.position_vectors(128),
        "mixed128": np.concatenate(mc.mixed_docs([40, 40], 128, 5)),
    }


def test_the_reference_equals_its_integer_restatement_on_every_case():
    from hiprag import mxfp4_quantize_reference
    for name, bits in _cases().items():
        codes, scales = mxfp4_quantize_reference(bits)
        c2, s2 = mc.quantize(bits)
        n, dim = bits.shape
        assert codes.dtype == np.uint8 and scales.dtype == np.uint8 and codes.shape == (n, dim // 2) and scales.shape == (n, dim // 32)
        assert codes.tobytes() == c2.tobytes() and scales.tobytes() == s2.tobytes(), name
        assert not np.any(mc.nibbles(codes) == 8), name                       # no -0 code
        assert scales.min() >= 27 and scales.max() <= 185, name               # what hipmv_load accepts
    codes, scales = mxfp4_quantize_reference(np.zeros((0, 128), np.uint16))
    assert codes.shape == (0, 64) and scales.shape == (0, 4)


def test_every_mutant_changes_a_128d_case_set():
    from hiprag import mxfp4_quantize_reference
    cases = {name: bits for name, bits in _cases().items() if bits.shape[1] == 128}
    ref = {name: mxfp4_quantize_reference(bits) for name, bits in cases.items()}
    for m in mc.MUTANTS:
        differs = [name for name, bits in cases.items()
                   if any(a.tobytes() != b.tobytes() for a, b in zip(mc.quantize(bits, m), ref[name]))]
        print(f"mutant {m}: differs on {differs}")
        assert differs, m
    # unit vectors alone catch every mutant but the floor, which needs a block below 2^-98; the specials catch that
    for m in mc.MUTANTS:
        hit = any(a.tobytes() != b.tobytes() for a, b in zip(mc.quantize(cases["unit128"], m), ref["unit128"]))
        assert hit == (m != "no_floor"), m
    assert any(a.tobytes() != b.tobytes() for a, b in zip(mc.quantize(cases["special128"], "no_floor"), ref["special128"]))


def test_dequantised_values_survive_a_bf16_round_trip():
    from hiprag import mxfp4_dequantize, mxfp4_quantize_reference
    for name, bits in _cases().items():
        codes, scales = mxfp4_quantize_reference(bits)
        back = mxfp4_dequantize(codes, scales)                                # asserts that no bit is lost below bf16
        assert back.dtype == np.uint16 and back.tobytes() == mc.dequantize(codes, scales).tobytes(), name      # from the bit fields
        vals = bf16_values(back)
        assert np.all(np.isfinite(vals)) and np.array_equal(bf16_bits(vals), back), name
        # a second quantisation of the dequantised vectors changes nothing: they are codes times their block's power of two
        c2, s2 = mxfp4_quantize_reference(back)
        assert np.array_equal(bf16_values(mxfp4_dequantize(c2, s2)), vals), name


@pytest.mark.parametrize("dim", (128, 1024))
def test_the_error_bound_on_unit_vectors(dim):
    from hiprag import mxfp4_quantize_reference
    bits = mc.unit_vectors(256 if dim == 128 else 32, dim, 7)
    codes, scales = mxfp4_quantize_reference(bits)
    r = mc.error_ratio(bits, codes, scales)
    print(f"mxfp4 dim {dim}: worst |v - deq| / max(|v| / 4, 2^(E - 2)) = {r:.6g}")
    assert r <= 1.0
    # every block's maximum scales into [4, 8)
    bmax = np.abs(bf16_values(bits)).reshape(len(bits), -1, 32).max(axis=2)
    scaled = bmax / np.exp2(scales.astype(np.float64) - 127)
    assert np.all((scaled >= 4) & (scaled < 8))


def test_the_special_vectors_behave_as_specified():
    from hiprag import mxfp4_quantize_reference
    rows = mc.special_rows(128)
    names = list(rows)
    bits = mc.special_vectors(128)
    codes, scales = mxfp4_quantize_reference(bits)
    nib = mc.nibbles(codes)
    at = names.index
    zero = ("zero", "neg_zero", "inf", "neg_inf", "nan", "above", "above_2", "below", "below_2", "only_subnormal")
    for name in names:
        i = at(name)
        if name in zero:                                                      # the zero vector: codes 0x0, scale bytes 127
            assert not codes[i].any() and np.all(scales[i] == 127), name
        else:
            assert codes[i].any() and mc.error_ratio(bits[i:i + 1], codes[i:i + 1], scales[i:i + 1]) <= 1.0, name
    assert mc.guarded_count(bits) == mc.N_GUARDED_SPECIAL == len(zero) - 2    # zero and -0 are not counted
    # -0, and what rounds to -0 (the tie -0.25 included), are stored as 0x0; -0.26 is -0.5
    assert nib[at("to_neg_zero"), :6].tolist() == [6, 0, 0, 0, 0, 9]
    # ties go to the even mantissa, at E = 0, at E = -7 and beside a block maximum of 6
    tie_codes = [int(np.flatnonzero(np.asarray([0, 0.5, 1, 1.5, 2, 3, 4, 6]) == v)[0]) for v in mc.TIES_ROUND_TO]
    want = tie_codes + [c | 8 if c else 0 for c in tie_codes]
    t = at("ties")
    assert scales[t].tolist() == [127, 120, 127, 127]
    assert nib[t, 0:15].tolist() == [6] + want and nib[t, 32:47].tolist() == [6] + want and nib[t, 64:79].tolist() == [15] + want
    # saturation: 6.5, 7.0 and 7.96875 become 6 and keep E (the scaled maximum stays in [4, 8)), at position 20 of their blocks
    s = at("saturation")
    assert scales[s].tolist() == [127, 127, 127, 136]
    assert nib[s, [20, 52, 84, 116]].tolist() == [7, 15, 7, 7]
    assert nib[s, 0:3].tolist() == [7, 15, 7] and nib[s, 32:35].tolist() == [7, 6, 5] and nib[s, 64:67].tolist() == [15, 7, 0]
    assert nib[s, 96:98].tolist() == [7, 15]
    # the edges of the domain are inside: scale bytes 185 = 58 + 127 and 65 = -62 + 127
    assert scales[at("amax_2^60")].tolist() == [185, 145, 127, 127] and scales[at("amax_2^-60")].tolist() == [65, 64, 127, 127]
    # normal | bf16 subnormals | zero | normal: the subnormal block takes E = -100 and codes 0, the zero block byte 127
    b = at("subnormal_block")
    assert scales[b].tolist() == [125, 27, 127, 120] and not nib[b, 32:96].any() and nib[b, 0:3].tolist() == [6, 10, 5]
    # block maxima 2^-110, 1.5 * 2^-99 and 1.5 * 2^-98 all take E = -100: codes 0 | 3, 1 (2^-100 = 0.5 * 2^-99 -> 1.0), -0.5 | 6, -2
    f = at("floor")
    assert scales[f].tolist() == [75, 27, 27, 27]
    assert nib[f, 32:34].tolist() == [0, 0] and nib[f, 64:67].tolist() == [5, 2, 9] and nib[f, 96:98].tolist() == [7, 12]


def test_every_position_of_a_block_decides_its_scale():
    from hiprag import mxfp4_quantize_reference
    for dim in (128, 1024):
        codes, scales = mxfp4_quantize_reference(mc.position_vectors(dim))
        want = np.full((dim, dim // 32), 119, np.uint8)                       # 2^-6: E = -8
        want[np.arange(dim), np.arange(dim) // 32] = 125                      # 1.0: E = -2
        assert np.array_equal(scales, want)
        assert np.all(mc.nibbles(codes)[np.arange(dim), np.arange(dim)] == 6)  # 1.0 * 2^2 = 4.0


def test_the_names_of_the_format(monkeypatch):
    import hiprag.colbert as hc
    from rag.config import config
    assert hc.FORMATS["bf16"] == 0 and hc.FORMATS["fp8"] == 1 and hc.FORMATS["mxfp4"] == 4 and len(hc.FORMATS) == 3
    for name in ("bf16", "fp8", "mxfp4"):
        monkeypatch.setenv("HIP_COLBERT_FORMAT", name)
        assert config.HIP_COLBERT_FORMAT == name
    monkeypatch.setenv("HIP_COLBERT_FORMAT", " MXFP4 ")
    assert config.HIP_COLBERT_FORMAT == "mxfp4"
    for name in ("fp4", "int8", ""):
        monkeypatch.setenv("HIP_COLBERT_FORMAT", name)
        with pytest.raises(ValueError, match="HIP_COLBERT_FORMAT"):
            config.HIP_COLBERT_FORMAT
    monkeypatch.delenv("HIP_COLBERT_FORMAT")
    assert config.HIP_COLBERT_FORMAT == "bf16"
    from rag.storage.hip_index.collection import mv_entry
    assert mv_entry(128, "mxfp4") == {"dim": 128, "format": "mxfp4"} and mv_entry(128, "bf16") == {"dim": 128}
    with pytest.raises(ValueError, match="fp4"):
        mv_entry(128, "fp4")
