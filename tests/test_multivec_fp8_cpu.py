"""
The fp8 format of the multi-vector store on the CPU: hiprag.colbert.fp8_quantize_reference (the specification, torch's
float8_e4m3fn cast as the rounding) against its integer restatement in tests/fp8_cases.py, the error bound, the lossless
and exact properties, the domain guard -- and the proof that the cases can fail: every mutant of fp8_cases differs from the
reference on at least one of them.  No GPU.
"""
import numpy as np
import pytest

import fp8_cases as fc
from oracle.linear_cases import bf16_bits, bf16_values


def _cases():
    return {
        "unit128": fc.unit_vectors(64, 128, 1),
        "unit1024": fc.unit_vectors(16, 1024, 2),
        "int128": fc.integer_vectors(32, 128, 3),
        "int1024": fc.integer_vectors(8, 1024, 4),
        "special": fc.special_vectors(128),
        "exhaustive": fc.exhaustive_vectors(128),
        "mixed": np.concatenate(fc.mixed_docs([40, 40], 128, 5)),
    }


def test_the_reference_equals_its_integer_restatement_on_every_case():
    from hiprag import fp8_quantize_reference
    for name, bits in _cases().items():
        codes, scales = fp8_quantize_reference(bits)
        c2, s2 = fc.quantize(bits)
        assert codes.dtype == np.uint8 and scales.dtype == np.float32 and codes.shape == bits.shape and scales.shape == (len(bits),)
        assert codes.tobytes() == c2.tobytes() and scales.tobytes() == s2.tobytes(), name
        assert not np.any((codes & 0x7F) == 0x7F), name                      # no NaN code
        assert not np.any(codes == 0x80), name                                # no -0 code


@pytest.mark.parametrize("dim", (128, 1024))
def test_the_error_bound_on_unit_vectors(dim):
    from hiprag import fp8_quantize_reference
    bits = fc.unit_vectors(256 if dim == 128 else 32, dim, 7)
    codes, scales = fp8_quantize_reference(bits)
    r = fc.error_ratio(bits, codes, scales)
    print(f"fp8 dim {dim}: worst |v - deq| / max(2^-4 |v|, 2^-10 scale) = {r:.6g}")
    assert r <= 1.0
    # a unit vector's largest component lies in [dim^-1/2, 1]: the scales are the powers of two that take it to [128, 256)
    amax = np.abs(bf16_values(bits)).max(axis=1)
    assert np.all((amax / scales >= 128) & (amax / scales < 256))


def test_integers_are_lossless_and_dequantised_values_are_bf16_exact():
    from hiprag import fp8_dequantize, fp8_quantize_reference
    for name in ("int128", "int1024"):
        bits = _cases()[name]
        codes, scales = fp8_quantize_reference(bits)
        assert np.array_equal(bf16_values(fp8_dequantize(codes, scales)), bf16_values(bits)), name      # -0 may have become +0
        assert fc.error_ratio(bits, codes, scales) == 0.0
    for name, bits in _cases().items():
        codes, scales = fp8_quantize_reference(bits)
        deq = fc.dequantized(codes, scales)                                   # float64, from the bit fields
        back = fp8_dequantize(codes, scales)                                  # asserts that no bit is lost below bf16
        assert np.array_equal(bf16_values(back).astype(np.float64), deq), name
        assert np.array_equal(bf16_bits(deq.astype(np.float32)), back), name
        assert np.all(np.isfinite(deq)), name


def test_zero_negative_zero_non_finite_and_out_of_domain_vectors():
    from hiprag import fp8_quantize_reference
    bits = fc.special_vectors(128)
    codes, scales = fp8_quantize_reference(bits)
    vals = bf16_values(bits)
    zeroed = 0
    for i in range(len(bits)):
        amax = np.abs(vals[i]).max()
        inside = np.all(np.isfinite(vals[i])) and 2.0 ** -60 <= amax <= 2.0 ** 60
        if not inside:                                                        # zero, or guarded: the zero vector, scale 1.0
            assert not codes[i].any() and scales[i] == np.float32(1.0), i
            zeroed += int(amax != 0 or not np.all(np.isfinite(vals[i])))
        else:
            assert 128 <= amax / scales[i] < 256 and codes[i, int(np.abs(vals[i]).argmax())] & 0x7F >= 0x70, i
            assert fc.error_ratio(bits[i:i + 1], codes[i:i + 1], scales[i:i + 1]) <= 1.0, i
    assert zeroed == fc.N_GUARDED_SPECIAL == fc.guarded_count(bits)
    # -0 and what rounds to it are stored as +0; ties go to the even code
    assert codes[2, :4].tolist() == [0x78 - 8, 0, 0, 0]                       # 128 = 2^7: exponent field 14, mantissa 0
    assert fc.code_values(codes[3, 1:6]).tolist() == [16.0, 20.0, -16.0, 20.0, 24.0]
    assert (fc.code_values(codes[4, 1:7]) * 512).tolist() == [0.0, 2.0, 2.0, -2.0, 8.0, 0.0]
    assert scales[5] == np.float32(2.0 ** -8) and codes[5, 0] == 0x78              # e = 8: 255 rounds up to 256
    assert fc.code_values(codes[5, 1:3]).tolist() == [1.0, -0.5]


def test_requantising_is_not_relied_on_and_the_mutants_are_caught():
    from hiprag import fp8_quantize_reference
    cases = _cases()
    ref = {name: fp8_quantize_reference(bits) for name, bits in cases.items()}
    for m in fc.MUTANTS:
        differs = [name for name, bits in cases.items()
                   if any(a.tobytes() != b.tobytes() for a, b in zip(fc.quantize(bits, m), ref[name]))]
        print(f"mutant {m}: differs on {differs}")
        assert differs, m
    # the exhaustive case alone catches every rounding and exponent mutant
    ex = cases["exhaustive"]
    for m in ("truncate", "e_plus_one", "e_minus_one", "keep_neg_zero", "scale_is_2e"):
        assert any(a.tobytes() != b.tobytes() for a, b in zip(fc.quantize(ex, m), ref["exhaustive"])), m
