"""CPU proof for the fp8 append attention tests: on every case of
tests/append_fp8_cases.py each wrong kernel — the range, table, causal and
combine mutants of the bf16 append proof and the seven scale mutants of the
fp8 decode proof — lands at least MUTANT_FACTOR * T away from the oracle, so
the GPU comparison at T cannot pass one of them."""

import pytest

import append_fp8_cases as afc
from attention_oracle import MUTANT_FACTOR


@pytest.mark.parametrize("name", afc.FP8_APPEND_CASE_NAMES)
def test_structural_mutants_are_visible(name):
    c = afc.fp8_append_case(name)
    assert 0 < c.noise < 2e-2
    worst = None
    for mname, knobs in c.mutants():
        err = c.mutant_err(knobs)
        if worst is None or err < worst[1]:
            worst = (mname, err)
        assert err >= MUTANT_FACTOR * c.tol, (
            f"{name}: mutant {mname} at {err / c.tol:.2f} T (N={c.noise:.2e})")
    print(f"\nAPPEND_FP8_ORACLE {name} N={c.noise:.2e} weakest={worst[0]} "
          f"at {worst[1] / c.tol:.1f} T")


@pytest.mark.parametrize("name", afc.FP8_APPEND_CASE_NAMES)
def test_scale_mutants_are_visible(name):
    c = afc.fp8_append_case(name)
    muts = c.scale_mutants()
    assert len(muts) == (7 if c.Hk >= 2 else 4)
    for mname, (ks, vs) in muts.items():
        err = c.scale_mutant_err(ks, vs)
        assert err >= MUTANT_FACTOR * c.tol, (
            f"{name}: scale mutant {mname} at {err / c.tol:.2f} T (N={c.noise:.2e})")


def test_codes_all_covers_every_code():
    """The parity case builds (its constructor asserts the coverage) and has
    a usable tolerance."""
    c = afc.fp8_append_case(afc.CODES_ALL)
    assert (c.B, c.G, c.Hk, c.bs, c.nsplit, c.lens_list, c.qlens) == (1, 4, 2, 16, 2, [100], [5])
    assert 0 < c.noise < 2e-2
    # subnormals and both zeros are among the codes some row sees
    for codes in (c.k_codes, c.v_codes):
        seen = set(codes.unique().tolist())
        assert {0x00, 0x80, 0x01, 0x07, 0x81, 0x87, 0x7E, 0xFE} <= seen
