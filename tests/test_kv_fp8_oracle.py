"""CPU proof that the fp8-KV decode test (tests/test_kv_fp8_gpu.py) can fail.

The fp8 counterpart of tests/test_attention_oracle.py, on ten of its decode
cases rebuilt by tests/kv_fp8_cases.py (V rows rescaled, cache quantised with
torch_ref.quant_fp8, oracle on the dequantised cache). For each case

  N = row_rel_err(kernel-precision emulation, fp64 oracle), T = 4 N

and every wrong kernel must land at >= 4 T: the range / block-table / combine
mutants of the bf16 proof, and the scale mutants (V scale ignored, K and V
scales exchanged, a scale taken from the next slot, from the next head, or
from head 0). "K scale ignored" is not listed: on rows whose weight already
sits on the probes it only sharpens them; the writer test covers the K scale.
Run with -s to see N, T and the weakest mutant per case.
"""

import pytest
import torch

import attention_oracle as ao
import kv_fp8_cases as kc8
from opsagent_amd.ops import torch_ref


@pytest.mark.parametrize("name", kc8.FP8_CASES)
def test_fp8_decode_mutants_visible(name):
    case = kc8.fp8_case(name)
    n, t = case.noise, case.tol
    assert 0.0 < n < 0.02, f"{name}: implausible noise floor {n}"
    errs = [(m, case.mutant_err(knobs)) for m, knobs in case.mutants()]
    serrs = [(m, case.scale_mutant_err(ks, vs)) for m, (ks, vs) in case.scale_mutants().items()]
    assert len(serrs) == (7 if case.Hk >= 2 else 4)
    w_name, w = min(errs, key=lambda x: x[1])
    s_name, s = min(serrs, key=lambda x: x[1])
    print(f"\n{name}: N={n:.5f} T={t:.5f} range mutants={len(errs)} weakest={w_name} "
          f"({w / t:.1f} T); scale mutants weakest={s_name} ({s / t:.1f} T)")
    weak = [(m, e) for m, e in errs + serrs if not e >= ao.MUTANT_FACTOR * t]
    assert not weak, f"{name}: T={t:.5f}, mutants under 4T: {weak}"


def test_cases_cover_every_instantiation_the_launcher_dispatches():
    """(G, pipeline form) pairs of the ten cases against the launcher's rule,
    and the reference decode runs on each case's quantised cache."""
    cases = [kc8.fp8_case(n) for n in kc8.FP8_CASES]
    assert len(cases) == 10
    got = {(c.G, kc8.pipeline_form(c.B, c.G)) for c in cases}
    assert got == {(1, "deep8"), (2, "deep8"), (4, "deep8"),
                   (1, "deep4"), (2, "deep4"), (4, "deep4"), (8, "deep4")}
    assert {c.bs for c in cases} == {16, 32, 128} and min(c.bs for c in cases) >= 4
    assert any(c.scale is not None for c in cases)


def test_v_factors_are_applied_and_shared_case_is_untouched():
    name = kc8.FP8_CASES[1]
    base_vc = ao.decode_case(name).vc.clone()
    case = kc8.fp8_case(name)
    assert torch.equal(ao.decode_case(name).vc, base_vc)
    ratio = case.vc_raw.float().abs().amax(-1) / base_vc.float().abs().amax(-1)
    assert set(ratio.unique().tolist()) == set(kc8.V_FACTORS)
    # per-row scales follow: the format stores one scale per (slot, head)
    assert case.v_scale.shape == base_vc.shape[:-1]
    want = case.vc_raw.float().abs().amax(-1).clamp_min(1e-8) / 448.0
    assert torch.allclose(case.v_scale, want, rtol=1e-6, atol=0)


def test_reference_decode_matches_oracle_on_dequantised_cache():
    case = kc8.fp8_case("b2_g2_bs32_s3")
    got = torch_ref.attention_decode_paged_fp8(
        case.q.float(), case.k_codes, case.v_codes, case.k_scale, case.v_scale,
        case.bt, case.lens, case.scale)
    assert ao.row_rel_err(got, case.ref) < 1e-5
