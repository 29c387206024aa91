"""CPU proof that the GPU attention edge tests can fail.

For every case tests/test_attention_edges_gpu.py runs (same builders, same
seeds) this file computes, from the references alone,

  N = row_rel_err(kernel-precision emulation, fp64 oracle)   the noise floor
  T = 4 N                                                     the GPU tolerance

and asserts that every applicable wrong-kernel mutant of the oracle lands at
row_rel_err >= 4 T. Run with -s to see N, T and the weakest mutant per case.
"""

import pytest
import torch

import attention_oracle as ao
from opsagent_amd.ops import torch_ref

# mutants skipped per case: {case name: {mutant name: reason}} — none needed
SKIPPED = {}


def _check_case(case):
    n, t = case.noise, case.tol
    assert 0.0 < n < 0.02, f"{case.name}: implausible noise floor {n}"
    muts = case.mutants()
    skipped = SKIPPED.get(case.name, {})
    assert len(skipped) * 10 < len(muts)
    worst_name, worst = None, float("inf")
    weak = []
    for name, knobs in muts:
        if name in skipped:
            continue
        e = case.mutant_err(knobs)
        if e < worst:
            worst_name, worst = name, e
        if not e >= ao.MUTANT_FACTOR * t:
            weak.append((name, e))
    print(f"\n{case.name}: N={n:.5f} T={t:.5f} mutants={len(muts)} "
          f"weakest={worst_name} err={worst:.4f} ({worst / t:.1f} T)")
    assert not weak, f"{case.name}: T={t:.5f}, mutants under 4T: {weak}"


@pytest.mark.parametrize("name", [c[0] for c in ao.PREFILL_CASES])
def test_prefill_mutants_visible(name):
    _check_case(ao.prefill_case(name))


@pytest.mark.parametrize("name", [c[0] for c in ao.DECODE_CASES])
def test_decode_mutants_visible(name):
    _check_case(ao.decode_case(name))


@pytest.mark.parametrize("name", [c[0] for c in ao.ROPE_CASES])
def test_rope_decode_mutants_visible(name):
    _check_case(ao.rope_case_with_reference(name, torch_ref.rope_apply))


def test_prefill_oracle_agrees_with_torch_ref():
    torch.manual_seed(11)
    for B, Hq, Hk, Sq, Skv, scale in [(2, 4, 2, 37, 37, None), (1, 8, 1, 20, 75, 0.2)]:
        q = torch.randn(B, Sq, Hq, 128)
        k = torch.randn(B, Skv, Hk, 128)
        v = torch.randn(B, Skv, Hk, 128)
        ref = torch_ref.attention_prefill(
            q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale
        ).transpose(1, 2)
        got = ao.prefill_oracle(q, k, v, scale)
        assert (got - ref.double()).abs().max() < 1e-5


def test_decode_oracle_agrees_with_torch_ref():
    torch.manual_seed(12)
    for B, Hq, Hk, bs, scale in [(3, 8, 2, 16, None), (2, 4, 4, 32, 0.2)]:
        nb, maxb = 24, 6
        kc = torch.randn(nb, bs, Hk, 128)
        vc = torch.randn(nb, bs, Hk, 128)
        q = torch.randn(B, Hq, 128)
        bt = torch.randperm(nb)[: B * maxb].view(B, maxb).to(torch.int32)
        lens = torch.tensor([maxb * bs, 1, bs + 3][:B], dtype=torch.int32)
        ref = torch_ref.attention_decode_paged(q, kc, vc, bt, lens, scale)
        got = ao.decode_oracle(q, kc, vc, bt, lens, scale)
        assert (got - ref.double()).abs().max() < 1e-5


def test_row_rel_err():
    ref = torch.tensor([[1.0, -4.0], [0.5, 0.25]])
    got = torch.tensor([[1.0, -3.0], [0.5, 0.25]])
    assert ao.row_rel_err(got, ref) == pytest.approx(0.25)
    assert ao.row_rel_err(ref, ref) == 0.0
    bad = got.clone()
    bad[1, 0] = float("nan")
    assert ao.row_rel_err(bad, ref) == float("inf")


def test_partition_matches_kernel_formulas():
    # chunk = ceil(n / nsplit); wave sub-range = ceil(span / 4)
    assert ao.split_ranges(9, 8) == [(0, 0, 2), (1, 2, 4), (2, 4, 6), (3, 6, 8), (4, 8, 9)]
    assert ao.wave_ranges(10, 1) == [(0, 0, 0, 3), (0, 1, 3, 6), (0, 2, 6, 9), (0, 3, 9, 10)]
    # rope: the newest key is not part of any wave's cached range
    assert ao.wave_ranges(10, 1, rope=True) == [(0, 0, 0, 3), (0, 1, 3, 6), (0, 2, 6, 9)]
    assert ao.wave_ranges(1, 4, rope=True) == []


def test_case_tables_cover_the_dispatch():
    """Every G, block size and nsplit appears with B <= 4 (4-deep pipeline)
    and with B >= 5 (2-deep); lens hold the edge values; poison ids valid."""
    for table in (ao.DECODE_CASES,):
        for deep in (True, False):
            rows = [c for c in table if (c[1] <= 4) == deep]
            assert {c[2] for c in rows} == {1, 2, 4, 8}
            assert {c[4] for c in rows} == {16, 32, 128}
            assert {c[5] for c in rows} == {1, 3, 4, 8}
    for deep in (True, False):
        assert {c[2] for c in ao.ROPE_CASES if (c[1] <= 4) == deep} == {1, 2, 4, 8}
    assert any(c[7] is not None for c in ao.DECODE_CASES)
    assert any(c[6] is not None for c in ao.PREFILL_CASES)
    seen = set()
    for c in ao.DECODE_CASES + ao.ROPE_CASES:
        case = ao.decode_case(c[0])
        bs, ns = case.bs, case.nsplit
        assert max(case.lens_list) == case.maxlen <= 640
        assert int(case.bt.min()) >= 0 and int(case.bt.max()) < case.kc.shape[0]
        if case.B == 9:
            want = {1, 2, bs - 1, bs, bs + 1, case.maxlen}
            assert want <= set(case.lens_list), (c[0], case.lens_list)
            assert any(n % 4 and n % 16 for n in case.lens_list)
            if ns >= 3:
                assert any(len(ao.split_ranges(n, ns)) < ns for n in case.lens_list)
        seen |= {("rope" if case.rope else "plain", n == 1) for n in case.lens_list}
    assert ("rope", True) in seen
