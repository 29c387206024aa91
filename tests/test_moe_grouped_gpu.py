"""The grouped MoE GEMVs of moe_gemv.hip on a real MI355X (`pytest -m gpu`):
oa_moe_gateup, oa_moe_down and their expert-major forms, each on its own, in
bf16 and fp8, against the fp64 oracle of tests/linear_cases.py, and
ops.moe_grouped_mlp end to end on both families against the two-stage oracle.

Pair-major: E = 3, T = 4, P = 6 with repeated tokens, a zero and a negative
routing weight; rows 5, 9 (K tail: 528 bf16 / 1040 fp8) and 2052 (the
grid-stride pass). Expert-major: E = 5 with 0, 1, 8, 9 and 17 pairs in
shuffled order (the EMAJ_GROUP boundary), rows 5, 9 and 260 (past the 64 x 4
grid), and P = 2048 on one expert (the pair-list capacity). Outputs sit in a
larger NaN-filled buffer. tests/test_linear_oracle.py proves on the CPU that
every wrong-kernel mutant lands at >= 4 T on these cases. Each comparison
prints `LIN <family> <case> err T ratio` (visible with -s).
"""

import pytest
import torch

import linear_cases as lc
from opsagent_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib():
    from opsagent_amd.ops import hip_lib

    return hip_lib, hip_lib.get_lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


STAGE_KEYS = [k for k in lc.MOE_KEYS if k[0] != "mlp"]
MLP_KEYS = [k for k in lc.MOE_KEYS if k[0] == "mlp"]


def _report(case, got, what):
    err, tol = lc.row_rel_err(got, case.ref), case.tol
    print(f"\nLIN {lc.moe_family(case)} | {what} err={err:.5f} T={tol:.5f} ratio={err / tol:.3f}")
    assert err <= tol, f"{what}: row_rel_err {err:.5f} > T {tol:.5f}"


def _run_stage(case, monkeypatch, eids=None):
    hip_lib, lib = _lib()
    lc.set_env(monkeypatch, {})
    P, E, rows, K, fp8 = case.P, case.E, case.rows, case.K, int(case.fp8)
    out = lc.Guarded(P, rows, torch.bfloat16, float("nan"), DEV)
    x, w, ws = _dev(case.x), _dev(case.w1), _dev(case.w1_scale)
    eids, tids, pw = _dev(case.eids if eids is None else eids), _dev(case.tids), _dev(case.pw)
    stream = hip_lib.current_stream_ptr()
    head = (stream, x.data_ptr(), w.data_ptr(), _ptr(ws), eids.data_ptr())
    if case.kind == "gateup" and case.family == "pair":
        rc = lib.oa_moe_gateup(*head, tids.data_ptr(), out.t.data_ptr(), P, rows, K, fp8)
    elif case.kind == "gateup":
        rc = lib.oa_moe_gateup_emaj(*head, tids.data_ptr(), out.t.data_ptr(), P, E, rows, K, fp8)
    elif case.family == "pair":
        rc = lib.oa_moe_down(*head, pw.data_ptr(), out.t.data_ptr(), P, rows, K, fp8)
    else:
        rc = lib.oa_moe_down_emaj(*head, pw.data_ptr(), out.t.data_ptr(), P, E, rows, K, fp8)
    torch.cuda.synchronize()
    assert rc == 0, f"{case.name}: rc={rc}"
    got = out.t.cpu()
    assert torch.isfinite(got.float()).all(), f"{case.name}: non-finite or unwritten output element"
    out.assert_outside_untouched(case.name)
    return got


@pytest.mark.parametrize("key", STAGE_KEYS, ids=[lc.moe_id(k) for k in STAGE_KEYS])
def test_moe_stage(key, monkeypatch):
    case = lc.moe_case(*key)
    _report(case, _run_stage(case, monkeypatch), lc.moe_id(key))


@pytest.mark.parametrize("family", ["pair", "emaj"])
def test_comparison_sees_the_next_expert(family, monkeypatch):
    """The harness itself: the real kernel fed expert ids + 1 computes the
    `weights and scales of expert e + 1` mutant and must land far above T."""
    case = lc.moe_case("gateup", family, True, 9, 1040)
    got = _run_stage(case, monkeypatch, eids=(case.eids + 1) % case.E)
    err = lc.row_rel_err(got, case.ref)
    want = case.mutant_err({"wexpert_shift": 1, "sexpert_shift": 1})
    # the kernel is within T of ITS answer's row maximum, at most (1 + want) of the reference's
    assert err >= lc.MUTANT_FACTOR * case.tol and abs(err - want) <= case.tol * (1 + want), (err, want)


@pytest.mark.parametrize("key", MLP_KEYS, ids=[lc.moe_id(k) for k in MLP_KEYS])
def test_moe_grouped_mlp(key, monkeypatch):
    """ops.moe_grouped_mlp at P = 35: OPSAGENT_MOE_EMAJ_MIN_P=1 selects the
    expert-major kernels, a large value the pair-major ones."""
    case = lc.moe_case(*key)
    lc.set_env(monkeypatch, {"OPSAGENT_MOE_EMAJ_MIN_P": "1" if case.family == "emaj" else "100000"})
    assert case.P == 35 and case.E == 5
    y = ops.moe_grouped_mlp(
        _dev(case.x), _dev(case.w1), _dev(case.w1_scale), _dev(case.w2), _dev(case.w2_scale),
        _dev(case.eids), _dev(case.tids), _dev(case.pw), case.I, case.fp8, num_experts=case.E)
    torch.cuda.synchronize()
    assert y.shape == (case.P, case.H) and y.device.type == DEV
    got = y.cpu()
    assert torch.isfinite(got.float()).all()
    _report(case, got, lc.moe_id(key))
