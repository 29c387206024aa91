"""The bf16 dense GEMV family of gemv.hip on a real MI355X (`pytest -m gpu`)
against fp64 oracles on the bf16 operands themselves: gemv_kernel at one, two
and four rows per wave (M 1 and 2 at depth 1 and the shipped depth of each
class, all four modes, the partial unit-row, every piece of the 8/4/2/1 walk,
odd N, the grid-stride pass), gemv_gateup_kernel, the M 3..16 instantiations
of both, and gemv_bf16_mfma_kernel (one ring fill and refills, tail row groups,
N = 1, the 98 KB and 131 KB x images, M 2..16, gate-up at PF = 4).

Cases, oracle and tolerances come from tests/dense_cases.py and are proven
able to fail by tests/test_dense_oracle.py. The raw C entries are called so
the output can sit inside a larger NaN-filled buffer: every element of the
output must be finite, every bit outside it unchanged. The public wrappers
allocate their own output and are held to the oracle alone. Each comparison
prints `DENSE <family> | <run> err T ratio` (visible with -s).
"""

import ctypes

import pytest
import torch

import dense_cases as dc
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


def launch(case: dc.DenseCase, run: dc.Run, monkeypatch, wn=None, res=None):
    """Run the case through the run's raw C entry; returns (rc, Guarded output)."""
    hip_lib, lib = _lib()
    dc.set_env(monkeypatch, run.env)
    M, N, K, mode = case.M, case.N, case.K, case.mode
    out = dc.Guarded(M, N, torch.bfloat16, float("nan"), DEV)
    x, w = _dev(case.x), _dev(case.w)
    wn = _dev(case.wn if wn is None else wn)
    res = _dev(case.res if res is None else res)
    stream = hip_lib.current_stream_ptr()
    o = out.t.data_ptr()
    if run.entry == "ku":
        rc = lib.oa_gemv_ku(stream, x.data_ptr(), w.data_ptr(), o, _ptr(wn), _ptr(res), M, N, K,
                            dc.EPS, mode, run.rw, run.ku)
    elif run.entry == "gu_ku":
        rc = lib.oa_gemv_gateup_ku(stream, x.data_ptr(), w.data_ptr(), o, _ptr(wn), M, N, K,
                                   dc.EPS, mode & 1, run.ku)
    elif run.entry == "ex":
        rc = lib.oa_gemv_ex(stream, x.data_ptr(), w.data_ptr(), o, _ptr(wn), _ptr(res), M, N, K,
                            dc.EPS, mode)
    elif run.entry == "gu_ex":
        rc = lib.oa_gemv_gateup_ex(stream, x.data_ptr(), w.data_ptr(), o, _ptr(wn), M, N, K,
                                   dc.EPS, mode & 1)
    elif run.entry == "rw4":
        assert M == 1 and mode == 0
        # a probe entry the loader does not declare: pointers must not pass as C ints
        lib.oa_gemv_rw4.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3
        lib.oa_gemv_rw4.restype = ctypes.c_int
        rc = lib.oa_gemv_rw4(stream, x.data_ptr(), w.data_ptr(), o, M, N, K)
    else:
        raise AssertionError(run.entry)
    torch.cuda.synchronize()
    return rc, out


def _report(case, run, got):
    rid = dc.run_id(run)
    assert torch.isfinite(got.float()).all(), f"{rid}: non-finite or unwritten output element"
    err, tol = dc.row_rel_err(got, case.ref), case.tol
    print(f"\nDENSE {dc.family(run)} | {rid} err={err:.5f} T={tol:.5f} ratio={err / tol:.3f}")
    assert err <= tol, f"{rid}: row_rel_err {err:.5f} > T {tol:.5f}"


def check(run, monkeypatch):
    case = dc.dense_case(*run.key)
    rc, out = launch(case, run, monkeypatch)
    rid = dc.run_id(run)
    assert rc == 0, f"{rid}: rc={rc}"
    out.assert_outside_untouched(rid)
    _report(case, run, out.t.cpu())


def _ids(runs):
    return [dc.run_id(r) for r in runs]


@pytest.mark.parametrize("run", dc.VALU_RUNS, ids=_ids(dc.VALU_RUNS))
def test_valu_gemv(run, monkeypatch):
    check(run, monkeypatch)


@pytest.mark.parametrize("run", dc.RW4_RUNS, ids=_ids(dc.RW4_RUNS))
def test_valu_gemv_rw4(run, monkeypatch):
    check(run, monkeypatch)


@pytest.mark.parametrize("run", dc.VALU_GU_RUNS, ids=_ids(dc.VALU_GU_RUNS))
def test_valu_gateup(run, monkeypatch):
    check(run, monkeypatch)


@pytest.mark.parametrize("run", dc.VALU_WIDE_RUNS, ids=_ids(dc.VALU_WIDE_RUNS))
def test_valu_wide_m(run, monkeypatch):
    check(run, monkeypatch)


@pytest.mark.parametrize("run", dc.MFMA_RUNS, ids=_ids(dc.MFMA_RUNS))
def test_mfma_gemv(run, monkeypatch):
    check(run, monkeypatch)


@pytest.mark.parametrize("run", dc.MFMA_GU_RUNS, ids=_ids(dc.MFMA_GU_RUNS))
def test_mfma_gateup(run, monkeypatch):
    check(run, monkeypatch)


@pytest.mark.parametrize("run", dc.OPS_RUNS, ids=_ids(dc.OPS_RUNS))
def test_public_wrappers(run, monkeypatch):
    case = dc.dense_case(*run.key)
    dc.set_env(monkeypatch, run.env)
    x, w, wn, res = _dev(case.x), _dev(case.w), _dev(case.wn), _dev(case.res)
    if run.entry == "linear":
        got = ops.linear(x, w)
    elif run.entry == "linear_norm":
        got = ops.linear_norm(x, wn, dc.EPS, w)
    elif run.entry == "linear_addres":
        got = ops.linear_addres(x, w, res)
    elif run.entry == "gateup_silu":
        got = ops.gateup_silu(x, w, case.N)
    else:
        got = ops.gateup_silu_norm(x, wn, dc.EPS, w, case.N)
    torch.cuda.synchronize()
    assert got.shape == (case.M, case.N) and got.dtype == torch.bfloat16
    _report(case, run, got.cpu())


@pytest.mark.parametrize("run", dc.SELF_CHECK_RUNS, ids=_ids(dc.SELF_CHECK_RUNS))
@pytest.mark.parametrize("what", ["norm_weight_rolled_2", "residual_rolled_1_row"])
def test_comparison_sees_a_wrong_operand(run, what, monkeypatch):
    """The harness itself: the real kernel fed the norm weight rolled by two
    elements, or the residual rolled by one batch row, is a mutant of the CPU
    proof. It must be >= 4 T from the true oracle and within the mutant's own
    T of the mutant's oracle."""
    case = dc.dense_case(*run.key)
    if what == "norm_weight_rolled_2":
        knobs, fed = {"normw_shift": True}, {"wn": case.wn.roll(2)}
    else:
        knobs, fed = {"res_roll": 1}, {"res": case.res.roll(1, 0)}
    rc, out = launch(case, run, monkeypatch, **fed)
    assert rc == 0
    got = out.t.cpu()
    err = dc.row_rel_err(got, case.ref)
    own, own_tol = dc.row_rel_err(got, case.mutant_ref(knobs)), case.mutant_tol(knobs)
    print(f"\nDENSE self-check {what} | {dc.run_id(run)} err={err / case.tol:.1f} T, "
          f"own err={own:.5f} own T={own_tol:.5f}")
    assert err >= dc.MUTANT_FACTOR * case.tol, (err, case.tol)
    assert own <= own_tol, (own, own_tol)
