"""The fp8 linear family of fp8_moe.hip on a real MI355X (`pytest -m gpu`)
against fp64 oracles on operands the oracle knows exactly: quant_fp8, the VALU
gemv_fp8 / gemv_gateup_fp8 kernels (every instantiated M, all four modes, the
RW=1 and XS forms, odd N, the grid-stride pass), the MFMA GEMV with both
quantisers (tail row groups, the 128 KiB x image, K = 32768, M = 5 / 7
gate-up) and gemm_fp8 (glds and register staging, N tail, K = 128, odd step
counts, the shipped deep-K dispatch).

Cases, oracles and tolerances come from tests/linear_cases.py and are proven
able to fail by tests/test_linear_oracle.py. The raw C entries are called so
the output can sit inside a larger NaN-filled buffer: every element of the
output must be finite, every bit outside it unchanged. Each comparison prints
`LIN <family> <run> err T ratio` (visible with -s).
"""

import pytest
import torch

import linear_cases as lc
from opsagent_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib():
    from opsagent_amd.ops import hip_lib

    return hip_lib, hip_lib.get_lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def launch(case: lc.LinCase, env, monkeypatch, wscale=None):
    """Run the case through its raw C entry; returns (rc, Guarded output)."""
    hip_lib, lib = _lib()
    lc.set_env(monkeypatch, env)
    M, N, K = case.M, case.N, case.K
    out = lc.Guarded(M, N, torch.bfloat16, float("nan"), DEV)
    w8, ws = _dev(case.wcodes), _dev(case.wscale if wscale is None else wscale)
    stream = hip_lib.current_stream_ptr()
    if case.kind == "gemm":
        a8, asc = _dev(case.acodes), _dev(case.ascale)
        rc = lib.oa_gemm_fp8(stream, a8.data_ptr(), w8.data_ptr(), asc.data_ptr(), ws.data_ptr(),
                             out.t.data_ptr(), M, N, K)
    else:
        x, wn, res = _dev(case.x), _dev(case.wn), _dev(case.res)
        if case.gateup:
            rc = lib.oa_gemv_gateup_fp8(stream, x.data_ptr(), w8.data_ptr(), ws.data_ptr(),
                                        out.t.data_ptr(), _ptr(wn), M, N, K, lc.EPS, case.mode & 1)
        else:
            rc = lib.oa_gemv_fp8_ex(stream, x.data_ptr(), w8.data_ptr(), ws.data_ptr(),
                                    out.t.data_ptr(), _ptr(wn), _ptr(res), M, N, K, lc.EPS,
                                    case.mode)
    torch.cuda.synchronize()
    return rc, out


def check(case, run, monkeypatch, family=None):
    key, env = run
    rc, out = launch(case, env, monkeypatch)
    rid = lc.run_id(run)
    assert rc == 0, f"{rid}: rc={rc}"
    got = out.t.cpu()
    assert torch.isfinite(got.float()).all(), f"{rid}: non-finite or unwritten output element"
    out.assert_outside_untouched(rid)
    err, tol = lc.row_rel_err(got, case.ref), case.tol
    print(f"\nLIN {family or lc.lin_family(case)} | {rid} err={err:.5f} T={tol:.5f} ratio={err / tol:.3f}")
    assert err <= tol, f"{rid}: row_rel_err {err:.5f} > T {tol:.5f}"


def _ids(runs):
    return [lc.run_id(r) for r in runs]


@pytest.mark.parametrize("run", lc.VALU_RUNS, ids=_ids(lc.VALU_RUNS))
def test_valu_gemv(run, monkeypatch):
    check(lc.lin_case(*run[0]), run, monkeypatch)


@pytest.mark.parametrize("run", lc.VALU_GU_RUNS, ids=_ids(lc.VALU_GU_RUNS))
def test_valu_gateup(run, monkeypatch):
    check(lc.lin_case(*run[0]), run, monkeypatch)


@pytest.mark.parametrize("run", lc.MFMA_RUNS, ids=_ids(lc.MFMA_RUNS))
def test_mfma_gemv(run, monkeypatch):
    check(lc.lin_case(*run[0]), run, monkeypatch)


@pytest.mark.parametrize("run", lc.MFMA_GU_RUNS, ids=_ids(lc.MFMA_GU_RUNS))
def test_mfma_gateup(run, monkeypatch):
    check(lc.lin_case(*run[0]), run, monkeypatch)


@pytest.mark.parametrize("run", lc.GEMM_RUNS, ids=_ids(lc.GEMM_RUNS))
def test_gemm_fp8(run, monkeypatch):
    key, env = run
    stage = env.get("OPSAGENT_FP8_STAGE", "reg" if key[3] > 16384 else "glds")
    check(lc.lin_case(*key), run, monkeypatch, family=f"gemm_fp8, {stage}")


@pytest.mark.parametrize("run", [lc.VALU_RUNS[4], lc.MFMA_RUNS[4], lc.GEMM_RUNS[8]],
                         ids=_ids([lc.VALU_RUNS[4], lc.MFMA_RUNS[4], lc.GEMM_RUNS[8]]))
def test_comparison_sees_a_neighbours_scale(run, monkeypatch):
    """The harness itself: the real kernel fed the weight scales rolled by one
    row is the `wscale_row-1` mutant and must land where the CPU proof puts it."""
    case = lc.lin_case(*run[0])
    rc, out = launch(case, run[1], monkeypatch, wscale=case.wscale.roll(1))
    assert rc == 0
    err = lc.row_rel_err(out.t.cpu(), case.ref)
    want = case.mutant_err({"wscale_shift": 1})
    # the kernel is within T of ITS answer's row maximum, at most (1 + want) of the reference's
    assert err >= lc.MUTANT_FACTOR * case.tol and abs(err - want) <= case.tol * (1 + want), (err, want)


def test_gemv_m_without_instantiation_is_an_error(monkeypatch):
    """No quiet fall-back: an M the VALU family does not instantiate returns
    an error code and writes nothing."""
    case = lc.lin_case("valu", 5, 5, 1040, 0, True)    # gate-up has no M = 5 off the MFMA path
    rc, out = launch(case, lc.VALU_OFF, monkeypatch)
    assert rc == -101
    assert torch.isnan(out.t.float()).all()


# ------------------------------------------------------------------ quantiser
def _quant(x):
    """oa_quant_fp8 on x [T, K] with one guard row before and two after."""
    hip_lib, lib = _lib()
    T, K = x.shape
    q = torch.full(((T + 3), K), 0xA5, dtype=torch.uint8, device=DEV)
    sc = torch.full((T + 3,), -1.0, dtype=torch.float32, device=DEV)
    xd = x.to(DEV).contiguous()
    rc = lib.oa_quant_fp8(hip_lib.current_stream_ptr(), xd.data_ptr(), q[1:].data_ptr(),
                          sc[1:].data_ptr(), T, K)
    torch.cuda.synchronize()
    assert rc == 0
    q, sc = q.cpu(), sc.cpu()
    assert (q[0] == 0xA5).all() and (q[T + 1:] == 0xA5).all(), "code rows outside [0, T) changed"
    assert sc[0] == -1.0 and (sc[T + 1:] == -1.0).all(), "scales outside [0, T) changed"
    return q[1:T + 1], sc[1:T + 1]


def _check_quant(x, msg):
    c, s = _quant(x)
    xf = x.float()
    amax = xf.abs().amax(-1)
    want_s = (amax.double().clamp_min(1e-8) / 448.0).float()
    assert torch.allclose(s, want_s, rtol=1e-6, atol=0), f"{msg}: scale"
    assert ((c & 0x7F) != 0x7F).all(), f"{msg}: NaN code"
    y = xf.double() / s.double().unsqueeze(-1)
    c0 = y.float().to(torch.float8_e4m3fn).double()
    cg = c.view(torch.float8_e4m3fn).double()
    slack = (cg - y).abs() - (c0 - y).abs() - 1e-6 * y.abs()
    assert (slack <= 0).all(), f"{msg}: codes, worst excess {slack.max():.3e}"
    assert (c[amax == 0] == 0).all(), f"{msg}: an all-zero row must give codes 0"
    for t in range(x.shape[0]):
        if amax[t] > 0:
            j = int(xf[t].abs().argmax())
            assert int(c[t, j]) == (0xFE if xf[t, j] < 0 else 0x7E), f"{msg}: absmax code, row {t}"
    return c, s


QUANT_SHAPES = [(1, 8), (4, 520), (5, 2056), (9, 4096)]


@pytest.mark.parametrize("T,K", QUANT_SHAPES)
def test_quant_fp8_rows(T, K):
    g = torch.Generator().manual_seed(1000 * T + K)
    x = torch.randn(T, K, generator=g) * torch.logspace(-2, 2, T).view(T, 1) + 0.01
    _check_quant(x.to(torch.bfloat16), f"quant T{T} K{K}")


@pytest.mark.parametrize("K", [K for _, K in QUANT_SHAPES])
def test_quant_fp8_special_rows(K):
    """An all-zero row, a row whose absmax element is negative, and a row of
    exact-grid values that must reproduce its codes."""
    g = torch.Generator().manual_seed(77 + K)
    x = (torch.randn(3, K, generator=g) * 0.7).to(torch.bfloat16)
    x[0] = 0
    x[1, K // 3] = -(x[1].float().abs().max() + 1.0)
    x[2] = lc.grid_x(1, K, [], g)[0]
    c, s = _check_quant(x, f"quant special K{K}")
    assert s[0] == pytest.approx(1e-8 / 448.0, rel=1e-6)
    want_c, want_s = torch_ref.quant_fp8(x[2:3])
    assert s[2] == want_s[0], "grid row: scale is a power of two, exactly"
    assert torch.equal(c[2], want_c[0]), "grid row: codes reproduced exactly"
