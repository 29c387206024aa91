"""K-depth pipeline of the decode GEMVs (gemv.hip): every depth must give the
bits of depth 1, must not depend on memory next to W, and the public paths
must still match the fp32 torch reference.

Shapes are the smallest at which the piece logic can go wrong: K below one
unit-row (8), one unit-row plus a partial one (520), exactly one piece
(512*ku), one piece plus one unit (512*ku + 8), one piece plus one unit-row
(512*(ku+1)), and the down-projection K (14336 = 28 unit-rows: 3 pieces of 8
plus a 4-deep one). N covers a single row, rows that do not fill a block, more
than two blocks' worth of waves, and the real o_proj width."""

import pytest
import torch

from opsagent_amd import ops

pytestmark = pytest.mark.gpu

EPS = 1e-5
DEPTHS = (2, 4, 8)  # every depth the dispatcher can ship, and depth 8
KS = sorted({8, 520, 14336}
            | {k for ku in DEPTHS for k in (512 * ku, 512 * ku + 8, 512 * (ku + 1))})
MAXN, MAXK = 8200 * 2, 14336


def dev():
    return "cuda"


def assert_close_bf16(got, ref32, atol=2e-2, rtol=2e-2, msg=""):
    # the check tests/test_kernels_gpu.py uses for these ops
    g = got.float().cpu()
    r = ref32.float().cpu()
    denom = r.abs().clamp_min(1.0)
    err = (g - r).abs() / denom
    assert torch.isfinite(g).all(), f"{msg}: non-finite output"
    assert err.max() <= atol + rtol, f"{msg}: max rel err {err.max():.4f}"


@pytest.fixture(scope="module")
def pool():
    """One seeded, asymmetric pool of inputs; tests take contiguous copies of
    its corners and never write to it."""
    g = torch.Generator(device=dev()).manual_seed(1234)
    w = (torch.randn(4096, MAXK, device=dev(), generator=g) * 0.3 + 0.02).to(torch.bfloat16)
    x = (torch.randn(2, MAXK, device=dev(), generator=g) * 0.3 - 0.05).to(torch.bfloat16)
    wn = (torch.rand(MAXK, device=dev(), generator=g) + 0.5).to(torch.bfloat16)
    res = torch.randn(2, MAXN, device=dev(), generator=g).to(torch.bfloat16)
    wide = (torch.randn(MAXN, 264, device=dev(), generator=g) * 0.3 + 0.02).to(torch.bfloat16)
    return {"w": w, "x": x, "wn": wn, "res": res, "wide": wide}


def _lib():
    from opsagent_amd.ops import hip_lib

    return hip_lib, hip_lib.get_lib()


def gemv_ku(x, w, wn, res, mode, rw, ku):
    hip_lib, lib = _lib()
    M, K = x.shape
    N = w.shape[0]
    # NaN-filled: a row the kernel fails to write cannot pass torch.equal
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=x.device)
    rc = lib.oa_gemv_ku(
        hip_lib.current_stream_ptr(), x.data_ptr(), w.data_ptr(), out.data_ptr(),
        wn.data_ptr() if mode & 1 else None, res.data_ptr() if mode & 2 else None,
        M, N, K, EPS, mode, rw, ku)
    assert rc == 0, f"oa_gemv_ku rc={rc}"
    return out


def gateup_ku(x, w, wn, norm, ku):
    hip_lib, lib = _lib()
    M, K = x.shape
    I = w.shape[0] // 2
    out = torch.full((M, I), float("nan"), dtype=torch.bfloat16, device=x.device)
    rc = lib.oa_gemv_gateup_ku(
        hip_lib.current_stream_ptr(), x.data_ptr(), w.data_ptr(), out.data_ptr(),
        wn.data_ptr() if norm else None, M, I, K, EPS, int(norm), ku)
    assert rc == 0, f"oa_gemv_gateup_ku rc={rc}"
    return out


def corner(pool, M, N, K, src="w"):
    x = pool["x"][:M, :K].contiguous()
    w = pool[src][:N, :K].contiguous()
    wn = pool["wn"][:K].contiguous()
    res = pool["res"][:M, :N].contiguous()
    return x, w, wn, res


def same_bits(a, b):
    # torch.equal treats NaN as unequal, so an unwritten row fails too
    return torch.equal(a.view(torch.int16), b.view(torch.int16)) and not torch.isnan(a).any()


class TestBitIdentityAcrossDepth:
    @pytest.mark.parametrize("M", [1, 2])
    @pytest.mark.parametrize("N", [1, 5, 9, 4096])
    def test_rw1(self, pool, M, N):
        for K in KS:
            x, w, wn, res = corner(pool, M, N, K)
            for mode in (0, 1, 2, 3):
                base = gemv_ku(x, w, wn, res, mode, 1, 1)
                for ku in DEPTHS:
                    got = gemv_ku(x, w, wn, res, mode, 1, ku)
                    assert same_bits(got, base), f"rw1 M{M} N{N} K{K} mode{mode} ku{ku}"

    @pytest.mark.parametrize("M", [1, 2])
    def test_rw2(self, pool, M):
        # N = 6146 with K = 264: odd row count over many blocks, partial
        # unit-row only; then the piece shapes at an odd N
        cases = [(6146, 264, "wide")] + [(9, K, "w") for K in KS]
        for N, K, src in cases:
            x, w, wn, res = corner(pool, M, N, K, src)
            for mode in (0, 1, 2, 3):
                base = gemv_ku(x, w, wn, res, mode, 2, 1)
                for ku in DEPTHS:
                    got = gemv_ku(x, w, wn, res, mode, 2, ku)
                    assert same_bits(got, base), f"rw2 M{M} N{N} K{K} mode{mode} ku{ku}"

    @pytest.mark.parametrize("M", [1, 2])
    @pytest.mark.parametrize("norm", [False, True])
    def test_gateup(self, pool, M, norm):
        # I = 8200 (> 2048 blocks * 4 waves): the grid-stride loop runs a
        # second row pair per wave
        cases = [(8200, 264, "wide")] + [(I, K, "w") for I in (3, 1030) for K in KS]
        for I, K, src in cases:
            x, w, wn, _ = corner(pool, M, 2 * I, K, src)
            base = gateup_ku(x, w, wn, norm, 1)
            for ku in DEPTHS:
                got = gateup_ku(x, w, wn, norm, ku)
                assert same_bits(got, base), f"gateup M{M} I{I} K{K} norm{norm} ku{ku}"


class TestNoOverRead:
    """W as the last rows of an exactly sized allocation against the same W
    surrounded by NaNs elsewhere: the result must not depend on neighbours."""

    @pytest.mark.parametrize("K", [8, 520, 4104, 14336])
    @pytest.mark.parametrize("ku", [1, 2, 4, 8])
    def test_neighbours_do_not_matter(self, pool, K, ku):
        N, I = 9, 5
        x, w, wn, res = corner(pool, 2, N, K)
        tail = torch.empty((3 + N) * K, dtype=torch.bfloat16, device=dev())
        tail[: 3 * K] = 1.0
        w_end = tail[3 * K:].view(N, K)
        w_end.copy_(w)
        island = torch.full(((N + 2) * K,), float("nan"), dtype=torch.bfloat16, device=dev())
        w_mid = island[K:(N + 1) * K].view(N, K)
        w_mid.copy_(w)
        for rw in (1, 2):
            for mode in (0, 3):
                a = gemv_ku(x, w_end, wn, res, mode, rw, ku)
                b = gemv_ku(x, w_mid, wn, res, mode, rw, ku)
                assert same_bits(a, b), f"rw{rw} mode{mode} K{K} ku{ku}"
        # gate-up reads rows r and I + r of a [2I, K] weight
        gu_end = tail[(3 + N - 2 * I) * K:].view(2 * I, K)
        gu_mid = island[K:(2 * I + 1) * K].view(2 * I, K)
        gu_mid.copy_(gu_end)
        for norm in (False, True):
            a = gateup_ku(x, gu_end, wn, norm, ku)
            b = gateup_ku(x, gu_mid, wn, norm, ku)
            assert same_bits(a, b), f"gateup norm{norm} K{K} ku{ku}"


def _rms(x32, wn32):
    return x32 * torch.rsqrt(x32.pow(2).mean(-1, keepdim=True) + EPS) * wn32


class TestPublicPathsVsFp32:
    """ops.* at the dispatcher's shipped depths against fp32 torch, with the
    tolerances tests/test_kernels_gpu.py uses for these ops."""

    @pytest.mark.parametrize("M", [1, 2])
    @pytest.mark.parametrize("N,K", [(1, 8), (5, 520), (9, 4104), (4096, 4096),
                                     (4096, 14336), (9, 4608), (6146, 264)])
    def test_linear_family(self, pool, M, N, K):
        x, w, wn, res = corner(pool, M, N, K, "wide" if K == 264 else "w")
        x32, w32 = x.float(), w.float()
        ref = x32 @ w32.T
        assert_close_bf16(ops.linear(x, w), ref, atol=3e-2, msg=f"linear {M}x{N}x{K}")
        assert_close_bf16(ops.linear_addres(x, w, res), ref + res.float(), atol=3e-2,
                          msg=f"linear_addres {M}x{N}x{K}")
        refn = _rms(x32, wn.float()) @ w32.T
        assert_close_bf16(ops.linear_norm(x, wn, EPS, w), refn, atol=3e-2,
                          msg=f"linear_norm {M}x{N}x{K}")

    @pytest.mark.parametrize("M", [1, 2])
    @pytest.mark.parametrize("I,K", [(3, 8), (3, 520), (1030, 4104), (1030, 4096),
                                     (3, 14336), (8200, 264)])
    def test_gateup_family(self, pool, M, I, K):
        x, w, wn, _ = corner(pool, M, 2 * I, K, "wide" if K == 264 else "w")
        x32, w32 = x.float(), w.float()

        def ref_of(xin):
            g, u = (xin @ w32.T).split([I, I], dim=-1)
            return torch.nn.functional.silu(g) * u

        assert_close_bf16(ops.gateup_silu(x, w, I), ref_of(x32), atol=3e-2,
                          msg=f"gateup {M}x{I}x{K}")
        assert_close_bf16(ops.gateup_silu_norm(x, wn, EPS, w, I), ref_of(_rms(x32, wn.float())),
                          atol=3e-2, msg=f"gateup_norm {M}x{I}x{K}")

    @pytest.mark.parametrize("M", [1, 2])
    def test_norm_with_outliers(self, pool, M):
        # a few large entries dominate sum(x^2): a wrong rstd cannot hide
        N, K = 4096, 4096
        x, w, wn, _ = corner(pool, M, N, K)
        x[:, 7] = 48.0
        x[:, 1030] = -64.0
        x[M - 1, 4095] = 96.0
        x32, w32 = x.float(), w.float()
        xn = _rms(x32, wn.float())
        assert_close_bf16(ops.linear_norm(x, wn, EPS, w), xn @ w32.T, atol=3e-2,
                          msg=f"linear_norm outliers M{M}")
        I = 1030
        g, u = (xn @ w32[: 2 * I].T).split([I, I], dim=-1)
        assert_close_bf16(ops.gateup_silu_norm(x, wn, EPS, w[: 2 * I].contiguous(), I),
                          torch.nn.functional.silu(g) * u, atol=3e-2,
                          msg=f"gateup_norm outliers M{M}")
