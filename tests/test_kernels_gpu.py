"""HIP kernel numerics tests vs the plain-PyTorch fp32 references
(opsagent_amd.ops.torch_ref) — run on a real MI355X (`pytest -m gpu`).

Transpose-detecting inputs per CDNA guide §5.4 rule 16: random (asymmetric)
tensors everywhere; attention additionally checks a spiked-K row to exercise
the online-softmax rescale path (rule 26).
"""

import math

import pytest
import torch

from opsagent_amd import ops
from opsagent_amd.ops import torch_ref

pytestmark = pytest.mark.gpu


def dev():
    return "cuda"


def assert_close_bf16(got: torch.Tensor, ref32: torch.Tensor, atol=2e-2, rtol=2e-2, msg=""):
    g = got.float().cpu()
    r = ref32.float().cpu()
    denom = r.abs().clamp_min(1.0)
    err = (g - r).abs() / denom
    assert torch.isfinite(g).all(), f"{msg}: non-finite output"
    assert err.max() <= atol + rtol, f"{msg}: max rel err {err.max():.4f}"


class TestRMSNorm:
    @pytest.mark.parametrize("rows,dim", [(1, 4096), (33, 4096), (256, 8192), (7, 128)])
    def test_rmsnorm(self, rows, dim):
        x = torch.randn(rows, dim, dtype=torch.bfloat16, device=dev())
        w = torch.randn(dim, dtype=torch.bfloat16, device=dev()) * 0.5 + 1.0
        out = ops.rms_norm(x, w, 1e-5)
        ref = torch_ref.rms_norm(x.float().cpu(), w.float().cpu(), 1e-5)
        assert_close_bf16(out, ref, msg="rmsnorm")

    def test_fused_add(self):
        rows, dim = 64, 4096
        x = torch.randn(rows, dim, dtype=torch.bfloat16, device=dev())
        res = torch.randn(rows, dim, dtype=torch.bfloat16, device=dev())
        res_copy = res.clone()
        out, new_res = ops.fused_add_rms_norm(x, res, torch.ones(dim, dtype=torch.bfloat16, device=dev()), 1e-5)
        ref_out, ref_res = torch_ref.fused_add_rms_norm(
            x.float().cpu(), res_copy.float().cpu(), torch.ones(dim), 1e-5
        )
        assert_close_bf16(out, ref_out, msg="fused_add_rmsnorm out")
        assert_close_bf16(new_res, ref_res, msg="fused_add_rmsnorm residual")


class TestRoPE:
    def test_rope(self):
        T, Hq, Hk, D = 50, 8, 2, 128
        cos, sin = ops.rope_cos_sin(256, D, 500000.0)
        q = torch.randn(T, Hq, D, dtype=torch.bfloat16, device=dev())
        k = torch.randn(T, Hk, D, dtype=torch.bfloat16, device=dev())
        pos = torch.randint(0, 256, (T,), dtype=torch.int32, device=dev())
        q_ref, k_ref = torch_ref.rope_apply(
            q.float().cpu(), k.float().cpu(), cos, sin, pos.cpu().long()
        )
        q2, k2 = ops.rope_apply_(q, k, cos.to(dev()), sin.to(dev()), pos)
        assert_close_bf16(q2, q_ref, msg="rope q")
        assert_close_bf16(k2, k_ref, msg="rope k")


class TestSiluMul:
    def test_silu_mul(self):
        g = torch.randn(1000, 512, dtype=torch.bfloat16, device=dev())
        u = torch.randn(1000, 512, dtype=torch.bfloat16, device=dev())
        out = ops.silu_mul(g, u)
        ref = torch_ref.silu_mul(g.float().cpu(), u.float().cpu())
        assert_close_bf16(out, ref, msg="silu_mul")


class TestKVWrite:
    def test_scatter(self):
        nb, bs, hk, d = 8, 32, 4, 128
        kc = torch.zeros(nb, bs, hk, d, dtype=torch.bfloat16, device=dev())
        vc = torch.zeros_like(kc)
        T = 47
        k = torch.randn(T, hk, d, dtype=torch.bfloat16, device=dev())
        v = torch.randn(T, hk, d, dtype=torch.bfloat16, device=dev())
        slots = torch.randperm(nb * bs, device=dev())[:T].to(torch.int32)
        ops.kv_cache_write(kc, vc, k, v, slots)
        flat = kc.view(nb * bs, hk, d)
        assert torch.equal(flat[slots.long()], k)
        assert torch.equal(vc.view(nb * bs, hk, d)[slots.long()], v)


class TestPrefillAttention:
    @pytest.mark.parametrize(
        "B,Hq,Hk,Sq,Skv",
        [
            (1, 4, 4, 128, 128),     # MHA, one tile
            (1, 8, 2, 256, 256),     # GQA 4:1
            (2, 4, 1, 200, 200),     # ragged Sq (not multiple of 128)
            (1, 4, 2, 64, 320),      # chunked prefill: past KV (offset 256)
            (1, 32, 8, 1024, 1024),  # llama3-8B shape
        ],
    )
    def test_parity(self, B, Hq, Hk, Sq, Skv):
        D = 128
        torch.manual_seed(Sq + Hq)
        q = torch.randn(B, Sq, Hq, D, dtype=torch.bfloat16, device=dev()) * 0.5
        k = torch.randn(B, Skv, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        v = torch.randn(B, Skv, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        out = ops.attention_prefill(q, k, v)
        ref = torch_ref.attention_prefill(
            q.float().cpu().transpose(1, 2),
            k.float().cpu().transpose(1, 2),
            v.float().cpu().transpose(1, 2),
        ).transpose(1, 2)
        assert_close_bf16(out, ref, atol=3e-2, msg=f"prefill {B}x{Hq}x{Sq}x{Skv}")

    def test_spiked_key_rescale(self):
        """Force the online-softmax rescale across tiles (guide rule 26)."""
        B, Hq, Hk, S, D = 1, 4, 4, 256, 128
        torch.manual_seed(0)
        q = torch.randn(B, S, Hq, D, dtype=torch.bfloat16, device=dev()) * 0.1
        k = torch.randn(B, S, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.1
        v = torch.randn(B, S, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        # spike key 200 against query row 240 (tile 3): max jumps mid-scan
        k[0, 200] = q[0, 240] * 8.0
        out = ops.attention_prefill(q, k, v)
        ref = torch_ref.attention_prefill(
            q.float().cpu().transpose(1, 2),
            k.float().cpu().transpose(1, 2),
            v.float().cpu().transpose(1, 2),
        ).transpose(1, 2)
        assert_close_bf16(out, ref, atol=3e-2, msg="spiked rescale")


class TestDecodeAttention:
    @pytest.mark.parametrize(
        "B,Hq,Hk,maxlen,nsplit",
        [
            (1, 4, 4, 100, 1),
            (1, 8, 2, 500, 4),
            (3, 32, 8, 1000, 2),
            (2, 8, 1, 64, 8),      # splits exceed keys: empty partials
        ],
    )
    def test_parity(self, B, Hq, Hk, maxlen, nsplit):
        D, bs = 128, 32
        torch.manual_seed(B * maxlen)
        nblocks = B * ((maxlen + bs - 1) // bs) + 2
        kc = torch.randn(nblocks, bs, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        vc = torch.randn(nblocks, bs, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        q = torch.randn(B, Hq, D, dtype=torch.bfloat16, device=dev()) * 0.5
        maxb = (maxlen + bs - 1) // bs
        # distinct random blocks per sequence
        perm = torch.randperm(nblocks)[: B * maxb].view(B, maxb)
        bt = perm.to(torch.int32).to(dev())
        lens = torch.randint(1, maxlen + 1, (B,), dtype=torch.int32)
        lens[0] = maxlen
        out = ops.attention_decode_paged(q, kc, vc, bt, lens.to(dev()), nsplit=nsplit)
        ref = torch_ref.attention_decode_paged(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(), lens
        )
        assert_close_bf16(out, ref, atol=3e-2, msg=f"decode {B}x{Hq}x{maxlen}s{nsplit}")


class TestSampling:
    def test_masked_argmax(self):
        B, V = 5, 128256
        torch.manual_seed(1)
        logits = torch.randn(B, V, dtype=torch.bfloat16, device=dev())
        words = (V + 31) // 32
        # random mask allowing ~1% of tokens
        allow = torch.rand(B, V) < 0.01
        allow[:, 7] = True  # guarantee non-empty
        import numpy as np

        bits = np.packbits(
            allow.numpy().astype(np.uint8), axis=1, bitorder="little"
        )
        pad = words * 4 - bits.shape[1]
        bits = np.pad(bits, ((0, 0), (0, pad)))
        mask = torch.from_numpy(bits.view(np.int32).copy()).to(dev())
        got = ops.greedy_sample_masked(logits, mask).cpu()
        ref = torch_ref.greedy_sample_masked(logits.float().cpu(), allow)
        assert torch.equal(got.long(), ref)

    def test_unmasked_argmax(self):
        B, V = 3, 50000
        logits = torch.randn(B, V, dtype=torch.bfloat16, device=dev())
        got = ops.greedy_sample_masked(logits, None).cpu()
        ref = logits.float().cpu().argmax(dim=-1)
        assert torch.equal(got.long(), ref)


def test_native_lib_is_loaded():
    """The in-tree .so must be what the GPU path runs (driver contract)."""
    from opsagent_amd.ops import hip_lib

    lib = hip_lib.get_lib()
    assert "libopsagent_kernels.so" in str(lib._name)
    maps = open("/proc/self/maps").read()
    assert "libopsagent_kernels.so" in maps


class TestGemv:
    @pytest.mark.parametrize("M,N,K", [(1, 6144, 4096), (1, 128256, 4096),
                                       (4, 4096, 14336), (8, 28672, 4096),
                                       (2, 512, 512)])
    def test_parity_vs_blaslt(self, M, N, K):
        torch.manual_seed(M * N)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        got = ops.linear(x, w)
        ref = torch.nn.functional.linear(x.float(), w.float())
        assert_close_bf16(got, ref, atol=3e-2, msg=f"gemv {M}x{N}x{K}")

    def test_3d_input(self):
        x = torch.randn(1, 2, 1024, dtype=torch.bfloat16, device=dev())
        w = torch.randn(512, 1024, dtype=torch.bfloat16, device=dev())
        got = ops.linear(x, w)
        assert got.shape == (1, 2, 512)
        ref = torch.nn.functional.linear(x.float(), w.float())
        assert_close_bf16(got, ref, msg="gemv 3d")


class TestFusedRopeKV:
    def test_parity(self):
        T, Hq, Hk, D, bs, nb = 37, 8, 2, 128, 32, 4
        torch.manual_seed(3)
        cos, sin = ops.rope_cos_sin(128, D, 500000.0)
        q = torch.randn(T, Hq, D, dtype=torch.bfloat16, device=dev())
        k = torch.randn(T, Hk, D, dtype=torch.bfloat16, device=dev())
        v = torch.randn(T, Hk, D, dtype=torch.bfloat16, device=dev())
        q0, k0, v0 = q.clone(), k.clone(), v.clone()
        pos = torch.randint(0, 128, (T,), dtype=torch.int32, device=dev())
        slots = torch.randperm(nb * bs, device=dev())[:T].to(torch.int32)
        kc = torch.zeros(nb, bs, Hk, D, dtype=torch.bfloat16, device=dev())
        vc = torch.zeros_like(kc)
        ops.rope_kv_fused(q, k, v, kc, vc, cos.to(dev()), sin.to(dev()), pos, slots)
        q_ref, k_ref = torch_ref.rope_apply(
            q0.float().cpu(), k0.float().cpu(), cos, sin, pos.cpu().long()
        )
        assert_close_bf16(q, q_ref, msg="fused rope q")
        assert_close_bf16(k, k_ref, msg="fused rope k")
        flat_k = kc.view(nb * bs, Hk, D)[slots.long()]
        assert_close_bf16(flat_k, k_ref, msg="fused rope k-cache")
        assert torch.equal(vc.view(nb * bs, Hk, D)[slots.long()], v0)


class TestGateUpSilu:
    @pytest.mark.parametrize("M,I,K", [(1, 14336, 4096), (4, 1408, 2048), (8, 3584, 8192)])
    def test_parity(self, M, I, K):
        torch.manual_seed(M + I)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.2
        w = torch.randn(2 * I, K, dtype=torch.bfloat16, device=dev()) * 0.2
        got = ops.gateup_silu(x, w, I)
        gu = torch.nn.functional.linear(x.float(), w.float())
        g, u = gu.split([I, I], dim=-1)
        ref = torch.nn.functional.silu(g) * u
        assert_close_bf16(got, ref, atol=3e-2, msg=f"gateup {M}x{I}x{K}")


class TestFp8:
    def test_quant_roundtrip(self):
        T, K = 16, 2048
        torch.manual_seed(0)
        x = torch.randn(T, K, dtype=torch.bfloat16, device=dev()) * 3.0
        q, s = ops.quant_fp8(x)
        deq = torch_ref.dequant_fp8(q.cpu(), s.cpu())
        err = (deq - x.float().cpu()).abs().max() / x.float().abs().max().cpu()
        assert err < 0.08, f"quant error {err:.3f}"
        # parity with the torch reference quantizer
        q_ref, s_ref = torch_ref.quant_fp8(x.float().cpu())
        assert torch.allclose(s.cpu(), s_ref, rtol=1e-2)

    @pytest.mark.parametrize("M,N,K", [(1, 1408, 2048), (4, 2816, 1024), (8, 512, 512)])
    def test_gemv_fp8_parity(self, M, N, K):
        torch.manual_seed(M + N)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        q, s = ops.quant_fp8(w)
        got = ops.linear_fp8(x, q, s)
        ref = torch_ref.linear_fp8(x.float().cpu(), q.cpu(), s.cpu())
        assert_close_bf16(got, ref, atol=4e-2, msg=f"gemv_fp8 {M}x{N}x{K}")

    @pytest.mark.parametrize("M,N,K", [(128, 1408, 2048), (200, 512, 1024), (1024, 2816, 2048)])
    def test_gemm_fp8_parity(self, M, N, K):
        torch.manual_seed(M + N)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        wq, ws = ops.quant_fp8(w)
        # reference on the SAME quantized operands (two independent fp8
        # roundings of x would differ by quantizer-mismatch, not kernel error)
        xq, xs = ops.quant_fp8(x)
        from opsagent_amd.ops import hip_lib

        lib = hip_lib.get_lib()
        got = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
        rc = lib.oa_gemm_fp8(
            hip_lib.current_stream_ptr(), xq.data_ptr(), wq.data_ptr(),
            xs.data_ptr(), ws.data_ptr(), got.data_ptr(), M, N, K,
        )
        assert rc == 0
        xd = torch_ref.dequant_fp8(xq.cpu(), xs.cpu())
        wd = torch_ref.dequant_fp8(wq.cpu(), ws.cpu())
        ref = xd @ wd.T
        assert_close_bf16(got, ref, atol=4e-2, msg=f"gemm_fp8 {M}x{N}x{K}")


class TestMoeGrouped:
    @pytest.mark.parametrize("fp8", [False, True])
    def test_grouped_matches_loop(self, fp8):
        """Grouped MoE kernels == per-expert loop on the same weights."""
        import dataclasses

        from opsagent_amd.engine.config import get_model_spec
        from opsagent_amd.engine.moe import MoEMLP
        from opsagent_amd.parallel import state

        state.set_tp_state(0, 1, None)
        spec = get_model_spec("moe-micro")
        if fp8:
            spec = dataclasses.replace(spec, moe_dtype="fp8")
        gen = torch.Generator(device="cuda").manual_seed(3)
        moe = MoEMLP(spec, torch.bfloat16, gen).to("cuda")
        x = (torch.randn(5, spec.hidden_size, device="cuda") * 0.3).to(torch.bfloat16)
        out_grouped = moe(x)              # T=5 -> pair-major grouped kernels
        out_loop = moe.forward_loop(x)    # reference loop path
        err = (out_grouped.float() - out_loop.float()).abs().max()
        scale = out_loop.float().abs().max().clamp_min(1e-3)
        assert err / scale < 0.05, f"grouped vs loop rel err {err/scale:.4f}"

    @pytest.mark.parametrize("fp8", [False, True])
    def test_expert_major_matches_loop(self, fp8):
        """Expert-major grouped kernels (big-batch decode, one weight stream
        per 8 matched pairs) == per-expert loop on the same weights."""
        import dataclasses
        import os as _os

        from opsagent_amd.engine.config import get_model_spec
        from opsagent_amd.engine.moe import MoEMLP
        from opsagent_amd.parallel import state

        state.set_tp_state(0, 1, None)
        spec = get_model_spec("moe-micro")
        if fp8:
            spec = dataclasses.replace(spec, moe_dtype="fp8")
        gen = torch.Generator(device="cuda").manual_seed(4)
        moe = MoEMLP(spec, torch.bfloat16, gen).to("cuda")
        # T=40, top_k=4 -> P=160 >= the default expert-major threshold (64)
        x = (torch.randn(40, spec.hidden_size, device="cuda") * 0.3).to(torch.bfloat16)
        _os.environ["OPSAGENT_MOE_EMAJ_MIN_P"] = "64"
        try:
            out_emaj = moe(x)
        finally:
            _os.environ.pop("OPSAGENT_MOE_EMAJ_MIN_P", None)
        out_loop = moe.forward_loop(x)
        err = (out_emaj.float() - out_loop.float()).abs().max()
        scale = out_loop.float().abs().max().clamp_min(1e-3)
        assert err / scale < 0.05, f"expert-major vs loop rel err {err/scale:.4f}"


class TestStridedViews:
    def test_rope_kv_and_attention_on_qkv_slices(self):
        """q/k/v as head-slices of one fused qkv buffer (no copies) must match
        the contiguous path."""
        T, Hq, Hk, D, bs, nb = 40, 8, 2, 128, 32, 8
        torch.manual_seed(7)
        S = (Hq + 2 * Hk) * D
        qkv = torch.randn(T, S, dtype=torch.bfloat16, device=dev())
        q, k, v = qkv.split([Hq * D, Hk * D, Hk * D], dim=-1)
        qs = q.view(T, Hq, D)
        ks = k.view(T, Hk, D)
        vs = v.view(T, Hk, D)
        qc, kc_, vc_ = qs.contiguous(), ks.contiguous(), vs.contiguous()

        cos, sin = ops.rope_cos_sin(64, D, 500000.0)
        cos, sin = cos.to(dev()), sin.to(dev())
        pos = torch.arange(T, dtype=torch.int32, device=dev())
        slots = torch.arange(T, dtype=torch.int32, device=dev())
        cache1 = [torch.zeros(nb, bs, Hk, D, dtype=torch.bfloat16, device=dev()) for _ in range(2)]
        cache2 = [torch.zeros_like(cache1[0]) for _ in range(2)]

        ops.rope_kv_fused(qs, ks, vs, cache1[0], cache1[1], cos, sin, pos, slots)
        ops.rope_kv_fused(qc, kc_, vc_, cache2[0], cache2[1], cos, sin, pos, slots)
        assert torch.equal(qs.contiguous(), qc)
        assert torch.equal(cache1[0], cache2[0])
        assert torch.equal(cache1[1], cache2[1])

        out_s = ops.attention_prefill(qs.unsqueeze(0), ks.unsqueeze(0), vs.unsqueeze(0))
        out_c = ops.attention_prefill(qc.unsqueeze(0), kc_.unsqueeze(0), vc_.unsqueeze(0))
        assert torch.equal(out_s, out_c)

        # decode with a strided q (first batch rows of a larger buffer)
        big = torch.randn(3, S, dtype=torch.bfloat16, device=dev())
        qd = big[:, : Hq * D].view(3, Hq, D)
        bt = torch.arange(3, dtype=torch.int32, device=dev()).reshape(3, 1)
        lens = torch.full((3,), 16, dtype=torch.int32, device=dev())
        out_sd = ops.attention_decode_paged(qd, cache1[0], cache1[1], bt, lens, nsplit=2)
        out_cd = ops.attention_decode_paged(
            qd.contiguous(), cache1[0], cache1[1], bt, lens, nsplit=2
        )
        assert torch.equal(out_sd, out_cd)


class TestFusedDecodeCombine:
    @pytest.mark.parametrize("B,Hq,Hk,maxlen,nsplit", [
        (1, 32, 8, 2000, 32), (3, 8, 2, 700, 8), (2, 8, 1, 64, 8),
    ])
    def test_fused_equals_two_kernel(self, B, Hq, Hk, maxlen, nsplit):
        D, bs = 128, 32
        torch.manual_seed(B + maxlen)
        maxb = (maxlen + bs - 1) // bs
        nb = B * maxb + 1
        kc = torch.randn(nb, bs, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        vc = torch.randn_like(kc)
        q = torch.randn(B, Hq, D, dtype=torch.bfloat16, device=dev()) * 0.5
        bt = torch.randperm(nb)[: B * maxb].view(B, maxb).to(torch.int32).to(dev())
        lens = torch.randint(1, maxlen + 1, (B,), dtype=torch.int32)
        lens[0] = maxlen
        lens_d = lens.to(dev())
        out_f = ops.attention_decode_paged(q, kc, vc, bt, lens_d, nsplit=nsplit,
                                           fused_combine=True)
        out_2 = ops.attention_decode_paged(q, kc, vc, bt, lens_d, nsplit=nsplit,
                                           fused_combine=False)
        # summation ORDER differs between the two reducers -> compare to
        # rounding, not bitwise
        df = (out_f.float() - out_2.float()).abs().max()
        assert df < 1e-2, f"fused combine diverges from two-kernel: {df}"
        ref = torch_ref.attention_decode_paged(
            q.float().cpu(), kc.float().cpu(), vc.float().cpu(), bt.cpu(), lens
        )
        assert_close_bf16(out_f, ref, atol=3e-2, msg="fused decode")

    def test_fused_repeatable(self):
        """Run the fused path repeatedly — a broken hand-off is often rare/
        timing-dependent (guide G16 pitfall 3: test under varied conditions)."""
        D, bs, B, Hq, Hk = 128, 32, 4, 32, 8
        maxb = 40
        nb = B * maxb + 1
        kc = torch.randn(nb, bs, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        vc = torch.randn_like(kc)
        q = torch.randn(B, Hq, D, dtype=torch.bfloat16, device=dev()) * 0.5
        bt = torch.arange(B * maxb, dtype=torch.int32, device=dev()).view(B, maxb)
        lens = torch.full((B,), 1234, dtype=torch.int32, device=dev())
        first = ops.attention_decode_paged(q, kc, vc, bt, lens, nsplit=16)
        for _ in range(20):
            again = ops.attention_decode_paged(q, kc, vc, bt, lens, nsplit=16)
            assert torch.equal(first, again)


class TestGemvM16:
    @pytest.mark.parametrize("M", [12, 16])
    def test_batched_decode_shapes(self, M):
        """M=12/16 instantiations stay correct (dispatch prefers hipBLASLt
        there — measured faster — but the kernels remain usable)."""
        import ctypes

        from opsagent_amd.ops import hip_lib

        torch.manual_seed(M)
        K, N = 4096, 6144
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        lib = hip_lib.get_lib()
        got = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
        rc = lib.oa_gemv(hip_lib.current_stream_ptr(), x.data_ptr(), w.data_ptr(),
                         got.data_ptr(), M, N, K)
        assert rc == 0
        ref = torch.nn.functional.linear(x.float(), w.float())
        assert_close_bf16(got, ref, atol=3e-2, msg=f"gemv M={M}")



class TestDecodeAttentionRope:
    @pytest.mark.parametrize(
        "B,Hq,Hk,maxlen,nsplit",
        [
            (1, 4, 4, 100, 1),
            (1, 8, 2, 500, 4),
            (3, 32, 8, 1000, 2),
            (2, 8, 1, 64, 8),   # splits exceed keys
            (1, 32, 8, 2, 4),   # n=2: one cached key + the new one
        ],
    )
    def test_parity_vs_separate(self, B, Hq, Hk, maxlen, nsplit):
        """Fused RoPE+scatter+attention must match rope_kv followed by the
        plain decode kernel — identical inputs, BOTH cache scatters compared
        too (roped k and raw v land in the right slots)."""
        D, bs = 128, 32
        torch.manual_seed(B * maxlen + Hq)
        nblocks = B * ((maxlen + bs - 1) // bs) + 2
        kc1 = torch.randn(nblocks, bs, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        vc1 = torch.randn(nblocks, bs, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        kc2, vc2 = kc1.clone(), vc1.clone()
        # raw (un-roped) qkv as ONE fused buffer with head-slice views
        qkv = torch.randn(B, (Hq + 2 * Hk) * D, dtype=torch.bfloat16, device=dev()) * 0.5
        maxb = (maxlen + bs - 1) // bs
        perm = torch.randperm(nblocks)[: B * maxb].view(B, maxb)
        bt = perm.to(torch.int32).to(dev())
        lens = torch.randint(1, maxlen + 1, (B,), dtype=torch.int32)
        lens[0] = maxlen
        lens_d = lens.to(dev())
        pos = (lens - 1).to(torch.int32).to(dev())
        slots = (bt.cpu()[torch.arange(B), (lens - 1) // bs] * bs
                 + (lens - 1) % bs).to(torch.int32).to(dev())
        cos, sin = torch_ref.rope_cos_sin(4096, D, 500000.0)
        cos, sin = cos.to(dev()), sin.to(dev())

        def views(t):
            q = t[:, : Hq * D].view(B, Hq, D)
            k = t[:, Hq * D : (Hq + Hk) * D].view(B, Hk, D)
            v = t[:, (Hq + Hk) * D :].view(B, Hk, D)
            return q, k, v

        # reference path: rope_kv kernel then plain decode attention
        buf_ref = qkv.clone()
        q1, k1, v1 = views(buf_ref)
        q1, k1, v1 = ops.rope_kv_fused(q1, k1, v1, kc1, vc1, cos, sin, pos, slots)
        out_ref = ops.attention_decode_paged(q1, kc1, vc1, bt, lens_d, nsplit=nsplit)

        # fused path on the raw buffer
        buf = qkv.clone()
        q2, k2, v2 = views(buf)
        out = ops.attention_decode_rope(
            q2, k2, v2, kc2, vc2, bt, lens_d, cos, sin, slots, nsplit=nsplit
        )
        assert_close_bf16(out, out_ref.float().cpu(), atol=3e-2,
                          msg=f"rope-fused decode {B}x{Hq}x{maxlen}s{nsplit}")
        assert torch.equal(kc1, kc2), "scattered roped-k mismatch"
        assert torch.equal(vc1, vc2), "scattered v mismatch"


class TestFp8Fused:
    @pytest.mark.parametrize("M", [1, 2, 4])
    def test_linear_norm_fp8_parity(self, M):
        K, N = 1024, 512
        torch.manual_seed(M)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        nw = torch.randn(K, dtype=torch.bfloat16, device=dev()) * 0.1 + 1.0
        q, s = ops.quant_fp8(w)
        got = ops.linear_norm_fp8(x, nw, 1e-5, q, s)
        # fp32 reference WITHOUT the bf16 rounding of the two-kernel path
        # (the fused kernel normalizes in fp32 — slightly MORE precise)
        xf = x.float().cpu()
        xn = xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-5)
        xn = xn * nw.float().cpu()
        ref = xn @ torch_ref.dequant_fp8(q.cpu(), s.cpu()).T
        assert_close_bf16(got, ref, atol=4e-2, msg=f"norm_fp8 M{M}")

    @pytest.mark.parametrize("M", [1, 2])
    def test_linear_addres_fp8_parity(self, M):
        K, N = 1024, 768
        torch.manual_seed(M + 9)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        res = torch.randn(M, N, dtype=torch.bfloat16, device=dev())
        q, s = ops.quant_fp8(w)
        got = ops.linear_addres_fp8(x, q, s, res)
        ref = ops.linear_fp8(x, q, s) + res
        assert_close_bf16(got, ref.float().cpu(), atol=4e-2, msg=f"addres_fp8 M{M}")

    @pytest.mark.parametrize("M,norm", [(1, False), (1, True), (4, True)])
    def test_gateup_silu_fp8_parity(self, M, norm):
        K, I = 1024, 1408
        torch.manual_seed(M + 31)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(2 * I, K, dtype=torch.bfloat16, device=dev()) * 0.3
        nw = torch.randn(K, dtype=torch.bfloat16, device=dev()) * 0.1 + 1.0
        q, s = ops.quant_fp8(w)
        got = ops.gateup_silu_fp8(
            x, q, s, I, norm_w=nw if norm else None, eps=1e-5
        )
        # reference mirrors the dispatch: at M==1 the wrapper PRE-normalizes
        # (rmsnorm kernel -> bf16 round -> plain stream, measured faster than
        # the in-loop fp32 norm); otherwise the norm stays fused in fp32.
        # silu near its zero crossing amplifies whichever rounding the real
        # path has, so the reference must round exactly where it does.
        xf = x.float().cpu()
        if norm:
            xf = xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-5)
            xf = xf * nw.float().cpu()
            if M == 1:
                xf = xf.to(torch.bfloat16).float()
        gu = xf @ torch_ref.dequant_fp8(q.cpu(), s.cpu()).T
        g, u = gu.split([I, I], dim=-1)
        ref = torch.nn.functional.silu(g) * u
        assert_close_bf16(got, ref, atol=4e-2,
                          msg=f"gateup_fp8 M{M} norm={norm}")


def test_linear_fp8_mid_m_routes_to_gemm():
    """8 < M routes through the MX tile GEMM (catch-up / verify sizes): the
    activation is fp8-quantized per token there, so compare against a
    reference on the SAME double-quantized operands."""
    M, N, K = 14, 512, 1024
    torch.manual_seed(3)
    x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
    w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
    q, s = ops.quant_fp8(w)
    got = ops.linear_fp8(x, q, s)
    xq, xs = ops.quant_fp8(x)
    xd = torch_ref.dequant_fp8(xq.cpu(), xs.cpu())
    wd = torch_ref.dequant_fp8(q.cpu(), s.cpu())
    ref = (xd @ wd.T).to(torch.bfloat16)
    assert_close_bf16(got, ref, atol=4e-2, msg="fp8 mid-M GEMM route")


class TestFp8MfmaGemv:
    """The M>=2 MFMA stream path (gemv_fp8_mfma3_kernel): quantizes x to fp8
    (per-row absmax/448) and runs v_mfma_scale_f32_16x16x128_f8f6f4, so the
    reference double-quantizes BOTH operands. Shapes chosen to satisfy the
    dispatch guard (K % 4096 == 0 plain / % 2048 gateup, M 2..8)."""

    @staticmethod
    def _dquant(t):
        amax = t.float().abs().amax(dim=-1, keepdim=True).clamp_min(1e-8)
        sc = amax / 448.0
        return ((t.float() / sc).clamp(-448, 448)
                .to(torch.float8_e4m3fn).float() * sc)

    @staticmethod
    def _assert_robust(got, ref, msg):
        """Independent quantizers (torch ref vs v_cvt_pk_fp8) round a few
        borderline values to adjacent fp8 codes, and silu's zero crossing
        multiplies such a one-quantum slip by |u| — so bound the DISTRIBUTION
        (a wiring/race bug breaks most elements), not the max."""
        g = got.float().cpu()
        r = ref.float().cpu()
        err = (g - r).abs() / r.abs().clamp_min(1.0)
        assert torch.isfinite(g).all(), f"{msg}: non-finite"
        assert err.mean() <= 1e-2, f"{msg}: mean rel err {err.mean():.4f}"
        assert err.quantile(0.99) <= 5e-2, \
            f"{msg}: p99 rel err {err.quantile(0.99):.4f}"
        frac_big = (err > 0.1).float().mean()
        assert frac_big <= 0.01, f"{msg}: {frac_big:.3%} elements over 0.1"

    @pytest.mark.parametrize("M,N,K", [(2, 512, 4096), (4, 1000, 4096),
                                       (8, 544, 8192)])
    def test_mfma_gemv_parity(self, M, N, K):
        torch.manual_seed(M + N)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        q, s = ops.quant_fp8(w)
        got = ops.linear_fp8(x, q, s)
        ref = self._dquant(x.cpu()) @ self._dquant(w.cpu()).T
        # both operands fp8 + a 4-way split-K sum: worst-case elements land
        # just past 8e-2 relative (measured 0.085 at M4/K4096)
        assert_close_bf16(got, ref, atol=9e-2, msg=f"mfma_gemv {M}x{N}x{K}")

    def test_mfma_matches_valu_policy(self):
        """M=1 must stay on the VALU kernel (measured faster); forcing the
        MFMA path with OPSAGENT_FP8_GEMV_MFMA=2 must still be correct."""
        import os
        M, N, K = 1, 768, 4096
        torch.manual_seed(3)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        q, s = ops.quant_fp8(w)
        ref = self._dquant(x.cpu()) @ self._dquant(w.cpu()).T
        os.environ["OPSAGENT_FP8_GEMV_MFMA"] = "2"
        try:
            got = ops.linear_fp8(x, q, s)
        finally:
            os.environ.pop("OPSAGENT_FP8_GEMV_MFMA", None)
        assert_close_bf16(got, ref, atol=6e-2, msg="forced mfma M1")

    @pytest.mark.parametrize("M,norm", [(2, True), (4, False), (8, True)])
    def test_mfma_gateup_parity(self, M, norm):
        K, I = 4096, 992
        torch.manual_seed(M + 77)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(2 * I, K, dtype=torch.bfloat16, device=dev()) * 0.3
        nw = torch.randn(K, dtype=torch.bfloat16, device=dev()) * 0.1 + 1.0
        q, s = ops.quant_fp8(w)
        got = ops.gateup_silu_fp8(x, q, s, I, norm_w=nw if norm else None,
                                  eps=1e-5)
        xf = x.float().cpu()
        if norm:
            xf = xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-5)
            xf = xf * nw.float().cpu()
        gu = self._dquant(xf) @ self._dquant(w.cpu()).T
        g, u = gu[:, :I], gu[:, I:]
        ref = g * torch.sigmoid(g) * u
        self._assert_robust(got, ref, f"mfma_gateup M{M}n{norm}")

    @pytest.mark.parametrize("M", [2, 4])
    def test_mfma_addres_parity(self, M):
        N, K = 640, 4096
        torch.manual_seed(M + 13)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        res = torch.randn(M, N, dtype=torch.bfloat16, device=dev())
        q, s = ops.quant_fp8(w)
        got = ops.linear_addres_fp8(x, q, s, res)
        ref = self._dquant(x.cpu()) @ self._dquant(w.cpu()).T \
            + res.float().cpu()
        self._assert_robust(got, ref, f"mfma_addres M{M}")


class TestPrefillV3:
    """The swapped-QK^T 32x32 kernel (variant 8) only auto-dispatches when
    the 256-row grid fills the chip, which no small pytest shape does — pin
    the variant so regressions can't hide behind the v2 fallback."""

    def _run(self, B, Hq, Hk, Sq, Skv, seed=0, spike=False):
        import os
        D = 128
        torch.manual_seed(seed + Sq + Hq)
        q = torch.randn(B, Sq, Hq, D, dtype=torch.bfloat16, device=dev()) * 0.5
        k = torch.randn(B, Skv, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        v = torch.randn(B, Skv, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        if spike:
            # force the online-softmax rescale across 128-key tiles AND the
            # wave-vote alpha-skip path (guide rule 26): late key spikes
            # against a late query row
            k[0, min(Skv - 56, 200)] = q[0, Sq - 16] * 8.0
        os.environ["OPSAGENT_PREFILL_VARIANT"] = "8"
        try:
            out = ops.attention_prefill(q, k, v)
        finally:
            os.environ.pop("OPSAGENT_PREFILL_VARIANT", None)
        ref = torch_ref.attention_prefill(
            q.float().cpu().transpose(1, 2),
            k.float().cpu().transpose(1, 2),
            v.float().cpu().transpose(1, 2),
        ).transpose(1, 2)
        assert_close_bf16(out, ref, atol=3e-2,
                          msg=f"prefill_v3 {B}x{Hq}x{Sq}/{Skv}")

    @pytest.mark.parametrize(
        "B,Hq,Hk,Sq,Skv",
        [
            (1, 8, 2, 512, 512),     # two 256-row tiles, GQA
            (1, 4, 4, 300, 300),     # ragged rows (tail q-tile + tail keys)
            (2, 4, 1, 256, 640),     # chunked prefill: causal offset 384
            (1, 32, 8, 1024, 1024),  # bench chunk geometry
        ],
    )
    def test_parity(self, B, Hq, Hk, Sq, Skv):
        self._run(B, Hq, Hk, Sq, Skv)

    def test_spiked_rescale(self):
        self._run(1, 4, 4, 512, 512, seed=3, spike=True)


class TestBf16MfmaGemv:
    """MFMA batched-decode bf16 GEMV (default dispatch: M 3..8, K <= 6144;
    the M 12 and 16 cases below go to hipBLASLt, M 9..16 on the kernel is in
    tests/test_dense_bf16_gpu.py). Pin eligibility via shapes; references are
    plain fp32 matmuls (norm staged in fp32 then rounded to bf16 exactly where
    the kernel rounds)."""

    @pytest.mark.parametrize("M,N,K", [(3, 512, 1024), (8, 1000, 4096),
                                       (16, 544, 2048)])
    def test_plain_parity(self, M, N, K):
        torch.manual_seed(M + N)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.5
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        got = ops.linear(x, w)
        ref = x.float().cpu() @ w.float().cpu().T
        assert_close_bf16(got, ref, atol=3e-2, msg=f"bf16_mfma {M}x{N}x{K}")

    @pytest.mark.parametrize("M", [4, 8])
    def test_norm_parity(self, M):
        N, K = 640, 2048
        torch.manual_seed(M)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.5
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        nw = torch.randn(K, dtype=torch.bfloat16, device=dev()) * 0.1 + 1.0
        got = ops.linear_norm(x, nw, 1e-5, w)
        xf = x.float().cpu()
        xn = xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-5)
        xn = (xn * nw.float().cpu()).to(torch.bfloat16).float()  # stage round
        ref = xn @ w.float().cpu().T
        assert_close_bf16(got, ref, atol=3e-2, msg=f"bf16_mfma_norm M{M}")

    @pytest.mark.parametrize("M", [4, 12])
    def test_gateup_parity(self, M):
        K, I = 1024, 992
        torch.manual_seed(M + 5)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.5
        w = torch.randn(2 * I, K, dtype=torch.bfloat16, device=dev()) * 0.3
        got = ops.gateup_silu(x, w, I)
        gu = x.float().cpu() @ w.float().cpu().T
        g, u = gu[:, :I], gu[:, I:]
        ref = g * torch.sigmoid(g) * u
        assert_close_bf16(got, ref, atol=4e-2, msg=f"bf16_mfma_gateup M{M}")

    def test_addres_parity(self):
        M, N, K = 6, 512, 4096
        torch.manual_seed(9)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.5
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        res = torch.randn(M, N, dtype=torch.bfloat16, device=dev())
        got = ops.linear_addres(x, w, res)
        ref = x.float().cpu() @ w.float().cpu().T + res.float().cpu()
        assert_close_bf16(got, ref, atol=3e-2, msg="bf16_mfma_addres")


class TestFp8MfmaWideM:
    """fp8 MFMA GEMV at M 9..16 (VALU has no 9-11/13-15 instantiations —
    these batch sizes exist only through the MFMA stream)."""

    @pytest.mark.parametrize("M", [9, 13, 16])
    def test_wide_m_parity(self, M):
        N, K = 768, 4096
        torch.manual_seed(M)
        x = torch.randn(M, K, dtype=torch.bfloat16, device=dev()) * 0.3
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev()) * 0.3
        q, s = ops.quant_fp8(w)
        got = ops.linear_fp8(x, q, s)
        dq = TestFp8MfmaGemv._dquant
        ref = dq(x.cpu()) @ dq(w.cpu()).T
        assert_close_bf16(got, ref, atol=9e-2, msg=f"fp8_mfma_wide M{M}")


class TestPrefillV4:
    """GQA-merged prefill (variant 9): GQ q-heads per workgroup share each
    staged KV tile (GQ = 4 and 8 instantiations). Exercises the head/row
    mapping and keeps the causal mask/rescale paths honest."""

    def _run(self, B, Hq, Hk, Sq, Skv, spike=False):
        import os
        D = 128
        torch.manual_seed(Sq + Hq)
        q = torch.randn(B, Sq, Hq, D, dtype=torch.bfloat16, device=dev()) * 0.5
        k = torch.randn(B, Skv, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        v = torch.randn(B, Skv, Hk, D, dtype=torch.bfloat16, device=dev()) * 0.5
        if spike:
            k[0, Skv - 40] = q[0, Sq - 8, :Hk] * 8.0
        os.environ["OPSAGENT_PREFILL_VARIANT"] = "9"
        try:
            out = ops.attention_prefill(q, k, v)
        finally:
            os.environ.pop("OPSAGENT_PREFILL_VARIANT", None)
        ref = torch_ref.attention_prefill(
            q.float().cpu().transpose(1, 2),
            k.float().cpu().transpose(1, 2),
            v.float().cpu().transpose(1, 2),
        ).transpose(1, 2)
        assert_close_bf16(out, ref, atol=3e-2,
                          msg=f"prefill_v4 {B}x{Hq}/{Hk}x{Sq}/{Skv}")

    @pytest.mark.parametrize(
        "B,Hq,Hk,Sq,Skv",
        [
            (1, 8, 2, 256, 256),     # GQ4, multi-tile
            (1, 32, 8, 1024, 1024),  # GQ4, bench chunk geometry
            (1, 8, 1, 512, 512),     # GQ8 (70B head geometry class)
            (1, 8, 4, 384, 384),     # GQ2
            (2, 4, 1, 130, 450),     # GQ4, ragged rows + causal offset
        ],
    )
    def test_parity(self, B, Hq, Hk, Sq, Skv):
        self._run(B, Hq, Hk, Sq, Skv)

    def test_spiked_rescale(self):
        self._run(1, 8, 2, 512, 512, spike=True)
