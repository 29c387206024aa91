"""fp8 paged KV cache kernels on a real MI355X (`pytest -m gpu`): the
quantising write, the gather-dequant, split-K decode attention against the
fp64 oracle (cases and tolerances from tests/kv_fp8_cases.py, proven able to
fail by tests/test_kv_fp8_oracle.py), and the engine with kv_cache_dtype fp8.
Decode tests print `KV_FP8 <family> <case> err T ratio` (visible with -s).
"""

import json

import pytest
import torch

import attention_oracle as ao
import kv_fp8_cases as kc8
from opsagent_amd import ops
from opsagent_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = ao.D_HEAD


def _assert_close_bf16(got, ref32, atol=2e-2, rtol=2e-2, msg=""):
    # the assertion of the rope_kv parity test (tests/test_kernels_gpu.py)
    g = got.float().cpu()
    r = ref32.float().cpu()
    err = (g - r).abs() / r.abs().clamp_min(1.0)
    assert torch.isfinite(g).all(), f"{msg}: non-finite output"
    assert err.max() <= atol + rtol, f"{msg}: max rel err {err.max():.4f}"


# ------------------------------------------------------------------ writer
def _write_inputs(T, Hq, Hk, seed):
    gen = torch.Generator().manual_seed(seed)
    nb, bs = 8, 16
    qkv = torch.randn(T, (Hq + 2 * Hk) * D, generator=gen)
    # rows of very different magnitude, and one all-zero v row
    qkv[:, Hq * D:] *= torch.logspace(-3, 2, T).view(T, 1)
    qkv = qkv.to(torch.bfloat16)
    qkv[T // 2, (Hq + Hk) * D: (Hq + Hk + 1) * D] = 0
    pos = torch.randint(0, 1024, (T,), generator=gen, dtype=torch.int32)
    pos[0] = 1023
    slots = torch.randperm(nb * bs, generator=gen)[:T].to(torch.int32)
    return qkv, pos, slots, nb, bs


@pytest.mark.parametrize("Hq,Hk", [(8, 2), (4, 4), (8, 1)])
@pytest.mark.parametrize("T", [1, 5, 67])
def test_rope_kv_fp8_write(T, Hq, Hk):
    qkv0, pos, slots, nb, bs = _write_inputs(T, Hq, Hk, 100 * T + Hq + Hk)
    cos, sin = ops.rope_cos_sin(1024, D, 500000.0)
    qkv = qkv0.to(DEV)
    qf, kf, vf = qkv.split([Hq * D, Hk * D, Hk * D], dim=-1)
    q, k, v = qf.view(T, Hq, D), kf.view(T, Hk, D), vf.view(T, Hk, D)
    assert T == 1 or not k.is_contiguous()
    kc = torch.full((nb, bs, Hk, D), 0xA5, dtype=torch.uint8, device=DEV)
    vc = kc.clone()
    ks = torch.full((nb, bs, Hk), -1.0, dtype=torch.float32, device=DEV)
    vs = ks.clone()
    ops.rope_kv_fused_fp8(q, k, v, kc, vc, ks, vs, cos.to(DEV), sin.to(DEV),
                          pos.to(DEV), slots.to(DEV))
    torch.cuda.synchronize()

    q0, k0, v0 = (t.float() for t in qkv0.split([Hq * D, Hk * D, Hk * D], dim=-1))
    q_ref, k_ref = torch_ref.rope_apply(
        q0.view(T, Hq, D), k0.view(T, Hk, D), cos, sin, pos.long())
    _assert_close_bf16(q, q_ref, msg="rope q")
    _assert_close_bf16(k, k_ref, msg="rope k")
    assert torch.equal(v.cpu(), qkv0[:, (Hq + Hk) * D:].view(T, Hk, D)), "v changed"

    # rows not named in slots are untouched, bit for bit
    rest = torch.ones(nb * bs, dtype=torch.bool)
    rest[slots.long()] = False
    for codes in (kc, vc):
        assert (codes.cpu().view(nb * bs, Hk, D)[rest] == 0xA5).all()
    for sc in (ks, vs):
        assert (sc.cpu().view(nb * bs, Hk)[rest] == -1.0).all()

    for name, x, codes, sc in (("k", k, kc, ks), ("v", v, vc, vs)):
        x = x.cpu().float()                                     # the GPU's own bf16 rows
        s = sc.cpu().view(nb * bs, Hk)[slots.long()]            # [T, Hk]
        c = codes.cpu().view(nb * bs, Hk, D)[slots.long()]
        want_s = (x.abs().amax(-1).double().clamp_min(1e-8) / 448.0).float()
        assert torch.allclose(s, want_s, rtol=1e-6, atol=0), f"{name} scale"
        y = x.double() / s.double().unsqueeze(-1)
        c0 = y.float().to(torch.float8_e4m3fn).double()
        cg = c.view(torch.float8_e4m3fn).double()
        slack = (cg - y).abs() - (c0 - y).abs() - 1e-6 * y.abs()
        assert (slack <= 0).all(), f"{name} codes: worst excess {slack.max():.3e}"
        zero = x.abs().amax(-1) == 0
        assert (c[zero] == 0).all(), f"{name}: all-zero row must give codes 0"
    assert (v.cpu().float().abs().amax(-1) == 0).any()


# ------------------------------------------------------------------ gather
@pytest.mark.parametrize("Hk", [1, 4])
def test_kv_gather_fp8_exact(Hk):
    gen = torch.Generator().manual_seed(40 + Hk)
    nb, bs, Skv = 8, 16, 77
    raw_k = torch.randn(nb, bs, Hk, D, generator=gen) * torch.logspace(-2, 2, bs).view(1, bs, 1, 1)
    raw_v = torch.randn(nb, bs, Hk, D, generator=gen)
    kc, ks = kc8.quantise_cache(raw_k)
    vc, vs = kc8.quantise_cache(raw_v)
    slots = torch.randperm(nb * bs, generator=gen)[:Skv]
    kg, vg = ops.kv_gather_fp8(kc.to(DEV), vc.to(DEV), ks.to(DEV), vs.to(DEV),
                               slots.to(DEV))                  # int64 slots: converted
    kr, vr = torch_ref.kv_gather_fp8(kc, vc, ks, vs, slots, dtype=torch.bfloat16)
    assert kg.shape == (Skv, Hk, D) and kg.dtype == torch.bfloat16 and kg.is_contiguous()
    assert torch.equal(kg.cpu(), kr)
    assert torch.equal(vg.cpu(), vr)


# ------------------------------------------------------------------ decode
def _check(family, case, got, ref, tol):
    err = ao.row_rel_err(got, ref)
    print(f"\nKV_FP8 {family} {case.name} err={err:.5f} T={tol:.5f} ratio={err / tol:.3f}")
    assert err <= tol, f"{family} {case.name}: row_rel_err {err:.5f} > T {tol:.5f}"


@pytest.mark.parametrize("name", kc8.FP8_CASES)
def test_decode_fp8_edges(name):
    c = kc8.fp8_case(name)
    out = ops.attention_decode_paged_fp8(
        c.q.to(DEV), c.k_codes.to(DEV), c.v_codes.to(DEV), c.k_scale.to(DEV),
        c.v_scale.to(DEV), c.bt.to(DEV), c.lens.to(DEV), scale=c.scale, nsplit=c.nsplit,
    )
    family = "decode_fp8_" + kc8.pipeline_form(c.B, c.G)
    fmt = ao.row_rel_err(out, c.ref_unquantised)
    print(f"\nKV_FP8_FORMAT {name} row_rel_err vs oracle on the unquantised cache = {fmt:.4f}")
    _check(family, c, out, c.ref, c.tol)


def test_decode_fp8_rejects_blocks_smaller_than_a_key_quad():
    """The kernel reads two block-table entries per key quad, which covers
    the quad only at block_size >= 4; smaller blocks are an error."""
    from opsagent_amd.ops import hip_lib

    lib = hip_lib.get_lib()
    B, Hq, Hk, bs, nb = 1, 2, 1, 2, 4
    q = torch.zeros(B, Hq, D, dtype=torch.bfloat16, device=DEV)
    codes = torch.zeros(nb, bs, Hk, D, dtype=torch.uint8, device=DEV)
    sc = torch.zeros(nb, bs, Hk, dtype=torch.float32, device=DEV)
    bt = torch.zeros(B, nb, dtype=torch.int32, device=DEV)
    lens = torch.ones(B, dtype=torch.int32, device=DEV)
    with pytest.raises(AssertionError):
        ops.attention_decode_paged_fp8(q, codes, codes, sc, sc, bt, lens)
    ws = torch.zeros(64, dtype=torch.float32, device=DEV)
    rc = lib.oa_attention_decode_fp8(
        hip_lib.current_stream_ptr(), q.data_ptr(), codes.data_ptr(), codes.data_ptr(),
        sc.data_ptr(), sc.data_ptr(), bt.data_ptr(), lens.data_ptr(), ws.data_ptr(),
        ws.data_ptr(), q.data_ptr(), B, Hq, Hk, D, nb, bs, 1, 1.0, q.stride(0))
    assert rc == -101


def test_decode_fp8_from_gpu_writer_end_to_end():
    """Cache filled by the GPU writer (position 0: RoPE is the identity, so
    the probes stay aligned with q); oracle on the dequantised GPU codes."""
    c = kc8.fp8_case("b9_g4_bs32_s4")
    nb, bs, Hk, _ = c.kc_raw.shape
    T = nb * bs
    cos, sin = ops.rope_cos_sin(8, D, 500000.0)
    k = c.kc_raw.reshape(T, Hk, D).to(DEV)
    v = c.vc_raw.reshape(T, Hk, D).to(DEV)
    q_dummy = torch.zeros(T, Hk, D, dtype=torch.bfloat16, device=DEV)
    kcod = torch.zeros(nb, bs, Hk, D, dtype=torch.uint8, device=DEV)
    vcod = torch.zeros_like(kcod)
    ks = torch.zeros(nb, bs, Hk, dtype=torch.float32, device=DEV)
    vs = torch.zeros_like(ks)
    ops.rope_kv_fused_fp8(
        q_dummy, k, v, kcod, vcod, ks, vs, cos.to(DEV), sin.to(DEV),
        torch.zeros(T, dtype=torch.int32, device=DEV),
        torch.arange(T, dtype=torch.int32, device=DEV))
    assert torch.equal(k.cpu(), c.kc_raw.reshape(T, Hk, D)), "RoPE at position 0 must be exact"
    out = ops.attention_decode_paged_fp8(
        c.q.to(DEV), kcod, vcod, ks, vs, c.bt.to(DEV), c.lens.to(DEV),
        scale=c.scale, nsplit=c.nsplit)
    kc_eff = kc8.dequantise_cache(kcod.cpu(), ks.cpu())
    vc_eff = kc8.dequantise_cache(vcod.cpu(), vs.cpu())
    ref = ao.decode_oracle(c.q, kc_eff, vc_eff, c.bt, c.lens, c.scale)
    noise = ao.row_rel_err(
        ao.decode_emulation(c.q, kc_eff, vc_eff, c.bt, c.lens, c.scale), ref)
    _check("decode_fp8_written", c, out, ref, ao.TOL_FACTOR * noise)


# ------------------------------------------------------------------ engine
MICRO_CFG = {
    "model": "llama3-micro",
    "max_seq_len": 2048,
    "kv_block_size": 32,
    "kv_cache_gb": 2,
    "max_batch_size": 8,
    "use_hipgraph": True,
    "seed": 5,
    "kv_cache_dtype": "fp8",
}


@pytest.fixture(scope="module")
def engine():
    from opsagent_amd.engine.engine import LLMEngine

    return LLMEngine(dict(MICRO_CFG))


def test_engine_fp8_graph_vs_eager_same_tokens(engine):
    from opsagent_amd.engine.engine import SamplingParams

    assert engine.kv.layers[0][0].dtype == torch.uint8
    assert engine.cache_stats()["kv_cache_dtype"] == "fp8"
    ids = engine.tokenizer.encode("compare graph and eager", add_bos=True)
    out_g, _ = engine.generate(ids, SamplingParams(max_new_tokens=16))
    assert engine.use_hipgraph and engine._graphs, "decode was not graph-captured"
    engine.use_hipgraph = False
    out_e, _ = engine.generate(ids, SamplingParams(max_new_tokens=16))
    engine.use_hipgraph = True
    assert len(out_g) == 16 and out_g == out_e


def test_engine_fp8_grammar_json(engine):
    from opsagent_amd.engine.engine import SamplingParams
    from opsagent_amd.engine.grammar import GrammarMode

    ids = engine.tokenizer.encode("emit json", add_bos=True)
    out, _ = engine.generate(
        ids, SamplingParams(max_new_tokens=64, grammar=GrammarMode.TOOLPROMPT))
    obj = json.loads(engine.tokenizer.decode_text(out))
    assert "final_answer" in obj


def test_engine_fp8_prefix_reuse(engine):
    from opsagent_amd.engine.engine import SamplingParams

    ids = engine.tokenizer.encode("a shared conversation prefix across turns " * 8, add_bos=True)
    first, r1 = engine.generate(ids, SamplingParams(max_new_tokens=4))
    before = engine.kv.stats["reused_blocks"]
    second, r2 = engine.generate(ids, SamplingParams(max_new_tokens=4))
    assert engine.kv.stats["reused_blocks"] > before
    assert len(second) == len(first) == 4


def test_engine_fp8_holds_1_9x_the_blocks():
    from opsagent_amd.engine.engine import LLMEngine

    free = {}
    for dt in ("bf16", "fp8"):
        eng = LLMEngine(dict(MICRO_CFG, kv_cache_gb=1, kv_cache_dtype=dt, use_hipgraph=False))
        free[dt] = eng.cache_stats()["free_blocks"]
        del eng
        torch.cuda.empty_cache()
    assert free["fp8"] >= 1.9 * free["bf16"], free
