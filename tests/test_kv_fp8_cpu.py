"""fp8 paged KV cache on the CPU: reference write/gather round trip, cache
shapes, a CPU engine with kv_cache_dtype fp8, sizing arithmetic, exported
symbols and compile-time resources of the new kernels."""

import ctypes
import json
import os
import shutil
import subprocess

import pytest
import torch

from opsagent_amd import ops
from opsagent_amd.engine.kv_cache import PagedKVCache
from opsagent_amd.ops import torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opsagent_amd", "ops", "csrc")
LIB = os.path.join(ROOT, "opsagent_amd", "ops", "libopsagent_kernels.so")

ENGINE_CFG = {
    "model": "llama3-micro",
    "max_seq_len": 512,
    "kv_block_size": 16,
    "max_batch_size": 4,
    "seed": 5,
    "kv_cache_dtype": "fp8",
}


# ------------------------------------------------------------ reference ops
def test_write_then_gather_round_trips_within_e4m3_bound():
    torch.manual_seed(0)
    T, Hq, Hk, D, nb, bs = 37, 4, 2, 128, 6, 16
    cos, sin = ops.rope_cos_sin(256, D, 500000.0)
    q = torch.randn(T, Hq, D)
    k = torch.randn(T, Hk, D) * 3.0
    v = torch.randn(T, Hk, D) * torch.logspace(-2, 2, T).view(T, 1, 1)
    v[3] = 0.0                                        # an all-zero row
    pos = torch.randint(0, 256, (T,), dtype=torch.int32)
    slots = torch.randperm(nb * bs)[:T].to(torch.int32)
    kv = PagedKVCache(1, Hk, D, bs, nb, "cpu", "fp8")
    (kc, vc), (ks, vs) = kv.layers[0], kv.scales[0]
    vs.fill_(-1.0)
    q2, k2, v2 = ops.rope_kv_fused_fp8(q, k, v, kc, vc, ks, vs, cos, sin, pos, slots)
    q_ref, k_ref = torch_ref.rope_apply(q, k, cos, sin, pos)
    assert torch.equal(q2, q_ref) and torch.equal(k2, k_ref) and torch.equal(v2, v)
    kg, vg = ops.kv_gather_fp8(kc, vc, ks, vs, slots, dtype=torch.float32)
    # e4m3 has 3 mantissa bits: rounding error <= 2^-4 of the value for
    # normals, and at most half the smallest subnormal step (2^-10 of 448
    # ulps, i.e. 2^-10 * scale) below 2^-6 * scale
    for got, want, sc in ((kg, k_ref, ks), (vg, v, vs)):
        s = sc.view(nb * bs, Hk)[slots.long()].unsqueeze(-1)
        bound = torch.maximum(want.abs() * 2.0 ** -4, s * 2.0 ** -10) * 1.001
        assert ((got - want).abs() <= bound).all()
        amax = want.abs().amax(-1, keepdim=True).clamp_min(1e-8)
        assert torch.allclose(s, amax / 448.0, rtol=1e-6, atol=0)
    assert (vg[3] == 0).all()
    # rows not named in slots keep their initial contents
    rest = torch.ones(nb * bs, dtype=torch.bool)
    rest[slots.long()] = False
    assert (kc.view(nb * bs, Hk, D)[rest] == 0).all()
    assert (vs.view(nb * bs, Hk)[rest] == -1.0).all()


def test_reference_decode_is_attention_over_dequantised_cache():
    torch.manual_seed(1)
    B, Hq, Hk, D, nb, bs = 3, 8, 2, 128, 12, 16
    kraw, vraw = torch.randn(nb, bs, Hk, D), torch.randn(nb, bs, Hk, D) * 5
    kc, ks = torch_ref.quant_fp8(kraw)
    vc, vs = torch_ref.quant_fp8(vraw)
    ks, vs = ks.view(nb, bs, Hk), vs.view(nb, bs, Hk)
    q = torch.randn(B, Hq, D)
    bt = torch.randperm(nb)[: B * 4].view(B, 4).to(torch.int32)
    lens = torch.tensor([64, 1, 19], dtype=torch.int32)
    got = ops.attention_decode_paged_fp8(q, kc, vc, ks, vs, bt, lens)
    want = torch_ref.attention_decode_paged(
        q, torch_ref.dequant_fp8(kc, ks), torch_ref.dequant_fp8(vc, vs), bt, lens)
    assert torch.equal(got, want)


# -------------------------------------------------------------------- cache
def test_paged_cache_fp8_shapes_and_dtypes():
    kv = PagedKVCache(3, 2, 128, 16, 8, "cpu", "fp8")
    assert len(kv.layers) == len(kv.scales) == 3
    for (k, v), (ks, vs) in zip(kv.layers, kv.scales):
        assert k.dtype == v.dtype == torch.uint8
        assert k.shape == v.shape == (8, 16, 2, 128)
        assert ks.dtype == vs.dtype == torch.float32
        assert ks.shape == vs.shape == (8, 16, 2)
    bf = PagedKVCache(1, 2, 128, 16, 8, "cpu", torch.bfloat16)
    assert bf.scales is None and bf.layers[0][0].dtype == torch.bfloat16
    assert PagedKVCache.block_bytes(3, 2, 128, 16, True) == 2 * 3 * 16 * 2 * 132
    assert PagedKVCache.block_bytes(3, 2, 128, 16, False) == 2 * 3 * 16 * 2 * 256


# ------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def engine():
    from opsagent_amd.engine.engine import LLMEngine

    return LLMEngine(dict(ENGINE_CFG))


def test_engine_fp8_cache_generates(engine):
    from opsagent_amd.engine.engine import SamplingParams
    from opsagent_amd.engine.grammar import GrammarMode

    assert engine.kv.layers[0][0].dtype == torch.uint8
    assert engine.kv.scales[0][0].dtype == torch.float32
    assert engine.cache_stats()["kv_cache_dtype"] == "fp8"
    ids = engine.tokenizer.encode("analyze pod nginx", add_bos=True)
    out, _ = engine.generate(ids, SamplingParams(max_new_tokens=12))
    assert len(out) > 0
    ids = engine.tokenizer.encode("emit json", add_bos=True)
    out, _ = engine.generate(
        ids, SamplingParams(max_new_tokens=64, grammar=GrammarMode.TOOLPROMPT))
    obj = json.loads(engine.tokenizer.decode_text(out))
    assert "final_answer" in obj


def test_engine_fp8_prefix_reuse_returns_the_same_tokens(engine):
    from opsagent_amd.engine.engine import SamplingParams

    assert engine.kv.scales is not None and engine.kv.layers[0][0].dtype == torch.uint8
    ids = engine.tokenizer.encode("a shared conversation prefix across turns " * 2, add_bos=True)
    assert len(ids) >= 3 * engine.block_size + 1
    first, _ = engine.generate(ids, SamplingParams(max_new_tokens=8))
    before = engine.kv.stats["reused_blocks"]
    second, _ = engine.generate(ids, SamplingParams(max_new_tokens=8))
    assert engine.kv.stats["reused_blocks"] >= before + 3
    assert second == first


def test_default_stays_bf16_and_env_selects_fp8(monkeypatch):
    from opsagent_amd.engine.engine import LLMEngine

    cfg = {k: v for k, v in ENGINE_CFG.items() if k != "kv_cache_dtype"}
    monkeypatch.delenv("OPSAGENT_KV_CACHE_DTYPE", raising=False)
    eng = LLMEngine(dict(cfg))
    assert eng.kv.scales is None and eng.cache_stats()["kv_cache_dtype"] == "bf16"
    monkeypatch.setenv("OPSAGENT_KV_CACHE_DTYPE", "fp8")
    assert LLMEngine(dict(cfg)).kv.layers[0][0].dtype == torch.uint8
    # the config key wins over the environment
    assert LLMEngine(dict(cfg, kv_cache_dtype="bf16")).kv.scales is None
    with pytest.raises(ValueError):
        LLMEngine(dict(cfg, kv_cache_dtype="int4"))
    # the fp8 decode kernel needs blocks of at least one key quad
    with pytest.raises(ValueError):
        LLMEngine(dict(cfg, kv_cache_dtype="fp8", kv_block_size=2))


def test_pick_num_blocks_counts_real_bytes(engine, monkeypatch):
    """Equal byte budgets: fp8 gets >= 1.9x the bf16 block count (256/132)."""
    counts = {}
    monkeypatch.setattr(engine, "device", "cuda")   # take the budget branch
    for dt in ("bf16", "fp8"):
        monkeypatch.setattr(engine, "kv_cache_dtype", dt)
        counts[dt] = engine._pick_num_blocks({"kv_cache_gb": 1})
    per_bf16 = PagedKVCache.block_bytes(
        engine.spec.num_layers, engine.spec.num_kv_heads, engine.spec.head_dim,
        engine.block_size, False)
    assert counts["bf16"] == (1 << 30) // per_bf16
    assert counts["fp8"] >= 1.9 * counts["bf16"]


# ----------------------------------------------------------- native library
def test_library_exports_fp8_kv_symbols():
    if not os.path.exists(LIB):
        from opsagent_amd.ops.build import build

        build(verbose=False)
    lib = ctypes.CDLL(LIB)
    for sym in ("oa_rope_kv_fp8", "oa_kv_gather_fp8", "oa_attention_decode_fp8"):
        assert hasattr(lib, sym), sym


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_kv_fp8_kernels_have_no_scratch(tmp_path):
    out = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
         "-Rpass-analysis=kernel-resource-usage",
         "-c", os.path.join(CSRC, "kv_fp8.hip"), "-o", str(tmp_path / "k.o")],
        capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    fns, spills, current_fn = set(), [], ""
    for ln in out.stderr.splitlines():
        if "Function Name:" in ln:
            current_fn = ln.rsplit(None, 2)[-2]
            fns.add(current_fn)
        if "ScratchSize" in ln and "ScratchSize [bytes/lane]: 0" not in ln:
            spills.append(f"{current_fn}: {ln.strip()}")
    assert not spills, "scratch in kv_fp8.hip:\n" + "\n".join(spills)
    for frag in ("rope_kv_fp8_kernel", "kv_gather_fp8_kernel"):
        assert any(frag in f for f in fns), frag
    # G in {1, 2, 4, 8}, every instantiation the launcher dispatches
    assert sum("decode_attn_fp8_kernel" in f for f in fns) >= 7
