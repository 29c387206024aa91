"""Append attention over the fp8 KV cache on the CPU: the reference against
its per-token fp8 decode expansion, ops dispatch, the exported symbol and
compile-time resources of the fp8 instantiations, and a CPU engine with an fp8
cache whose tokens must not change when `append_attention_fp8` routes
catch-up, verify and mixed steps through the append path."""

import ctypes
import logging
import os
import re
import shutil
import subprocess

import pytest
import torch

from opsagent_amd import ops
from opsagent_amd.ops import torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opsagent_amd", "ops", "csrc")
LIB = os.path.join(ROOT, "opsagent_amd", "ops", "libopsagent_kernels.so")

MICRO_CFG = {
    "model": "llama3-micro",
    "max_seq_len": 512,
    "kv_block_size": 16,
    "max_batch_size": 8,
    "use_hipgraph": False,
    "seed": 7,
    "kv_cache_dtype": "fp8",
}


# ------------------------------------------------------------ reference ops
def _random_paged_fp8(B, Hq, Hk, D, bs, lens, qlens, seed):
    gen = torch.Generator().manual_seed(seed)
    nblk = [(n + bs - 1) // bs for n in lens]
    nb = sum(nblk) + 1
    kc = torch.randn(nb, bs, Hk, D, generator=gen)
    vc = torch.randn(nb, bs, Hk, D, generator=gen) * torch.rand(nb, bs, Hk, 1, generator=gen)
    perm = torch.randperm(nb, generator=gen).tolist()
    bt = torch.zeros(B, max(nblk), dtype=torch.int32)
    for b in range(B):
        for i in range(nblk[b]):
            bt[b, i] = perm.pop()
    q = torch.randn(sum(qlens), Hq, D, generator=gen)
    cu = torch.tensor([0] + torch.tensor(qlens).cumsum(0).tolist(), dtype=torch.int32)
    kq, ks = torch_ref.quant_fp8(kc)
    vq, vs = torch_ref.quant_fp8(vc)
    return (q, kq, vq, ks.reshape(nb, bs, Hk), vs.reshape(nb, bs, Hk), bt,
            torch.tensor(lens, dtype=torch.int32), cu)


@pytest.mark.parametrize("Hq,Hk,D,bs,scale", [(8, 2, 128, 16, None), (4, 4, 32, 32, 0.3)])
def test_reference_equals_per_token_fp8_decode(Hq, Hk, D, bs, scale):
    lens, qlens = [70, 9, 33, 1], [5, 9, 1, 1]
    q, kq, vq, ks, vs, bt, sl, cu = _random_paged_fp8(4, Hq, Hk, D, bs, lens, qlens, 3)
    got = torch_ref.attention_append_paged_fp8(q, kq, vq, ks, vs, bt, sl, cu, scale)
    assert got.shape == q.shape
    for b in range(4):
        for j in range(qlens[b]):
            t = int(cu[b]) + j
            ref = torch_ref.attention_decode_paged_fp8(
                q[t:t + 1], kq, vq, ks, vs, bt[b:b + 1],
                torch.tensor([lens[b] - qlens[b] + j + 1], dtype=torch.int32), scale)
            assert (got[t] - ref[0]).abs().max() < 1e-5, (b, j)


def test_ops_dispatch_on_cpu():
    q, kq, vq, ks, vs, bt, sl, cu = _random_paged_fp8(2, 4, 2, 128, 16, [40, 5], [3, 5], 4)
    got = ops.attention_append_paged_fp8(q, kq, vq, ks, vs, bt, sl, cu, 5)
    ref = torch_ref.attention_append_paged_fp8(q, kq, vq, ks, vs, bt, sl, cu)
    assert torch.equal(got, ref)
    assert "attention_append_paged_fp8" in ops.__all__


# ----------------------------------------------------------- native library
def test_library_exports_append_fp8_symbol():
    if not os.path.exists(LIB):
        pytest.skip("kernel library not built")
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "oa_attention_append_fp8")
    assert hasattr(lib, "oa_attention_append")


def _nrt_and_format(fn: str):
    """(NRT, is_fp8) of an append_attn_kernel<NRT, SMALLBS, FP8> mangled name."""
    m = re.search(r"append_attn_kernelILi(\d)ELb([01])ELb([01])E", fn)
    assert m, fn
    return int(m.group(1)), m.group(3) == "1"


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_fp8_append_kernels_have_no_scratch_and_keep_occupancy(tmp_path):
    """Every fp8 instantiation: 0 B scratch, and waves/SIMD not below the
    bf16 instantiation with the same NRT, read from the same compile."""
    out = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
         "-Rpass-analysis=kernel-resource-usage",
         "-c", os.path.join(CSRC, "attention_append.hip"), "-o", str(tmp_path / "a.o")],
        capture_output=True, text=True, timeout=300,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    res, current_fn = {}, ""
    for ln in out.stderr.splitlines():
        if "Function Name:" in ln:
            current_fn = ln.rsplit(None, 2)[-2]
            res[current_fn] = {}
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m:
            res[current_fn]["scratch"] = int(m.group(1))
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", ln)
        if m:
            res[current_fn]["occ"] = int(m.group(1))
    kernels = {fn: r for fn, r in res.items() if "append_attn_kernel" in fn}
    fp8 = {fn: r for fn, r in kernels.items() if _nrt_and_format(fn)[1]}
    bf16 = {fn: r for fn, r in kernels.items() if not _nrt_and_format(fn)[1]}
    # one and two row tiles per wave, both block-table paths, both formats
    assert len(fp8) == 4 and len(bf16) == 4, sorted(kernels)
    yard = {}
    for fn, r in bf16.items():
        nrt = _nrt_and_format(fn)[0]
        yard[nrt] = min(yard.get(nrt, r["occ"]), r["occ"])
    for fn, r in fp8.items():
        nrt = _nrt_and_format(fn)[0]
        assert r["scratch"] == 0, f"{fn}: {r['scratch']} B scratch"
        assert r["occ"] >= yard[nrt], f"{fn}: occupancy {r['occ']} < bf16's {yard[nrt]}"


# ------------------------------------------------------------------- engine
def _engine(flag, **over):
    from opsagent_amd.engine.engine import LLMEngine
    from opsagent_amd.parallel import state

    state.set_tp_state(0, 1, None)
    cfg = dict(MICRO_CFG, **over)
    if flag is not None:
        cfg["append_attention_fp8"] = flag
    return LLMEngine(cfg)


def _metric_sum(name):
    from opsagent_amd.utils.perf import get_perf_stats

    s = get_perf_stats().get_metric_stats(name)
    return 0.0 if s is None else s["count"] * s["avg"]


def _reset_metrics():
    from opsagent_amd.utils.perf import get_perf_stats

    get_perf_stats().reset()


def _run_all(eng, reqs, steps=6000):
    rids = [eng.add_request(ids, params) for ids, params in reqs]
    for _ in range(steps):
        if all(eng.requests[r].finished for r in rids):
            break
        eng.step()
    out = [eng.requests.pop(r) for r in rids]
    assert all(r.finished for r in out)
    return [(r.output_ids, r.finish_reason) for r in out]


def test_jump_ahead_tokens_identical():
    from opsagent_amd.engine.engine import SamplingParams
    from opsagent_amd.engine.grammar import GrammarMode

    outs = {}
    for flag in (False, True):
        _reset_metrics()
        eng = _engine(flag)
        assert eng.kv_cache_dtype == "fp8"
        assert eng.cache_stats()["append_attention"] is flag
        ids = eng.tokenizer.encode("diagnose the failing pod", add_bos=True)
        outs[flag] = eng.generate(
            ids, SamplingParams(max_new_tokens=64, grammar=GrammarMode.TOOLPROMPT))
        assert _metric_sum("engine_ff_catchup_tokens") > 0
        assert (_metric_sum("engine_append_steps") > 0) is flag
    assert outs[True] == outs[False]


def test_spec_decode_tokens_identical():
    from opsagent_amd.engine.engine import SamplingParams

    prompt = "pods pods pods crashloop crashloop pods crashloop " * 3
    outs = {}
    for flag in (False, True):
        _reset_metrics()
        eng = _engine(flag, spec_decode=True, spec_min_ema=0.0, grammar_fastforward=False,
                      seed=23, max_batch_size=4)
        ids = eng.tokenizer.encode(prompt, add_bos=True)
        outs[flag] = eng.generate(ids, SamplingParams(max_new_tokens=64))
        assert eng.spec_stats["verify_passes"] > 0
        # verify takes the append path: one row per pass
        assert (_metric_sum("engine_append_steps") > 0) is flag
    assert outs[True] == outs[False]


def test_mixed_steps_form_and_tokens_identical():
    """Six concurrent grammar requests with the jump-ahead gate opened: the
    catch-ups share their step with the other rows, and nothing changes."""
    from opsagent_amd.engine.engine import SamplingParams
    from opsagent_amd.engine.grammar import GrammarMode

    outs = {}
    for flag in (False, True):
        _reset_metrics()
        eng = _engine(flag, grammar_ff_max_batch=64, spec_decode=False)
        tok = eng.tokenizer
        reqs = [
            (tok.encode(f"request number {i} wants json " + "pod " * i, add_bos=True),
             SamplingParams(max_new_tokens=48,
                            grammar=GrammarMode.TOOLPROMPT if i % 3 else GrammarMode.TOOLCALLS))
            for i in range(6)
        ]
        outs[flag] = _run_all(eng, reqs)
        steps, rows = _metric_sum("engine_append_steps"), _metric_sum("engine_append_rows")
        if flag:
            assert steps > 0 and rows > steps, (steps, rows)
        else:
            assert steps == 0
    assert outs[True] == outs[False]


def _warnings_while(make):
    records = []
    handler = logging.Handler(level=logging.WARNING)
    handler.emit = records.append
    elog = logging.getLogger("opsagent.engine")
    elog.addHandler(handler)
    try:
        eng = make()
    finally:
        elog.removeHandler(handler)
    return eng, [r for r in records if "append_attention" in r.getMessage()]


def test_config_key_and_environment(monkeypatch):
    monkeypatch.delenv("OPSAGENT_APPEND_ATTN", raising=False)
    monkeypatch.delenv("OPSAGENT_APPEND_ATTN_FP8", raising=False)
    # default: off
    eng, warned = _warnings_while(lambda: _engine(None))
    assert eng.append_attention is False and not warned
    # key off or absent with append_attention: the old single warning, still off
    for flag in (None, False):
        eng, warned = _warnings_while(lambda: _engine(flag, append_attention=True))
        assert eng.append_attention is False and eng.cache_stats()["append_attention"] is False
        assert len(warned) == 1
    # key on: no warning, on — with or without append_attention
    for extra in ({}, {"append_attention": True}):
        eng, warned = _warnings_while(lambda: _engine(True, **extra))
        assert eng.append_attention is True and eng.cache_stats()["append_attention"] is True
        assert not warned
    # the environment variable applies only when the key is absent
    monkeypatch.setenv("OPSAGENT_APPEND_ATTN_FP8", "1")
    assert _engine(None).append_attention is True
    assert _engine(False).append_attention is False
    monkeypatch.delenv("OPSAGENT_APPEND_ATTN_FP8")
    # the bf16 append variable does not reach the fp8 key
    monkeypatch.setenv("OPSAGENT_APPEND_ATTN", "1")
    eng, warned = _warnings_while(lambda: _engine(None))
    assert eng.append_attention is False and len(warned) == 1


def test_key_has_no_effect_with_a_bf16_cache(monkeypatch):
    monkeypatch.delenv("OPSAGENT_APPEND_ATTN", raising=False)
    monkeypatch.delenv("OPSAGENT_APPEND_ATTN_FP8", raising=False)
    eng, warned = _warnings_while(lambda: _engine(True, kv_cache_dtype="bf16"))
    assert eng.kv_cache_dtype == "bf16"
    assert eng.append_attention is False and eng.cache_stats()["append_attention"] is False
    assert not warned
    eng = _engine(True, kv_cache_dtype="bf16", append_attention=True)
    assert eng.append_attention is True
