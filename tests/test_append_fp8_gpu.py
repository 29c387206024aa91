"""Paged append attention over the fp8 KV cache on a real MI355X
(`pytest -m gpu`): the kernel against the fp64 oracle over the DEQUANTISED
cache on every case of tests/append_fp8_cases (whose wrong-kernel mutants
tests/test_append_fp8_oracle.py proves visible at >= 4 T on the CPU), on the
fp8 decode cases as all-L=1 batches, behind the real quantising write, with
two scale mutants run through the real kernel, inside a NaN-filled buffer and
inside the engine. Each kernel test prints `APPEND_FP8 <family> <case> err T
ratio` (visible with -s).
"""

import json

import pytest
import torch

import append_cases as ac
import append_fp8_cases as afc
import attention_oracle as ao
import kv_fp8_cases as kf
from opsagent_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _check(family, name, got, ref, tol):
    err = ao.row_rel_err(got, ref)
    print(f"\nAPPEND_FP8 {family} {name} err={err:.5f} T={tol:.5f} ratio={err / tol:.3f}")
    assert err <= tol, f"{family} {name}: row_rel_err {err:.5f} > T {tol:.5f}"


def _family(c):
    rows = max(c.qlens) * c.G
    return "fp8_nrt1" if rows <= 16 else ("fp8_keys" if rows <= 32 else "fp8_rows")


def _run(c, k_scale=None, v_scale=None, workspace=None):
    D = ao.D_HEAD
    qkv = c.qkv.to(DEV)
    q = qkv[:, : c.Hq * D].view(c.T, c.Hq, D)      # head-slice view, as the engine passes it
    assert q.stride(0) == (c.Hq + 2 * c.Hk) * D
    ks = c.k_scale if k_scale is None else k_scale
    vs = c.v_scale if v_scale is None else v_scale
    return ops.attention_append_paged_fp8(
        q, c.k_codes.to(DEV), c.v_codes.to(DEV), ks.contiguous().to(DEV),
        vs.contiguous().to(DEV), c.bt.to(DEV), c.lens.to(DEV), c.cu.to(DEV), c.max_q,
        scale=c.scale, workspace=workspace, nsplit=c.nsplit,
    )


@pytest.mark.parametrize("own_ws", [False, True], ids=["alloc", "workspace"])
@pytest.mark.parametrize("name", afc.ALL_CASE_NAMES)
def test_append_fp8_edges(name, own_ws):
    c = afc.fp8_append_case(name)
    ws = None
    if own_ws:
        ws = ops.append_workspace(c.B, c.T, c.Hk, c.G, c.nsplit, device=DEV, max_q=c.max_q)
        for t in ws:
            t.fill_(float("nan"))       # a partial read before it is written shows
    out = _run(c, workspace=ws)
    assert out.shape == (c.T, c.Hq, ao.D_HEAD) and out.is_contiguous()
    if c.ref_unquantised is not None:
        # a description of the format, not an assertion
        print(f"\nAPPEND_FP8 format {name} err_vs_unquantised="
              f"{ao.row_rel_err(out, c.ref_unquantised):.4f}")
    _check(_family(c), name, out, c.ref, c.tol)


@pytest.mark.parametrize(
    "name", ["b2_g1_bs16_s1", "b2_g4_bs128_s4", "b5_g2_bs128_s8", "b5_g8_bs32_s3", "b9_g4_bs32_s4"])
def test_all_single_token_rows_match_fp8_decode_oracle(name):
    """An all-L=1 append batch is decode attention: same codes and scales,
    same oracle, same tolerance as the fp8 decode case."""
    c = kf.fp8_case(name)
    cu = torch.arange(c.B + 1, dtype=torch.int32, device=DEV)
    out = ops.attention_append_paged_fp8(
        c.q.to(DEV), c.k_codes.to(DEV), c.v_codes.to(DEV), c.k_scale.to(DEV),
        c.v_scale.to(DEV), c.bt.to(DEV), c.lens.to(DEV), cu, 1, scale=c.scale,
        nsplit=c.nsplit,
    )
    _check("fp8_l1", name, out, c.ref, c.tol)


def test_append_fp8_after_quantising_write():
    """The engine's order: the cache holds quantised past keys,
    rope_kv_fused_fp8 ropes q in place and writes the new tokens' codes and
    scales at their real positions, then append attention reads them there.
    Oracle: the dequantised codes and scales read back from the device, with
    the GPU's own roped q."""
    B, G, Hk, bs, D = 2, 4, 2, 32, ao.D_HEAD
    Hq = G * Hk
    lens, qlens, nsplit = [150, 41], [9, 4], 3
    gen = torch.Generator().manual_seed(77)
    nblk = [-(-n // bs) for n in lens]
    nb = sum(nblk) + 1
    kc = (torch.randn(nb, bs, Hk, D, generator=gen) * ao.PEAK).to(torch.bfloat16)
    vc = torch.randn(nb, bs, Hk, D, generator=gen).to(torch.bfloat16)
    ids = torch.randperm(nb - 1, generator=gen).tolist()
    bt = torch.full((B, max(nblk) + 1), nb - 1, dtype=torch.int32)     # poison behind
    kc[nb - 1] = 30.0
    vc[nb - 1] = 50.0
    T = sum(qlens)
    raw = (torch.randn(T, (Hq + 2 * Hk) * D, generator=gen) * ao.PEAK).to(torch.bfloat16)
    raw[:, (Hq + Hk) * D:] /= ao.PEAK
    pos, slots, cu = [], [], [0]
    for b in range(B):
        mine = [ids.pop() for _ in range(nblk[b])]
        bt[b, : nblk[b]] = torch.tensor(mine, dtype=torch.int32)
        for p in range(lens[b] - qlens[b], lens[b]):
            pos.append(p)
            slots.append(mine[p // bs] * bs + p % bs)
        cu.append(cu[-1] + qlens[b])
    pos_t = torch.tensor(pos, dtype=torch.int32)
    slot_t = torch.tensor(slots, dtype=torch.int32)
    cos, sin = ao.rope_tables()
    k_codes, k_scale = kf.quantise_cache(kc)
    v_codes, v_scale = kf.quantise_cache(vc)

    rawd = raw.to(DEV)
    qd = rawd[:, : Hq * D].view(T, Hq, D)
    kd = rawd[:, Hq * D: (Hq + Hk) * D].view(T, Hk, D)
    vd = rawd[:, (Hq + Hk) * D:].view(T, Hk, D)
    kcd, vcd, ksd, vsd = (t.to(DEV) for t in (k_codes, v_codes, k_scale, v_scale))
    before = kcd.clone()
    q2, _, _ = ops.rope_kv_fused_fp8(
        qd, kd, vd, kcd, vcd, ksd, vsd, cos.to(DEV), sin.to(DEV), pos_t.to(DEV),
        slot_t.to(DEV))
    # the writer wrote the new slots and nothing else
    changed = (kcd != before).flatten(2).any(dim=2).view(nb * bs)
    assert set(changed.nonzero().flatten().tolist()) <= set(slots)
    assert changed.sum().item() == T
    out = ops.attention_append_paged_fp8(
        q2, kcd, vcd, ksd, vsd, bt.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV),
        torch.tensor(cu, dtype=torch.int32, device=DEV), max(qlens), nsplit=nsplit)

    kc_eff = kf.dequantise_cache(kcd.cpu(), ksd.cpu())
    vc_eff = kf.dequantise_cache(vcd.cpu(), vsd.cpu())
    args = (kc_eff, vc_eff, bt, lens, cu)
    q_cpu = q2.cpu().contiguous()
    ref = ac.append_oracle(q_cpu, *args)
    noise = ao.row_rel_err(ac.append_emulation(q_cpu, *args), ref)
    _check("fp8_rope_kv", "g4_hk2_bs32_s3", out, ref, ao.TOL_FACTOR * noise)


@pytest.mark.parametrize("mutant", ["v_scale_from_slot+1", "kv_scales_exchanged"])
def test_real_kernel_with_wrong_scales_is_caught(mutant):
    """The comparison itself, checked on the GPU: the real kernel fed a
    mutant's scales is at least 4 T from the true oracle, and within the
    mutant's own 4 N of the CPU mutant's oracle."""
    c = afc.fp8_append_case("g4_hk2_bs32_s3")
    ks, vs = c.scale_mutants()[mutant]
    out = _run(c, k_scale=ks, v_scale=vs)
    err_true = ao.row_rel_err(out, c.ref)
    tol_mut = ao.TOL_FACTOR * c.scale_mutant_noise(ks, vs)
    err_mut = ao.row_rel_err(out, c.scale_mutant_ref(ks, vs))
    print(f"\nAPPEND_FP8 mutant {mutant} err_true={err_true:.5f} T={c.tol:.5f} "
          f"ratio={err_true / c.tol:.1f} err_mutant={err_mut:.5f} T_mutant={tol_mut:.5f} "
          f"ratio={err_mut / tol_mut:.3f}")
    assert err_true >= ao.MUTANT_FACTOR * c.tol
    assert err_mut <= tol_mut


def test_output_inside_a_nan_filled_buffer():
    """The C entry with `out` pointing into the middle of a NaN-filled
    tensor: every output element is finite, every bit outside is unchanged."""
    from opsagent_amd.ops import hip_lib

    c = afc.fp8_append_case("mixed_g4_hk2_bs16_s4")
    D = ao.D_HEAD
    n_out = c.T * c.Hq * D
    pad = 4096
    buf = torch.full((pad + n_out + pad,), float("nan"), dtype=torch.bfloat16, device=DEV)
    bits0 = buf.view(torch.int16).clone()
    q = c.q.contiguous().to(DEV)
    ten = [t.to(DEV) for t in (c.k_codes, c.v_codes, c.k_scale, c.v_scale, c.bt, c.lens, c.cu)]
    o_part, ml_part = ops.append_workspace(
        c.B, c.T, c.Hk, c.G, c.nsplit, device=DEV, max_q=c.max_q)
    lib = hip_lib.get_lib()
    rc = lib.oa_attention_append_fp8(
        hip_lib.current_stream_ptr(), q.data_ptr(), *(t.data_ptr() for t in ten),
        o_part.data_ptr(), ml_part.data_ptr(), buf.data_ptr() + 2 * pad,
        c.B, c.T, c.Hq, c.Hk, D, c.bt.shape[1], c.bs, c.nsplit, D ** -0.5, q.stride(0),
        c.max_q)
    assert rc == 0
    torch.cuda.synchronize()
    inner = buf[pad: pad + n_out]
    assert torch.isfinite(inner.float()).all()
    bits1 = buf.view(torch.int16)
    assert torch.equal(bits1[:pad], bits0[:pad]) and torch.equal(bits1[pad + n_out:], bits0[pad + n_out:])
    _check(_family(c), c.name + "_in_buffer", inner.view(c.T, c.Hq, D), c.ref, c.tol)


def test_launcher_rejects_what_it_does_not_serve():
    c = afc.fp8_append_case("g2_hk2_bs32_s2")
    args = tuple(t.to(DEV) for t in (c.k_codes, c.v_codes, c.k_scale, c.v_scale, c.bt, c.lens, c.cu))
    with pytest.raises(RuntimeError, match="-104"):
        ops.attention_append_paged_fp8(c.q.to(DEV), *args, ops.append_max_q(c.G) + 1)
    q3 = torch.zeros(c.T, 3 * c.Hk, ao.D_HEAD, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="-102"):
        ops.attention_append_paged_fp8(q3, *args, 4)


# ------------------------------------------------------------------- engine
MICRO_CFG = {
    "model": "llama3-micro",
    "max_seq_len": 2048,
    "kv_block_size": 32,
    "kv_cache_gb": 2,
    "max_batch_size": 8,
    "use_hipgraph": True,
    "seed": 5,
    "kv_cache_dtype": "fp8",
    "append_attention_fp8": True,
}


def _metric_sum(name):
    from opsagent_amd.utils.perf import get_perf_stats

    s = get_perf_stats().get_metric_stats(name)
    return 0.0 if s is None else s["count"] * s["avg"]


def test_engine_append_attention_fp8_gpu():
    """fp8 KV with the key on, HIP path: jump-ahead catch-ups run as append
    steps over the fp8 cache, the output is deterministic across runs and
    always grammar-valid, a mixed batch completes, and verify takes the
    append path on a repeating prompt."""
    from opsagent_amd.engine.engine import LLMEngine, SamplingParams
    from opsagent_amd.engine.grammar import GrammarMode
    from opsagent_amd.utils.perf import get_perf_stats

    get_perf_stats().reset()
    eng = LLMEngine(dict(MICRO_CFG, grammar_ff_max_batch=64, spec_decode=True, spec_min_ema=0.0))
    assert eng.kv_cache_dtype == "fp8"
    assert eng.cache_stats()["append_attention"] is True
    tok = eng.tokenizer
    ids = tok.encode("emit a tool prompt", add_bos=True)
    for mode in (GrammarMode.TOOLPROMPT, GrammarMode.TOOLCALLS):
        out1, r1 = eng.generate(ids, SamplingParams(max_new_tokens=96, grammar=mode))
        out2, r2 = eng.generate(ids, SamplingParams(max_new_tokens=96, grammar=mode))
        assert (out1, r1) == (out2, r2), f"fp8 append attention nondeterministic for {mode}"
        assert r1.startswith("grammar")
        json.loads(tok.decode_text(out1))
    steps = _metric_sum("engine_append_steps")
    assert steps > 0

    # mixed batch: grammar rows (catch-ups) beside plain decode rows
    rids = [
        eng.add_request(
            tok.encode(f"mixed row {i} " + "pod " * i, add_bos=True),
            SamplingParams(max_new_tokens=48,
                           grammar=GrammarMode.TOOLPROMPT if i % 2 == 0 else None))
        for i in range(6)
    ]
    for _ in range(4000):
        if all(eng.requests[r].finished for r in rids):
            break
        eng.step()
    done = [eng.requests.pop(r) for r in rids]
    assert all(r.finished and r.finish_reason != "kv_exhausted" for r in done)
    for i, r in enumerate(done):
        if i % 2 == 0 and r.finish_reason.startswith("grammar"):
            json.loads(tok.decode_text(r.output_ids))
    assert _metric_sum("engine_append_rows") > _metric_sum("engine_append_steps")

    # speculative verify on a repeating prompt
    before = _metric_sum("engine_append_steps")
    ids = tok.encode("repeat repeat repeat repeat", add_bos=True)
    out1, _ = eng.generate(ids, SamplingParams(max_new_tokens=48))
    out2, _ = eng.generate(ids, SamplingParams(max_new_tokens=48))
    assert out1 == out2 and len(out1) > 0
    assert eng.spec_stats["verify_passes"] > 0, "verify never engaged"
    assert _metric_sum("engine_append_steps") > before
    del eng
    torch.cuda.empty_cache()
