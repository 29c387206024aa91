"""Whole-model oracle for the fp8 KV cache on the CPU: a simulated device
(the bf16 emulation attending its own quantised cache) passes the row and
the write criterion, every mutant of the read and the write side lands
>= 4x its bound or is a recorded gap, and a CPU engine with
kv_cache_dtype fp8 runs under the recorder that the GPU test uses. See
docs/KERNELS.md, "whole model, fp8 KV cache"."""

import functools

import pytest
import torch

import model_cases as mc
import model_fp8_cases as f8
from opsagent_amd.engine.config import get_model_spec
from opsagent_amd.engine.engine import LLMEngine
from opsagent_amd.engine.model import LlamaForCausalLM

CPU_CFG = {
    "model": "llama3-micro",
    "max_seq_len": 512,
    "kv_block_size": 32,
    "kv_num_blocks": 48,
    "max_batch_size": 8,
    "use_hipgraph": False,
    "spec_decode": False,
    "seed": 5,
    "kv_cache_dtype": "fp8",
}

# Measured err / T where a mutant stays under 4 T (see docs/KERNELS.md).
# A key read unquantised differs from the cache's value by that key's own
# quantisation error, which is what two correct quantisers may differ by, so
# no constructed model separates the two; the whole cold prefill read that
# way (the bf16 path's form) reaches 1.4 to 2.7 T. The newest key not
# attended is the bf16 suite's gap on the same two scenarios.
KNOWN_GAPS = {
    ("own_key_unquantised", "solo"): 0.66, ("own_key_unquantised", "batch"): 0.68,
    ("own_key_unquantised", "chunked"): 0.40, ("own_key_unquantised", "prefix"): 0.48,
    ("own_key_unquantised", "verify"): 0.87, ("own_key_unquantised", "catchup"): 0.60,
    ("cold_prefill_unquantised", "solo"): 2.73, ("cold_prefill_unquantised", "batch"): 1.89,
    ("cold_prefill_unquantised", "chunked"): 1.58, ("cold_prefill_unquantised", "prefix"): 2.08,
    ("cold_prefill_unquantised", "verify"): 2.21, ("cold_prefill_unquantised", "catchup"): 1.41,
    ("newest_key_dropped", "chunked"): 3.21, ("newest_key_dropped", "prefix"): 2.21,
}


@functools.lru_cache(maxsize=None)
def micro_weights():
    spec = get_model_spec("llama3-micro")
    model = LlamaForCausalLM(spec, torch.bfloat16, "cpu", 5)
    mc.construct_model_(model)
    return mc.weights_of(model)


@functools.lru_cache(maxsize=None)
def simulated(name):
    W = micro_weights()
    S = mc.scripted(name, get_model_spec("llama3-micro").vocab_size)
    rows, dev = f8.simulate(W, S)
    sc = S.script
    J = f8.judge(W, sc.tok, sc.positions(), sc.count(), dev.cache(), f8.roots_of(S),
                 f8.gathered_rows(S), bf16=True)
    return S, rows, dev, J


@pytest.mark.parametrize("name", mc.SCRIPTED)
def test_simulated_device_passes_both_criteria(name):
    S, rows, dev, J = simulated(name)
    ratio = f8.row_ratios(J, rows)
    val, sc = J["val_ratio"], J["scale_ratio"]
    N_w, N_k = J["N_w"], J["N_k"]
    print(f"{name}: entries {len(S.script)} N {max(J['N']):.3e} T {4 * max(J['N']):.3e} "
          f"N_w K {float(N_w[:, 0].max()):.4f} V {float(N_w[:, 1].max()):.4f} "
          f"N_k K {float(N_k[:, 0].max()):.2e} V {float(N_k[:, 1].max()):.2e} | "
          f"row {max(ratio):.3f} value {float(val.max()):.3f} scale {float(sc.max()):.3f}")
    assert max(ratio) <= 1.0
    assert float(val.max()) <= 1.0 and float(sc.max()) <= 1.0
    # forcing brings N back to the bf16 level; N_w is at most the half step of
    # e4m3's top binade (16 / 448 of the row's absmax) plus the row's own
    # error N_k, and a root's worst row comes close to the half step
    assert 1e-3 < max(J["N"]) < 6e-2
    assert 16 / 448 * 0.9 < float(N_w.min())
    assert bool((N_w <= 16 / 448 * (1 + N_k) + N_k).all())
    # one code step of the top binade stays inside the value bound
    assert 32 / 448 < f8.TOL_FACTOR * float(N_w.min())


def _margins(mutant, fn):
    applied = 0
    for name in mc.SCRIPTED:
        ratio = fn(name)
        if ratio is None:
            continue
        applied += 1
        print(f"{mutant} on {name}: {ratio:.2f}")
        gap = KNOWN_GAPS.get((mutant, name))
        if gap is not None:
            assert ratio < f8.MUTANT_FACTOR, "no longer a gap: drop it from KNOWN_GAPS"
            assert ratio == pytest.approx(gap, abs=0.05)
        else:
            assert ratio >= f8.MUTANT_FACTOR, f"{mutant} on {name}: {ratio:.2f}"
    assert applied >= 1


@pytest.mark.parametrize("mutant", f8.READ_MUTANTS)
def test_read_mutant_margin(mutant):
    """err(mutant, forced oracle) / T on the simulated device's codes."""
    W = micro_weights()

    def one(name):
        S, _, dev, J = simulated(name)
        return f8.read_mutant_margin(S, mutant, W, dev.cache(), J["hidden"], max(J["N"]))

    _margins(mutant, one)


@pytest.mark.parametrize("mutant", f8.WRITE_MUTANTS)
def test_write_mutant_margin(mutant):
    """The write criterion's larger figure over its bound, largest entry."""
    def one(name):
        _, _, dev, J = simulated(name)
        return f8.write_mutant_margin(J, dev, mutant)

    _margins(mutant, one)


# --------------------------------------------------------------------------
# the CPU engine with an fp8 cache through the recorder
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    e = LLMEngine(dict(CPU_CFG))
    mc.construct_model_(e.model)
    assert e.kv.fp8
    return e


@pytest.mark.parametrize("name", ["solo", "batch", "prefix"])
def test_cpu_engine_scenario(engine, name):
    rec, params = mc.run_scenario(name, engine, exact=True, recorder=f8.Fp8Recorder)
    assert rec.records and rec.padding_rows == 0 and rec.integrity_checks > 0
    bf16 = engine.model.embed.dtype == torch.bfloat16
    J = f8.check_recorded(mc.weights_of(engine.model), rec, bf16=bf16)
    val, sc = float(J["val_ratio"].max()), float(J["scale_ratio"].max())
    print(f"{name}: {len(rec.records)} rows, N {max(J['N']):.3e}, row {max(J['ratio']):.3f} "
          f"value {val:.3f} scale {sc:.3f}, integrity {rec.integrity_checks} steps "
          f"{rec.integrity_slots} slots")
    assert max(J["ratio"]) <= 1.0
    assert val <= 1.0 and sc <= 1.0
    assert mc.check_tokens(engine, rec, params) > 0
