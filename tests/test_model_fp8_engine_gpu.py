"""Every engine forward path over the fp8 KV cache on the MI355X against the
teacher-forced whole-model fp64 oracle: each hidden row within T = 4 N of
the oracle that attends the device's own codes and scales, each written
code row and scale within the write criterion of the oracle's own k and v,
the cache bit-for-bit what its last recorded write left after every step,
and every greedy token the argmax of its own row. Machinery and the CPU
proof of the mutant margins: tests/model_fp8_cases.py,
tests/test_model_fp8_oracle.py; docs/KERNELS.md, "whole model, fp8 KV
cache"."""

import collections

import pytest
import torch

import model_cases as mc
import model_fp8_cases as f8

pytestmark = pytest.mark.gpu

MICRO_CFG = {
    "model": "llama3-micro",
    "max_seq_len": 512,
    "kv_block_size": 32,
    "kv_num_blocks": 48,
    "max_batch_size": 8,
    "use_hipgraph": True,
    "spec_decode": False,
    "seed": 5,
    "kv_cache_dtype": "fp8",
}

FP8_OPS = ["rope_kv_fused_fp8", "kv_gather_fp8", "attention_decode_paged_fp8"]
# variant -> (config overrides, environment, ops that must run on a GPU tensor,
#             ops that must not)
VARIANTS = {
    "graphed": ({}, {}, FP8_OPS, ["attention_decode_rope"]),
    "eager": ({"use_hipgraph": False}, {}, FP8_OPS, ["attention_decode_rope"]),
    "fused_norm": ({}, {"OPSAGENT_FUSED_DECODE_MAX_B": "8"},
                   FP8_OPS + ["linear_norm", "linear_addres", "gateup_silu_norm"],
                   ["attention_decode_rope"]),
    "append": ({"append_attention_fp8": True}, {},
               FP8_OPS + ["attention_append_paged_fp8"],
               ["attention_decode_rope", "attention_append_paged"]),
}
WATCHED = FP8_OPS + ["attention_append_paged_fp8", "attention_append_paged",
                     "attention_decode_rope", "attention_decode_paged", "rope_kv_fused",
                     "linear_norm", "linear_addres", "gateup_silu_norm", "attention_prefill"]

_ENGINES = {}
_WEIGHTS = {}
_CALLS = collections.defaultdict(collections.Counter)     # variant -> op -> GPU calls
_RESULTS = {}                                             # (variant, scenario) -> (rec, J)


def _enter(variant, monkeypatch):
    """Environment and the op counters of one variant; the engine is built
    under them the first time."""
    from opsagent_amd import ops
    from opsagent_amd.engine.engine import LLMEngine

    over, env, _, _ = VARIANTS[variant]
    for k in ("OPSAGENT_ROPE_ATTN_FUSED", "OPSAGENT_FUSED_DECODE_MAX_B",
              "OPSAGENT_DECODE_FUSED_MAX_B", "OPSAGENT_APPEND_ATTN", "OPSAGENT_APPEND_ATTN_FP8",
              "OPSAGENT_FUSED_HEAD", "OPSAGENT_FUSED_SAMPLER", "OPSAGENT_KV_CACHE_DTYPE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    counts = _CALLS[variant]
    for name in WATCHED:
        orig = getattr(ops, name)

        def w(*a, _orig=orig, _name=name, **k):
            if any(isinstance(t, torch.Tensor) and t.is_cuda for t in a):
                counts[_name] += 1
            return _orig(*a, **k)

        monkeypatch.setattr(ops, name, w)
    if variant not in _ENGINES:
        e = LLMEngine(dict(MICRO_CFG, **over))
        mc.construct_model_(e.model)
        assert e.kv.fp8 and e.kv.layers[0][0].is_cuda
        _ENGINES[variant] = e
        if "W" not in _WEIGHTS:
            _WEIGHTS["W"] = mc.weights_of(e.model)
    e = _ENGINES[variant]
    W = _WEIGHTS["W"]
    assert torch.equal(e.model.layers[1].post_norm_w.cpu().double(), W["layers"][1]["post_w"])
    assert torch.equal(e.model.layers[3].attn.qkv_w.cpu().double(), W["layers"][3]["qkv"])
    return e, W


def _paths(rec, ratios):
    worst = collections.defaultdict(float)
    for r, x in zip(rec.records, ratios):
        key = (r.kind, "graph" if r.graphed else "eager",
               f"B{r.B}/{r.bucket}" if r.kind == "decode" else "")
        worst[key] = max(worst[key], x)
    return worst


def _run(variant, name, monkeypatch):
    e, W = _enter(variant, monkeypatch)
    gathers = _CALLS[variant]["kv_gather_fp8"]
    rec, params = mc.run_scenario(name, e, recorder=f8.Fp8Recorder)
    # the row criterion cannot tell a key read unquantised from its cached
    # value (a recorded gap), so: every prefill-form forward, a cold one
    # included, went through the gather once per layer
    forwards = {r.call for r in rec.records if r.kind in f8.GATHER_KINDS}
    assert _CALLS[variant]["kv_gather_fp8"] - gathers == len(forwards) * len(e.kv.layers)
    J = f8.check_recorded(W, rec, bf16=True)
    _RESULTS[(variant, name)] = (rec, J)
    return e, W, rec, params, J


@pytest.mark.parametrize("name", list(mc.SCENARIOS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rows_writes_and_tokens(variant, name, monkeypatch):
    e, W, rec, params, J = _run(variant, name, monkeypatch)
    for key, x in sorted(_paths(rec, J["ratio"]).items()):
        print(f"MODELFP8 {variant} {name} {' '.join(key)} err/T {x:.3f}")
    val, sc = J["val_ratio"], J["scale_ratio"]
    print(f"MODELFP8 {variant} {name} rows {len(rec.records)} padding {rec.padding_rows} "
          f"N {max(J['N']):.3e} T {4 * max(J['N']):.3e} N_w {float(J['N_w'].max()):.4f} "
          f"N_k {float(J['N_k'].max()):.3e} value/bound {float(val.max()):.3f} "
          f"scale/bound {float(sc.max()):.3f} integrity {rec.integrity_checks} steps "
          f"{rec.integrity_slots} slots")
    worst = max(J["ratio"])
    assert worst <= 1.0, f"{variant}/{name}: a row is {worst:.2f} T from its forced oracle"
    for what, x in (("value", val), ("scale", sc)):
        if float(x.max()) > 1.0:
            l, kv, i, h = (x == x.max()).nonzero()[0].tolist()
            r = rec.records[i]
            raise AssertionError(
                f"{variant}/{name}: written {what} of layer {l} {'KV'[kv]} head {h}, {r.kind} "
                f"row of request {r.rid} at position {r.pos} (slot {r.slot}), is "
                f"{float(x.max()):.2f}x its bound")
    assert rec.integrity_checks > 0

    # the sampled rows' logits, one head GEMM over all of them
    sampled = [(r, i) for i, r in enumerate(rec.records) if r.sampled is not None]
    assert sampled
    with torch.inference_mode():
        got = e.model.compute_logits(torch.stack([r.row for r, _ in sampled]))
    lr = 0.0
    for (r, i), g in zip(sampled, got):
        TL = mc.TOL_FACTOR * J["NL"][J["root_of"][i]]
        lr = max(lr, mc.row_rel_err(g[None].float(), J["logits"][i][None]) / TL)
    print(f"MODELFP8 {variant} {name} logits err/T {lr:.3f}")
    assert lr <= 1.0
    assert mc.check_tokens(e, rec, params) == len(sampled)

    # what the scenario is there to drive
    kinds = {r.kind for r in rec.records}
    dec = {(r.B, r.bucket) for r in rec.records if r.kind == "decode"}
    if name == "batch":
        assert {b for b, _ in dec} == {1, 2, 3, 4, 5}
        if e.use_hipgraph:
            assert {(5, 8), (3, 4)} <= dec and rec.padding_rows > 0
    if not e.use_hipgraph:
        assert rec.padding_rows == 0
    if name == "preempt":
        assert rec.preemptions > 0
    if name == "verify":
        assert ("verify+append" if variant == "append" else "verify") in kinds
    if name == "catchup":
        if variant == "append":
            mixed = [r for r in rec.records if r.kind == "append"]
            assert mixed and max(r.B for r in mixed) == 3
        assert "catchup" in kinds                      # 17 tokens: prefill form


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variant_ran_its_ops(variant, monkeypatch):
    """A variant counts only if the op entries it is about ran on GPU
    tensors (graphed steps call them at capture)."""
    if not any(v == variant for v, _ in _RESULTS):
        _run(variant, "batch", monkeypatch)
    if variant == "append" and (variant, "catchup") not in _RESULTS:
        _run(variant, "catchup", monkeypatch)
    _, _, must, must_not = VARIANTS[variant]
    c = _CALLS[variant]
    for op in must:
        assert c[op] > 0, f"{variant}: ops.{op} never ran on the GPU"
    for op in must_not + ["attention_decode_paged", "rope_kv_fused"]:
        assert c[op] == 0, f"{variant}: ops.{op} ran"


@pytest.mark.parametrize("name", ["solo", "chunked", "prefix", "verify"])
def test_graphed_equals_eager_bitwise(name, monkeypatch):
    """Same kernels, same inputs: on the scenarios that run one request at a
    time (bucket == B for every step) the graphed and the eager engine
    compute the same rows in the same order and leave the same codes and
    scales, bit for bit."""
    got = {}
    for variant in ("graphed", "eager"):
        if (variant, name) not in _RESULTS:
            with pytest.MonkeyPatch.context() as mp:
                _run(variant, name, mp)
        got[variant] = _RESULTS[(variant, name)][0]
    g, e = got["graphed"], got["eager"]
    assert [(r.kind, r.prefix) for r in g.records] == [(r.kind, r.prefix) for r in e.records], (
        "the two runs sampled different tokens")
    dec = [r for r in g.records if r.kind == "decode"]
    assert len(dec) >= 5 and all(r.graphed and r.bucket == r.B for r in dec)
    for i, (a, b) in enumerate(zip(g.records, e.records)):
        assert torch.equal(a.row, b.row), f"{a.kind} row {i} at position {a.pos} differs"
    cg, ce = g.cache(), e.cache()
    assert torch.equal(cg.codes, ce.codes)
    assert torch.equal(cg.scales.view(torch.int32), ce.scales.view(torch.int32))


def _read_side_mutant(e, mutant, monkeypatch):
    """Wrap the ops that read the cache so that they get the K and V scale
    tensors exchanged, or the scale tensors of the layer below."""
    from opsagent_amd import ops

    layer_of = {ks.data_ptr(): l for l, (ks, _) in enumerate(e.kv.scales)}
    seen = collections.Counter()

    def scales(ks, vs):
        assert ks.is_cuda
        l = layer_of[ks.data_ptr()]
        seen[l] += 1
        if mutant == "kv_scales_exchanged":
            return vs, ks
        return e.kv.scales[max(l - 1, 0)]

    for name, at in (("kv_gather_fp8", 2), ("attention_decode_paged_fp8", 3)):
        orig = getattr(ops, name)

        def w(*a, _orig=orig, _at=at, **k):
            a = list(a)
            a[_at], a[_at + 1] = scales(a[_at], a[_at + 1])
            return _orig(*a, **k)

        monkeypatch.setattr(ops, name, w)
    return seen


@pytest.mark.parametrize("mutant", ["kv_scales_exchanged", "scales_prev_layer"])
def test_gpu_comparison_checks_itself(mutant, monkeypatch):
    """The engine reading the cache with its K and V scale tensors
    exchanged, or layer l's codes with the scales of layer l - 1 (the write
    side untouched), must leave the true forced oracle by >= 4 T, as far as
    the same mutant of the oracle predicts, and match that mutant's oracle."""
    e, W = _enter("eager", monkeypatch)
    seen = _read_side_mutant(e, mutant, monkeypatch)
    monkeypatch.setattr(mc, "SALT", 1000 if mutant == "kv_scales_exchanged" else 2000)
    rec, _ = mc.run_scenario("solo", e, recorder=f8.Fp8Recorder)
    assert set(seen) == set(range(len(e.kv.scales)))
    true = f8.check_recorded(W, rec, bf16=True)
    own = f8.check_recorded(W, rec, bf16=True, values=f8.mutate_values(rec.cache(), mutant))
    T = mc.TOL_FACTOR * max(true["N"])
    predicted = mc.row_rel_err(own["hidden"], true["hidden"]) / T
    got = max(true["ratio"])
    wr = max(float(own["val_ratio"].max()), float(own["scale_ratio"].max()))
    print(f"MODELFP8 selfcheck {mutant}: own {max(own['ratio']):.3f} T, write {wr:.3f}, "
          f"true {got:.2f} T, predicted {predicted:.2f} T")
    assert max(own["ratio"]) <= 1.0 and wr <= 1.0
    assert got >= mc.MUTANT_FACTOR
    assert abs(got - predicted) <= 1.5
