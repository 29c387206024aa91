"""Every engine forward path on the MI355X against the whole-model fp64
oracle: each hidden row the engine computes, on any path, must lie within
T = 4 N of the oracle of the token prefix it was computed for, and every
greedy token must be the argmax of its own row's logits. Machinery, the
constructed model and the CPU proof of the mutant margins:
tests/model_cases.py, tests/test_model_oracle.py; docs/KERNELS.md,
"Verification method"."""

import collections

import pytest
import torch

import model_cases as mc

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
}

# variant -> (config overrides, environment, ops that must run on a GPU tensor,
#             ops that must not)
VARIANTS = {
    "graphed": ({}, {}, ["attention_decode_rope", "head_argmax"], []),
    "eager": ({"use_hipgraph": False}, {}, ["attention_decode_rope", "head_argmax"], []),
    "rope_unfused": ({}, {"OPSAGENT_ROPE_ATTN_FUSED": "0"},
                     ["rope_kv_fused", "attention_decode_paged"], ["attention_decode_rope"]),
    "fused_norm": ({}, {"OPSAGENT_FUSED_DECODE_MAX_B": "8", "OPSAGENT_DECODE_FUSED_MAX_B": "8"},
                   ["linear_norm", "linear_addres", "gateup_silu_norm",
                    "attention_decode_rope:fused_combine"], []),
    "append": ({"append_attention": True}, {}, ["attention_append_paged"], []),
}
WATCHED = ["attention_decode_rope", "attention_decode_paged", "rope_kv_fused", "head_argmax",
           "linear_norm", "linear_addres", "gateup_silu_norm", "attention_append_paged",
           "attention_prefill"]

_ENGINES = {}
_WEIGHTS = {}
_CALLS = collections.defaultdict(collections.Counter)     # variant -> op -> GPU calls
_RESULTS = {}                                             # (variant, scenario) -> recorder


def _enter(variant, monkeypatch):
    """Environment, the cached module global and the op counters of one
    variant; the engine is built under them the first time."""
    from opsagent_amd import ops
    from opsagent_amd.engine import model as model_mod
    from opsagent_amd.engine.engine import LLMEngine

    over, env, _, _ = VARIANTS[variant]
    for k in ("OPSAGENT_ROPE_ATTN_FUSED", "OPSAGENT_FUSED_DECODE_MAX_B",
              "OPSAGENT_DECODE_FUSED_MAX_B", "OPSAGENT_APPEND_ATTN", "OPSAGENT_FUSED_HEAD",
              "OPSAGENT_FUSED_SAMPLER", "OPSAGENT_KV_CACHE_DTYPE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(model_mod, "_ROPE_ATTN_FUSED", None)   # re-read; restored afterwards
    counts = _CALLS[variant]
    for name in WATCHED:
        orig = getattr(ops, name)

        def w(*a, _orig=orig, _name=name, **k):
            if any(isinstance(t, torch.Tensor) and t.is_cuda for t in a):
                counts[_name] += 1
                if k.get("fused_combine"):
                    counts[_name + ":fused_combine"] += 1
            return _orig(*a, **k)

        monkeypatch.setattr(ops, name, w)
    if variant not in _ENGINES:
        e = LLMEngine(dict(MICRO_CFG, **over))
        mc.construct_model_(e.model)
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
    rec, params = mc.run_scenario(name, e)
    _RESULTS[(variant, name)] = rec
    res = mc.check_rows(W, rec.records, bf16=True)
    return e, W, rec, params, res


@pytest.mark.parametrize("name", list(mc.SCENARIOS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rows_and_tokens(variant, name, monkeypatch):
    e, W, rec, params, res = _run(variant, name, monkeypatch)
    for key, x in sorted(_paths(rec, res["ratio"]).items()):
        print(f"MODELORACLE {variant} {name} {' '.join(key)} err/T {x:.3f}")
    print(f"MODELORACLE {variant} {name} rows {len(rec.records)} padding {rec.padding_rows} "
          f"N {max(res['N']):.3e} T {4 * max(res['N']):.3e}")
    worst = max(res["ratio"])
    assert worst <= 1.0, f"{variant}/{name}: a row is {worst:.2f} T from its oracle"

    # the sampled rows' logits, one head GEMM over all of them
    sampled = [(r, i) for r, i in zip(rec.records, res["where"]) if r.sampled is not None]
    assert sampled
    with torch.inference_mode():
        got = e.model.compute_logits(torch.stack([r.row for r, _ in sampled]))
    lr = 0.0
    for (r, i), g in zip(sampled, got):
        TL = mc.TOL_FACTOR * res["NL"][res["root_of"][i]]
        lr = max(lr, mc.row_rel_err(g[None].float(), res["logits"][i][None]) / TL)
    print(f"MODELORACLE {variant} {name} logits err/T {lr:.3f}")
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
    if name == "verify":
        assert ("verify+append" if variant == "append" else "verify") in kinds
    if name == "catchup":
        if variant == "append":
            mixed = [r for r in rec.records if r.kind == "append"]
            assert mixed and max(r.B for r in mixed) == 3
            assert "catchup" in kinds                  # 17 tokens: prefill form
        else:
            assert "catchup" in kinds


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
        assert c[op] > 0, f"{variant}: ops.{op.replace(':', ' with ')} never ran on the GPU"
    for op in must_not:
        assert c[op] == 0, f"{variant}: ops.{op} ran"


@pytest.mark.parametrize("name", ["solo", "chunked", "prefix", "verify"])
def test_graphed_equals_eager_bitwise(name, monkeypatch):
    """Same kernels, same inputs: a graphed decode row whose bucket equals B
    is bit-identical to the eager one. Compared on the scenarios that run one
    request at a time, where every earlier step that filled the cache also
    ran at bucket == B (in a batch the cache behind a B = 4 step was written
    by a B = 5 step that the graph ran at M = 8)."""
    recs = {}
    for variant in ("graphed", "eager"):
        if (variant, name) not in _RESULTS:
            with pytest.MonkeyPatch.context() as mp:
                _run(variant, name, mp)
        recs[variant] = _RESULTS[(variant, name)]
    # two requests of one scenario can share a prefix (verify repeats the
    # plain run's prompt) behind different cache histories: pair the rows
    # request by request, in the order the requests were added
    def by_request(rec):
        order = {rid: i for i, rid in enumerate(sorted(rec.prompt_len))}
        return {(order[r.rid], r.prefix): r for r in rec.records if r.kind == "decode"}

    eager = by_request(recs["eager"])
    graphed = by_request(recs["graphed"])
    assert len(graphed) >= 5
    for key, r in graphed.items():
        assert r.graphed and r.bucket == r.B
        assert key in eager, "the two runs sampled different tokens"
        assert torch.equal(r.row, eager[key].row), f"request {key[0]}, position {r.pos} differs"


@pytest.mark.parametrize("mutant", ["norms_exchanged", "rope_rolled"])
def test_gpu_comparison_checks_itself(mutant, monkeypatch):
    """The engine with two norm weights of layer 1 exchanged, or with its
    RoPE tables rolled by one position, must leave the true oracle by >= 4 T,
    as far as the CPU mutant predicts, and match the mutant's own oracle."""
    e, W = _enter("eager", monkeypatch)
    Wm = mc.mutate_weights(W, mutant)
    m = e.model
    L = m.layers[1]
    saved = [t.clone() for t in (L.input_norm_w.data, L.post_norm_w.data, m.rope_cos, m.rope_sin)]
    monkeypatch.setattr(mc, "SALT", 1000 if mutant == "norms_exchanged" else 2000)
    try:
        if mutant == "norms_exchanged":
            L.input_norm_w.data.copy_(saved[1])
            L.post_norm_w.data.copy_(saved[0])
        else:
            m.rope_cos.copy_(saved[2].roll(1, 0))
            m.rope_sin.copy_(saved[3].roll(1, 0))
        rec, _ = mc.run_scenario("solo", e)
    finally:
        for t, s in zip((L.input_norm_w.data, L.post_norm_w.data, m.rope_cos, m.rope_sin), saved):
            t.copy_(s)
    own = mc.check_rows(Wm, rec.records, bf16=True)
    true = mc.check_rows(W, rec.records, bf16=True)
    T = mc.TOL_FACTOR * max(true["N"])
    predicted = mc.row_rel_err(own["hidden"], true["hidden"]) / T
    got = max(true["ratio"])
    print(f"MODELORACLE selfcheck {mutant}: own {max(own['ratio']):.3f} T, true {got:.2f} T, "
          f"predicted {predicted:.2f} T")
    assert max(own["ratio"]) <= 1.0
    assert got >= mc.MUTANT_FACTOR
    assert abs(got - predicted) <= 1.5
