"""The engine's fused-sampler path on CPU (ops.sample_masked falls to
torch_ref.sample_masked there): default off, seeded determinism, batch
independence, greedy equivalences, logit_bias, and the seed's way through the
wire format and the chat-completions handler."""

import json

import pytest

from opsagent_amd import ops
from opsagent_amd.engine import engine as engine_mod
from opsagent_amd.engine.engine import (
    LLMEngine, SamplingParams, _params_from_wire, _params_to_wire,
)

TINY_CFG = {
    "model": "llama3-tiny",
    "max_seq_len": 256,
    "kv_block_size": 16,
    "max_batch_size": 8,
    "use_hipgraph": False,
    "seed": 7,
}


@pytest.fixture(scope="module")
def fused():
    return LLMEngine(dict(TINY_CFG, fused_sampler=True))


@pytest.fixture(scope="module")
def legacy():
    return LLMEngine(dict(TINY_CFG))


def run_batch(eng, prompts, params):
    rids = [eng.add_request(p, sp) for p, sp in zip(prompts, params)]
    while not all(eng.requests[r].finished for r in rids):
        eng.step()
    return [eng.requests.pop(r).output_ids for r in rids]


def prompt(eng, text):
    return eng.tokenizer.encode(text, add_bos=True)


def test_exports_and_default_off(legacy, monkeypatch):
    assert "sample_masked" in ops.__all__ and "sample_ws_bytes" in ops.__all__
    assert legacy.fused_sampler is False
    calls = {"transform": 0, "fused": 0}
    real = LLMEngine._transform_logits

    def spy(self, batch, lf):
        calls["transform"] += 1
        return real(self, batch, lf)

    def never(*a, **k):
        calls["fused"] += 1
        raise AssertionError("ops.sample_masked called with fused_sampler off")

    monkeypatch.setattr(LLMEngine, "_transform_logits", spy)
    monkeypatch.setattr(engine_mod.ops, "sample_masked", never)
    out, _ = legacy.generate(prompt(legacy, "legacy path"),
                             SamplingParams(max_new_tokens=6, temperature=0.9, seed=3))
    assert calls["transform"] > 0 and calls["fused"] == 0 and len(out) > 0


def test_environment_switch(monkeypatch):
    monkeypatch.setenv("OPSAGENT_FUSED_SAMPLER", "1")
    assert LLMEngine(dict(TINY_CFG)).fused_sampler is True
    assert LLMEngine(dict(TINY_CFG, fused_sampler=False)).fused_sampler is False


def test_key_on_skips_the_legacy_transform(fused, monkeypatch):
    def never(*a, **k):
        raise AssertionError("_transform_logits called with fused_sampler on")

    monkeypatch.setattr(LLMEngine, "_transform_logits", never)
    out, _ = fused.generate(prompt(fused, "fused path"),
                            SamplingParams(max_new_tokens=6, temperature=0.9, seed=3))
    assert len(out) > 0


def test_same_seed_same_ids_other_seed_differs(fused):
    ids = prompt(fused, "sampling with a seed")
    sp = dict(max_new_tokens=24, temperature=1.0, top_p=0.95)
    a, _ = fused.generate(ids, SamplingParams(seed=42, **sp))
    b, _ = fused.generate(ids, SamplingParams(seed=42, **sp))
    c, _ = fused.generate(ids, SamplingParams(seed=43, **sp))
    assert a == b
    assert a != c


def test_seed_differing_in_the_high_word_only(fused):
    ids = prompt(fused, "sampling with a seed")
    sp = dict(max_new_tokens=24, temperature=1.0)
    a, _ = fused.generate(ids, SamplingParams(seed=42, **sp))
    b, _ = fused.generate(ids, SamplingParams(seed=42 + (1 << 32), **sp))
    assert a != b


def test_solo_equals_batched_beside_sampled_neighbours(fused):
    ids = prompt(fused, "one request among others")
    mine = SamplingParams(max_new_tokens=16, temperature=0.9, top_k=50, seed=99)
    solo, _ = fused.generate(ids, mine)
    others = [SamplingParams(max_new_tokens=16, temperature=1.1, top_p=0.9, seed=s,
                             presence_penalty=0.5) for s in (1, 2, 3)]
    prompts = [prompt(fused, t) for t in ("first other", "second one", "third neighbour")]
    outs = run_batch(fused, prompts[:1] + [ids] + prompts[1:], others[:1] + [mine] + others[1:])
    assert outs[1] == solo


@pytest.mark.parametrize("which", ["fused", "legacy"])
def test_greedy_beside_sampled_equals_solo_greedy(which, fused, legacy):
    eng = fused if which == "fused" else legacy
    ids = prompt(eng, "a greedy request")
    greedy = SamplingParams(max_new_tokens=12)
    solo, _ = eng.generate(ids, greedy)
    others = [SamplingParams(max_new_tokens=12, temperature=1.0, seed=s) for s in (5, 6)]
    outs = run_batch(eng, [prompt(eng, "noise a"), ids, prompt(eng, "noise b")],
                     [others[0], greedy, others[1]])
    assert outs[1] == solo


def test_top_k_1_and_tiny_top_p_equal_greedy(fused):
    ids = prompt(fused, "filters that leave one token")
    # a bias makes the maximum unique: tied maxima may legally draw either
    bias = {65: 4.0}
    g, _ = fused.generate(ids, SamplingParams(max_new_tokens=8, logit_bias=bias))
    k1, _ = fused.generate(ids, SamplingParams(max_new_tokens=8, temperature=1.3, top_k=1,
                                               logit_bias=bias, seed=1))
    p0, _ = fused.generate(ids, SamplingParams(max_new_tokens=8, temperature=1.3, top_p=1e-9,
                                               logit_bias=bias, seed=2))
    assert g == k1 == p0


def test_logit_bias_steers(fused):
    ids = prompt(fused, "steer me")
    out, _ = fused.generate(ids, SamplingParams(max_new_tokens=6, temperature=0.7, seed=8,
                                                logit_bias={"66": 100.0}, stop_on_eos=False))
    assert out == [66] * 6
    # a frequency penalty large enough forbids repeats
    out, _ = fused.generate(ids, SamplingParams(max_new_tokens=12, frequency_penalty=100.0))
    assert len(set(out)) == len(out)


def test_default_seed_replays_with_the_request_stream():
    outs = []
    for _ in range(2):
        eng = LLMEngine(dict(TINY_CFG, fused_sampler=True))
        ids = prompt(eng, "no seed given")
        outs.append([eng.generate(ids, SamplingParams(max_new_tokens=10, temperature=1.0))[0]
                     for _ in range(2)])
    assert outs[0] == outs[1]
    assert outs[0][0] != outs[0][1]  # the request id enters the derived seed


def test_seed_survives_the_wire():
    p = SamplingParams(temperature=0.5, seed=(1 << 40) + 3)
    q = _params_from_wire(json.loads(json.dumps(_params_to_wire(p))))
    assert q.seed == p.seed and q == p
    assert _params_from_wire(_params_to_wire(SamplingParams())).seed is None


def test_chat_completions_accepts_seed():
    from fastapi.testclient import TestClient

    from opsagent_amd.config import Config, DEFAULTS
    from opsagent_amd.engine.openai_api import ChatCompletionAPI
    from opsagent_amd.server.app import create_app

    ChatCompletionAPI.reset_instance()
    cfg = Config(json.loads(json.dumps(DEFAULTS)))
    cfg._data["engine"] = dict(TINY_CFG, max_seq_len=512, grammar="auto", open_api=True,
                               fused_sampler=True)
    try:
        with TestClient(create_app(cfg)) as client:
            body = {"model": "llama3-tiny", "messages": [{"role": "user", "content": "hi"}],
                    "max_tokens": 12, "temperature": 1.0, "seed": 77}
            a = client.post("/v1/chat/completions", json=body)
            b = client.post("/v1/chat/completions", json=body)
            c = client.post("/v1/chat/completions", json=dict(body, seed=78))
            assert a.status_code == b.status_code == c.status_code == 200
            text = [r.json()["choices"][0]["message"]["content"] for r in (a, b, c)]
            assert text[0] == text[1]
            assert text[0] != text[2]
            r = client.post("/v1/chat/completions", json=dict(body, stream=True))
            assert r.status_code == 200 and "[DONE]" in r.text
    finally:
        ChatCompletionAPI.reset_instance()
