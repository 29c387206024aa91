"""GPU half of the seeded sampler's verification: every case of
tests/sampling_cases.py through ops.sample_masked against the fp64 oracle
(info exact, tokens under the draw window), bit-level reproducibility, a
self-check of the comparison with two real mutations of the kernel's inputs,
graph capture, and the engine with fused_sampler on."""

import json

import numpy as np
import pytest
import torch

import sampling_cases as sc

pytestmark = pytest.mark.gpu

R = sc.ROWS_PER_LAUNCH


class Packed:
    """The 16 rows every launch of a size shares (spec b % m in row b); only
    the steps change from launch to launch."""

    def __init__(self, V, rows=None, use_mask=True):
        self.V = V
        self.specs = sc.specs_for(V)
        m = len(self.specs)
        self.rows = list(range(R)) if rows is None else rows
        sp = [self.specs[b % m] for b in self.rows]
        dev = "cuda"
        self.logits = torch.from_numpy(np.stack([s.logits for s in sp])).to(dev).to(torch.bfloat16)
        ones = np.ones(V, bool)
        self.mask = None
        if use_mask:
            self.mask = torch.from_numpy(np.stack(
                [sc.pack_mask(s.mask if s.mask is not None else ones) for s in sp])).to(dev)
        self.inv_temp = torch.tensor([float(s.inv_temp) for s in sp], dtype=torch.float32, device=dev)
        self.top_k = torch.tensor([s.top_k for s in sp], dtype=torch.int32, device=dev)
        self.top_p = torch.tensor([s.top_p for s in sp], dtype=torch.float32, device=dev)
        self.seed = torch.from_numpy(np.array([s.seed for s in sp], np.uint64).view(np.int64)).to(dev)
        ptr = np.zeros(len(sp) + 1, np.int32)
        ptr[1:] = np.cumsum([s.adj_tok.shape[0] for s in sp])
        self.adj = (
            torch.from_numpy(ptr).to(dev),
            torch.from_numpy(np.concatenate([s.adj_tok for s in sp])).to(dev),
            torch.from_numpy(np.concatenate([s.adj_val for s in sp])).to(dev),
        )
        self.step0 = np.array([s.step0 for s in sp], np.uint64)

    def steps(self, n_launches):
        """int64 [L, rows]: row b of launch j draws step index (16 j + b) // m."""
        m = len(self.specs)
        j = np.arange(n_launches, dtype=np.uint64)[:, None]
        b = np.array(self.rows, np.uint64)[None, :]
        st = self.step0[None, :] + (np.uint64(R) * j + b) // np.uint64(m)
        return torch.from_numpy(st.view(np.int64)).cuda()

    def run(self, steps, mask=None):
        """One launch per row of `steps`; returns tokens [L, rows], info [L, rows, 2]."""
        from opsagent_amd import ops

        L, B = steps.shape
        out = torch.empty(L, B, dtype=torch.int32, device="cuda")
        info = torch.empty(L, B, 2, dtype=torch.int32, device="cuda")
        mk = self.mask if mask is None else mask
        for j in range(L):
            ops.sample_masked(self.logits, mk, self.inv_temp, self.top_k, self.top_p,
                              self.seed, steps[j], adj=self.adj, out=out[j], info=info[j])
        return out.cpu().numpy().astype(np.int64), info.cpu().numpy()


def by_spec(V, tokens):
    """tokens [L, 16] in launch order -> one array per spec in step order."""
    m = len(sc.specs_for(V))
    flat = tokens.reshape(-1)
    return [flat[i::m] for i in range(m)]


@pytest.fixture(scope="module")
def packed():
    return {V: Packed(V) for V in sc.VOCABS}


@pytest.fixture(scope="module")
def full_runs(packed):
    """Every draw of every size, once; shared by the tests below."""
    runs = {}
    for V, pk in packed.items():
        L = len(sc.launches(V))
        runs[V] = pk.run(pk.steps(L))
    return runs


@pytest.mark.parametrize("V", sc.VOCABS)
def test_every_case_matches_the_oracle(V, full_runs):
    tokens, info = full_runs[V]
    specs = sc.specs_for(V)
    m = len(specs)
    for b in range(R):
        want = (specs[b % m].expect.kept, specs[b % m].expect.zmin_bits)
        got = {(int(a), int(c)) for a, c in info[:, b, :]}
        assert got == {want}, (specs[b % m].name, got, want)
    for s, toks in zip(specs, by_spec(V, tokens)):
        wrong, amb = sc.compare(s.expect, toks)
        print(f"{s.name}: {toks.shape[0]} draws, {amb} ambiguous, {wrong} wrong")
        assert wrong == 0, s.name


@pytest.mark.parametrize("V", sc.VOCABS)
def test_batch_size_and_position_do_not_matter(V, packed, full_runs):
    tokens, info = full_runs[V]
    specs = sc.specs_for(V)
    m = len(specs)
    # B = 1: each spec alone, steps of launch 0; no mask tensor where the spec has none
    for i, s in enumerate(specs):
        pk = Packed(V, rows=[i], use_mask=s.mask is not None)
        t1, i1 = pk.run(pk.steps(1))
        assert t1[0, 0] == tokens[0, i], s.name
        assert (i1[0, 0] == info[0, i]).all(), s.name
    # B = 3: rows 0..2 of launch 0
    pk = Packed(V, rows=[0, 1, 2])
    t3, i3 = pk.run(pk.steps(1))
    assert (t3[0] == tokens[0, :3]).all() and (i3[0] == info[0, :3]).all()
    # the same 16 rows again: identical bits
    pk = packed[V]
    t2, i2 = pk.run(pk.steps(2))
    assert (t2 == tokens[:2]).all() and (i2 == info[:2]).all()


def test_writes_stay_inside_out_and_info(packed):
    from opsagent_amd import ops

    pk = packed[4104]
    steps = pk.steps(1)[0]
    out = torch.full((R + 8,), -777, dtype=torch.int32, device="cuda")
    info = torch.full((R + 4, 2), -777, dtype=torch.int32, device="cuda")
    ops.sample_masked(pk.logits, pk.mask, pk.inv_temp, pk.top_k, pk.top_p, pk.seed, steps,
                      adj=pk.adj, out=out[4:4 + R], info=info[2:2 + R])
    out, info = out.cpu(), info.cpu()
    assert (out[:4] == -777).all() and (out[4 + R:] == -777).all()
    assert (info[:2] == -777).all() and (info[2 + R:] == -777).all()
    assert (out[4:4 + R] != -777).all() and (info[2:2 + R] != -777).all()


@pytest.mark.parametrize("V", [40, 4104, 128256])
def test_greedy_rows_equal_masked_argmax(V):
    from opsagent_amd import ops

    B = 5
    g = torch.Generator().manual_seed(V)
    logits = (3 * torch.randn(B, V, generator=g)).to(torch.bfloat16).cuda()
    mask = torch.randint(-2**31, 2**31 - 1, (B, (V + 31) // 32), generator=g,
                         dtype=torch.int64).to(torch.int32).cuda()
    zeros_f = torch.zeros(B, dtype=torch.float32, device="cuda")
    zeros_i = torch.zeros(B, dtype=torch.int32, device="cuda")
    ones_f = torch.ones(B, dtype=torch.float32, device="cuda")
    z64 = torch.zeros(B, dtype=torch.int64, device="cuda")
    for mk in (None, mask):
        got = ops.sample_masked(logits, mk, zeros_f, zeros_i, ones_f, z64, z64)
        want = ops.greedy_sample_masked(logits, mk)
        assert torch.equal(got.cpu(), want.cpu())
    # the rule itself, on rows of tests/argmax_cases.py: -0 ties with +0 and the
    # lowest index wins wherever the pair falls, all -inf and nothing allowed give -1
    import argmax_cases as ac

    for masked in (False, True):
        rs = [r for r in ac.rows(V, masked)
              if r.name.startswith("zero_") or r.name in ("allowed_all_neg_inf", "nothing_allowed",
                                                          "neg_inf_beside_finite")]
        B = len(rs)
        logits = torch.from_numpy(np.stack([r.logits for r in rs])).to(torch.bfloat16).cuda()
        mk = None
        if masked:
            words = np.stack([ac.pack_mask(r.mask, r.high_bits) for r in rs]).view(np.int32)
            mk = torch.from_numpy(words.copy()).cuda()
        zf = torch.zeros(B, dtype=torch.float32, device="cuda")
        z64 = torch.zeros(B, dtype=torch.int64, device="cuda")
        got = ops.sample_masked(logits, mk, zf, torch.zeros(B, dtype=torch.int32, device="cuda"),
                                zf + 1, z64, z64)
        want = ops.greedy_sample_masked(logits, mk)
        assert got.cpu().tolist() == [r.expect for r in rs]
        assert want.cpu().tolist() == [r.expect for r in rs]


def test_launcher_rejects_v_not_multiple_of_8():
    from opsagent_amd import ops

    B, V = 2, 12
    logits = torch.zeros(B, V, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(B, dtype=torch.float32, device="cuda")
    i = torch.zeros(B, dtype=torch.int32, device="cuda")
    z = torch.zeros(B, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="-100"):
        ops.sample_masked(logits, None, f, i, f, z, z)


@pytest.mark.parametrize("V", sc.VOCABS)
def test_the_comparison_catches_real_mutations(V, packed):
    """Feed the kernel row b+1's mask, then all-zero steps: each run must leave
    the true oracle at least as often as the CPU mutant predicts and agree
    with the mutant's own oracle."""
    pk = packed[V]
    specs = sc.specs_for(V)
    m = len(specs)
    n = sc.mutant_steps(V)
    L = n * m // R
    assert L * R == n * m
    steps = pk.steps(L)
    runs = {
        "mask_row+1": pk.run(steps, mask=torch.roll(pk.mask, -1, dims=0)),
        "step_ignored": pk.run(torch.from_numpy(
            np.broadcast_to(np.zeros(1, np.int64), (L, R)).copy()).cuda()),
    }
    for mut, (tokens, _info) in runs.items():
        pred = sc.mutant_results(V, mut)
        left = need = 0
        for s, mres, toks in zip(specs, pred, by_spec(V, tokens)):
            need += sc.count_departures(s.expect, mres)
            amb = s.expect.ambiguous()[:n]
            left += int(np.count_nonzero((toks != s.expect.tokens[:n]) & ~amb))
            wrong, _ = sc.compare(mres, toks)
            assert wrong == 0, (mut, s.name)
        print(f"V {V} {mut}: kernel leaves the oracle on {left} draws, mutant predicts {need}")
        assert left >= need


GRAPH_CHILD = r"""
import sys
import numpy as np
import torch
from opsagent_amd import ops

d = np.load(sys.argv[1])
t = {k: torch.from_numpy(d[k]).cuda() for k in d.files}
logits = t["logits"].view(torch.bfloat16)
R, V = logits.shape
step_buf = t["steps"][0].clone()
out = torch.empty(R, dtype=torch.int32, device="cuda")
info = torch.empty(R, 2, dtype=torch.int32, device="cuda")
ws = torch.empty(max(1, ops.sample_ws_bytes(R, V)), dtype=torch.uint8, device="cuda")


def call():
    ops.sample_masked(logits, t["mask"], t["inv_temp"], t["top_k"], t["top_p"], t["seed"],
                      step_buf, adj=(t["adj_ptr"], t["adj_tok"], t["adj_val"]),
                      out=out, ws=ws, info=info)


side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    call()
torch.cuda.current_stream().wait_stream(side)
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    call()
step_buf.copy_(t["steps"][2])
graph.replay()
torch.cuda.synchronize()
np.savez(sys.argv[2], tokens=out.cpu().numpy(), info=info.cpu().numpy())
del graph
"""


def test_graph_capture_and_replay(packed, full_runs, tmp_path):
    """One torch.cuda.graph capture of the op with preallocated out / ws,
    replayed once after the step buffer was rewritten in place.

    The capture runs in a process of its own. While any graph is alive torch
    keeps one generator state per process and updates it in place at every
    capture and replay; the engine captures its decode graphs in inference
    mode, so with an engine of an earlier test still alive that state consists
    of inference tensors and a capture in this process fails before it starts,
    whatever is captured. A fresh process makes the test about the op alone."""
    import os
    import subprocess
    import sys

    V = 4104
    pk = packed[V]
    steps = pk.steps(3)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(
        src, logits=pk.logits.view(torch.int16).cpu().numpy(), mask=pk.mask.cpu().numpy(),
        inv_temp=pk.inv_temp.cpu().numpy(), top_k=pk.top_k.cpu().numpy(),
        top_p=pk.top_p.cpu().numpy(), seed=pk.seed.cpu().numpy(),
        adj_ptr=pk.adj[0].cpu().numpy(), adj_tok=pk.adj[1].cpu().numpy(),
        adj_val=pk.adj[2].cpu().numpy(), steps=steps.cpu().numpy(),
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", GRAPH_CHILD, src, dst],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(dst)
    toks = got["tokens"].astype(np.int64)
    specs = sc.specs_for(V)
    m = len(specs)
    for b in range(R):
        s = specs[b % m]
        idx = (2 * R + b) // m
        wrong, _ = sc.compare(s.expect, toks[b:b + 1], lo=idx)
        assert wrong == 0, (s.name, idx)
    # and the replay's bits are those of the plain launch with the same steps
    tokens, info = full_runs[V]
    assert (toks == tokens[2]).all() and (got["info"] == info[2]).all()


MICRO_CFG = {
    "model": "llama3-micro",
    "max_seq_len": 2048,
    "kv_block_size": 32,
    "kv_cache_gb": 2,
    "max_batch_size": 8,
    "use_hipgraph": True,
    "seed": 5,
    "fused_sampler": True,
}


def test_engine_with_fused_sampler():
    from opsagent_amd.engine.engine import LLMEngine, SamplingParams
    from opsagent_amd.engine.grammar import GrammarMode

    eng = LLMEngine(dict(MICRO_CFG))
    ids = eng.tokenizer.encode("sample with a seed", add_bos=True)
    sp = SamplingParams(max_new_tokens=24, temperature=0.9, top_k=40, top_p=0.95, seed=1234)
    a, _ = eng.generate(ids, sp)
    b, _ = eng.generate(ids, sp)
    assert a == b and len(a) > 0
    out, reason = eng.generate(ids, SamplingParams(
        max_new_tokens=64, temperature=0.8, top_p=0.3, seed=7, grammar=GrammarMode.JSON))
    assert reason != "grammar_dead_end"
    json.loads(eng.tokenizer.decode_text(out))
