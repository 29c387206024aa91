"""Interleaved A/B of the seeded sampler (oa_sample) against the
path it replaces: the torch op sequence of LLMEngine._transform_logits on the
same logits followed by oa_masked_argmax. One process, hipGraph replay, V =
128256, B in {1, 4, 16, 64}.

_transform_logits itself cannot be captured (it builds device tensors from
host lists and reads a flag back), so the legacy side here is the same device
ops in the same order with the per-row parameters staged beforehand: fp32 copy,
sparse adjustments (index_put where the engine counts with bincount, which
reads a size back and cannot be captured), temperature divide, topk + gather
+ masked_fill, sort + softmax + cumsum + masked_fill + scatter, rand_like +
two logs + where, the bf16 round, masked argmax. That leaves out the legacy path's host work and
synchronisation, so the comparison favours it.

Parameter sets: temperature only; top-k 50; top-p 0.9; both; both with a
256-entry adjustment list per row; each with and without a grammar-sized mask
(2 % of the vocabulary allowed). Prints us per call for both and the ratio."""

import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from opsagent_amd import ops

dev = "cuda"
V = 128256
NODES = 16
NL = 4
ROUNDS = int(os.environ.get("SAMPLE_AB_ROUNDS", "10"))
BATCHES = [int(b) for b in os.environ.get("SAMPLE_AB_B", "1,4,16,64").split(",")]
WORDS = (V + 31) // 32

SETS = [
    ("temp", 0, 1.0, 0),
    ("top-k 50", 50, 1.0, 0),
    ("top-p 0.9", 0, 0.9, 0),
    ("both", 50, 0.9, 0),
    ("both + 256 adj", 50, 0.9, 256),
]


def pack(allowed):
    import numpy as np

    pad = np.zeros((allowed.shape[0], WORDS * 32), dtype=np.uint8)
    pad[:, :V] = allowed.numpy().astype(np.uint8)
    return torch.from_numpy(
        np.packbits(pad, axis=1, bitorder="little").view(np.int32).copy()
    ).to(dev)


def legacy(lg, mask, temp, k, p, adj_rows, adj_tok, adj_val):
    lf = lg.float()
    if adj_rows is not None:
        lf.index_put_((adj_rows, adj_tok), adj_val, accumulate=True)
    sub = lf / temp
    if k > 0:
        kth = torch.topk(sub, k, dim=-1).values[:, k - 1:k]
        sub = sub.masked_fill(sub < kth, float("-inf"))
    if p < 1.0:
        srt, order = torch.sort(sub, dim=-1, descending=True)
        probs = torch.softmax(srt, dim=-1)
        cum = probs.cumsum(-1)
        srt = srt.masked_fill((cum - probs) > p, float("-inf"))
        sub = sub.scatter(1, order, srt)
    noise = -torch.log(-torch.log(torch.rand_like(sub) + 1e-20) + 1e-20)
    sub = torch.where(torch.isinf(sub), sub, sub + noise)
    return ops.greedy_sample_masked(sub.to(torch.bfloat16).contiguous(), mask)


torch.manual_seed(0)
stream = torch.cuda.Stream()
for B in BATCHES:
    logits = [(3 * torch.randn(B, V, device=dev)).to(torch.bfloat16) for _ in range(NL)]
    allowed = (torch.arange(V).unsqueeze(0) * 2654435761 + torch.arange(B).unsqueeze(1)) % 50 == 0
    masks = {"no mask": None, "mask 2%": pack(allowed)}
    seed = torch.arange(B, dtype=torch.int64, device=dev) + 1000
    step = torch.arange(B, dtype=torch.int64, device=dev)
    out = torch.empty(B, dtype=torch.int32, device=dev)
    ws = torch.empty(max(16, ops.sample_ws_bytes(B, V)), dtype=torch.uint8, device=dev)
    for name, k, p, nadj in SETS:
        inv_temp = torch.full((B,), 1.0 / 0.8, dtype=torch.float32, device=dev)
        top_k = torch.full((B,), k, dtype=torch.int32, device=dev)
        top_p = torch.full((B,), p, dtype=torch.float32, device=dev)
        adj = adj_rows = adj_tok64 = adj_val = None
        if nadj:
            toks = torch.stack([torch.randperm(V)[:nadj].sort().values for _ in range(B)])
            adj_val = (torch.rand(B * nadj) * 4 - 2).to(dev)
            adj = (
                (torch.arange(B + 1, dtype=torch.int32) * nadj).to(dev),
                toks.reshape(-1).to(torch.int32).to(dev),
                adj_val,
            )
            adj_rows = torch.arange(B).repeat_interleave(nadj).to(dev)
            adj_tok64 = toks.reshape(-1).to(dev)
        for mname, mask in masks.items():
            def run_new(lg):
                ops.sample_masked(lg, mask, inv_temp, top_k, top_p, seed, step, adj=adj, out=out, ws=ws)

            def run_old(lg):
                legacy(lg, mask, 0.8, k, p, adj_rows, adj_tok64, adj_val)

            graphs = {}
            with torch.cuda.stream(stream):
                for label, fn in (("legacy", run_old), ("fused", run_new)):
                    for i in range(NL):
                        fn(logits[i])
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=stream):
                        for i in range(NODES):
                            fn(logits[i % NL])
                    graphs[label] = g
                for g in graphs.values():
                    g.replay()
                torch.cuda.synchronize()
                times = {n: [] for n in graphs}
                for _ in range(ROUNDS):
                    for n, g in graphs.items():
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record()
                        g.replay()
                        e1.record()
                        e1.synchronize()
                        times[n].append(e0.elapsed_time(e1) * 1e3 / NODES)
            med = {n: statistics.median(t) for n, t in times.items()}
            print(
                f"B={B:3d} {name:>15s} {mname:>8s}: legacy {med['legacy']:8.1f}us "
                f"(min {min(times['legacy']):8.1f})  fused {med['fused']:7.1f}us "
                f"(min {min(times['fused']):7.1f})  legacy/fused {med['legacy'] / med['fused']:6.2f}x",
                flush=True,
            )
            del graphs
