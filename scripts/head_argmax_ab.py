"""Interleaved A/B of the fused decode head (oa_head_argmax) against the unfused
pair it replaces (oa_gemv + oa_masked_argmax), in one process under hipGraph
replay, at the flagship head shape V = 128256, K = 4096, M = 1 and 2.

Live shares: 100 % (all-ones mask), 25 % (the first 32064 rows — what a 32k
tokenizer leaves of a 128k vocabulary) and about 1 % (scattered rows). Every
graph holds NODES head calls that cycle over NW distinct W tensors, and the
1 % case also over disjoint row sets, so that what a pass streams (live bytes x
distinct combinations) exceeds the 256 MiB Infinity Cache and comes from HBM
as in a decode step.

Prints, per (M, share): us per head call for the unfused pair, the fused head
at the shipped depth and (M = 1) at depth 2, the bytes the fused head streams
and its TB/s. The tokens of all variants are compared first."""

import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from opsagent_amd.ops import hip_lib

lib = hip_lib.get_lib()
dev = "cuda"
V, K = 128256, 4096
NW = int(os.environ.get("HEAD_AB_NW", "4"))
NODES = 32
ROUNDS = int(os.environ.get("HEAD_AB_ROUNDS", "12"))
WORDS = (V + 31) // 32


def pack(allowed):
    import numpy as np

    pad = np.zeros((allowed.shape[0], WORDS * 32), dtype=np.uint8)
    pad[:, :V] = allowed.cpu().numpy().astype(np.uint8)
    return torch.from_numpy(
        np.packbits(pad, axis=1, bitorder="little").view(np.int32).copy()
    ).to(dev)


def masks_for(share, M):
    """list of (packed mask [M, WORDS], live rows); nodes cycle over the list"""
    idx = torch.arange(V)
    if share == "100%":
        sets = [torch.ones(V, dtype=torch.bool)]
    elif share == "25%":
        sets = [idx < 32064]
    else:  # ~1 %, scattered; eight disjoint row sets
        h = (idx * 2654435761) % 100
        sets = [h == j for j in range(8)]
    return [(pack(s.expand(M, V)), int(s.sum())) for s in sets]


torch.manual_seed(0)
ws = [(torch.randn(V, K, device=dev) * 0.05).to(torch.bfloat16) for _ in range(NW)]
stream = torch.cuda.Stream()

for M in (1, 2):
    x = torch.randn(M, K, device=dev).to(torch.bfloat16)
    logits = torch.empty(M, V, dtype=torch.bfloat16, device=dev)
    grid = lib.oa_head_argmax_grid(V, M)
    key_ws = torch.empty(M * grid, dtype=torch.int64, device=dev)
    scan_ws = torch.empty(M, dtype=torch.int64, device=dev)
    out = torch.empty(M, dtype=torch.int32, device=dev)

    def unfused(w, mask):
        s = hip_lib.current_stream_ptr()
        rc = lib.oa_gemv(s, x.data_ptr(), w.data_ptr(), logits.data_ptr(), M, V, K)
        assert rc == 0, rc
        rc = lib.oa_masked_argmax(s, logits.data_ptr(), mask.data_ptr(),
                                  scan_ws.data_ptr(), out.data_ptr(), M, V)
        assert rc == 0, rc

    def fused(ku):
        def run(w, mask):
            rc = lib.oa_head_argmax_ku(
                hip_lib.current_stream_ptr(), x.data_ptr(), w.data_ptr(),
                mask.data_ptr(), key_ws.data_ptr(), out.data_ptr(), M, V, K, ku)
            assert rc == 0, rc
        return run

    variants = {"unfused": unfused, "fused ku1": fused(1)}
    if M == 1:
        variants["fused ku2"] = fused(2)

    for share in ("100%", "25%", "1%"):
        ms = masks_for(share, M)
        live = statistics.mean(n for _, n in ms)
        # same tokens from every variant, on every (W, mask) combination used
        for i in range(max(NW, len(ms))):
            w, (mask, _) = ws[i % NW], ms[i % len(ms)]
            toks = {}
            for name, fn in variants.items():
                out.fill_(-5)
                fn(w, mask)
                toks[name] = out.cpu().tolist()
            assert len({tuple(t) for t in toks.values()}) == 1, (share, i, toks)
        graphs = {}
        with torch.cuda.stream(stream):
            for name, fn in variants.items():
                for i in range(NODES):  # warm-up, also the graph's own sequence
                    fn(ws[i % NW], ms[(i // NW) % len(ms)][0])
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=stream):
                    for i in range(NODES):
                        fn(ws[i % NW], ms[(i // NW) % len(ms)][0])
                graphs[name] = g
            for g in graphs.values():
                g.replay()
            torch.cuda.synchronize()
            times = {name: [] for name in graphs}
            for _ in range(ROUNDS):
                for name, g in graphs.items():
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    g.replay()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / NODES)
        med = {n: statistics.median(t) for n, t in times.items()}
        gb = live * K * 2 / 1e9
        cells = [f"{n} {med[n]:6.1f}us (min {min(times[n]):6.1f})" for n in med]
        print(
            f"M={M} live {share:>4s} ({live:8.0f} rows, {gb * 1e3:7.1f} MB): "
            + "  ".join(cells)
            + f"  fused ku1 {gb / med['fused ku1'] * 1e3:5.2f} TB/s"
            + f"  speed-up {med['unfused'] / med['fused ku1']:.2f}x",
            flush=True,
        )
        del graphs
