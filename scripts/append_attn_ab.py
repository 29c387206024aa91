"""Interleaved A/B of paged APPEND attention against what the engine does
without it (one process, alternating variants, medians over rounds).

  A  ops.attention_append_paged (attention + its combine) over the paged
     cache in place
  B  index-gather of past+new K and V by slot, then ops.attention_prefill
     with Sq = L — the catch-up / verify path of the engine today

Grid: Hq 32 / Hk 8 and Hq 8 / Hk 1, block size 32, B = 1, L in {3, 9, 16},
past in {1024, 4096, 8192}; mixed steps of B in {4, 8, 16} rows with one
L = 9 row and the rest L = 1, where B additionally pays one
attention_decode_paged launch for the L = 1 rows; and all-L=1 batches against
attention_decode_paged (report only: the engine keeps the decode kernel when
no row has L > 1).

The KV blocks of every sequence are scattered over a shuffled pool and each
timed pass cycles through NSETS disjoint block sets whose footprint together
is POOL_BYTES (default 1 GiB, four times the 256 MB Infinity Cache), so a
pass streams from HBM. Each variant's pass is captured in a hipGraph and the
replay is timed with device events after a warm-up; --eager times the eager
dispatch instead. Per shape: us per call for A and B (B with min..max over the
rounds — its spread), B/A, and A's effective KV TB/s.

Usage: python scripts/append_attn_ab.py [--rounds N] [--eager] [--out FILE]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from opsagent_amd import ops

DEV = "cuda"
D, BS = 128, 32
POOL_BYTES = int(os.environ.get("OPSAGENT_AB_POOL_BYTES", str(1 << 30)))


def time_passes(passes, rounds, nsets, eager):
    for fn in passes.values():
        fn()
    torch.cuda.synchronize()
    if not eager:
        keep = []
        for name, fn in list(passes.items()):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep.append(fn())
            g.replay()
            passes[name] = g.replay
        torch.cuda.synchronize()
    times = {k: [] for k in passes}
    for _ in range(rounds):
        for k, fn in passes.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / nsets)   # us per call
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    gen = torch.Generator().manual_seed(0)
    lines = ["timing: " + ("eager dispatch" if args.eager else "hipGraph replay")
             + f", pool {POOL_BYTES >> 20} MiB, rounds {args.rounds}"]
    print(lines[0], flush=True)

    shapes = []
    for hq, hk in ((32, 8), (8, 1)):
        for past in (1024, 4096, 8192):
            for L in (3, 9, 16):
                shapes.append(("single", hq, hk, [L], past))
    for past in (1024, 4096, 8192):
        for B in (4, 8, 16):
            shapes.append(("mixed", 32, 8, [9] + [1] * (B - 1), past))
    for B in (1, 8, 16):
        shapes.append(("all_l1", 32, 8, [1] * B, 4096))

    pools = {}
    for kind, HQ, HK, qlens, past in shapes:
        G = HQ // HK
        tok_bytes = 2 * HK * D * 2
        if HK not in pools:
            pools.clear()
            torch.cuda.empty_cache()
            nb = POOL_BYTES // (tok_bytes * BS)
            pools[HK] = (
                (torch.randn(nb, BS, HK, D, device=DEV) * 1.5).to(torch.bfloat16),
                torch.randn(nb, BS, HK, D, device=DEV).to(torch.bfloat16),
            )
        kc, vc = pools[HK]
        nb = kc.shape[0]
        flat_k, flat_v = kc.view(nb * BS, HK, D), vc.view(nb * BS, HK, D)
        B = len(qlens)
        T = sum(qlens)
        max_q = max(qlens)
        lens_l = [past + L for L in qlens]
        maxb = -(-max(lens_l) // BS)
        nsets = max(1, nb // (B * maxb))
        perm = torch.randperm(nb, generator=gen)[: nsets * B * maxb].to(torch.int32)
        tables = [t.contiguous().to(DEV) for t in perm.view(nsets, B, maxb)]
        lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
        cu = torch.tensor([0] + torch.tensor(qlens).cumsum(0).tolist(),
                          dtype=torch.int32, device=DEV)
        qkv = (torch.randn(T, (HQ + 2 * HK) * D, device=DEV) * 1.5).to(torch.bfloat16)
        q = qkv[:, : HQ * D].view(T, HQ, D)
        nsplit = ops.decode_nsplit(B, HK, max(lens_l))
        ws = ops.append_workspace(B, T, HK, G, nsplit, device=DEV, max_q=max_q)
        dws = (
            torch.empty(B * HK * nsplit, G, D, dtype=torch.float32, device=DEV),
            torch.empty(B * HK * nsplit, G, 2, dtype=torch.float32, device=DEV),
            torch.empty(B * HK, dtype=torch.int32, device=DEV),
        )
        # B path: flat slots of every key (past + new) of row 0, per set
        skv = lens_l[0]
        ar = torch.arange(skv, device=DEV)
        slot_sets = [
            (t[0].long()[ar // BS] * BS + ar % BS).contiguous() for t in tables
        ]
        L0 = qlens[0]

        def run_a():
            out = None
            for bt in tables:
                out = ops.attention_append_paged(
                    q, kc, vc, bt, lens, cu, max_q, workspace=ws, nsplit=nsplit)
            return out

        def run_b():
            out = None
            for bt, slots in zip(tables, slot_sets):
                k_full = flat_k[slots].view(1, skv, HK, D)
                v_full = flat_v[slots].view(1, skv, HK, D)
                out = ops.attention_prefill(q[:L0].unsqueeze(0), k_full, v_full)
                if B > 1:   # the L = 1 rows take the decode kernel
                    out2 = ops.attention_decode_paged(
                        q[L0:], kc, vc, bt[1:], lens[1:], workspace=dws, nsplit=nsplit)
                    out = (out, out2)
            return out

        def run_dec():
            out = None
            for bt in tables:
                out = ops.attention_decode_paged(
                    q, kc, vc, bt, lens, workspace=dws, nsplit=nsplit)
            return out

        # sanity on the last set: A agrees with B
        a = run_a().float()
        b = run_dec() if kind == "all_l1" else run_b()
        torch.cuda.synchronize()
        b0 = (b[0] if isinstance(b, tuple) else b).float().reshape(-1, HQ, D)
        rel = float((a[: b0.shape[0]] - b0).abs().max() / b0.abs().max())
        assert rel < 0.05, f"append disagrees with the reference path: {rel}"

        passes = {"A": run_a, "B": run_dec if kind == "all_l1" else run_b}
        times = time_passes(passes, args.rounds, nsets, args.eager)
        a_us = statistics.median(times["A"])
        b_us = statistics.median(times["B"])
        kv_bytes = sum(lens_l) * tok_bytes
        line = (
            f"{kind:<7s} Hq{HQ:<2d} Hk{HK} B{B:<2d} L{max_q:<2d} past{past:<5d} nsplit{nsplit:<3d} "
            f"sets{nsets:<5d} rel {rel:.4f} | A {a_us:8.1f} us "
            f"[{min(times['A']):.1f}..{max(times['A']):.1f}] {kv_bytes / a_us / 1e6:5.2f} TB/s | "
            f"B {b_us:8.1f} us [{min(times['B']):.1f}..{max(times['B']):.1f}] | "
            f"B/A {b_us / a_us:5.2f}x"
        )
        print(line, flush=True)
        lines.append(line)
        del tables, slot_sets
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
