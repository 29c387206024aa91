"""Interleaved A/B of paged decode attention over a bf16 and an fp8 KV cache
(one process, alternating variants, medians over rounds).

Hq 32, Hk 8, block size 32, B in {1, 16, 64} x len in {2048, 8192}. The KV
blocks of every sequence are scattered over a shuffled pool, and each timed
pass cycles through NSETS disjoint block sets whose bf16 footprint together
is at least POOL_BYTES (default 1 GiB, four times the 256 MB Infinity Cache),
so a pass streams from HBM the way a decode step of a busy engine does.

Four timings per shape, us per call and effective TB/s (KV bytes / time):
  bf16      ops.attention_decode_paged           (attention + combine)
  fp8       ops.attention_decode_paged_fp8       (attention + combine)
  bf16_eng  ops.attention_decode_rope            (what the engine runs: RoPE +
                                                  write fused into attention)
  fp8_eng   ops.rope_kv_fused_fp8 + the fp8 attention (one more launch)

Each variant's pass is captured in a hipGraph and the replay is timed, as
the engine replays its decode step: host launch overhead, which bounds
eagerly dispatched calls of a few tens of microseconds, stays out of the
figures. --eager times the eager dispatch instead.

Usage: python scripts/decode_attn_kv_ab.py [--rounds N] [--eager] [--out FILE]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from opsagent_amd import ops

DEV = "cuda"
HQ, HK, D, BS = 32, 8, 128, 32
SHAPES = [(B, n) for B in (1, 16, 64) for n in (2048, 8192)]
POOL_BYTES = int(os.environ.get("OPSAGENT_AB_POOL_BYTES", str(1 << 30)))
BF16_TOKEN_BYTES = 2 * HK * D * 2          # K and V
FP8_TOKEN_BYTES = 2 * HK * (D + 4)


def build(B, n, gen):
    per_set = B * n
    nsets = max(2, -(-POOL_BYTES // (per_set * BF16_TOKEN_BYTES)))
    nb = nsets * per_set // BS
    kc = torch.randn(nb, BS, HK, D, dtype=torch.bfloat16, device=DEV)
    vc = torch.randn(nb, BS, HK, D, dtype=torch.bfloat16, device=DEV)
    k8, ks = ops.quant_fp8(kc.view(-1, D))
    v8, vs = ops.quant_fp8(vc.view(-1, D))
    k8, v8 = k8.view(nb, BS, HK, D), v8.view(nb, BS, HK, D)
    ks, vs = ks.view(nb, BS, HK), vs.view(nb, BS, HK)
    perm = torch.randperm(nb, generator=gen).to(torch.int32).view(nsets, B, n // BS)
    tables = [perm[s].contiguous().to(DEV) for s in range(nsets)]
    return nsets, (kc, vc), (k8, v8, ks, vs), tables


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    gen = torch.Generator().manual_seed(0)
    cos, sin = ops.rope_cos_sin(8192, D, 500000.0)
    cos, sin = cos.to(DEV), sin.to(DEV)
    lines = ["timing: " + ("eager dispatch" if args.eager else "hipGraph replay")]
    print(lines[0], flush=True)
    for B, n in SHAPES:
        nsets, (kc, vc), (k8, v8, ks, vs), tables = build(B, n, gen)
        lens = torch.full((B,), n, dtype=torch.int32, device=DEV)
        pos = lens - 1
        qkv = (torch.randn(B, (HQ + 2 * HK) * D, device=DEV) * 1.5).to(torch.bfloat16)
        nsplit = ops.decode_nsplit(B, HK, n)
        G = HQ // HK
        ws = (
            torch.empty(B * HK * nsplit, G, D, dtype=torch.float32, device=DEV),
            torch.empty(B * HK * nsplit, G, 2, dtype=torch.float32, device=DEV),
            torch.empty(B * HK, dtype=torch.int32, device=DEV),
        )
        # the new token's slot: last position of each sequence
        slot_sets = [
            (t[:, -1].to(torch.int64) * BS + (BS - 1)).to(torch.int32).contiguous()
            for t in tables
        ]

        def views():
            buf = qkv.clone()
            q, k, v = buf.split([HQ * D, HK * D, HK * D], dim=-1)
            return q.view(B, HQ, D), k.view(B, HK, D), v.view(B, HK, D)

        def run(variant):
            out = None
            for bt, slots in zip(tables, slot_sets):
                q, k, v = views()
                if variant == "bf16":
                    out = ops.attention_decode_paged(
                        q, kc, vc, bt, lens, workspace=ws, nsplit=nsplit)
                elif variant == "fp8":
                    out = ops.attention_decode_paged_fp8(
                        q, k8, v8, ks, vs, bt, lens, workspace=ws, nsplit=nsplit)
                elif variant == "bf16_eng":
                    out = ops.attention_decode_rope(
                        q, k, v, kc, vc, bt, lens, cos, sin, slots,
                        workspace=ws, nsplit=nsplit)
                else:
                    ops.rope_kv_fused_fp8(q, k, v, k8, v8, ks, vs, cos, sin, pos, slots)
                    out = ops.attention_decode_paged_fp8(
                        q, k8, v8, ks, vs, bt, lens, workspace=ws, nsplit=nsplit)
            return out

        variants = ("bf16", "fp8", "bf16_eng", "fp8_eng")
        # sanity: fp8 answers agree with bf16 to format accuracy
        a = run("bf16").float()
        b = run("fp8").float()
        torch.cuda.synchronize()
        rel = float((a - b).abs().max() / a.abs().max())
        assert rel < 0.25, f"fp8 decode disagrees with bf16: {rel}"
        for v_ in variants:
            run(v_)
        torch.cuda.synchronize()

        def clone_pass():
            for _s in range(nsets):
                views()

        passes = {v_: (lambda v_=v_: run(v_)) for v_ in variants}
        passes["clone"] = clone_pass
        if not args.eager:
            keep = []
            for name, fn in list(passes.items()):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    keep.append(fn())
                g.replay()
                passes[name] = g.replay
            torch.cuda.synchronize()
        # the q/k/v clone in views() is timed too: subtract it
        times = {v_: [] for v_ in variants + ("clone",)}
        for _ in range(args.rounds):
            for v_ in variants + ("clone",):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                passes[v_]()
                e1.record()
                e1.synchronize()
                times[v_].append(e0.elapsed_time(e1) * 1e3 / nsets)   # us per call
        clone_us = statistics.median(times["clone"])
        tokens = B * n
        row = [f"B{B:<3d} len{n:<5d} nsplit{nsplit:<3d} sets{nsets:<3d} fp8-vs-bf16 rel {rel:.3f} |"]
        med = {}
        for v_ in variants:
            us = statistics.median(times[v_]) - clone_us
            med[v_] = us
            byts = tokens * (BF16_TOKEN_BYTES if v_.startswith("bf16") else FP8_TOKEN_BYTES)
            row.append(f"{v_} {us:8.1f} us {byts / us / 1e6:5.2f} TB/s |")
        row.append(f"kernel bf16/fp8 {med['bf16'] / med['fp8']:.2f}x "
                   f"engine-path bf16/fp8 {med['bf16_eng'] / med['fp8_eng']:.2f}x")
        line = " ".join(row)
        print(line, flush=True)
        lines.append(line)
        del kc, vc, k8, v8, ks, vs, tables
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
