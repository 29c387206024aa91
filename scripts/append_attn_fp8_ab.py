"""Interleaved A/B of paged APPEND attention over the fp8 KV cache (one
process, alternating variants, medians over rounds), on the method and the
shape list of scripts/append_attn_ab.py.

  A  ops.attention_append_paged_fp8 (attention + its combine) reading codes
     and scales in place
  a  what the fp8 engine does without it: ops.kv_gather_fp8 of past+new K and
     V by slot (dequantised to contiguous bf16), then ops.attention_prefill
     with Sq = L; in a mixed step the L = 1 rows additionally pay one
     attention_decode_paged_fp8 launch
  b  ops.attention_append_paged, the bf16 append kernel, on a bf16 cache of
     the same shape and the same block tables
  c  all-L=1 batches only: ops.attention_decode_paged_fp8 (report only: the
     engine keeps the decode kernel when no row has L > 1)

Grid: Hq 32 / Hk 8 and Hq 8 / Hk 1, block size 32, B = 1, L in {3, 9, 16},
past in {1024, 4096, 8192}; mixed steps of B in {4, 8, 16} rows with one
L = 9 row and the rest L = 1; all-L=1 batches of B in {1, 8, 16} at 4096.

The KV blocks of every sequence are scattered over a shuffled pool and each
timed pass cycles through NSETS disjoint block sets whose fp8 footprint
together is POOL_BYTES (default 1 GiB, four times the 256 MB Infinity Cache;
the bf16 twin of the pool is 1.94x that), so a pass streams from HBM. Each
variant's pass is captured in a hipGraph and the replay is timed with device
events after a warm-up; --eager times the eager dispatch instead. Per shape:
us per call for every variant with min..max over the rounds, the ratios to A,
and A's effective KV TB/s (fp8 bytes: 132 B per key, head and tensor).

Usage: python scripts/append_attn_fp8_ab.py [--rounds N] [--eager] [--out FILE]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

from append_attn_ab import time_passes
from opsagent_amd import ops

DEV = "cuda"
D, BS = 128, 32
POOL_BYTES = int(os.environ.get("OPSAGENT_AB_POOL_BYTES", str(1 << 30)))


def quantise(x):
    """[nb, BS, HK, D] bf16 -> (uint8 e4m3 codes, f32 scales [nb, BS, HK])."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True).clamp_min(1e-8)
    codes = (xf * (448.0 / amax)).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.contiguous(), (amax / 448.0).squeeze(-1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    gen = torch.Generator().manual_seed(0)
    lines = ["timing: " + ("eager dispatch" if args.eager else "hipGraph replay")
             + f", fp8 pool {POOL_BYTES >> 20} MiB, rounds {args.rounds}"]
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
        tok_bytes = 2 * HK * (D + 4)
        if HK not in pools:
            pools.clear()
            torch.cuda.empty_cache()
            nb = POOL_BYTES // (tok_bytes * BS)
            kc = (torch.randn(nb, BS, HK, D, device=DEV) * 1.5).to(torch.bfloat16)
            vc = torch.randn(nb, BS, HK, D, device=DEV).to(torch.bfloat16)
            pools[HK] = (kc, vc) + quantise(kc) + quantise(vc)
        kc, vc, k8, ks, v8, vs = pools[HK]
        nb = kc.shape[0]
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
        )
        # gather path: flat slots of every key (past + new) of row 0, per set
        skv = lens_l[0]
        ar = torch.arange(skv, device=DEV)
        slot_sets = [
            (t[0].long()[ar // BS] * BS + ar % BS).to(torch.int32).contiguous() for t in tables
        ]
        L0 = qlens[0]

        def run_A():
            out = None
            for bt in tables:
                out = ops.attention_append_paged_fp8(
                    q, k8, v8, ks, vs, bt, lens, cu, max_q, workspace=ws, nsplit=nsplit)
            return out

        def run_gather():
            out = None
            for bt, slots in zip(tables, slot_sets):
                k_full, v_full = ops.kv_gather_fp8(k8, v8, ks, vs, slots)
                out = ops.attention_prefill(
                    q[:L0].unsqueeze(0), k_full.unsqueeze(0), v_full.unsqueeze(0))
                if B > 1:   # the L = 1 rows take the fp8 decode kernel
                    out2 = ops.attention_decode_paged_fp8(
                        q[L0:], k8, v8, ks, vs, bt[1:], lens[1:], workspace=dws, nsplit=nsplit)
                    out = (out, out2)
            return out

        def run_bf16():
            out = None
            for bt in tables:
                out = ops.attention_append_paged(
                    q, kc, vc, bt, lens, cu, max_q, workspace=ws, nsplit=nsplit)
            return out

        def run_dec():
            out = None
            for bt in tables:
                out = ops.attention_decode_paged_fp8(
                    q, k8, v8, ks, vs, bt, lens, workspace=dws, nsplit=nsplit)
            return out

        # sanity on the last set: A agrees with the path it replaces
        a = run_A().float()
        b = run_dec() if kind == "all_l1" else run_gather()
        torch.cuda.synchronize()
        b0 = (b[0] if isinstance(b, tuple) else b).float().reshape(-1, HQ, D)
        rel = float((a[: b0.shape[0]] - b0).abs().max() / b0.abs().max())
        assert rel < 0.05, f"fp8 append disagrees with the reference path: {rel}"

        passes = {"A": run_A, "b": run_bf16}
        passes["c" if kind == "all_l1" else "a"] = run_dec if kind == "all_l1" else run_gather
        times = time_passes(passes, args.rounds, nsets, args.eager)
        med = {k: statistics.median(v) for k, v in times.items()}
        kv_bytes = sum(lens_l) * tok_bytes
        line = (
            f"{kind:<7s} Hq{HQ:<2d} Hk{HK} B{B:<2d} L{max_q:<2d} past{past:<5d} nsplit{nsplit:<3d} "
            f"sets{nsets:<5d} rel {rel:.4f} | A {med['A']:8.1f} us "
            f"[{min(times['A']):.1f}..{max(times['A']):.1f}] {kv_bytes / med['A'] / 1e6:5.2f} TB/s"
        )
        for k in ("a", "b", "c"):
            if k in med:
                line += (f" | {k} {med[k]:8.1f} us [{min(times[k]):.1f}..{max(times[k]):.1f}] "
                         f"{k}/A {med[k] / med['A']:5.2f}x")
        print(line, flush=True)
        lines.append(line)
        del tables, slot_sets
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
