"""Within-probe interleaved A/B of the GEMV K-pipeline depth (guide rule 24):
depths 1/2/4/8 through the probe entry points oa_gemv_ku / oa_gemv_gateup_ku on
the decode shapes of llama3-8b, with REAL-SIZE weights that do NOT fit the
caches (NW distinct W tensors per shape, > 256 MiB in total, cycled so every
pass streams from HBM like a decode step does).

Prints us and TB/s per shape and depth. The probe picks CANDIDATE depths only;
the in-model A/B (bench.py) decides what ships — see profiles/README.md."""

import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from opsagent_amd.ops import hip_lib

lib = hip_lib.get_lib()
dev = "cuda"
EPS = 1e-5
DEPTHS = (1, 2, 4, 8)
ROUNDS = 10

# name, kind, N (gate-up: I), K, mode, rows per wave
SHAPES = [
    ("o_proj 4096x4096 res", "gemv", 4096, 4096, 2, 1),
    ("qkv 6144x4096 norm", "gemv", 6144, 4096, 1, 1),
    ("down 4096x14336 res", "gemv", 4096, 14336, 2, 1),
    ("gateup 2x14336x4096 norm", "gateup", 14336, 4096, 1, 2),
    ("lm_head 128256x4096", "gemv", 128256, 4096, 0, 2),
]


def copies(rows, K):
    """>= 12 distinct copies and > 256 MiB in total"""
    per = rows * K * 2
    return max(12, -(-(300 << 20) // per))


def launch(kind, ku, x, w, out, wn, res, N, K, mode, rw):
    s = hip_lib.current_stream_ptr()
    if kind == "gateup":
        rc = lib.oa_gemv_gateup_ku(s, x.data_ptr(), w.data_ptr(), out.data_ptr(),
                                   wn.data_ptr(), 1, N, K, EPS, mode & 1, ku)
    else:
        rc = lib.oa_gemv_ku(s, x.data_ptr(), w.data_ptr(), out.data_ptr(),
                            wn.data_ptr() if mode & 1 else None,
                            res.data_ptr() if mode & 2 else None,
                            1, N, K, EPS, mode, rw, ku)
    assert rc == 0, rc


for name, kind, N, K, mode, rw in SHAPES:
    torch.manual_seed(0)
    rows = 2 * N if kind == "gateup" else N
    nw = copies(rows, K)
    x = (torch.randn(1, K, device=dev) * 0.3).to(torch.bfloat16)
    wn = (torch.rand(K, device=dev) + 0.5).to(torch.bfloat16)
    res = torch.randn(1, N, device=dev).to(torch.bfloat16)
    ws = [(torch.randn(rows, K, device=dev) * 0.3).to(torch.bfloat16) for _ in range(nw)]
    out = torch.empty(1, N, dtype=torch.bfloat16, device=dev)
    # every depth must give the bits of depth 1
    launch(kind, 1, x, ws[0], out, wn, res, N, K, mode, rw)
    base = out.clone()
    for ku in DEPTHS[1:]:
        out.zero_()
        launch(kind, ku, x, ws[0], out, wn, res, N, K, mode, rw)
        assert torch.equal(out, base), f"{name}: depth {ku} differs from depth 1"
    for ku in DEPTHS:  # warmup
        for w in ws:
            launch(kind, ku, x, w, out, wn, res, N, K, mode, rw)
    torch.cuda.synchronize()
    times = {ku: [] for ku in DEPTHS}
    for _ in range(ROUNDS):
        for ku in DEPTHS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for w in ws:
                launch(kind, ku, x, w, out, wn, res, N, K, mode, rw)
            torch.cuda.synchronize()
            times[ku].append((time.perf_counter() - t0) / nw)
    gb = rows * K * 2 / 1e9
    cells = []
    for ku in DEPTHS:
        t = statistics.median(times[ku])
        cells.append(f"ku{ku} {t * 1e6:6.1f}us {gb / t / 1e3:5.2f}TB/s")
    print(f"{name:26s} x{nw:3d}: " + "  ".join(cells), flush=True)
    del ws
