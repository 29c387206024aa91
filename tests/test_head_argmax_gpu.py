"""The fused decode head (head_argmax.hip) on a real MI355X (`pytest -m gpu`).

Every case asserts two things:
  (a) the token EQUALS ops.greedy_sample_masked(ops.linear(x, w), mask) on the
      same tensors — both sides are bit-identical by construction, so no
      tolerance applies;
  (b) against a CPU fp64 product of the same bf16 operands the chosen row is
      allowed and its fp64 logit is within one bf16 rounding step of the
      largest allowed fp64 logit — this catches both paths being wrong
      together.

test_signed_zero_and_neg_inf_rows builds logits that are exactly -0, +0 and
-inf and holds both paths to the rule of tests/argmax_cases.py: -0 ties with
+0, the lowest index wins, -inf is never chosen.

Bound of (b): the kernel compares logits rounded to bf16 (8 significand bits),
so the chosen and the best row may differ by one bf16 step at the larger of
their magnitudes, 2^(floor(log2 |v|) - 7). The fp32 value that is rounded
carries the accumulation error of its chain — 8 * ceil(K / 512) fused
multiply-adds per lane, then 6 shuffle adds — bounded by chain * 2^-24 * sum_k
|x_k w_k| for each of the two rows. The tolerance is the sum of the two.

Grid geometry (head_argmax.hip): blocks of four waves, one row pair per wave
and trip, grid = min(cap, V / 8), trips stride by 4 * grid pairs. V = 16392 is
the smallest V at which a wave of the M = 1 grid (2048 blocks) takes a second
trip; at M = 2 (1792 blocks) it already has.
"""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(40, 1040), (2056, 4096), (32776, 512), (16392, 512), (16400, 512)]

_CACHE = {}


def _case(V, K, M):
    """x, w on the GPU and the fp64 logits of the same bf16 operands (CPU),
    computed once per shape and left unchanged."""
    key = (V, K, M)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * M + V + K)
        x = torch.randn(M, K, generator=g).to(torch.bfloat16)
        w = (torch.randn(V, K, generator=g) * 0.05).to(torch.bfloat16)
        x64, w64 = x.double(), w.double()
        _CACHE[key] = {
            "x": x.cuda(), "w": w.cuda(), "x64": x64, "w64": w64,
            "logits": x64 @ w64.t(), "absdot": x64.abs() @ w64.abs().t(),
        }
    return _CACHE[key]


def _pack(allowed):
    """bool [M, V] -> int32 packed [M, ceil(V/32)] on the GPU, bits >= V zero."""
    M, V = allowed.shape
    words = (V + 31) // 32
    pad = np.zeros((M, words * 32), dtype=np.uint8)
    pad[:, :V] = allowed.numpy().astype(np.uint8)
    packed = np.packbits(pad, axis=1, bitorder="little").view(np.int32)
    return torch.from_numpy(packed.copy()).cuda()


def _bf16_step(v):
    return 2.0 ** (math.floor(math.log2(abs(v))) - 7) if v != 0.0 else 0.0


def _check(name, c, w_gpu, logits, absdot, allowed, mask_gpu):
    """(a) and (b) for one mask. `allowed` bool [M, V] or None (all allowed);
    `mask_gpu` is what the kernels get (may be None, may carry bits >= V)."""
    from opsagent_amd import ops

    x = c["x"]
    M, K = x.shape
    V = w_gpu.shape[0]
    fused = ops.head_argmax(x, w_gpu, mask_gpu).cpu()
    ref = ops.greedy_sample_masked(ops.linear(x, w_gpu), mask_gpu).cpu()
    print(f"{name}: fused {fused.tolist()} unfused {ref.tolist()}")
    assert torch.equal(fused, ref), f"{name}: fused {fused} != unfused {ref}"
    chain = 8 * ((K + 511) // 512) + 6
    for m in range(M):
        t = int(fused[m])
        ok = torch.ones(V, dtype=torch.bool) if allowed is None else allowed[m]
        if not bool(ok.any()):
            assert t == -1, f"{name}: row {m} chose {t} with nothing allowed"
            continue
        assert 0 <= t < V, f"{name}: row {m} token {t} outside [0, {V})"
        assert bool(ok[t]), f"{name}: row {m} chose masked token {t}"
        lg = logits[m].masked_fill(~ok, float("-inf"))
        b = int(lg.argmax())
        best, got = float(lg[b]), float(logits[m, t])
        tol = _bf16_step(max(abs(best), abs(got))) + chain * 2.0 ** -24 * float(
            absdot[m, b] + absdot[m, t]
        )
        print(f"  row {m}: chose {t} ({got:.6f}), best {b} ({best:.6f}), tol {tol:.3g}")
        assert best - got <= tol, (
            f"{name}: row {m} chose {t} ({got}) but {b} has {best} (tol {tol})"
        )
    return fused


def _planted(c, rows_vals):
    """copy of w with rows replaced; returns (w_gpu, logits, absdot)"""
    w = c["w"].clone()
    logits, absdot = c["logits"].clone(), c["absdot"].clone()
    for r, val in rows_vals:
        vb = val.to(torch.bfloat16)
        w[r] = vb.cuda()
        logits[:, r] = c["x64"] @ vb.double()
        absdot[:, r] = c["x64"].abs() @ vb.double().abs()
    return w, logits, absdot


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("V,K", SHAPES)
def test_masks(V, K, M):
    from opsagent_amd import ops

    c = _case(V, K, M)
    w, logits, absdot = c["w"], c["logits"], c["absdot"]
    words = (V + 31) // 32
    nwaves = 4 * ops.head_argmax_grid(V, M)
    idx = torch.arange(V)

    _check("null", c, w, logits, absdot, None, None)
    ones = torch.full((M, words), -1, dtype=torch.int32).cuda()  # bits >= V too
    out = _check("ones", c, w, logits, absdot, None, ones)
    assert int(out.max()) < V
    zero = torch.zeros(M, V, dtype=torch.bool)
    out = _check("zero", c, w, logits, absdot, zero, _pack(zero))
    assert out.tolist() == [-1] * M

    # one bit: row 0, row V-1, second row of a pair, first row of a later
    # trip (where the grid has one), last row of block 0's range
    single = {"first": 0, "last": V - 1, "pair2": 1, "blockend": 7}
    if 2 * nwaves < V:
        single["trip2"] = 2 * nwaves
        single["trip2_pair2"] = 2 * nwaves + 3
    for name, r in single.items():
        a = zero.clone()
        a[:, r] = True
        out = _check(f"one:{name}", c, w, logits, absdot, a, _pack(a))
        # -inf cannot occur with finite operands, so the lone row is chosen
        assert out.tolist() == [r] * M

    a = (idx % 2 == 1).expand(M, V).clone()
    _check("odd", c, w, logits, absdot, a, _pack(a))
    a = (idx >= V // 2).expand(M, V).clone()
    _check("upper", c, w, logits, absdot, a, _pack(a))

    # a mask that excludes the unmasked argmax: plant 8 * x[0], then mask it
    r = (V // 3) | 1
    w2, lg2, ad2 = _planted(c, [(r, 8 * c["x"][0].cpu().float())])
    out = _check("plant", c, w2, lg2, ad2, None, None)
    assert int(out[0]) == r
    a = torch.ones(M, V, dtype=torch.bool)
    a[:, r] = False
    out = _check("plant-masked", c, w2, lg2, ad2, a, _pack(a))
    assert r not in out.tolist()

    # every allowed logit negative
    w3, lg3, ad3 = _planted(c, [(r, -8 * c["x"][0].cpu().float())])
    a = lg3 < 0
    assert bool(a.any(dim=1).all())
    out = _check("negative", c, w3, lg3, ad3, a, _pack(a))
    assert all(float(lg3[m, int(out[m])]) < 0 for m in range(M))


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("V,K", SHAPES)
def test_ties_lowest_index_wins(V, K, M):
    """One winning W row at four indices in different waves, blocks and (where
    the grid has them) trips: the lowest allowed index wins."""
    from opsagent_amd import ops

    c = _case(V, K, M)
    nwaves = 4 * ops.head_argmax_grid(V, M)
    later = 2 * nwaves + 4 if 2 * nwaves + 4 < V else V // 2 + 1
    rows = sorted({2, 25, later, V - 3})
    assert len(rows) == 4
    val = 8 * c["x"][0].cpu().float()
    w2, lg2, ad2 = _planted(c, [(r, val) for r in rows])
    a = torch.zeros(M, V, dtype=torch.bool)
    a[:, rows] = True
    out = _check("tie4", c, w2, lg2, ad2, a, _pack(a))
    assert out.tolist() == [rows[0]] * M
    out = _check("tie4-unmasked", c, w2, lg2, ad2, None, None)
    assert int(out[0]) == rows[0]
    a = torch.zeros(M, V, dtype=torch.bool)
    a[:, rows[2:]] = True
    out = _check("tie2", c, w2, lg2, ad2, a, _pack(a))
    assert out.tolist() == [rows[2]] * M


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("V,K", SHAPES)
def test_signed_zero_and_neg_inf_rows(V, K, M):
    """The rule of masked_argmax holds in the head too: -0 ties with +0 and the
    lowest index wins, wherever the two rows fall in the grid, and a row whose
    logit is -inf is never chosen (-1 if nothing else is allowed).

    The logits are exact by construction. Column k0 of x is 2^-70, column k1
    is 2^64 and column k1 of W is zero. A W row that is zero but for -2^-70 at
    k0 gives -2^-140, which rounds to bf16 -0; a zero row gives +0; a zero row
    with -2^100 at k1 overflows fp32 to -inf. Every other allowed logit is
    negative. Fused and unfused must both give the oracle's token."""
    from opsagent_amd import ops

    c = _case(V, K, M)
    nwaves = 4 * ops.head_argmax_grid(V, M)
    later = 2 * nwaves + 4 if 2 * nwaves + 4 < V else V // 2 + 1
    rows = sorted({2, 3, 25, later, V - 3})
    assert len(rows) == 5
    k0, k1 = 5, K - 3
    x = c["x"].clone()
    x[:, k0], x[:, k1] = 2.0 ** -70, 2.0 ** 64
    base = c["w"].clone()
    base[:, k1] = 0
    negz = torch.zeros(K, dtype=torch.bfloat16)
    negz[k0] = -(2.0 ** -70)
    posz = torch.zeros(K, dtype=torch.bfloat16)
    ninf = torch.zeros(K, dtype=torch.bfloat16)
    ninf[k1] = -(2.0 ** 100)
    bits = {"negz": -0x8000, "posz": 0, "ninf": -0x80}            # bf16 bits as int16
    background = x.cpu().double() @ base.cpu().double().t()       # [M, V]
    negative = background < -1e-3

    def run(plant, allowed_rows, want):
        w = base.clone()
        for r, kind in plant.items():
            w[r] = {"negz": negz, "posz": posz, "ninf": ninf}[kind].cuda()
        lg = ops.linear(x, w)
        for r, kind in plant.items():
            assert (lg[:, r].view(torch.int16).cpu() == bits[kind]).all(), (kind, lg[:, r])
        a = negative.clone()
        a[:, rows] = False
        a[:, allowed_rows] = True
        mask = _pack(a)
        fused = ops.head_argmax(x, w, mask).cpu().tolist()
        unfused = ops.greedy_sample_masked(lg, mask).cpu().tolist()
        print(f"{plant} allowed {allowed_rows}: fused {fused} unfused {unfused} want {want}")
        assert fused == [want] * M and unfused == [want] * M

    for low, rest in (("negz", "posz"), ("posz", "negz")):
        plant = {r: (low if r == rows[0] else rest) for r in rows}
        run(plant, rows, rows[0])
        run(plant, rows[1:], rows[1])
        run(plant, rows[2:], rows[2])
        run(plant, rows[3:], rows[3])
    # pairs of one +0 and one -0 only: the same wave, two waves, two trips
    for lo, hi in ((rows[0], rows[1]), (rows[0], rows[2]), (rows[2], rows[3]), (rows[3], rows[4])):
        for a_kind, b_kind in (("negz", "posz"), ("posz", "negz")):
            plant = {r: "ninf" for r in rows}
            plant[lo], plant[hi] = a_kind, b_kind
            run(plant, rows, lo)
    ones = torch.zeros(M, V, dtype=torch.bool)
    ones[:, rows] = True
    w = base.clone()
    for r in rows:
        w[r] = ninf.cuda()
    mask = _pack(ones)                                            # every allowed logit is -inf
    assert ops.head_argmax(x, w, mask).cpu().tolist() == [-1] * M
    assert ops.greedy_sample_masked(ops.linear(x, w), mask).cpu().tolist() == [-1] * M
    lone = 9                                                      # -inf beside one finite logit
    assert lone not in rows
    ones[:, lone] = True
    mask = _pack(ones)
    assert ops.head_argmax(x, w, mask).cpu().tolist() == [lone] * M
    assert ops.greedy_sample_masked(ops.linear(x, w), mask).cpu().tolist() == [lone] * M


@pytest.mark.parametrize("V,K", SHAPES)
def test_m2_disjoint_masks(V, K):
    """Row 0 allows even rows below V/2, row 1 odd rows above; each row's
    planted global winner sits where only the OTHER row may go — the pair is
    live through the OR, but must not enter the wrong row's best."""
    c = _case(V, K, 2)
    idx = torch.arange(V)
    a = torch.stack([(idx % 2 == 0) & (idx < V // 2), (idx % 2 == 1) & (idx > V // 2)])
    p0 = (V // 2 + 5) | 1        # row 0's winner: odd, above V/2
    p1 = (V // 4) & ~1           # row 1's winner: even, below V/2
    w2, lg2, ad2 = _planted(
        c, [(p0, 8 * c["x"][0].cpu().float()), (p1, 8 * c["x"][1].cpu().float())]
    )
    assert int(lg2[0].argmax()) == p0 and int(lg2[1].argmax()) == p1
    out = _check("disjoint", c, w2, lg2, ad2, a, _pack(a))
    assert int(out[0]) % 2 == 0 and int(out[0]) < V // 2
    assert int(out[1]) % 2 == 1 and int(out[1]) > V // 2


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("V,K", [(40, 1040), (16400, 512)])
def test_writes_stay_inside_out_and_ws(V, K, M):
    from opsagent_amd import ops

    c = _case(V, K, M)
    n = M * ops.head_argmax_grid(V, M)
    big_out = torch.full((M + 16,), -77, dtype=torch.int32, device="cuda")
    big_ws = torch.full((n + 32,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    out = ops.head_argmax(c["x"], c["w"], None, out=big_out[8:8 + M], ws=big_ws[16:16 + n])
    ref = ops.greedy_sample_masked(ops.linear(c["x"], c["w"]), None)
    assert torch.equal(out.cpu(), ref.cpu())
    bo, bw = big_out.cpu(), big_ws.cpu()
    assert bool((bo[:8] == -77).all()) and bool((bo[8 + M:] == -77).all())
    assert bool((bw[:16] == 0x5A5A5A5A5A5A).all())
    assert bool((bw[16 + n:] == 0x5A5A5A5A5A5A).all())


def test_launcher_error_codes():
    from opsagent_amd.ops import hip_lib

    lib = hip_lib.get_lib()
    x = torch.zeros(3, 64, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(48, 64, dtype=torch.bfloat16, device="cuda")
    ws = torch.zeros(4096, dtype=torch.int64, device="cuda")
    out = torch.full((4,), -77, dtype=torch.int32, device="cuda")
    s = hip_lib.current_stream_ptr()

    def call(M, V, K):
        return lib.oa_head_argmax(
            s, x.data_ptr(), w.data_ptr(), None, ws.data_ptr(), out.data_ptr(), M, V, K
        )

    assert call(3, 48, 64) < 0
    assert call(0, 48, 64) < 0
    assert call(1, 44, 64) < 0
    assert call(1, 48, 60) < 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-77] * 4, "a rejected call must launch nothing"
    assert call(1, 48, 64) == 0
    torch.cuda.synchronize()
    assert int(out[0]) == 0  # all logits equal (0): the lowest index


MICRO_CFG = {
    "model": "llama3-micro", "max_seq_len": 1024, "kv_block_size": 32,
    "kv_cache_gb": 1, "max_batch_size": 4, "use_hipgraph": True, "seed": 5,
}


def test_engine_fused_head_matches_unfused():
    """The micro model through the engine with the fused head on and off:
    equal ids in a grammar-constrained and an unconstrained greedy run, the
    fused path taken exactly when it may be (perf counter)."""
    from opsagent_amd.engine.engine import LLMEngine, SamplingParams
    from opsagent_amd.engine.grammar import GrammarMode

    runs = {}
    for flag in (True, False):
        eng = LLMEngine(dict(MICRO_CFG, fused_head=flag))
        assert eng.fused_head is flag
        ids = eng.tokenizer.encode("emit json for pod nginx", add_bos=True)
        eng.perf.reset()
        free, _ = eng.generate(ids, SamplingParams(max_new_tokens=24))
        st = eng.perf.get_metric_stats("engine_head_live_rows")
        if flag:
            assert st and st["count"] > 0 and st["min"] == eng.spec.vocab_size
        else:
            assert st is None
        eng.perf.reset()
        gram, _ = eng.generate(
            ids, SamplingParams(max_new_tokens=48, grammar=GrammarMode.TOOLPROMPT)
        )
        st = eng.perf.get_metric_stats("engine_head_live_rows")
        if flag:
            assert st and st["count"] > 0 and 1 <= st["min"] <= eng.spec.vocab_size
            eng.perf.reset()
            eng.generate(ids, SamplingParams(max_new_tokens=8, logprobs=True))
            eng.generate(ids, SamplingParams(max_new_tokens=8, temperature=0.7))
            assert eng.perf.get_metric_stats("engine_head_live_rows") is None
        runs[flag] = (free, gram)
        del eng
        torch.cuda.empty_cache()
    assert runs[True][0] == runs[False][0]
    assert runs[True][1] == runs[False][1]
