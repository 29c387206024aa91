"""The single-launch decode attention (in-launch split combine) against the
two-kernel path, and both against the arithmetic the stand-alone combine has
always had (run on a real MI355X: `pytest -m gpu`).

Inputs, probes, poison blocks and tolerances come from tests/attention_oracle,
as in tests/test_attention_edges_gpu.py. Three kinds of check:

  * fused_combine=True is bit-equal to fused_combine=False: output and, on the
    rope path, both scattered caches;
  * the two-kernel output is bit-equal to a combine done here in torch from
    the kernel's own o_part / ml_part, in the combine kernel's grouping and
    order: split s in group s & 3; per group the max over live splits, then
    lt / ot accumulated in ascending s with fma(x, e, acc); groups merged in
    order 1, 2, 3 with acc = fma(acc, a1, x * a2); divide; bf16 rounding.
    fma is emulated through fp64: the product of two fp32 is exact there, and
    the rounding error of the fp64 sum is recovered with a two-sum and folded
    into the sticky end of the value before the one rounding to fp32, so the
    result is the correctly rounded a * b + c;
    e = exp2((m - mt) * log2e_f32) is evaluated on the device, where
    exp2 of a normal-range argument is the same hardware instruction the
    kernel's __expf uses;
  * the rope path stays within the case's T of the fp64 reference.
"""

import contextlib

import pytest
import torch

import attention_oracle as ao
from opsagent_amd import ops
from opsagent_amd.ops import hip_lib, torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = ao.D_HEAD
LOG2E_F32 = 1.4426950408889634  # rounds to 0x3fb8aa3b, the kernel's constant


# ------------------------------------------------------------------ helpers
def _workspace(B, Hk, G, nsplit, fill=float("nan")):
    """(o_part, ml_part, tickets): partials poisoned, ticket words zero."""
    o_part = torch.full((B * Hk * nsplit, G, D), fill, dtype=torch.float32, device=DEV)
    ml_part = torch.full((B * Hk * nsplit, G, 2), fill, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(B * Hk, dtype=torch.int32, device=DEV)
    return o_part, ml_part, cnt


def _fma(a, b, c):
    """Correctly rounded fp32 a * b + c. p = a * b is exact in fp64; s = p + c
    rounds once, and two-sum gives that rounding's error e exactly. A plain
    cast of s could round a second time on an fp32 halfway case that e would
    have decided; nudging s by one fp64 ulp towards the true sum when e != 0
    (round-to-odd) makes the single cast correct."""
    p = a.double() * b.double()
    cd = c.double().expand_as(p) if c.dim() <= p.dim() else c.double()
    p, cd = torch.broadcast_tensors(p, cd)
    s = p + cd
    bb = s - p
    e = (p - (s - bb)) + (cd - bb)
    bits = s.contiguous().view(torch.int64)
    inexact = (e != 0) & torch.isfinite(s)
    even = (bits & 1) == 0
    # the true sum lies strictly between s and its neighbour on e's side
    away = ((e > 0) == (s > 0)) | (s == 0)
    step = torch.where(away, torch.ones_like(bits), -torch.ones_like(bits))
    odd = torch.where(inexact & even, bits + step, bits)
    return odd.view(torch.float64).float()


def _exp(x):
    return torch.exp2(x * LOG2E_F32)


def torch_combine(o_part, ml_part, B, Hk, G, nsplit):
    """decode_combine_kernel's arithmetic, fp32, same grouping and order."""
    o = o_part.view(B * Hk, nsplit, G, D)
    m = ml_part.view(B * Hk, nsplit, G, 2)[..., 0]
    l = ml_part.view(B * Hk, nsplit, G, 2)[..., 1]
    ninf = torch.full((B * Hk, G), float("-inf"), dtype=torch.float32, device=o.device)
    zero = torch.zeros_like(ninf)
    groups = []
    for sh in range(4):
        mt = ninf.clone()
        for s in range(sh, nsplit, 4):
            mt = torch.where(l[:, s] > 0, torch.maximum(mt, m[:, s]), mt)
        lt = zero.clone()
        ot = torch.zeros(B * Hk, G, D, dtype=torch.float32, device=o.device)
        for s in range(sh, nsplit, 4):
            live = l[:, s] > 0
            sc = _exp(m[:, s] - mt)
            lt = torch.where(live, _fma(l[:, s], sc, lt), lt)
            ot = torch.where(live[..., None], _fma(o[:, s], sc[..., None], ot), ot)
        groups.append((mt, lt, ot))
    mt, lt, ot = groups[0]
    for g2 in range(1, 4):
        m2, l2, o2 = groups[g2]
        mn = torch.maximum(mt, m2)
        a1 = torch.where(lt > 0, _exp(mt - mn), zero)
        a2 = torch.where(l2 > 0, _exp(m2 - mn), zero)
        ot = _fma(ot, a1[..., None], o2 * a2[..., None])
        lt = _fma(lt, a1, l2 * a2)
        mt = torch.where(lt > 0, mn, ninf)
    res = torch.where(lt[..., None] > 0, ot / lt[..., None], torch.zeros_like(ot))
    return res.to(torch.bfloat16).view(B, Hk * G, D)


def _report_equal(what, name, got, want):
    g = got.contiguous().view(torch.int16)
    w = want.contiguous().view(torch.int16)
    diff = int((g != w).sum())
    print(f"\nDECODE_FUSED {what} {name} differing_elements={diff} of {g.numel()}")
    assert diff == 0, f"{what} {name}: {diff} of {g.numel()} elements differ"


class RopeRun:
    """Device inputs of one rope case; every call starts from the case's
    cache (poison in the new token's slot) unless told to keep its own."""

    def __init__(self, c):
        self.c = c
        self.cos, self.sin = c.cos.to(DEV), c.sin.to(DEV)
        self.bt, self.lens, self.slots = c.bt.to(DEV), c.lens.to(DEV), c.slots.to(DEV)
        # q, k, v as head-slices of one fused qkv buffer, as the engine passes them
        self.raw = torch.cat(
            [c.q.flatten(1), c.k_new.flatten(1), c.v_new.flatten(1)], dim=-1).to(DEV)

    def views(self):
        c = self.c
        t = self.raw
        q = t[:, : c.Hq * D].view(c.B, c.Hq, D)
        k = t[:, c.Hq * D: (c.Hq + c.Hk) * D].view(c.B, c.Hk, D)
        v = t[:, (c.Hq + c.Hk) * D:].view(c.B, c.Hk, D)
        return q, k, v

    def caches(self):
        return self.c.kc.to(DEV), self.c.vc.to(DEV)

    def __call__(self, fused, ws=None, caches=None):
        c = self.c
        kc, vc = caches if caches is not None else self.caches()
        if ws is None:
            ws = _workspace(c.B, c.Hk, c.G, c.nsplit)
        q, k, v = self.views()
        out = ops.attention_decode_rope(
            q, k, v, kc, vc, self.bt, self.lens, self.cos, self.sin, self.slots,
            scale=c.scale, workspace=ws, nsplit=c.nsplit, fused_combine=fused)
        return out, kc, vc, ws


def _with_reference(c):
    if c.q_eff is None:
        pos = c.lens.long() - 1
        qr, kr = torch_ref.rope_apply(c.q.float(), c.k_new.float(), c.cos, c.sin, pos)
        c.set_roped(qr, kr)
    return c


@contextlib.contextmanager
def _fixed_lens(lens):
    """ao.DecodeCase draws its lengths from ao.decode_lens; the extra shapes
    below need exact ones."""
    saved = ao.decode_lens
    ao.decode_lens = lambda B, bs, nsplit, maxlen, rot: list(lens)
    try:
        yield
    finally:
        ao.decode_lens = saved


def _custom_case(name, G, Hk, bs, nsplit, lens, rope, index):
    with _fixed_lens(lens):
        return ao.DecodeCase(name, len(lens), G, Hk, bs, nsplit, max(lens), None,
                             rope=rope, index=index)


def _check_rope_case(name, c):
    run = RopeRun(c)
    out2, kc2, vc2, ws2 = run(False)
    out1, kc1, vc1, ws1 = run(True)
    torch.cuda.synchronize()
    err = ao.row_rel_err(out1, c.ref)
    print(f"\nDECODE_FUSED rope {name} err={err:.5f} T={c.tol:.5f}")
    _report_equal("rope_fused_vs_two_kernel", name, out1, out2)
    _report_equal("rope_k_cache", name, kc1, kc2)
    _report_equal("rope_v_cache", name, vc1, vc2)
    assert int(ws1[2].abs().sum()) == 0, "ticket words not handed back zeroed"
    assert err <= c.tol, f"{name}: row_rel_err {err:.5f} > T {c.tol:.5f}"
    ref = torch_combine(ws2[0], ws2[1], c.B, c.Hk, c.G, c.nsplit)
    _report_equal("rope_two_kernel_vs_torch_combine", name, out2, ref)


# ------------------------------------------------- the oracle's rope cases
@pytest.mark.parametrize("name", [c[0] for c in ao.ROPE_CASES])
def test_rope_fused_equals_two_kernel(name):
    c = ao.rope_case_with_reference(name, torch_ref.rope_apply)
    _check_rope_case(name, c)


# ------------------------------------------------ the oracle's plain cases
@pytest.mark.parametrize("name", [c[0] for c in ao.DECODE_CASES])
def test_paged_fused_equals_two_kernel(name):
    c = ao.decode_case(name)
    args = (c.q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.bt.to(DEV), c.lens.to(DEV))
    ws = _workspace(c.B, c.Hk, c.G, c.nsplit)
    out2 = ops.attention_decode_paged(
        *args, scale=c.scale, workspace=ws, nsplit=c.nsplit, fused_combine=False)
    out1 = ops.attention_decode_paged(
        *args, scale=c.scale, workspace=_workspace(c.B, c.Hk, c.G, c.nsplit),
        nsplit=c.nsplit, fused_combine=True)
    torch.cuda.synchronize()
    _report_equal("paged_fused_vs_two_kernel", name, out1, out2)
    ref = torch_combine(ws[0], ws[1], c.B, c.Hk, c.G, c.nsplit)
    _report_equal("paged_two_kernel_vs_torch_combine", name, out2, ref)


# ------------------------------------------------------------ extra shapes
# (name, G, Hk, block_size, nsplit, lens): the smallest that reach each branch
def _extra_cases():
    cases = []
    for ns in (1, 2, 3, 5, 8):
        # lengths 1, 2, nsplit-1, nsplit+1: empty splits and empty waves; the
        # newest key lands in the first split (n = 1) and past it
        lens = [1, 2, max(ns - 1, 1), ns + 1]
        cases.append((f"x_ns{ns}_short", 4, 2, 16, ns, lens))
    # newest key in the LAST split: alone there (57 = 7 * 8 + 1) and behind
    # seven cached keys (64); 200 runs the steady loop of the 4-deep ring
    cases.append(("x_ns8_last_split", 4, 2, 16, 8, [57, 64, 1, 200]))
    # G = 8 at B = 1: the 2-deep ring of the B <= 4 dispatch
    cases.append(("x_g8_b1", 8, 1, 32, 4, [150]))
    # block size 8: block-table entries loaded per lane
    cases.append(("x_bs8", 4, 2, 8, 3, [77, 9]))
    return cases


EXTRA = _extra_cases()


@pytest.mark.parametrize("spec", EXTRA, ids=[e[0] for e in EXTRA])
def test_rope_extra_shapes(spec):
    name, G, Hk, bs, nsplit, lens = spec
    c = _with_reference(
        _custom_case(name, G, Hk, bs, nsplit, lens, rope=True, index=EXTRA.index(spec)))
    _check_rope_case(name, c)


@pytest.mark.parametrize("spec", EXTRA, ids=[e[0] for e in EXTRA])
def test_paged_extra_shapes(spec):
    """The same edges through the plain entry: the non-rope kernels and their
    reducer see empty splits and waves, G = 8 at B = 1 and the per-lane table
    path too."""
    name, G, Hk, bs, nsplit, lens = spec
    c = _custom_case(name, G, Hk, bs, nsplit, lens, rope=False, index=EXTRA.index(spec))
    args = (c.q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.bt.to(DEV), c.lens.to(DEV))
    ws = _workspace(c.B, c.Hk, c.G, c.nsplit)
    out2 = ops.attention_decode_paged(
        *args, scale=c.scale, workspace=ws, nsplit=c.nsplit, fused_combine=False)
    out1 = ops.attention_decode_paged(
        *args, scale=c.scale, workspace=_workspace(c.B, c.Hk, c.G, c.nsplit),
        nsplit=c.nsplit, fused_combine=True)
    torch.cuda.synchronize()
    err = ao.row_rel_err(out2, c.ref)
    print(f"\nDECODE_FUSED paged {name} err={err:.5f} T={c.tol:.5f}")
    _report_equal("paged_fused_vs_two_kernel", name, out1, out2)
    ref = torch_combine(ws[0], ws[1], c.B, c.Hk, c.G, c.nsplit)
    _report_equal("paged_two_kernel_vs_torch_combine", name, out2, ref)
    assert err <= c.tol, f"{name}: row_rel_err {err:.5f} > T {c.tol:.5f}"


# ------------------------------------------------------- workspace handling
def test_workspace_reuse_and_graph_replay():
    """One workspace, as the layers of a step share it: partials start as NaN,
    ticket words as zero. Three calls back to back, then three replays of a
    graph that holds two consecutive calls: every result equals the first and
    the ticket words end at zero."""
    name = "rope_b2_g4_bs32_s8"
    c = ao.rope_case_with_reference(name, torch_ref.rope_apply)
    run = RopeRun(c)
    first, _, _, _ = run(False)
    ws = _workspace(c.B, c.Hk, c.G, c.nsplit)
    caches = run.caches()
    for i in range(3):
        out, _, _, _ = run(True, ws=ws, caches=caches)
        _report_equal(f"back_to_back_{i}", name, out, first)
    assert int(ws[2].abs().sum()) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(True, ws=ws, caches=caches)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o1, _, _, _ = run(True, ws=ws, caches=caches)
        o2, _, _, _ = run(True, ws=ws, caches=caches)
    for i in range(3):
        o1.fill_(float("nan"))
        o2.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _report_equal(f"graph_replay_{i}_call0", name, o1, first)
        _report_equal(f"graph_replay_{i}_call1", name, o2, first)
    assert int(ws[2].abs().sum()) == 0


# ------------------------------------------------------------- output guard
def test_fused_output_stays_inside_its_buffer():
    name = "rope_b2_g4_bs32_s8"
    c = ao.rope_case_with_reference(name, torch_ref.rope_apply)
    run = RopeRun(c)
    want, _, _, _ = run(False)
    pad = 4096
    n_out = c.B * c.Hq * D
    big = torch.full((pad + n_out + pad,), float("nan"), dtype=torch.bfloat16, device=DEV)
    before = big.view(torch.int16).clone()
    out = big[pad: pad + n_out].view(c.B, c.Hq, D)
    q, k, v = run.views()
    kc, vc = run.caches()
    o_part, ml_part, cnt = _workspace(c.B, c.Hk, c.G, c.nsplit)
    rc = hip_lib.get_lib().oa_attention_decode_rope_fused(
        hip_lib.current_stream_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        kc.data_ptr(), vc.data_ptr(), run.bt.data_ptr(), run.lens.data_ptr(),
        run.cos.data_ptr(), run.sin.data_ptr(), run.slots.data_ptr(),
        o_part.data_ptr(), ml_part.data_ptr(), cnt.data_ptr(), out.data_ptr(),
        c.B, c.Hq, c.Hk, D, run.bt.shape[1], c.bs, c.nsplit, D ** -0.5,
        q.stride(0), k.stride(0), v.stride(0))
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()), "non-finite value inside the output"
    after = big.view(torch.int16)
    assert torch.equal(after[:pad], before[:pad]), "wrote in front of the output"
    assert torch.equal(after[pad + n_out:], before[pad + n_out:]), "wrote past the output"
    _report_equal("guarded_output", name, out, want)
