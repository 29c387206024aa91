"""Attention kernels vs the fp64 oracle at the edges where kernels go wrong
(run on a real MI355X: `pytest -m gpu`).

Inputs, probes, poison blocks and tolerances come from tests/attention_oracle;
tests/test_attention_oracle.py proves on the CPU that every listed wrong
kernel (dropped tile, off-by-one mask, len-1, permuted block table, lost or
doubled split-boundary key, ...) lands at >= 4 T on exactly these cases, where
T = 4 x the bf16 noise floor of a correct kernel. Each test prints
`ATTN_EDGE <family> <case> err T ratio` (visible with -s).
"""

import os

import pytest
import torch

import attention_oracle as ao
from opsagent_amd import ops
from opsagent_amd.ops import torch_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _check(family, name, got, case):
    err = ao.row_rel_err(got, case.ref)
    tol = case.tol
    print(f"\nATTN_EDGE {family} {name} err={err:.5f} T={tol:.5f} ratio={err / tol:.3f}")
    assert err <= tol, f"{family} {name}: row_rel_err {err:.5f} > T {tol:.5f}"


# ---------------------------------------------------------------- prefill
_VARIANT_FAMILY = {7: "prefill_v2", 8: "prefill_v3", 9: "prefill_v4"}
_PREFILL_PARAMS = [
    pytest.param(variant, c[0], id=f"v{variant}-{c[0]}")
    for variant in (7, 8, 9)
    for c in ao.PREFILL_CASES
    # the GQA-merged kernel exists for Hq/Hk in {2, 4, 8} only
    if variant != 9 or c[2] // c[3] in (2, 4, 8)
]


@pytest.mark.parametrize("variant,name", _PREFILL_PARAMS)
def test_prefill_edges(variant, name):
    c = ao.prefill_case(name)
    if c.strided:
        # q, k, v as head-slices of one fused qkv buffer (token stride
        # (Hq + 2 Hk) * D), as the engine passes them
        D = ao.D_HEAD
        qkv = torch.cat([c.q.flatten(2), c.k.flatten(2), c.v.flatten(2)], dim=-1).to(DEV)
        qf, kf, vf = qkv.split([c.Hq * D, c.Hk * D, c.Hk * D], dim=-1)
        q = qf.view(c.B, c.Sq, c.Hq, D)
        k = kf.view(c.B, c.Skv, c.Hk, D)
        v = vf.view(c.B, c.Skv, c.Hk, D)
        assert not q.is_contiguous() and not k.is_contiguous()
    else:
        q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
    os.environ["OPSAGENT_PREFILL_VARIANT"] = str(variant)
    try:
        out = ops.attention_prefill(q, k, v, scale=c.scale)
    finally:
        os.environ.pop("OPSAGENT_PREFILL_VARIANT", None)
    _check(_VARIANT_FAMILY[variant], name, out, c)


# ----------------------------------------------------------------- decode
@pytest.mark.parametrize("fused", [False, True], ids=["two_kernel", "fused"])
@pytest.mark.parametrize("name", [c[0] for c in ao.DECODE_CASES])
def test_decode_edges(name, fused):
    c = ao.decode_case(name)
    out = ops.attention_decode_paged(
        c.q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.bt.to(DEV), c.lens.to(DEV),
        scale=c.scale, nsplit=c.nsplit, fused_combine=fused,
    )
    family = "decode_fused" if fused else ("decode_deep" if c.B <= 4 else "decode_shallow")
    _check(family, name, out, c)


# ------------------------------------------------------------ rope-fused decode
@pytest.mark.parametrize("name", [c[0] for c in ao.ROPE_CASES])
def test_decode_rope_edges(name):
    c = ao.rope_case_with_reference(name, torch_ref.rope_apply)
    B, Hq, Hk, D = c.B, c.Hq, c.Hk, ao.D_HEAD
    cos, sin = c.cos.to(DEV), c.sin.to(DEV)
    bt, lens, slots = c.bt.to(DEV), c.lens.to(DEV), c.slots.to(DEV)
    pos = (c.lens - 1).to(torch.int32).to(DEV)
    raw = torch.cat([c.q.flatten(1), c.k_new.flatten(1), c.v_new.flatten(1)], dim=-1).to(DEV)

    def views(t):
        q = t[:, : Hq * D].view(B, Hq, D)
        k = t[:, Hq * D: (Hq + Hk) * D].view(B, Hk, D)
        v = t[:, (Hq + Hk) * D:].view(B, Hk, D)
        return q, k, v

    kc2, vc2 = c.kc.to(DEV), c.vc.to(DEV)
    q2, k2, v2 = views(raw.clone())
    out = ops.attention_decode_rope(
        q2, k2, v2, kc2, vc2, bt, lens, cos, sin, slots, scale=c.scale, nsplit=c.nsplit
    )
    _check("decode_rope", name, out, c)

    # both cache scatters: bit-equal to the separate rope_kv kernel, and the
    # new token's slot (poisoned before the call) now holds roped k and raw v
    kc1, vc1 = c.kc.to(DEV), c.vc.to(DEV)
    q1, k1, v1 = views(raw.clone())
    ops.rope_kv_fused(q1, k1, v1, kc1, vc1, cos, sin, pos, slots)
    assert torch.equal(kc1, kc2), "scattered roped-k mismatch"
    assert torch.equal(vc1, vc2), "scattered v mismatch"
    nbs = kc2.shape[0] * kc2.shape[1]
    k_roped = c.kc_eff.view(nbs, Hk, D)[c.slots.long()]
    got_k = kc2.view(nbs, Hk, D)[slots.long()]
    # one bf16 rounding of an fp32 value: half an ulp, <= 2^-8 of the vector max
    assert ao.row_rel_err(got_k, k_roped) <= 2.0 ** -8 * 1.01
    assert torch.equal(vc2.view(nbs, Hk, D)[slots.long()].cpu(), c.v_new)
