"""fp8-KV counterparts of the decode cases in tests/attention_oracle.py, shared
by tests/test_kv_fp8_oracle.py (CPU mutant proof) and tests/test_kv_fp8_gpu.py.

Construction, per case:
  1. every (slot, head) row of `vc` is multiplied by a factor drawn from
     {0.25, 0.5, 1, 2, 4} (fixed seed per case), so V rows carry visibly
     different scales and a wrong V scale shows;
  2. `kc` and `vc` are quantised per row with torch_ref.quant_fp8;
  3. the oracle attends over the DEQUANTISED tensors (kc_eff / vc_eff), i.e.
     the test asks whether a kernel computes attention over the cache's own
     values, not how good the format is;
  4. T = 4 N with N = decode_emulation's row_rel_err on those same tensors.
"""

from __future__ import annotations

import functools
from typing import Dict, List, Tuple

import torch

import attention_oracle as ao
from opsagent_amd.ops import torch_ref

FP8_CASES = [
    "b2_g1_bs16_s1",
    "b2_g2_bs32_s3",
    "b2_g4_bs128_s4",
    "b2_g8_bs16_s8",
    "b5_g2_bs128_s8",
    "b5_g8_bs32_s3",
    "b5_g4_bs32_s4_scale02",
    "b9_g1_bs128_s3",
    "b9_g4_bs32_s4",
    "b9_g8_bs16_s1",
]
V_FACTORS = (0.25, 0.5, 1.0, 2.0, 4.0)


def pipeline_form(B: int, G: int) -> str:
    """The launcher's rule (oa_attention_decode_fp8): the 8-deep key-quad
    pipeline at B <= 4 and G <= 4, the 4-deep one otherwise."""
    return "deep8" if B <= 4 and G <= 4 else "deep4"


def quantise_cache(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[nb, bs, Hk, D] -> (uint8 codes [nb, bs, Hk, D], f32 scales [nb, bs, Hk])."""
    codes, scale = torch_ref.quant_fp8(x)
    return codes, scale.reshape(x.shape[:-1])


def dequantise_cache(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The reference read path over every slot, in fp32 (no bf16 rounding)."""
    nb, bs = codes.shape[:2]
    every = torch.arange(nb * bs, dtype=torch.int32)
    k, _ = torch_ref.kv_gather_fp8(codes, codes, scale, scale, every, dtype=torch.float32)
    return k.reshape(codes.shape)


class Fp8DecodeCase:
    def __init__(self, name: str):
        base = ao.decode_case(name)          # shared and cached: never mutated
        self.base = base
        self.name = name
        self.B, self.G, self.Hk, self.Hq, self.bs = base.B, base.G, base.Hk, base.Hq, base.bs
        self.nsplit, self.scale = base.nsplit, base.scale
        self.q, self.bt, self.lens = base.q, base.bt, base.lens
        index = [c[0] for c in ao.DECODE_CASES].index(name)
        gen = torch.Generator().manual_seed(9100 + index)
        nb, bs, Hk, _ = base.vc.shape
        pick = torch.randint(0, len(V_FACTORS), (nb, bs, Hk), generator=gen)
        fac = torch.tensor(V_FACTORS)[pick]
        # powers of two: exact in bf16
        self.kc_raw = base.kc
        self.vc_raw = (base.vc.float() * fac.unsqueeze(-1)).to(torch.bfloat16)
        self.k_codes, self.k_scale = quantise_cache(self.kc_raw)
        self.v_codes, self.v_scale = quantise_cache(self.vc_raw)
        self.kc_eff = dequantise_cache(self.k_codes, self.k_scale)
        self.vc_eff = dequantise_cache(self.v_codes, self.v_scale)

    # ---- oracle on the dequantised cache --------------------------------
    def _oracle(self, kc, vc, **knobs):
        return ao.decode_oracle(self.q, kc, vc, self.bt, self.lens, self.scale, **knobs)

    @functools.cached_property
    def ref(self) -> torch.Tensor:
        return self._oracle(self.kc_eff, self.vc_eff)

    @functools.cached_property
    def noise(self) -> float:
        return ao.row_rel_err(
            ao.decode_emulation(self.q, self.kc_eff, self.vc_eff, self.bt, self.lens, self.scale),
            self.ref)

    @property
    def tol(self) -> float:
        return ao.TOL_FACTOR * self.noise

    @functools.cached_property
    def ref_unquantised(self) -> torch.Tensor:
        """Oracle on the cache before quantisation (accuracy of the format)."""
        return self._oracle(self.kc_raw, self.vc_raw)

    # ---- mutants ----------------------------------------------------------
    def mutants(self) -> List[Tuple[str, dict]]:
        """The range / table / combine mutants of the bf16 proof, unchanged."""
        return self.base.mutants()

    def mutant_err(self, knobs: dict) -> float:
        return ao.row_rel_err(self._oracle(self.kc_eff, self.vc_eff, **knobs), self.ref)

    def scale_mutants(self) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """name -> (k_scale, v_scale) a wrong kernel would apply to the codes."""
        ks, vs = self.k_scale, self.v_scale
        nb, bs, Hk = ks.shape

        def next_slot(s):
            return s.reshape(nb * bs, Hk).roll(-1, dims=0).reshape(nb, bs, Hk)

        m = {
            "v_scale_ignored": (ks, torch.ones_like(vs)),
            "kv_scales_exchanged": (vs, ks),
            "k_scale_from_slot+1": (next_slot(ks), vs),
            "v_scale_from_slot+1": (ks, next_slot(vs)),
        }
        if Hk >= 2:
            m["k_scale_head_rolled"] = (ks.roll(1, dims=2), vs)
            m["v_scale_head_rolled"] = (ks, vs.roll(1, dims=2))
            m["head0_scale_for_all"] = (ks[..., :1].expand_as(ks), vs[..., :1].expand_as(vs))
        return m

    def scale_mutant_err(self, ks: torch.Tensor, vs: torch.Tensor) -> float:
        kc = dequantise_cache(self.k_codes, ks.contiguous())
        vc = dequantise_cache(self.v_codes, vs.contiguous())
        return ao.row_rel_err(self._oracle(kc, vc), self.ref)


@functools.lru_cache(maxsize=None)
def fp8_case(name: str) -> Fp8DecodeCase:
    return Fp8DecodeCase(name)
