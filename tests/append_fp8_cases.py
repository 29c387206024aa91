"""fp8-KV counterparts of the append cases in tests/append_cases.py, shared by
tests/test_append_fp8_oracle.py (CPU mutant proof) and
tests/test_append_fp8_gpu.py. CPU only; the pattern is that of
tests/kv_fp8_cases.py.

Construction, per case of APPEND_CASES:
  1. `kc` and `vc` of the (cached, never mutated) AppendCase are quantised AS
     THEY ARE, per (slot, head) row, with kv_fp8_cases.quantise_cache — poison
     blocks included, so every slot a clamped load may touch carries a valid
     scale. No V factors are added: the row absmax of the peaked, probed
     inputs already varies enough that every scale mutant is far out, and the
     decode cases' factors {0.25 .. 4} would push range mutants under 4 T;
  2. the oracle is append_oracle over the DEQUANTISED cache (fp32 code * scale,
     no bf16 rounding): the test asks whether a kernel computes attention over
     the cache's own values, not how good the format is;
  3. T = TOL_FACTOR * N with N = append_emulation's row_rel_err on those same
     tensors;
  4. mutants: the case's own range / table / causal / combine mutants, plus
     the seven scale mutants of Fp8DecodeCase.scale_mutants.

One extra parity case, `codes_all`, draws K and V codes uniformly from the 254
non-NaN e4m3fn codes (subnormals, both zeros and +-448 included) under
heterogeneous per-row scales, so a conversion shortcut — a bit trick that
mishandles exponent field 0, say — cannot pass.
"""

from __future__ import annotations

import functools
from typing import Dict, List, Tuple

import torch

import append_cases as ac
import kv_fp8_cases as kf
from attention_oracle import D_HEAD, PEAK, TOL_FACTOR, _ceil_div, row_rel_err

FP8_APPEND_CASE_NAMES = list(ac.APPEND_CASE_NAMES)
CODES_ALL = "codes_all"
ALL_CASE_NAMES = FP8_APPEND_CASE_NAMES + [CODES_ALL]


class _Fp8AppendBase:
    """Oracle, noise and tolerance over (k_codes, k_scale, v_codes, v_scale)."""

    def _oracle(self, kc, vc, **knobs):
        return ac.append_oracle(self.q, kc, vc, self.bt, self.lens_list, self.cu.tolist(),
                                self.scale, **knobs)

    @functools.cached_property
    def kc_eff(self) -> torch.Tensor:
        return kf.dequantise_cache(self.k_codes, self.k_scale)

    @functools.cached_property
    def vc_eff(self) -> torch.Tensor:
        return kf.dequantise_cache(self.v_codes, self.v_scale)

    @functools.cached_property
    def ref(self) -> torch.Tensor:
        return self._oracle(self.kc_eff, self.vc_eff)

    @functools.cached_property
    def noise(self) -> float:
        emu = ac.append_emulation(self.q, self.kc_eff, self.vc_eff, self.bt, self.lens_list,
                                  self.cu.tolist(), self.scale)
        return row_rel_err(emu, self.ref)

    @property
    def tol(self) -> float:
        return TOL_FACTOR * self.noise

    # ---- scale mutants ----------------------------------------------------
    def scale_mutants(self) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
        """name -> (k_scale, v_scale) a wrong kernel would apply to the codes:
        the seven of the decode proof."""
        return kf.Fp8DecodeCase.scale_mutants(self)

    def scale_mutant_ref(self, ks: torch.Tensor, vs: torch.Tensor) -> torch.Tensor:
        return self._oracle(kf.dequantise_cache(self.k_codes, ks.contiguous()),
                            kf.dequantise_cache(self.v_codes, vs.contiguous()))

    def scale_mutant_noise(self, ks: torch.Tensor, vs: torch.Tensor) -> float:
        """N of the mutant's own oracle: what a kernel applying (ks, vs) shows."""
        kc = kf.dequantise_cache(self.k_codes, ks.contiguous())
        vc = kf.dequantise_cache(self.v_codes, vs.contiguous())
        emu = ac.append_emulation(self.q, kc, vc, self.bt, self.lens_list, self.cu.tolist(),
                                  self.scale)
        return row_rel_err(emu, self._oracle(kc, vc))

    def scale_mutant_err(self, ks: torch.Tensor, vs: torch.Tensor) -> float:
        return row_rel_err(self.scale_mutant_ref(ks, vs), self.ref)


class Fp8AppendCase(_Fp8AppendBase):
    def __init__(self, name: str):
        base = ac.append_case(name)          # shared and cached: never mutated
        self.base = base
        self.name = name
        self.B, self.G, self.Hk, self.Hq, self.bs = base.B, base.G, base.Hk, base.Hq, base.bs
        self.nsplit, self.scale, self.T, self.max_q = base.nsplit, base.scale, base.T, base.max_q
        self.lens_list, self.qlens = base.lens_list, base.qlens
        self.qkv, self.q, self.bt, self.lens, self.cu = base.qkv, base.q, base.bt, base.lens, base.cu
        self.k_codes, self.k_scale = kf.quantise_cache(base.kc)
        self.v_codes, self.v_scale = kf.quantise_cache(base.vc)

    @functools.cached_property
    def ref_unquantised(self) -> torch.Tensor:
        """Oracle on the cache before quantisation (accuracy of the format)."""
        return self.base.ref

    def mutants(self) -> List[Tuple[str, dict]]:
        """The range / table / causal / combine mutants of the bf16 proof."""
        return self.base.mutants()

    def mutant_err(self, knobs: dict) -> float:
        return row_rel_err(self._oracle(self.kc_eff, self.vc_eff, **knobs), self.ref)


def _hetero_factor(shape, gen: torch.Generator) -> torch.Tensor:
    """2^randint(-3..3) * (1 + rand): a neighbour's scale is a wrong one."""
    e = torch.randint(-3, 4, shape, generator=gen).double()
    return torch.exp2(e) * (1 + torch.rand(shape, generator=gen).double())


class CodesAllCase(_Fp8AppendBase):
    """B 1, G 4, Hk 2, block 16, nsplit 2, n 100, L 5 over uniformly drawn
    codes. The construction asserts that every non-NaN code occurs in K and in
    V among the keys some row can see."""

    def __init__(self):
        self.name = CODES_ALL
        self.base = None
        self.B, self.G, self.Hk, self.bs, self.nsplit, self.scale = 1, 4, 2, 16, 2, None
        Hq = self.Hq = self.G * self.Hk
        n, L, D, bs, Hk = 100, 5, D_HEAD, self.bs, self.Hk
        self.lens_list, self.qlens = [n], [L]
        self.T = self.max_q = L
        gen = torch.Generator().manual_seed(9777)
        nblk = _ceil_div(n, bs)
        nb = nblk + 2
        ids = torch.randperm(nb, generator=gen).tolist()
        legal = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8)
        assert legal.numel() == 254
        self.k_codes = legal[torch.randint(0, 254, (nb, bs, Hk, D), generator=gen)]
        self.v_codes = legal[torch.randint(0, 254, (nb, bs, Hk, D), generator=gen)]
        kval = self.k_codes.view(torch.float8_e4m3fn).double()
        rms = kval.pow(2).mean(dim=-1).sqrt()
        # K rows at an rms of about PEAK, a different mantissa per row
        self.k_scale = (PEAK / rms * (0.75 + 0.75 * torch.rand(rms.shape, generator=gen).double())
                        ).float().contiguous()
        self.v_scale = (_hetero_factor((nb, bs, Hk), gen) / 448.0).float().contiguous()
        qkv = (torch.randn(L, (Hq + 2 * Hk) * D, generator=gen) * PEAK).to(torch.bfloat16)
        self.qkv = qkv
        self.q = qkv[:, : Hq * D].view(L, Hq, D)
        mine = [ids.pop() for _ in range(nblk)]
        self.bt = torch.full((1, nblk + 1), ids.pop(), dtype=torch.int32)
        self.bt[0, :nblk] = torch.tensor(mine, dtype=torch.int32)
        self.lens = torch.tensor([n], dtype=torch.int32)
        self.cu = torch.tensor([0, L], dtype=torch.int32)
        # every non-NaN code, in K and in V, on a key the last token attends
        slots = torch.tensor([mine[k // bs] * bs + k % bs for k in range(n)])
        for codes in (self.k_codes, self.v_codes):
            seen = codes.view(nb * bs, Hk, D)[slots].unique()
            assert torch.equal(seen, legal), "codes_all: a code is missing"
        self.ref_unquantised = None


@functools.lru_cache(maxsize=None)
def fp8_append_case(name: str):
    return CodesAllCase() if name == CODES_ALL else Fp8AppendCase(name)


__all__ = [
    "ALL_CASE_NAMES", "CODES_ALL", "FP8_APPEND_CASE_NAMES", "CodesAllCase", "Fp8AppendCase",
    "fp8_append_case",
]
