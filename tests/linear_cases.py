"""Exact-operand cases, fp64 oracles and wrong-kernel mutants for the fp8
linear family (fp8_moe.hip: quant_fp8, VALU gemv_fp8 / gemv_gateup_fp8, the
MFMA GEMV with its norm-fused quantiser, gemm_fp8) and the grouped MoE GEMVs
(moe_gemv.hip). CPU only, no pytest dependency; shared by
tests/test_linear_oracle.py (CPU proof that every mutant is visible) and the
GPU files tests/test_linear_fp8_gpu.py and tests/test_moe_grouped_gpu.py.

Method (the attention tests' one, tests/attention_oracle.py):

  * the oracle knows the operands EXACTLY. An fp8 weight is code * scale. The
    VALU and MoE kernels take bf16 x as it is. The MFMA GEMV quantises x on the
    device, so modes without a norm get x on the e4m3 grid: row m is
    (e4m3 value) * 2^e_m with one element at +-448 * 2^e_m, hence amax/448 and
    448/amax are powers of two and every x * inv is a code (`grid_x` asserts
    the round trip through torch_ref bit for bit). gemm_fp8 takes codes and
    scales for both operands.
  * per-row weight scales are heterogeneous, 2^randint(-3..3) * (1+rand)/448,
    drawn per row and per (expert, row): a neighbour's scale is a wrong one.
  * oracle = fp64 on the dequantised operands; emulation = the same in fp32,
    output rounded to bf16 (MoE MLP: act rounded to bf16 between the stages);
    N = row_rel_err(emulation, oracle), T = 4 N.
  * norm-fused quantisation (quant_norm_fp8_kernel): x*rstd*g*inv is not on
    the grid and the device's codes cannot be read back. The oracle quantises
    in fp64; an element is AMBIGUOUS when its fp64 pre-round value lies within
    2^-20 (relative) of a rounding midpoint, the fp32 evaluation error of four
    multiplies and an rsqrtf. N_q = row_rel_err between the oracle and one that
    rounds every ambiguous element the other way; T = 4 (N + N_q); at most
    1e-3 of a case's elements may be ambiguous.
  * PROBES sit where the kernel's own K partition changes hands (`probe_ks`):
    x and every W row are large there (|W code value| >= 192), so a lost or
    doubled element moves the whole row.
  * mutants are keyword knobs of the cores, listed by `case.mutants()`.
"""

from __future__ import annotations

import functools
import zlib
from typing import Dict, List, Tuple

import torch

from attention_oracle import MUTANT_FACTOR, TOL_FACTOR, row_rel_err  # noqa: F401
from opsagent_amd.ops import torch_ref

EPS = 1e-5
AMBIG_WINDOW = 2.0 ** -20
AMBIG_CAP = 1e-3

# value of every e4m3fn code (NaN at 0x7F / 0xFF); codes 0 .. 0x7E ascend
E4M3 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64)
_POS = E4M3[:0x7F].contiguous()
_MID = ((_POS[1:] + _POS[:-1]) / 2).contiguous()

ENV_KNOBS = ("OPSAGENT_FP8_GEMV_MFMA", "OPSAGENT_FP8_GEMV_RW", "OPSAGENT_FP8_GEMV_XS",
             "OPSAGENT_FP8_STAGE", "OPSAGENT_MOE_EMAJ_MIN_P")


def _gen(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


# --------------------------------------------------------------------------
# e4m3 helpers
# --------------------------------------------------------------------------
def round_e4m3(y: torch.Tensor, flip: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Round-to-nearest-even onto the e4m3fn grid (saturating at 448), from
    fp64. Returns (values fp64, ambiguous mask); with `flip` every ambiguous
    element takes the code on the other side of its midpoint."""
    y = y.to(torch.float64)
    a = y.abs().clamp_max(448.0)
    idx = torch.searchsorted(_MID, a.contiguous())          # mids strictly below a
    lo = (idx - 1).clamp_min(0)
    hi = idx.clamp_max(_MID.numel() - 1)
    near = torch.where((a - _MID[lo]).abs() <= (a - _MID[hi]).abs(), lo, hi)
    tie = a == _MID[near]
    idx = torch.where(tie, near + (near % 2), idx)          # even code wins a tie
    amb = ((a - _MID[near]).abs() <= AMBIG_WINDOW * a) & (a > 0)
    if flip:
        idx = torch.where(amb, torch.where(idx == near, near + 1, near), idx)
    return torch.sign(y) * _POS[idx], amb


def code_of(v: torch.Tensor) -> torch.Tensor:
    """uint8 code of exact grid values."""
    return v.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)


def _grid_values(lo: float, hi: float) -> torch.Tensor:
    return _POS[(_POS >= lo) & (_POS <= hi)].clone()


def _signed_pick(vals: torch.Tensor, shape, g: torch.Generator) -> torch.Tensor:
    pick = vals[torch.randint(0, vals.numel(), shape, generator=g)]
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return pick * sign


W_PROBE = _grid_values(192.0, 448.0)      # |W code value| at probe positions
X_GRID_BG = _grid_values(2.0 ** -6, 28.0)  # exact-grid x background
X_GRID_PROBE = _grid_values(320.0, 448.0)  # exact-grid x probes (>= 160)


def weight_codes(rows: int, K: int, probes: List[int], g: torch.Generator) -> torch.Tensor:
    """Random e4m3fn codes without NaN; large values at the probe columns."""
    c = torch.randint(0, 256, (rows, K), generator=g, dtype=torch.int64)
    c = torch.where((c & 0x7F) == 0x7F, c - 1, c).to(torch.uint8)
    if probes:
        c[:, probes] = code_of(_signed_pick(W_PROBE, (rows, len(probes)), g))
    return c


def weight_scales(shape, g: torch.Generator) -> torch.Tensor:
    e = torch.randint(-3, 4, shape, generator=g).double()
    return (torch.exp2(e) * (1 + torch.rand(shape, generator=g).double()) / 448.0).float()


def pin_last_rows(scale: torch.Tensor, rows: int) -> torch.Tensor:
    """The last two rows of every block of `rows` get the largest scale class
    with different mantissas: the answer of a row computed from its
    neighbour (a clamp one row early) then differs where the vector is
    largest. scale: [..., n_blocks * rows]."""
    if rows >= 2:
        # per expert (leading axis) another factor: expert e + 1's is wrong too
        ef = 1.0 + 0.0625 * torch.arange(scale.shape[0] if scale.dim() == 2 else 1).float()
        ef = ef if scale.dim() == 2 else ef[0]
        for b, base in enumerate(range(0, scale.shape[-1], rows)):
            # another pair of mantissas per block: up's scale is not gate's
            scale[..., base + rows - 1] = ef * 8.0 * (1.75 - 0.375 * (b % 2)) / 448.0
            scale[..., base + rows - 2] = ef * 8.0 * (1.25 - 0.125 * (b % 2)) / 448.0
    return scale


def grid_x(M: int, K: int, probes: List[int], g: torch.Generator, e0: int = -2) -> torch.Tensor:
    """bf16 [M, K] that quantises per row without rounding."""
    v = _signed_pick(X_GRID_BG, (M, K), g)
    if probes:
        v[:, probes] = _signed_pick(X_GRID_PROBE, (M, len(probes)), g)
    pset = set(probes)
    free = [k for k in range(K) if k not in pset]
    for m in range(M):
        v[m, free[(3 + 5 * m) % len(free)]] = 448.0 if m % 2 == 0 else -448.0
    e = torch.tensor([(m % 5) + e0 for m in range(M)], dtype=torch.float64)
    x = (v * torch.exp2(e)[:, None]).to(torch.bfloat16)
    assert torch.equal(x.double(), v * torch.exp2(e)[:, None]), "grid x not exact in bf16"
    back = torch_ref.dequant_fp8(*torch_ref.quant_fp8(x))
    assert torch.equal(back, x.float()), "grid x does not survive quantisation bit for bit"
    return x


def _near_midpoint(y: torch.Tensor, window: float = 0.02) -> torch.Tensor:
    a = y.abs().double().clamp_max(448.0)
    idx = torch.searchsorted(_MID, a.contiguous())
    lo, hi = (idx - 1).clamp_min(0), idx.clamp_max(_MID.numel() - 1)
    return torch.minimum((a - _MID[lo]).abs(), (a - _MID[hi]).abs()) <= window * a


def soft_x(M: int, K: int, probes: List[int], g: torch.Generator, big: float = 28.0,
           factor: float = 1.0) -> torch.Tensor:
    """Any-bf16 x: asymmetric randn, rows of different magnitude (so another
    row's rstd is a wrong one), outliers at the probe columns. One probe per
    row is raised by 1, 1.5 or 2 (by m % 3) and is the row's absmax, so the
    per-row quantisation scale of the norm-fused path differs between
    neighbouring rows even after the norm has removed the row's magnitude.
    The other probes are redrawn until 448 * |x| / absmax keeps 2 % clear of
    every e4m3 rounding midpoint: bf16 ratios of small integers hit midpoints
    exactly, and a probe whose code is a coin toss would widen T."""
    x = torch.randn(M, K, generator=g) * 0.5 + 0.1
    if probes:
        n = len(probes)
        mag = big * (1 + 0.25 * torch.rand(M, n, generator=g))
        for m in range(M):
            top = m % n
            mag[m, top] = big * 1.3 * (1 + 0.5 * (m % 3))
            mag[m] = mag[m].to(torch.bfloat16).float()
            for _ in range(64):
                bad = _near_midpoint(448.0 * mag[m] / mag[m, top])
                bad[top] = False
                if not bad.any():
                    break
                redo = big * (1 + 0.25 * torch.rand(n, generator=g))
                mag[m] = torch.where(bad, redo.to(torch.bfloat16).float(), mag[m])
            assert not bad.any()
        sign = torch.randint(0, 2, (M, n), generator=g).float() * 2 - 1
        x[:, probes] = mag * sign
    x *= factor * torch.exp2(torch.tensor([(m % 3) - 1.0 for m in range(M)]))[:, None]
    return x.to(torch.bfloat16)


def norm_weight(K: int, probes: List[int], g: torch.Generator, factor: float = 1.0) -> torch.Tensor:
    """rand + 0.5, and 2.0 at the probe columns: shifted by a word, every
    probe meets a weight at most 3/4 of its own."""
    wn = torch.rand(K, generator=g) + 0.5
    if probes:
        wn[probes] = 2.0
    return (wn * factor).to(torch.bfloat16)


# --------------------------------------------------------------------------
# where each kernel's K partition changes hands
# --------------------------------------------------------------------------
def probe_ks(kind: str, K: int, gateup: bool = False, bf16w: bool = False) -> List[int]:
    ks = {0, K - 1}
    if kind in ("valu", "moe"):
        chunk = 8 if bf16w else 16          # elements per lane per pass
        wave_pass = chunk * 64              # 1024 fp8 / 512 bf16
        ks |= {chunk - 1, chunk, wave_pass - 1, wave_pass}
        if bf16w:
            ks |= {15, 16}
        if K % wave_pass:
            ks |= {K - K % wave_pass, K - 1}   # the partial last pass
    elif kind == "mfma":
        q = K // 4                           # one wave's quarter
        pf = 4 if gateup else 8              # prefetch ring depth
        ks |= {31, 32, 127, 128}
        for w in range(1, 4):
            ks |= {w * q - 1, w * q}
        for w in range(4):
            if 128 * pf < q:
                ks |= {w * q + 128 * pf - 1, w * q + 128 * pf}
    elif kind == "gemm":
        ks |= {15, 16, 127, 128, K - 128}
    return sorted(k for k in ks if 0 <= k < K)


def silu(x: torch.Tensor) -> torch.Tensor:
    return x / (1 + torch.exp(-x))


# --------------------------------------------------------------------------
# linear cases (GEMV families and gemm_fp8)
# --------------------------------------------------------------------------
def _k_mutations(q: torch.Tensor, wv: torch.Tensor, mut: dict):
    """Mutations of the K axis shared by every core: q is [rows, K] on the
    activation side, wv [.., K] on the weight side."""
    if not any(k in mut for k in ("drop_k", "twice_k", "drop_range", "twice_range",
                                  "slice_swap", "ring_stale", "a_swizzle")):
        return q, wv
    q0, w0 = q, wv
    q = q.clone()
    if "drop_k" in mut:
        q[..., mut["drop_k"]] = 0
    if "twice_k" in mut:
        q[..., mut["twice_k"]] *= 2
    if "drop_range" in mut:
        a, b = mut["drop_range"]
        q[..., a:b] = 0
    if "twice_range" in mut:
        a, b = mut["twice_range"]
        q[..., a:b] *= 2
    if "slice_swap" in mut:                  # W bytes [a, a+n) read from [b, b+n)
        a, b, n = mut["slice_swap"]
        wv = wv.clone()
        wv[..., a:a + n] = w0[..., b:b + n]
    if mut.get("ring_stale"):                # odd steps see the even buffer's data
        wv = wv.clone()
        for t in range(1, q.shape[-1] // 128, 2):
            q[..., t * 128:(t + 1) * 128] = q0[..., (t - 1) * 128:t * 128]
            wv[..., t * 128:(t + 1) * 128] = w0[..., (t - 1) * 128:t * 128]
    if mut.get("a_swizzle"):                 # A units XOR-permuted, B not
        K = q.shape[-1]
        view0 = q0.reshape(q0.shape[0], K // 128, 8, 16)
        view = q.reshape(q.shape[0], K // 128, 8, 16)
        for m in range(q.shape[0]):
            perm = [u ^ (m & 7) for u in range(8)]
            view[m] = view0[m][:, perm]
        q = view.reshape(q0.shape)
    return q, wv


class LinCase:
    """One GEMV / GEMM case. kind: valu | mfma | gemm; gateup: rows are I and
    the weight is [2I, K]; mode bit 0 = fused rmsnorm, bit 1 = residual."""

    def __init__(self, kind: str, M: int, N: int, K: int, mode: int = 0, gateup: bool = False):
        self.kind, self.M, self.N, self.K, self.mode, self.gateup = kind, M, N, K, mode, gateup
        self.name = f"{kind}{'_gu' if gateup else ''}_m{M}_n{N}_k{K}_mode{mode}"
        g = _gen(self.name)
        self.probes = probe_ks(kind, K, gateup)
        rows_w = 2 * N if gateup else N
        self.wcodes = weight_codes(rows_w, K, self.probes, g)
        self.wscale = pin_last_rows(weight_scales((rows_w,), g), N)
        # gate-up: keep silu's argument near its knee, not in its relu tails
        self.wn = norm_weight(K, self.probes, g, 2.0 ** -6 if gateup else 1.0) if mode & 1 else None
        self.acodes = self.ascale = self.x = None
        if kind == "gemm":
            self.quant = "codes"
            self.acodes = weight_codes(M, K, self.probes, g)
            self.ascale = weight_scales((M,), g)
        elif kind == "mfma":
            self.quant = "norm" if mode & 1 else "grid"
            if mode & 1:
                self.x = soft_x(M, K, self.probes, g)
            else:
                self.x = grid_x(M, K, self.probes, g, -12 if gateup else -2)
        else:
            self.quant = "none"
            self.x = soft_x(M, K, self.probes, g, factor=2.0 ** -6 if gateup and not mode & 1 else 1.0)
        self.res = None
        if mode & 2:
            plain = self._core(torch.float64)
            self.res = (torch.randn(M, N, generator=g).double() * 0.3
                        * plain.abs().amax(-1, keepdim=True)).to(torch.bfloat16)

    # ---- the computation, with mutant knobs ------------------------------
    def _core(self, dtype, flip: bool = False, **mut) -> torch.Tensor:
        M, N = self.M, self.N
        wv = E4M3[self.wcodes.long()].to(dtype)
        ws = self.wscale.to(dtype)
        self._amb = None
        if self.kind == "gemm":
            q, xs = E4M3[self.acodes.long()].to(dtype), self.ascale.to(dtype)
            if mut.get("x_roll"):
                q = q.roll(1, 0)
        else:
            xv = self.x.to(dtype)
            if mut.get("x_roll"):
                xv = xv.roll(1, 0)
            rstd = None
            if self.mode & 1:
                rstd = torch.rsqrt(xv.pow(2).mean(-1) + EPS)
                gw = self.wn.to(dtype)
                if mut.get("rstd_roll"):
                    rstd = rstd.roll(1)
                if mut.get("normw_shift"):
                    gw = gw.roll(2)
                xg = xv * gw
                xn = xv * rstd[:, None] * gw
            else:
                xg = xn = xv
            if self.quant == "none":
                q, xs = xn, torch.ones(M, dtype=dtype)
            else:
                amax = xg.abs().amax(-1).clamp_min(1e-8)
                if rstd is not None:
                    amax = amax * rstd
                xs = amax / 448.0
                qv, self._amb = round_e4m3(xn * (448.0 / amax)[:, None], flip)
                q = qv.to(dtype)
        if "xscale_shift" in mut:
            xs = xs.roll(mut["xscale_shift"])
        if "wscale_shift" in mut:
            ws = ws.roll(mut["wscale_shift"])
        if mut.get("wscale_ignored"):
            ws = torch.ones_like(ws)
        if mut.get("scales_exchanged"):      # gemm: ascale[n], bscale[m]
            xs, ws = (self.wscale.to(dtype)[torch.arange(M) % N],
                      self.ascale.to(dtype)[torch.arange(N) % M])
        q, wv = _k_mutations(q, wv, mut)
        if mut.get("clamp_row") and N >= 2:  # last W row read one row early
            wv, ws = wv.clone(), ws.clone()
            for base in ((0, N) if self.gateup else (0,)):
                wv[base + N - 1] = wv[base + N - 2]
                ws[base + N - 1] = ws[base + N - 2]
        acc = q @ wv.T
        out = acc * xs[:, None] * ws[None, :]
        if self.gateup:
            gt, up = out[:, :N], out[:, N:]
            if mut.get("up_scale_from_gate"):
                up = acc[:, N:] * xs[:, None] * ws[None, :N]
            if mut.get("gate_up_exchanged"):
                gt, up = up, gt
            out = silu(gt) * up
        if self.res is not None and not mut.get("res_missing"):
            out = out + self.res.to(dtype).roll(mut.get("res_roll", 0), 0)
        if mut.get("out_roll"):
            out = out.roll(1, -1)
        if mut.get("col_missing"):
            out = out.clone()
            out[M - 1] = 0
        if mut.get("clamp_m") and M >= 2:    # gemm: tile tail from the clamped row
            out = out.clone()
            out[M - 1] = out[M - 2]
        return out

    @functools.cached_property
    def ref(self) -> torch.Tensor:
        out = self._core(torch.float64)
        self._amb_share = 0.0 if self._amb is None else float(self._amb.double().mean())
        return out

    @property
    def ambiguous_share(self) -> float:
        self.ref
        return self._amb_share

    @functools.cached_property
    def noise(self) -> float:
        return row_rel_err(self._core(torch.float32).to(torch.bfloat16), self.ref)

    @functools.cached_property
    def noise_q(self) -> float:
        if self.quant != "norm":
            return 0.0
        return row_rel_err(self._core(torch.float64, flip=True), self.ref)

    @property
    def tol(self) -> float:
        return TOL_FACTOR * (self.noise + self.noise_q)

    def mutant_err(self, knobs: dict) -> float:
        return row_rel_err(self._core(torch.float64, **knobs), self.ref)

    # ---- which wrong kernels apply to this case --------------------------
    def mutants(self) -> List[Tuple[str, dict]]:
        M, N, K = self.M, self.N, self.K
        m: List[Tuple[str, dict]] = []
        for k in self.probes:
            m.append((f"probe{k}_dropped", {"drop_k": [k]}))
            m.append((f"probe{k}_twice", {"twice_k": [k]}))
        m.append(("wscale_ignored", {"wscale_ignored": True}))
        if self.wscale.numel() >= 2:
            m += [("wscale_row+1", {"wscale_shift": -1}), ("wscale_row-1", {"wscale_shift": 1})]
        if N >= 2:
            m += [("out_rows_rolled", {"out_roll": True}), ("last_row_clamped", {"clamp_row": True})]
        if M >= 2:
            m += [("x_rows_rolled", {"x_roll": True}), ("col_M-1_missing", {"col_missing": True})]
            if self.quant != "none":
                m += [("xscale_m+1", {"xscale_shift": -1}), ("xscale_m-1", {"xscale_shift": 1})]
        if self.gateup:
            # SiLU applied to up is the same wrong answer as gate and up exchanged
            m += [("gate_up_exchanged", {"gate_up_exchanged": True}),
                  ("up_scale_from_gate", {"up_scale_from_gate": True})]
        if self.mode & 1:
            m.append(("normw_shifted_word", {"normw_shift": True}))
            if M >= 2:
                m.append(("rstd_other_row", {"rstd_roll": True}))
        if self.mode & 2:
            m.append(("res_missing", {"res_missing": True}))
            if M >= 2:
                m += [("res_m+1", {"res_roll": -1}), ("res_m-1", {"res_roll": 1})]
        if self.kind == "valu" and K % 1024:
            m.append(("last_partial_pass_dropped", {"drop_range": (K - K % 1024, K)}))
        if self.kind == "mfma":
            q4 = K // 4
            for w in range(4):
                m.append((f"wave{w}_quarter_dropped", {"drop_range": (w * q4, (w + 1) * q4)}))
                m.append((f"wave{w}_quarter_twice", {"twice_range": (w * q4, (w + 1) * q4)}))
            m.append(("ring_step_dropped", {"drop_range": (q4, q4 + 128)}))
            m.append(("slice_from_next_lane_group", {"slice_swap": (0, 32, 32)}))
        if self.kind == "gemm":
            m.append(("k_step_dropped", {"drop_range": (K - 128, K)}))
            if M * N > 1:
                m.append(("ascale_bscale_exchanged", {"scales_exchanged": True}))
            if K >= 256:
                m.append(("ring_buffers_exchanged", {"ring_stale": True}))
            if M >= 2:
                m += [("a_swizzle_only", {"a_swizzle": True}), ("tail_row_clamped", {"clamp_m": True})]
        return m


@functools.lru_cache(maxsize=None)
def lin_case(kind: str, M: int, N: int, K: int, mode: int = 0, gateup: bool = False) -> LinCase:
    return LinCase(kind, M, N, K, mode, gateup)


VALU_OFF = {"OPSAGENT_FP8_GEMV_MFMA": "0"}
XS_ON = {**VALU_OFF, "OPSAGENT_FP8_GEMV_XS": "1"}
RW1 = {**VALU_OFF, "OPSAGENT_FP8_GEMV_RW": "1"}

# every GPU run: (case key, environment). The key is lin_case's argument tuple.
VALU_RUNS = (
    [(("valu", M, 9, 1040, mode, False), VALU_OFF)
     for M in (1, 2, 3, 4, 5, 6, 7, 8, 12, 16) for mode in (0, 1, 2, 3)]
    + [(("valu", M, N, K, mode, False), VALU_OFF)
       for M in (1, 2) for N, K in ((1, 16), (2, 16), (7, 2048), (32777, 16)) for mode in (0, 1, 2, 3)]
    + [(("valu", 1, 9, 1040, mode, False), RW1) for mode in (0, 1, 2, 3)]
    + [(("valu", M, 9, 1040, mode, False), XS_ON) for M in (1, 2) for mode in (0, 1, 2, 3)]
)
VALU_GU_RUNS = (
    [(("valu", M, 5, 1040, norm, True), VALU_OFF) for M in (1, 2, 3, 4, 6, 8) for norm in (0, 1)]
    + [(("valu", M, I, 16, norm, True), VALU_OFF)
       for M in (1, 2) for I in (1, 32777) for norm in (0, 1)]
    + [(("valu", M, 5, 1040, norm, True), XS_ON) for M in (1, 2) for norm in (0, 1)]
)
MFMA_SHAPES = [(2, 16, 4096), (3, 17, 4096), (9, 33, 4096), (15, 1, 4096), (1, 17, 4096),
               (16, 40, 8192), (4, 17, 32768)]
MFMA_RUNS = [(("mfma", M, N, K, mode, False), {"OPSAGENT_FP8_GEMV_MFMA": "2"} if M == 1 else {})
             for M, N, K in MFMA_SHAPES for mode in (0, 1, 2, 3)]
MFMA_GU_SHAPES = [(2, 17, 2048), (5, 16, 2048), (7, 1, 6144), (16, 33, 8192)]
MFMA_GU_RUNS = [(("mfma", M, I, K, norm, True), {})
                for M, I, K in MFMA_GU_SHAPES for norm in (0, 1)]
GEMM_SHAPES = [(1, 1, 128), (128, 128, 128), (129, 136, 256), (200, 72, 384)]
GEMM_RUNS = (
    [(("gemm", M, N, K, 0, False), env) for M, N, K in GEMM_SHAPES
     for env in ({"OPSAGENT_FP8_STAGE": "glds"}, {"OPSAGENT_FP8_STAGE": "reg"}, {})]
    + [(("gemm", 130, 257, 16512, 0, False), {})]
)
LIN_RUNS = VALU_RUNS + VALU_GU_RUNS + MFMA_RUNS + MFMA_GU_RUNS + GEMM_RUNS


def lin_keys() -> List[tuple]:
    """The distinct cases behind LIN_RUNS, in order."""
    seen: Dict[tuple, None] = {}
    for key, _ in LIN_RUNS:
        seen.setdefault(key)
    return list(seen)


def run_id(run) -> str:
    key, env = run
    kind, M, N, K, mode, gu = key
    tag = "".join(f"-{k.rsplit('_', 1)[-1]}{v}" for k, v in sorted(env.items()))
    return f"{kind}{'_gu' if gu else ''}-m{M}-n{N}-k{K}-mode{mode}{tag}"


def uses_mfma(M: int, K: int, gateup: bool, env: dict) -> bool:
    """gemv_fp8_use_mfma of fp8_moe.hip, for the reader and the CPU test."""
    e = env.get("OPSAGENT_FP8_GEMV_MFMA", "")
    if e[:1] == "0":
        return False
    if K % 512 or (K // 512) % (4 if gateup else 8) or K > 32768 or M > 16:
        return False
    if M < 2 and e[:1] != "2":
        return False
    return M * K <= 128 * 1024


# --------------------------------------------------------------------------
# grouped MoE
# --------------------------------------------------------------------------
EMAJ_GROUP = 8


def _moe_stage(kind: str, xin, wv, ws, eids, tids, pw, rows: int, dtype, **mut) -> torch.Tensor:
    """gateup: act[p] = silu(x[tok] @ gate_e^T) * (x[tok] @ up_e^T), wv [E, 2*rows, K];
    down: y[p] = (act[p] @ w2_e^T) * pw[p], wv [E, rows, K]. ws: per (expert, row)."""
    E, R, K = wv.shape
    P = eids.numel()
    gate = kind == "gateup"
    e = eids.long()
    src = tids.long() if gate else torch.arange(P)
    if mut.get("tids_ignored"):
        src = torch.arange(P) % xin.shape[0]
    lists = [[p for p in range(P) if int(e[p]) == ex] for ex in range(E)]
    if mut.get("ninth_as_first"):
        src = src.clone()
        for lst in lists:
            if len(lst) > EMAJ_GROUP:
                src[lst[EMAJ_GROUP]] = src[lst[0]]
    xp = xin.to(dtype)[src]
    wsd = ws.to(dtype)
    if "wscale_shift" in mut:
        wsd = wsd.reshape(-1).roll(mut["wscale_shift"]).reshape(E, R)
    if mut.get("wscale_ignored"):
        wsd = torch.ones_like(wsd)
    wvd = wv.to(dtype)
    xp, wvd = _k_mutations(xp, wvd, mut)
    if mut.get("clamp_row") and rows >= 2:
        wvd, wsd = wvd.clone(), wsd.clone()
        for base in ((0, rows) if gate else (0,)):
            wvd[:, base + rows - 1] = wvd[:, base + rows - 2]
            wsd[:, base + rows - 1] = wsd[:, base + rows - 2]
    ew = (e + mut.get("wexpert_shift", 0)) % E
    es = (e + mut.get("sexpert_shift", 0)) % E
    acc = torch.einsum("pk,prk->pr", xp, wvd[ew])
    out = acc * wsd[es]
    if gate:
        gt, up = out[:, :rows], out[:, rows:]
        if mut.get("up_scale_from_gate"):
            up = acc[:, rows:] * wsd[es][:, :rows]
        if mut.get("gate_up_exchanged"):
            gt, up = up, gt
        out = silu(gt) * up
    elif not mut.get("pw_missing"):
        out = out * pw.to(dtype).roll(mut.get("pw_shift", 0))[:, None]
    if mut.get("out_roll"):
        out = out.roll(1, -1)
    if mut.get("group_last_dropped") or mut.get("partial_slots_over_first"):
        out = out.clone()
        for lst in lists:
            for g0 in range(0, len(lst), EMAJ_GROUP):
                grp = lst[g0:g0 + EMAJ_GROUP]
                if mut.get("group_last_dropped"):
                    out[grp[-1]] = 0
                elif len(grp) < EMAJ_GROUP:     # idle slots store zeros to plist[g0]
                    out[grp[0]] = 0
    return out


class MoeCase:
    """One grouped-MoE launch. kind gateup | down | mlp; family pair | emaj."""

    def __init__(self, kind: str, family: str, fp8: bool, rows: int, K: int, big: bool = False):
        self.kind, self.family, self.fp8, self.rows, self.K = kind, family, fp8, rows, K
        self.name = f"moe_{kind}_{family}_{'fp8' if fp8 else 'bf16'}_r{rows}_k{K}{'_p2048' if big else ''}"
        g = _gen(self.name)
        if family == "pair" and kind != "mlp":
            self.E, self.T = 3, 4
            tids, eids = [3, 0, 0, 2, 1, 3], [2, 0, 2, 1, 0, 2]
            pw = [0.75, 0.0, -0.5, 1.25, 0.375, 0.875]
        elif big:
            self.E, self.T = 2, 7
            eids = [1] * 2048
            tids = torch.randint(0, 7, (2048,), generator=g).tolist()
            pw = (torch.rand(2048, generator=g) - 0.3).tolist()
        else:
            self.E, self.T = 5, 7
            counts = [0, 1, 8, 9, 17]
            eids = [ex for ex, c in enumerate(counts) for _ in range(c)]
            eids = [eids[i] for i in torch.randperm(len(eids), generator=g).tolist()]
            tids = torch.randint(0, 7, (len(eids),), generator=g).tolist()
            pw = (torch.rand(len(eids), generator=g) - 0.3).tolist()
            pw[3], pw[11] = 0.0, -0.625
        # the ninth pair of an expert must not share its token with the first
        for ex in range(self.E):
            lst = [p for p, v in enumerate(eids) if v == ex]
            if len(lst) > EMAJ_GROUP and tids[lst[EMAJ_GROUP]] == tids[lst[0]]:
                tids[lst[EMAJ_GROUP]] = (tids[lst[0]] + 1) % self.T
        self.P = len(eids)
        self.eids = torch.tensor(eids, dtype=torch.int32)
        self.tids = torch.tensor(tids, dtype=torch.int32)
        self.pw = torch.tensor(pw, dtype=torch.float32)
        E, P = self.E, self.P
        self.I = rows
        self.H = rows if kind != "mlp" else 9
        self.probes = probe_ks("moe", K, bf16w=not fp8)
        n_in = P if kind == "down" else self.T
        # gate-up: silu's argument near its knee
        fac = 1.0 if kind == "down" else (2.0 ** -4 if fp8 else 2.0 ** -6)
        self.x = soft_x(n_in, K, self.probes, g, big=12.0, factor=fac)
        self._pin = rows
        r1 = rows if kind == "down" else 2 * rows
        self.w1, self.w1_scale, self.w1v = self._weights(E, r1, K, self.probes, g)
        if kind == "mlp":
            p2 = probe_ks("moe", rows, bf16w=not fp8)
            self.w2, self.w2_scale, self.w2v = self._weights(E, self.H, rows, p2, g)

    def _weights(self, E, R, K, probes, g):
        """(device form, scales or None, exact values fp32)."""
        if self.fp8:
            codes = weight_codes(E * R, K, probes, g).view(E, R, K)
            scale = pin_last_rows(weight_scales((E, R), g), self._pin if R % self._pin == 0 else R)
            return codes, scale, E4M3[codes.long()].float()
        w = torch.randn(E, R, K, generator=g) * 0.3 + 0.02
        if probes:
            w[:, :, probes] = (3.0 + torch.rand(E, R, len(probes), generator=g)) * (
                torch.randint(0, 2, (E, R, len(probes)), generator=g).float() * 2 - 1)
        # bf16 weights carry no scales: rows of different magnitude instead
        mag = torch.exp2(torch.randint(-3, 4, (E, R), generator=g).float())
        pin = self._pin if R % self._pin == 0 else R
        if pin >= 2:
            for base in range(0, R, pin):
                mag[:, base + pin - 1] = mag[:, base + pin - 2] = 8.0
        w *= mag[:, :, None]
        w = w.to(torch.bfloat16)
        return w, None, w.float()

    def _ones(self, wv):
        return torch.ones(wv.shape[:2])

    def _core(self, dtype, **mut) -> torch.Tensor:
        s1 = self.w1_scale if self.fp8 else self._ones(self.w1v)
        if self.kind != "mlp":
            return _moe_stage(self.kind, self.x, self.w1v, s1, self.eids, self.tids, self.pw,
                              self.rows, dtype, **mut)
        m1 = {k[3:]: v for k, v in mut.items() if k.startswith("s1_")}
        m2 = {k[3:]: v for k, v in mut.items() if k.startswith("s2_")}
        act = _moe_stage("gateup", self.x, self.w1v, s1, self.eids, self.tids, self.pw,
                         self.I, dtype, **m1)
        if dtype != torch.float64:
            act = act.to(torch.bfloat16).to(dtype)
        s2 = self.w2_scale if self.fp8 else self._ones(self.w2v)
        return _moe_stage("down", act, self.w2v, s2, self.eids, self.tids, self.pw,
                          self.H, dtype, **m2)

    @functools.cached_property
    def ref(self) -> torch.Tensor:
        return self._core(torch.float64)

    @functools.cached_property
    def noise(self) -> float:
        return row_rel_err(self._core(torch.float32).to(torch.bfloat16), self.ref)

    @property
    def tol(self) -> float:
        return TOL_FACTOR * self.noise

    def mutant_err(self, knobs: dict) -> float:
        return row_rel_err(self._core(torch.float64, **knobs), self.ref)

    def mutants(self) -> List[Tuple[str, dict]]:
        if self.kind == "mlp":
            return [("gateup_expert+1", {"s1_wexpert_shift": 1}), ("down_expert+1", {"s2_wexpert_shift": 1}),
                    ("token_ids_ignored", {"s1_tids_ignored": True}),
                    ("pair_w_missing", {"s2_pw_missing": True}), ("pair_w_p+1", {"s2_pw_shift": -1})]
        K, rows = self.K, self.rows
        m: List[Tuple[str, dict]] = []
        for k in self.probes:
            m.append((f"probe{k}_dropped", {"drop_k": [k]}))
            m.append((f"probe{k}_twice", {"twice_k": [k]}))
        wave_pass = 1024 if self.fp8 else 512
        if K % wave_pass:
            m.append(("last_partial_pass_dropped", {"drop_range": (K - K % wave_pass, K)}))
        if rows >= 2:
            m += [("out_rows_rolled", {"out_roll": True}), ("last_row_clamped", {"clamp_row": True})]
        if self.fp8:
            m += [("wscale_row+1", {"wscale_shift": -1}), ("wscale_row-1", {"wscale_shift": 1}),
                  ("wscale_ignored", {"wscale_ignored": True}),
                  ("scales_expert+1", {"sexpert_shift": 1}), ("scales_expert-1", {"sexpert_shift": -1})]
        if self.E >= 2:
            m += [("weights_expert+1", {"wexpert_shift": 1}), ("weights_expert-1", {"wexpert_shift": -1})]
        if self.kind == "gateup":
            m += [("token_ids_ignored", {"tids_ignored": True}),
                  ("gate_up_exchanged", {"gate_up_exchanged": True})]
            if self.fp8:
                m.append(("up_scale_from_gate", {"up_scale_from_gate": True}))
        else:
            m += [("pair_w_p+1", {"pw_shift": -1}), ("pair_w_p-1", {"pw_shift": 1}),
                  ("pair_w_missing", {"pw_missing": True})]
        if self.family == "emaj":
            m += [("group_last_pair_dropped", {"group_last_dropped": True}),
                  ("ninth_pair_as_first", {"ninth_as_first": True})]
            counts = torch.bincount(self.eids.long())
            if (counts % EMAJ_GROUP != 0).any():
                m.append(("idle_slots_written_over_first", {"partial_slots_over_first": True}))
        return m


@functools.lru_cache(maxsize=None)
def moe_case(kind: str, family: str, fp8: bool, rows: int, K: int, big: bool = False) -> MoeCase:
    return MoeCase(kind, family, fp8, rows, K, big)


def _moe_keys() -> List[tuple]:
    keys = []
    for fp8 in (False, True):
        ktail = 1040 if fp8 else 528
        for kind in ("gateup", "down"):
            for rows, K in ((5, 16), (9, ktail), (2052, 16)):
                keys.append((kind, "pair", fp8, rows, K, False))
            for rows, K in ((5, 16), (9, 1040), (260, 16)):
                keys.append((kind, "emaj", fp8, rows, K, False))
            keys.append((kind, "emaj", fp8, 4, 16, True))
        for family in ("pair", "emaj"):
            keys.append(("mlp", family, fp8, 48, ktail, False))
    return keys


MOE_KEYS = _moe_keys()


def moe_id(key) -> str:
    kind, family, fp8, rows, K, big = key
    return f"{kind}-{family}-{'fp8' if fp8 else 'bf16'}-r{rows}-k{K}{'-p2048' if big else ''}"


# --------------------------------------------------------------------------
# families of the report (docs/KERNELS.md)
# --------------------------------------------------------------------------
def lin_family(c: "LinCase") -> str:
    if c.kind == "gemm":
        return "gemm_fp8"
    if c.kind == "valu":
        return "VALU gate-up" if c.gateup else "VALU GEMV"
    if c.gateup:
        return "MFMA GEMV, gate-up"
    return "MFMA GEMV, norm" if c.mode & 1 else "MFMA GEMV, plain"


def moe_family(c: "MoeCase") -> str:
    fam = "pair-major" if c.family == "pair" else "expert-major"
    return f"MoE {fam}, {'fp8' if c.fp8 else 'bf16'}"


# --------------------------------------------------------------------------
# shared by the GPU files
# --------------------------------------------------------------------------
PAD = 64  # guard elements on either side of an output


class Guarded:
    """A [rows, cols] tensor inside a larger buffer filled with a sentinel."""

    def __init__(self, rows, cols, dtype, fill, device, pad=PAD):
        self.n, self.pad = rows * cols, pad
        self.buf = torch.full((self.n + 2 * pad,), fill, dtype=dtype, device=device)
        self.before = self._bits().clone()
        self.t = self.buf[pad:pad + self.n].view(rows, cols)

    def _bits(self):
        ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[self.buf.element_size()]
        return self.buf.view(ints).cpu()

    def assert_outside_untouched(self, msg):
        now = self._bits()
        lo, hi = self.pad, self.pad + self.n
        assert torch.equal(now[:lo], self.before[:lo]), f"{msg}: wrote before the output"
        assert torch.equal(now[hi:], self.before[hi:]), f"{msg}: wrote past the output"


def set_env(monkeypatch, env):
    """Every knob of these kernels unset, then `env`; the C side reads them
    with getenv on every call."""
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
