"""Exact-operand cases, fp64 oracles and wrong-kernel mutants for the bf16
dense GEMV family (gemv.hip with gemv_pipe.h / gemv_tile.h: gemv_kernel,
gemv_gateup_kernel and gemv_bf16_mfma_kernel). CPU only, no pytest dependency;
shared by tests/test_dense_oracle.py (CPU proof that every mutant is visible)
and the GPU file tests/test_dense_bf16_gpu.py.

Method (the one of tests/linear_cases.py and tests/attention_oracle.py):

  * bf16 operands are exact as they stand, so the oracle is fp64 on x, W, the
    norm weight and the residual themselves: x * rsqrt(mean(x^2) + eps) * wn
    unrounded, silu(g) * u for gate-up, residual added.
  * W rows carry a magnitude class 2^randint(-3..3), the last two rows of each
    half pinned to the largest: a row taken from a neighbour, from `gate` for
    `up`, or from the clamped row is visibly wrong.
  * x rows are `soft_x` rows times a further power of two, so that cyclic
    neighbours differ in rms by >= 2x (asserted): rstd of row m+-1 is wrong.
  * a sum of probe products of random sign can cancel; a wrong last row, or
    the one row of an N = 1 case, would then move little. So x probes have
    one sign pattern in every batch row, and the last row of each half has
    some of its probe products aligned with it (`dense_weight`).
  * emulation = the same in fp32 with the output rounded to bf16. The VALU
    kernels keep x * rstd * wn in fp32; the MFMA kernel rounds it to bf16 when
    it stages x into LDS, and so does its emulation. Nothing else rounds.
    N = row_rel_err(emulation, oracle), T = 4 N, per case.
  * PROBES sit where each kernel's own K partition changes hands (`valu_probes`
    from the piece walk of gemv_tile.h, `mfma_probes` from the quarter / ring /
    step geometry of gemv_bf16_mfma_kernel): x, every W row and wn are large
    there, so a lost or doubled element moves the whole row.
  * mutants are keyword knobs of the core, listed by `case.mutants()`.

One mutant is a stand-in: gemv_kernel points the dead row of an odd N's last
pair at the live row, so the dead accumulator equals the live one and storing
it over the live row would not show. `dead_row_over_live` models the dead row
as what a predicated-off load chain leaves (zeros) stored over the live one.
"""

from __future__ import annotations

import collections
import functools
import math
from typing import List, Tuple

import torch

import linear_cases as lc
from linear_cases import EPS, Guarded, _gen, _k_mutations, norm_weight, silu, soft_x  # noqa: F401
from attention_oracle import MUTANT_FACTOR, TOL_FACTOR, row_rel_err  # noqa: F401

UNIT_ROW = 512            # bf16 elements of one unit-row (64 lanes x 16 B)
ENV_KNOBS = ("OPSAGENT_BF16_GEMV_MFMA", "OPSAGENT_BF16_PRENORM", "OPSAGENT_GEMV_MAX_M")
MFMA_M2 = {"OPSAGENT_BF16_GEMV_MFMA": "m2"}

# GEMV_KU_* of gemv.hip (the same at M = 1 and M = 2); test_dense_oracle.py
# reads the source and asserts this table against it
SHIPPED_KU = {"RW1": 8, "RW1_NORM": 2, "RW2": 1, "RW2_NORM": 1, "GATEUP": 1}


# --------------------------------------------------------------------------
# where each kernel's K partition changes hands
# --------------------------------------------------------------------------
def piece_walk(K: int, ku: int) -> List[Tuple[int, int]]:
    """(first unit-row, depth) of every unpredicated piece: gemv_piece_depth
    of gemv_tile.h walked as gemv_row_pieces does."""
    whole, r, out = K // UNIT_ROW, 0, []
    while True:
        left = whole - r
        d = ku if left >= ku else 4 if left >= 4 else 2 if left >= 2 else 1 if left >= 1 else 0
        if d == 0:
            return out
        out.append((r, d))
        r += d


def valu_probes(K: int) -> List[int]:
    ks = set(lc.probe_ks("valu", K, bf16w=True))     # 0, K-1, 7/8, 15/16, 511/512, K - K % 512
    for ku in (1, 2, 4, 8):
        for r, d in piece_walk(K, ku):
            ks |= {r * UNIT_ROW - 1, r * UNIT_ROW, (r + d) * UNIT_ROW - 1, (r + d) * UNIT_ROW}
    if K % UNIT_ROW:
        ks |= {K - K % UNIT_ROW, K - 8}              # partial unit-row: first element, last live lane's unit
    return sorted(k for k in ks if 0 <= k < K)


def mfma_probes(K: int, gateup: bool) -> List[int]:
    q, pf = K // 4, 4 if gateup else 8
    ks = {0, K - 1, 7, 8, 31, 32}
    for w in range(4):
        ks |= {w * q - 1, w * q}
        ks |= {(w + 1) * q - 32, (w + 1) * q - 1}    # the quarter's last step (the kb + 1 < nk path ends)
        if q > 32 * pf:
            ks |= {w * q + 32 * pf - 1, w * q + 32 * pf}
    return sorted(k for k in ks if 0 <= k < K)


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
def aligned_probes(n: int) -> List[int]:
    """Indices (into the probe list) of the A = min(n, ceil(2 sqrt n)) probes
    whose products all have one sign in a pinned row, evenly spread."""
    A = min(n, math.ceil(2 * math.sqrt(n)))
    return sorted({round(i * (n - 1) / max(A - 1, 1)) for i in range(A)})


def dense_weight(rows: int, halves: int, K: int, probes: List[int], xsign: torch.Tensor,
                 g: torch.Generator, must: List[int] = ()) -> torch.Tensor:
    """bf16 [halves * rows, K]: randn background, |w| in [3, 4) at the probe
    columns, a magnitude class per row, the last two rows of each half 8x.

    A sum of n probe products of random sign can cancel, and then a wrong last
    row (clamped, or a dead row stored over it) or the one row of an N = 1
    case moves little against the row maximum. So in the last row of a half
    the products of A probes (`aligned_probes`) with x (whose probes have the
    sign pattern `xsign` in every batch row) are all positive (all negative in
    the up half: silu(g) * u then differs from silu(u) * g in the relu tails
    too), the other probes alternate, and the row before it repeats it with
    ONE aligned sign turned: read one row early, the last row is wrong by
    twice a probe product with nothing to cancel against. A < n keeps one
    probe at >= 1/A of the row maximum. `must`: probe indices aligned as well
    (the partial unit-row's, which one mutant drops together)."""
    R = rows * halves
    w = torch.randn(R, K, generator=g) * 0.3 + 0.02
    n = len(probes)
    w[:, probes] = (3.0 + torch.rand(R, n, generator=g)) * (
        torch.randint(0, 2, (R, n), generator=g).float() * 2 - 1)
    mag = torch.exp2(torch.randint(-3, 4, (R,), generator=g).float())
    al = sorted(set(aligned_probes(n)) | set(must))
    pattern = torch.ones(n)
    rest = [i for i in range(n) if i not in al]
    pattern[rest] = torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(len(rest))])
    for h, base in enumerate(range(0, R, rows)):
        last = base + rows - 1
        mag[max(base, last - 1):last + 1] = 8.0
        w[last, probes] = w[last, probes].abs() * pattern * xsign * (1.0 if h == 0 else -1.0)
        if rows >= 2:
            w[last - 1, probes] = w[last, probes]
            w[last - 1, probes[al[len(al) // 2]]] *= -1
    return (w * mag[:, None]).to(torch.bfloat16)


def knee_factor(K: int, n: int, norm: bool) -> float:
    """Power of two that puts the aligned gate sum of a middle batch row at
    3..6, silu's knee: |x| ~ 30 at a probe (sqrt(K / n) after the norm, times
    wn = 2), |w| ~ 3.5 * 8."""
    A = len(aligned_probes(n))
    est = A * 28.0 * (2.0 * math.sqrt(K / n) if norm else 30.0)
    return 2.0 ** -math.floor(math.log2(est / 3.0))


def row_exponents(M: int) -> torch.Tensor:
    """Further power of two per batch row on top of soft_x's 2^(m % 3 - 1):
    rows then sit at 2^(2 (m % 3 - 1)), and a last row that would wrap onto
    row 0's class drops to 2^-5."""
    e = torch.tensor([(m % 3) - 1.0 for m in range(M)])
    if M > 1 and M % 3 == 1:
        e[M - 1] = -4.0
    return e


def rms_separation(x: torch.Tensor) -> float:
    """Smallest rms ratio between cyclic neighbours of the batch."""
    rms = x.double().pow(2).mean(-1).sqrt()
    r = rms / rms.roll(-1)
    return float(torch.maximum(r, 1 / r).min())


class DenseCase:
    """One GEMV case. kind: valu | mfma (which kernel's partition the probes
    follow and which roundings the emulation has); gateup: N is I and the
    weight is [2I, K]; mode bit 0 = fused rmsnorm, bit 1 = residual."""

    def __init__(self, kind: str, M: int, N: int, K: int, mode: int = 0, gateup: bool = False):
        assert kind in ("valu", "mfma") and K % 8 == 0 and not (gateup and mode & 2)
        self.kind, self.M, self.N, self.K, self.mode, self.gateup = kind, M, N, K, mode, gateup
        self.name = f"dense_{kind}{'_gu' if gateup else ''}_m{M}_n{N}_k{K}_mode{mode}"
        g = _gen(self.name)
        self.probes = mfma_probes(K, gateup) if kind == "mfma" else valu_probes(K)
        # gate-up: keep silu's argument near its knee, not in its relu tails
        knee = knee_factor(K, len(self.probes), bool(mode & 1)) if gateup else 1.0
        self.wn = norm_weight(K, self.probes, g, knee) if mode & 1 else None
        x = soft_x(M, K, self.probes, g, factor=1.0 if mode & 1 else knee).float()
        xsign = torch.sign(x[0, self.probes])            # one sign pattern for every batch row
        x[:, self.probes] = x[:, self.probes].abs() * xsign
        # odd batch rows keep every other probe at 1/8: with one sign pattern
        # a pinned row's sum sees only sum|x_p| / rms, so without this two
        # rows are alike after the norm and rolled rows would not show
        shape = torch.ones(M, len(self.probes))
        shape[1::2, 1::2] = 0.125
        x[:, self.probes] *= shape
        scaled = x * torch.exp2(row_exponents(M))[:, None]
        self.x = scaled.to(torch.bfloat16)
        assert torch.equal(self.x.float(), scaled), "row scaling is exact"
        must = [i for i, k in enumerate(self.probes)
                if kind == "valu" and K % UNIT_ROW and k >= K - K % UNIT_ROW]
        self.w = dense_weight(N, 2 if gateup else 1, K, self.probes, xsign, g, must)
        self.rms_sep = rms_separation(self.x) if M >= 2 else float("inf")
        assert self.rms_sep >= 2.0, f"{self.name}: neighbouring rows' rms within {self.rms_sep:.2f}x"
        self.res = None
        if mode & 2:
            plain = self._core(torch.float64)
            self.res = (torch.randn(M, N, generator=g).double() * 0.3
                        * plain.abs().amax(-1, keepdim=True)).to(torch.bfloat16)

    # ---- the computation, with mutant knobs ------------------------------
    def _core(self, dtype, **mut) -> torch.Tensor:
        M, N, K = self.M, self.N, self.K
        emul = dtype != torch.float64
        wv = self.w.to(dtype)
        xv = self.x.to(dtype)
        if mut.get("x_roll"):
            xv = xv.roll(1, 0)
        if self.mode & 1:
            rstd = torch.rsqrt(xv.pow(2).mean(-1) + EPS)
            gw = self.wn.to(dtype)
            if "rstd_shift" in mut:
                rstd = rstd.roll(mut["rstd_shift"])
            if mut.get("normw_shift"):
                gw = gw.roll(2)
            if self.kind == "mfma":
                q = xv * rstd[:, None] * gw
                if emul:                         # rounded when staged into LDS
                    q = q.to(torch.bfloat16).to(dtype)
            else:
                q = xv * (rstd[:, None] * gw)
        else:
            q = xv
        if mut.get("pitch_2k") and M >= 2:       # row m read 16 m bytes early
            img = torch.zeros(M, K + 8, dtype=dtype)
            img[:, :K] = q
            q = img.reshape(-1)[:M * K].reshape(M, K).clone()
        if mut.get("stale_last_step"):           # bnext never handed over
            q0, q = q, q.clone()
            for w in range(4):
                e = (w + 1) * (K // 4)
                q[:, e - 32:e] = q0[:, e - 64:e - 32]
        q, wv = _k_mutations(q, wv, mut)
        if mut.get("clamp_row") and N >= 2:      # last W row read one row early
            wv = wv.clone()
            for base in ((0, N) if self.gateup else (0,)):
                wv[base + N - 1] = wv[base + N - 2]
        acc = q @ wv.T
        if mut.get("dead_lane"):                 # first dead lane: the next rows' first unit
            acc = acc + q.roll(-1, 0)[:, :8] @ wv.roll(-1, 0)[:, :8].T
        if self.gateup:
            gt, up = acc[:, :N], acc[:, N:]
            if mut.get("up_row_minus_1"):
                up = acc[:, N - 1:2 * N - 1]
            if mut.get("gate_up_exchanged"):
                gt, up = up, gt
            out = silu(gt) * up
        else:
            out = acc
        res = self.res
        if res is not None and not mut.get("res_missing"):
            out = out + res.to(dtype).roll(mut.get("res_roll", 0), 0)
        if mut.get("out_roll"):
            out = out.roll(1, -1)
        if mut.get("pair_swap"):                 # rows 2i and 2i + 1 exchanged
            out = out.clone()
            even = torch.arange(0, N - 1, 2)
            out[:, even], out[:, even + 1] = out[:, even + 1].clone(), out[:, even].clone()
        if mut.get("dead_row_over_live"):
            out = out.clone()
            out[:, N - 1] = 0 if res is None else res.to(dtype)[:, N - 1]
        if mut.get("col_missing"):
            out = out.clone()
            out[M - 1] = 0
        return out

    @functools.cached_property
    def ref(self) -> torch.Tensor:
        return self._core(torch.float64)

    def emulation(self, **knobs) -> torch.Tensor:
        return self._core(torch.float32, **knobs).to(torch.bfloat16)

    @functools.cached_property
    def noise(self) -> float:
        return row_rel_err(self.emulation(), self.ref)

    @property
    def tol(self) -> float:
        return TOL_FACTOR * self.noise

    def mutant_ref(self, knobs: dict) -> torch.Tensor:
        return self._core(torch.float64, **knobs)

    def mutant_tol(self, knobs: dict) -> float:
        """T of the wrong kernel's own answer."""
        return TOL_FACTOR * row_rel_err(self.emulation(**knobs), self.mutant_ref(knobs))

    def mutant_err(self, knobs: dict) -> float:
        return row_rel_err(self.mutant_ref(knobs), self.ref)

    # ---- which wrong kernels apply to this case --------------------------
    def mutants(self) -> List[Tuple[str, dict]]:
        M, N, K = self.M, self.N, self.K
        m: List[Tuple[str, dict]] = []
        for k in self.probes:
            m.append((f"probe{k}_dropped", {"drop_k": [k]}))
            m.append((f"probe{k}_twice", {"twice_k": [k]}))
        if self.kind == "valu":
            if K % UNIT_ROW:
                m.append(("partial_unit_row_dropped", {"drop_range": (K - K % UNIT_ROW, K)}))
                m.append(("dead_lane_feeds_next_row", {"dead_lane": True}))
            last = {piece_walk(K, ku)[-1] for ku in (1, 2, 4, 8) if K >= UNIT_ROW}
            for r, d in sorted(last):
                m.append((f"last_piece_dropped_r{r}_d{d}",
                          {"drop_range": (r * UNIT_ROW, (r + d) * UNIT_ROW)}))
        else:
            q4, pf = K // 4, 4 if self.gateup else 8
            for w in range(4):
                m.append((f"wave{w}_quarter_dropped", {"drop_range": (w * q4, (w + 1) * q4)}))
                m.append((f"wave{w}_quarter_twice", {"twice_range": (w * q4, (w + 1) * q4)}))
            step = q4 + (32 * pf if q4 > 32 * pf else 0)     # wave 1: the refill's first step
            m.append(("ring_step_dropped", {"drop_range": (step, step + 32)}))
            m.append(("last_step_stale_x_fragment", {"stale_last_step": True}))
            m.append(("slice_from_next_lane_group", {"slice_swap": (0, 8, 8)}))
            if M >= 2:
                m.append(("x_row_at_m_2K_not_pitch", {"pitch_2k": True}))
        if N >= 2:
            m += [("out_rows_rolled", {"out_roll": True}), ("last_row_clamped", {"clamp_row": True})]
            if self.kind == "valu" and not self.gateup:
                m.append(("pair_rows_exchanged", {"pair_swap": True}))
        if self.kind == "valu" and not self.gateup and N % 2:
            m.append(("dead_row_over_live", {"dead_row_over_live": True}))
        if M >= 2:
            m += [("x_rows_rolled", {"x_roll": True}), ("col_M-1_missing", {"col_missing": True})]
        if self.mode & 1:
            m.append(("normw_shifted_word", {"normw_shift": True}))
            if M >= 2:
                m += [("rstd_m+1", {"rstd_shift": -1}), ("rstd_m-1", {"rstd_shift": 1})]
        if self.mode & 2:
            m.append(("res_missing", {"res_missing": True}))
            if M >= 2:
                m += [("res_m+1", {"res_roll": -1}), ("res_m-1", {"res_roll": 1})]
        if self.gateup:
            m += [("gate_up_exchanged", {"gate_up_exchanged": True}),
                  ("up_from_row_r+I-1", {"up_row_minus_1": True})]
        return m


@functools.lru_cache(maxsize=None)
def dense_case(kind: str, M: int, N: int, K: int, mode: int = 0, gateup: bool = False) -> DenseCase:
    return DenseCase(kind, M, N, K, mode, gateup)


# --------------------------------------------------------------------------
# every GPU run
# --------------------------------------------------------------------------
# key: dense_case's argument tuple. entry: ku (oa_gemv_ku) | gu_ku
# (oa_gemv_gateup_ku) | ex (oa_gemv_ex) | gu_ex (oa_gemv_gateup_ex) | rw4
# (oa_gemv_rw4) | a public wrapper's name. rw, ku: 0 where the entry has none.
Run = collections.namedtuple("Run", "key entry rw ku env")


def _run(key, entry, rw=0, ku=0, env=None) -> Run:
    return Run(key, entry, rw, ku, tuple(sorted((env or {}).items())))


def shipped_ku(rw: int, norm: bool) -> int:
    return SHIPPED_KU[f"RW{rw}{'_NORM' if norm else ''}"]


def _depths(shipped: int) -> List[int]:
    return sorted({1, shipped})


VALU_SHAPES = [(1, 8), (5, 520), (9, 4616), (9, 7688)]
GRID_STRIDE = {1: (8200, 16), 2: (16393, 16), 4: (32777, 16)}   # rows past 2048 blocks x 4 waves x RW

VALU_RUNS = [
    _run(("valu", M, N, K, mode, False), "ku", rw, ku)
    for rw in (1, 2) for M in (1, 2) for N, K in VALU_SHAPES + [GRID_STRIDE[rw]]
    for mode in (0, 1, 2, 3) for ku in _depths(shipped_ku(rw, bool(mode & 1)))
]
RW4_RUNS = [_run(("valu", 1, N, K, 0, False), "rw4", 4) for N, K in ((5, 520), GRID_STRIDE[4])]
OPS_RUNS = [
    _run(("valu", M, 9, 4616, mode, gu), entry)
    for M in (1, 2)
    for entry, mode, gu in (("linear", 0, False), ("linear_norm", 1, False), ("linear_addres", 2, False),
                            ("gateup_silu", 0, True), ("gateup_silu_norm", 1, True))
]
VALU_GU_SHAPES = [(1, 8), (3, 520), (5, 7688), (8200, 16)]
VALU_GU_RUNS = [
    _run(("valu", M, I, K, norm, True), "gu_ku", 2, ku)
    for M in (1, 2) for I, K in VALU_GU_SHAPES for norm in (0, 1) for ku in _depths(SHIPPED_KU["GATEUP"])
]
WIDE_MS = (3, 4, 5, 6, 7, 8, 12, 16)
_WIDE_SHAPES = [(M, 9, 1040) for M in WIDE_MS] + [(M, 6149, 16) for M in (3, 16)]
VALU_WIDE_RUNS = (
    [_run(("valu", M, N, K, mode, False), "ex") for M, N, K in _WIDE_SHAPES for mode in (0, 1, 2, 3)]
    + [_run(("valu", M, N, K, norm, True), "gu_ex") for M, N, K in _WIDE_SHAPES for norm in (0, 1)]
)
MFMA_SHAPES = [(3, 17, 1024), (5, 33, 2048), (8, 1, 4096), (8, 17, 6144),
               (2, 16, 1024), (9, 17, 4096), (15, 1, 2048), (16, 33, 4096)]
MFMA_GU_SHAPES = [(3, 17, 512), (5, 16, 1536), (8, 1, 4096), (16, 33, 4096)]


def _mfma_env(M: int) -> dict:
    return {} if 3 <= M <= 8 else MFMA_M2


MFMA_RUNS = [_run(("mfma", M, N, K, mode, False), "ex", env=_mfma_env(M))
             for M, N, K in MFMA_SHAPES for mode in (0, 1, 2, 3)]
MFMA_GU_RUNS = [_run(("mfma", M, I, K, norm, True), "gu_ex", env=_mfma_env(M))
                for M, I, K in MFMA_GU_SHAPES for norm in (0, 1)]
DENSE_RUNS = VALU_RUNS + RW4_RUNS + OPS_RUNS + VALU_GU_RUNS + VALU_WIDE_RUNS + MFMA_RUNS + MFMA_GU_RUNS

# the comparison itself, checked on the GPU: the real kernel fed a rolled
# norm weight or residual (mode 3 has both)
SELF_CHECK_RUNS = [_run(("valu", 2, 9, 4616, 3, False), "ku", 1, 2),
                   _run(("mfma", 5, 33, 2048, 3, False), "ex")]


def dense_keys() -> List[tuple]:
    """The distinct cases behind DENSE_RUNS, in order."""
    return list(dict.fromkeys(r.key for r in DENSE_RUNS + SELF_CHECK_RUNS))


def key_id(key) -> str:
    kind, M, N, K, mode, gu = key
    return f"{kind}{'_gu' if gu else ''}-m{M}-n{N}-k{K}-mode{mode}"


def run_id(run: Run) -> str:
    tag = run.entry + (f"-rw{run.rw}" if run.entry in ("ku", "gu_ku") else "")
    tag += f"-ku{run.ku}" if run.ku else ""
    tag += "".join(f"-{v}" for _, v in run.env)
    return f"{key_id(run.key)}-{tag}"


def family(run: Run) -> str:
    """Families of the report (docs/KERNELS.md)."""
    kind, M, N, K, mode, gu = run.key
    if kind == "mfma":
        return "MFMA gate-up" if gu else "MFMA norm" if mode & 1 else "MFMA plain"
    if M >= 3:
        return "VALU M >= 3"
    if gu:
        return "VALU gate-up"
    return f"VALU rw {run.rw or 1}"          # the wrappers' N = 9 is the one-row class


def set_env(monkeypatch, env) -> None:
    """Every knob of the bf16 dispatch unset, then `env`."""
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    lc.set_env(monkeypatch, dict(env))
