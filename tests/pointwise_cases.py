"""Exact-operand cases, fp64 oracles, fp32 emulations and wrong-kernel mutants
for the pointwise kernels: rmsnorm / fused_add_rmsnorm (rmsnorm.hip), rope
(rope.hip), rope_kv (rope_kv.hip), silu_mul and kv_write (elementwise.hip).
CPU only, no pytest dependency; shared by tests/test_pointwise_oracle.py (CPU
proof that every mutant is visible) and the GPU file tests/test_pointwise_gpu.py.

These kernels compute a few fp32 operations per element and round once to
bf16, so every output element is judged on its own (the rounding test):

    |got - r| <= ulp_bf16(r) / 2 + E,   ulp_bf16(r) = 2^(floor(log2 |r|) - 7)

r is the fp64 oracle on the exact bf16 / fp32 operands; inputs are chosen so
that every r is a bf16 normal or exactly 0 (asserted). E is the fp32 slack of
the chain, derived from the arithmetic and never from a kernel's output:

  rope      E = 2^-22 (|x1 c| + |x2 s|): two products and one add, contracted
            or not, are at most 3 roundings of 2^-24 of the terms. The terms
            and not |r|, because the difference can cancel.
  rmsnorm   E = 2^-18 |r|: the sum of squares takes <= 32 serial adds per
            thread, 6 shuffle adds and 4 more, <= 42 * 2^-24 on the sum, half
            of which reaches rstd; rsqrtf, 1 / dim and the two multiplies add
            a few 2^-24. Below 2^-19 in all.
  residual  E = 2^-24 |r|: one fp32 add, then the rounding to bf16.
  silu_mul  E = 2^-16 |r| on gates |g| <= 60: __expf is v_exp(x log2e), whose
            argument error makes a relative error of about |g| 2^-24 <= 2^-18;
            the divide and the two multiplies add the rest.

The emulation of a kernel is the same operations in fp32 with the output
rounded to bf16; it must pass with zero failing elements. A mutant is a knob
of the emulation; it must fail >= MIN_FAIL elements of every case it applies
to. kv_write and the V half of rope_kv copy bits and are compared bit for bit;
every bit of a cache outside the named slots must be unchanged, and a wrong bit
counts as a failing element.
"""

from __future__ import annotations

import functools
import zlib
from typing import Dict, List, Tuple

import numpy as np

MIN_FAIL = 4
E_ROPE, E_NORM, E_RES, E_SILU = 2.0 ** -22, 2.0 ** -18, 2.0 ** -24, 2.0 ** -16
BF16_MIN_NORMAL, BF16_MAX = 2.0 ** -126, (2.0 - 2.0 ** -7) * 2.0 ** 127
PATTERN = 0x7FC5            # bf16 bits of the guard fill (a NaN)


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


# --------------------------------------------------------------------------
# bf16 and the criterion
# --------------------------------------------------------------------------
def bf16_round(x) -> np.ndarray:
    """fp32 -> nearest-even bf16 value, as fp32 (f32_to_bf16 of common.h)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return (u << np.uint64(16)).astype(np.uint32).view(np.float32)


def to_bits(x) -> np.ndarray:
    """bf16-valued fp32 -> uint16 bits."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any(), "not a bf16 value"
    return (u >> np.uint32(16)).astype(np.uint16)


def from_bits(b) -> np.ndarray:
    return (np.asarray(b).astype(np.uint32) << np.uint32(16)).view(np.float32)


def _f64(x32: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):          # signalling NaN patterns are data here
        return x32.astype(np.float64)


def ulp_bf16(r: np.ndarray) -> np.ndarray:
    a = np.abs(r)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(a, where=a > 0, out=np.zeros_like(a)))
    return np.where(a > 0, np.exp2(e - 7), 0.0)


def assert_normal_or_zero(r: np.ndarray, name: str) -> None:
    a = np.abs(r)
    assert np.isfinite(r).all() and ((a == 0) | ((a >= BF16_MIN_NORMAL) & (a <= BF16_MAX))).all(), name


def judge(got_bits, r: np.ndarray, E: np.ndarray) -> Tuple[int, float]:
    """(failing elements, largest (|got - r| - ulp/2) / E) of bf16 bits
    against the oracle r with slack E."""
    got = _f64(from_bits(got_bits)).reshape(r.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - r)
        half = 0.5 * ulp_bf16(r)
        ok = d <= half + E
        ratio = np.where(E > 0, (d - half) / np.where(E > 0, E, 1.0), np.where(d == 0, -np.inf, np.inf))
    fails = int((~ok).sum())
    worst = float(np.nanmax(ratio)) if ratio.size and not np.isnan(got).all() else float("inf")
    if np.isnan(got).any():
        worst = float("inf")
    return fails, worst


def bit_mismatches(got_bits, want_bits) -> int:
    return int((np.asarray(got_bits).astype(np.uint16) != np.asarray(want_bits).astype(np.uint16)).sum())


class Verdict:
    """Failing elements and the worst ratio, per judged output and in all."""

    def __init__(self):
        self.parts: Dict[str, Tuple[int, int, float]] = {}

    def add(self, name: str, n: int, fails: int, worst: float = float("-inf")):
        self.parts[name] = (n, fails, worst)

    @property
    def fails(self) -> int:
        return sum(p[1] for p in self.parts.values())

    @property
    def n(self) -> int:
        return sum(p[0] for p in self.parts.values())

    @property
    def worst(self) -> float:
        return max(p[2] for p in self.parts.values())

    def __repr__(self):
        return " ".join(f"{k}:{f}/{n}" + (f"@{w:.3f}" if np.isfinite(w) else "")
                        for k, (n, f, w) in self.parts.items())


# --------------------------------------------------------------------------
# rmsnorm and fused add
# --------------------------------------------------------------------------
NORM_DIMS = (8, 128, 1032, 2048, 2056, 4096, 8184, 8192)
NORM_ROWS = (1, 6)
NORM_EPS = (1e-5, 1e-3)
PASS_ELEMS = 2048                       # 256 threads x 8 elements
_ROW_EXP_X = (0, -10, 2, -12, 4, -4)    # rows 1 and 3: mean square below eps
_ROW_EXP_R = (1, -11, 2, -11, 2, -2)
SMALL_ROWS = (1, 3)


def norm_probes(dim: int) -> List[int]:
    """Where a unit, a wave, a pass or the partial pass changes hands."""
    p0 = (dim // PASS_ELEMS) * PASS_ELEMS
    ks = {0, dim - 1, 7, 8, 511, 512, 2047, 2048}
    if dim % PASS_ELEMS:
        ks |= {p0 - 1, p0, p0 + (dim - p0) // 16 * 8, dim - 8}      # in the partial pass
    return sorted(k for k in ks if 0 <= k < dim)


class NormCase:
    def __init__(self, dim: int, rows: int, eps: float, fused: bool):
        self.dim, self.rows, self.fused = dim, rows, fused
        self.eps = float(np.float32(eps))          # the launcher takes a float
        self.name = f"{'fused_add_' if fused else ''}rmsnorm_d{dim}_r{rows}_eps{eps:g}"
        g = _rng(self.name)
        self.probes = norm_probes(dim)
        amp = float(bf16_round(np.float32([0.5 * np.sqrt(dim)]))[0])     # 4x the background's whole sum
        sign = g.integers(0, 2, len(self.probes)) * 2.0 - 1.0

        def operand(exps):
            a = g.standard_normal((rows, dim)) * 0.25
            a[:, self.probes] = amp * sign
            a = bf16_round(a.astype(np.float32)).astype(np.float64)
            return (a * np.exp2(np.array(exps[:rows], dtype=np.float64))[:, None]).astype(np.float32)

        self.x = operand(_ROW_EXP_X)
        self.res = operand(_ROW_EXP_R) if fused else None
        to_bits(self.x)
        w = bf16_round((g.uniform(0.5, 1.5, dim) * (g.integers(0, 2, dim) * 2 - 1)).astype(np.float32))
        for _ in range(64):                        # a rolled w must differ everywhere
            same = (w == np.roll(w, 1)) | (w == np.roll(w, 2))
            if not same.any():
                break
            w[same] = bf16_round((g.uniform(0.5, 1.5, int(same.sum()))
                                  * (g.integers(0, 2, int(same.sum())) * 2 - 1)).astype(np.float32))
        assert not ((w == np.roll(w, 1)) | (w == np.roll(w, 2))).any() or dim <= 2
        assert (np.abs(w) >= 0.5).all() and (np.abs(w) <= 1.5).all() and (w > 0).any() and (w < 0).any()
        self.w = w
        # conditions the method rests on
        s = self.x.astype(np.float64) + (self.res.astype(np.float64) if fused else 0.0)
        sq = s * s
        share = sq[:, self.probes] / sq.sum(-1, keepdims=True)
        assert (share >= 1.0 / 16).all(), f"{self.name}: a probe carries {share.min():.4f} of its row"
        rms = np.sqrt(sq.mean(-1))
        if rows > 1:
            ratio = rms / np.roll(rms, -1)
            self.rms_sep = float(np.maximum(ratio, 1 / ratio).min())
            assert self.rms_sep >= 4.0, f"{self.name}: neighbouring rows' rms within {self.rms_sep:.2f}x"
            assert (sq.mean(-1)[list(SMALL_ROWS)] < self.eps).all(), "eps decides the small rows"
        r_out, r_res = self._core(np.float64)
        assert_normal_or_zero(r_out, self.name)
        self.r_out, self.E_out = r_out, E_NORM * np.abs(r_out)
        if fused:
            assert_normal_or_zero(r_res, self.name)
            self.r_res, self.E_res = r_res, E_RES * np.abs(r_res)

    def _core(self, ft, w=None, **mut):
        """(out, new residual) in arithmetic `ft`, unrounded."""
        x = self.x.astype(ft)
        w = (self.w if w is None else w).astype(ft)
        res_in = None if self.res is None else self.res.astype(ft)
        s = x
        if self.fused:
            s = x + np.roll(res_in, mut.get("res_roll", 0), axis=0)
        sn = s
        if mut.get("norm_rounded_sum"):
            sn = bf16_round(s.astype(np.float32)).astype(ft)
        if mut.get("norm_x_alone"):
            sn = x
        sq = sn * sn
        for k in mut.get("drop_k", ()):
            sq[:, k] = 0
        for k in mut.get("twice_k", ()):
            sq[:, k] *= 2
        if mut.get("last_unit_dropped"):
            sq[:, self.dim - 8:] = 0
        inv_d = ft(1.0) / ft(self.dim)
        if mut.get("mean_half"):
            inv_d = inv_d * ft(2)
        ms = sq.sum(-1, dtype=ft) * inv_d
        eps = ft(0.0 if mut.get("eps_dropped") else self.eps)
        if mut.get("eps_outside"):
            scale = ft(1.0) / (np.sqrt(ms) + eps)
        else:
            scale = ft(1.0) / np.sqrt(ms + eps)
        scale = np.roll(scale.astype(ft), mut.get("rstd_roll", 0))
        w = np.roll(w, mut.get("w_roll", 0))
        out = sn * scale[:, None] * w
        if mut.get("out_roll"):
            out = np.roll(out, 1, axis=0)
        new_res = None
        if self.fused:
            new_res = res_in if mut.get("res_not_updated") else s
        return out, new_res

    def emulation(self, **mut) -> Dict[str, np.ndarray]:
        out, res = self._core(np.float32, **mut)
        d = {"out": to_bits(bf16_round(out))}
        if self.fused:
            d["res"] = to_bits(bf16_round(res))
        return d

    def verdict(self, got: Dict[str, np.ndarray], ref=None) -> Verdict:
        """`ref`: (r_out, r_res) of a mutant's own oracle instead of the true one."""
        r_out, r_res = ref if ref is not None else (self.r_out, self.r_res if self.fused else None)
        v = Verdict()
        v.add("out", r_out.size, *judge(got["out"], r_out, E_NORM * np.abs(r_out)))
        if self.fused:
            v.add("res", r_res.size, *judge(got["res"], r_res, E_RES * np.abs(r_res)))
        return v

    def mutant_ref(self, **mut):
        return self._core(np.float64, **mut)

    def mutants(self) -> List[Tuple[str, dict]]:
        m: List[Tuple[str, dict]] = []
        for k in self.probes:
            m += [(f"probe{k}_dropped", {"drop_k": [k]}), (f"probe{k}_twice", {"twice_k": [k]})]
        m += [("last_unit_dropped", {"last_unit_dropped": True}), ("mean_over_dim_half", {"mean_half": True}),
              ("w_rolled_1", {"w_roll": 1}), ("w_rolled_2", {"w_roll": 2})]
        if self.rows > 1:
            m += [("eps_dropped", {"eps_dropped": True}), ("eps_outside_root", {"eps_outside": True}),
                  ("rstd_row+1", {"rstd_roll": -1}), ("rstd_row-1", {"rstd_roll": 1}),
                  ("out_rows_rolled", {"out_roll": True})]
        if self.fused:
            m += [("residual_not_updated", {"res_not_updated": True}), ("norm_of_x_alone", {"norm_x_alone": True})]
            if self.rows * self.dim >= 1024:
                m.append(("norm_of_rounded_sum", {"norm_rounded_sum": True}))
            if self.rows > 1:
                m += [("residual_row+1", {"res_roll": -1}), ("residual_row-1", {"res_roll": 1})]
        return m


@functools.lru_cache(maxsize=None)
def norm_case(dim: int, rows: int, eps: float, fused: bool) -> NormCase:
    return NormCase(dim, rows, eps, fused)


def norm_keys() -> List[tuple]:
    return [(d, r, e, f) for f in (False, True) for d in NORM_DIMS for r in NORM_ROWS for e in NORM_EPS]


# --------------------------------------------------------------------------
# rope and rope_kv
# --------------------------------------------------------------------------
TABLE_P = 97
ROPE_DS = (16, 64, 128, 256)
ROPE_HEADS = ((1, 1), (6, 2), (8, 1), (5, 3))
ROPE_TS = (1, 37)
GRID_STRIDE_ROPE = (2050, 17, 1, 128)       # T * Hq * D / 8 rope items > 2048 * 256
GRID_STRIDE_ROPE_KV = (2050, 14, 1, 128)    # T * (Hq + 2 Hk) * D / 8 items > 2048 * 256


@functools.lru_cache(maxsize=None)
def tables(D: int) -> Tuple[np.ndarray, np.ndarray]:
    """Synthetic fp32 cos / sin [P, D/2]: n / 4096 with n in -4096..4096, the
    two independent and every (position, pair) cell different, so every pair of
    every position rotates by O(1) and every product is exact in fp64."""
    g = _rng(f"tables-{D}")
    while True:
        c = g.integers(-4096, 4097, (TABLE_P, D // 2))
        s = g.integers(-4096, 4097, (TABLE_P, D // 2))
        if np.unique(c * 10000 + s).size == c.size:
            return (c / 4096.0).astype(np.float32), (s / 4096.0).astype(np.float32)


def _lookup(table: np.ndarray, pos: np.ndarray, d2: int, pitch: int, pair_shift: int) -> np.ndarray:
    pair = (np.arange(d2) + pair_shift) % d2
    flat = table.reshape(-1)
    return flat[(pos[:, None] * pitch + pair[None, :]) % flat.size]        # [T, d2]


def rope_core(x: np.ndarray, cos: np.ndarray, sin: np.ndarray, pos: np.ndarray, ft, **mut):
    """Rotate-half rope of x [T, H, D] in arithmetic `ft`. Returns (out, terms)
    with terms = |x1 c| + |x2 s| per element."""
    D = x.shape[-1]
    d2 = D // 2
    pos = (pos + mut.get("pos_shift", 0)) % TABLE_P
    pitch = D if mut.get("pitch_D") else d2
    c = _lookup(cos, pos, d2, pitch, mut.get("pair_shift", 0)).astype(ft)[:, None, :]
    s = _lookup(sin, pos, d2, pitch, mut.get("pair_shift", 0)).astype(ft)[:, None, :]
    if mut.get("cos_sin_exchanged"):
        c, s = s, c
    if "sin_neg_from" in mut:
        s = s.copy()
        s[..., mut["sin_neg_from"]:] *= -1
    x = x.astype(ft)
    if mut.get("interleaved"):
        x1, x2 = x[..., 0::2], x[..., 1::2]
    else:
        x1, x2 = x[..., :d2], x[..., d2:]
    a, b = x1 * c, x2 * s
    o1 = a + b if mut.get("same_sign") else a - b
    o2 = x2 * c + x1 * s
    out = np.empty_like(x)
    if mut.get("interleaved"):
        out[..., 0::2], out[..., 1::2] = o1, o2
    else:
        out[..., :d2], out[..., d2:] = o1, o2
    terms = np.concatenate([np.abs(a) + np.abs(b), np.abs(x2 * c) + np.abs(x1 * s)], axis=-1)
    return out, terms


_ROPE_MUTANTS = [("sin_negated", {"sin_neg_from": 0}), ("cos_sin_exchanged", {"cos_sin_exchanged": True}),
                 ("interleaved_halves", {"interleaved": True}), ("halves_same_sign", {"same_sign": True}),
                 ("position+1", {"pos_shift": 1}), ("position-1", {"pos_shift": -1}),
                 ("table_pitch_D", {"pitch_D": True}), ("pair_index+4", {"pair_shift": 4})]


class RopeCase:
    """kind 'rope' (oa_rope: q and k contiguous, in place) or 'rope_kv'
    (oa_rope_kv: q, k, v head slices of one padded buffer, k and v scattered
    into pre-filled caches)."""

    def __init__(self, kind: str, T: int, Hq: int, Hk: int, D: int):
        assert kind in ("rope", "rope_kv")
        self.kind, self.T, self.Hq, self.Hk, self.D = kind, T, Hq, Hk, D
        self.name = f"{kind}_t{T}_hq{Hq}_hk{Hk}_d{D}"
        g = _rng(self.name)
        self.cos, self.sin = tables(D)
        pos = g.integers(0, TABLE_P, T)
        if T >= 3:
            pos[T // 2], pos[1] = 0, TABLE_P - 1
            assert (np.diff(pos) < 0).any() and (np.diff(pos) > 0).any(), "non-monotonic"
        else:
            pos[0] = TABLE_P - 1
        self.q = bf16_round(g.standard_normal((T, Hq, D)).astype(np.float32))
        self.k = bf16_round(g.standard_normal((T, Hk, D)).astype(np.float32))
        self.dup = []
        if kind == "rope_kv":
            self.S = T + 19
            self.slots = g.permutation(self.S)[:T].astype(np.int32)
            self.v = g.integers(0, 1 << 16, (T, Hk, D)).astype(np.uint16)
            flat = self.v.reshape(-1)
            flat[:: 5] = np.resize(np.array([0x8000, 0x7FC0, 0xFFFF, 0x7F81, 0x0000, 0xFF80], np.uint16),
                                   flat[:: 5].size)          # -0, NaN patterns, +0, -inf
            self.kc0 = g.integers(0, 1 << 16, (self.S, Hk, D)).astype(np.uint16)
            self.vc0 = g.integers(0, 1 << 16, (self.S, Hk, D)).astype(np.uint16)
            if T >= 37:
                # the engine's graph padding: later rows repeat a row, slot and position
                self.dup = [T - 3, T - 2, T - 1]
                for t in self.dup:
                    self.k[t], self.v[t] = self.k[T - 4], self.v[T - 4]
                    pos[t], self.slots[t] = pos[T - 4], self.slots[T - 4]
        self.pos = pos.astype(np.int32)
        self.rq, tq = rope_core(self.q, self.cos, self.sin, self.pos, np.float64)
        self.rk, tk = rope_core(self.k, self.cos, self.sin, self.pos, np.float64)
        self.Eq, self.Ek = E_ROPE * tq, E_ROPE * tk
        assert_normal_or_zero(self.rq, self.name)
        assert_normal_or_zero(self.rk, self.name)

    # ---- the kernel in fp32, with mutant knobs ----------------------------
    def emulation(self, cos=None, sin=None, **mut) -> Dict[str, np.ndarray]:
        cos = self.cos if cos is None else cos
        sin = self.sin if sin is None else sin
        rope_mut = {k: v for k, v in mut.items() if k in
                    ("sin_neg_from", "cos_sin_exchanged", "interleaved", "same_sign", "pos_shift",
                     "pitch_D", "pair_shift")}
        q = to_bits(bf16_round(rope_core(self.q, cos, sin, self.pos, np.float32, **rope_mut)[0]))
        k = to_bits(bf16_round(rope_core(self.k, cos, sin, self.pos, np.float32, **rope_mut)[0]))
        d = {"q": q, "k": k}
        if self.kind == "rope_kv":
            slots = np.roll(self.slots, mut.get("slot_roll", 0))
            kc, vc = self.kc0.copy(), self.vc0.copy()
            krow = to_bits(self.k) if mut.get("cache_k_not_roped") else k
            vrow = np.roll(self.v, mut.get("v_head_roll", 0), axis=1)
            h0 = 1 if mut.get("first_k_head_as_q") else 0       # head 0 roped in place, never scattered
            kc[slots, h0:] = krow[:, h0:]
            vc[slots] = vrow
            d["kc"], d["vc"] = kc, vc
        return d

    def verdict(self, got: Dict[str, np.ndarray], ref=None) -> Verdict:
        rq, rk, Eq, Ek = ref if ref is not None else (self.rq, self.rk, self.Eq, self.Ek)
        v = Verdict()
        v.add("q", rq.size, *judge(got["q"], rq, Eq))
        v.add("k", rk.size, *judge(got["k"], rk, Ek))
        if self.kind == "rope_kv":
            kc, vc = np.asarray(got["kc"]), np.asarray(got["vc"])
            v.add("cache_k", rk.size, *judge(kc[self.slots], rk, Ek))
            v.add("cache_k_is_k", rk.size, bit_mismatches(kc[self.slots], got["k"]))
            v.add("cache_v", self.v.size, bit_mismatches(vc[self.slots], self.v))
            other = np.setdiff1d(np.arange(self.S), self.slots)
            v.add("cache_rest", 2 * other.size * self.Hk * self.D,
                  bit_mismatches(kc[other], self.kc0[other]) + bit_mismatches(vc[other], self.vc0[other]))
        return v

    def mutant_ref(self, cos, sin):
        """Oracle of the same kernel on other tables."""
        rq, tq = rope_core(self.q, cos, sin, self.pos, np.float64)
        rk, tk = rope_core(self.k, cos, sin, self.pos, np.float64)
        return rq, rk, E_ROPE * tq, E_ROPE * tk

    def mutants(self) -> List[Tuple[str, dict]]:
        m = list(_ROPE_MUTANTS)
        if self.D // 2 > 48:
            m.append(("sin_negated_from_pair_48", {"sin_neg_from": 48}))
        if self.kind == "rope_kv":
            m += [("first_k_head_as_q_head", {"first_k_head_as_q": True}),
                  ("cache_k_not_roped", {"cache_k_not_roped": True})]
            if self.T > 1:
                m += [("slot_of_t+1", {"slot_roll": -1}), ("slot_of_t-1", {"slot_roll": 1})]
            if self.Hk > 1:
                m += [("v_from_head_h+1", {"v_head_roll": -1}), ("v_from_head_h-1", {"v_head_roll": 1})]
        return m


@functools.lru_cache(maxsize=None)
def rope_case(kind: str, T: int, Hq: int, Hk: int, D: int) -> RopeCase:
    return RopeCase(kind, T, Hq, Hk, D)


def rope_keys(kind: str) -> List[tuple]:
    keys = [(kind, T, Hq, Hk, D) for D in ROPE_DS for Hq, Hk in ROPE_HEADS for T in ROPE_TS]
    return keys + [(kind,) + (GRID_STRIDE_ROPE if kind == "rope" else GRID_STRIDE_ROPE_KV)]


# --------------------------------------------------------------------------
# the rope inside the rope-fused decode kernel (attention_decode.hip)
# --------------------------------------------------------------------------
DECODE_BS, DECODE_HK, DECODE_D = 32, 2, 128
DECODE_LENS = (1, 2, 33, 64)                 # block size 32: first key, second, a new block, a full table
DECODE_GS = (1, 4, 8)
DECODE_NSPLITS = (1, 4)


class DecodeRopeCase(RopeCase):
    """One decode step of B sequences of `lens` keys: the kernel ropes the new
    k with table row n - 1 and scatters it and v into the paged cache. B 1 and
    B 5 reach the new k by the 4-deep and the 2-deep form. Judged: the cache k
    row at the new slot by the criterion, the v row bit for bit, every other
    cache bit unchanged. Caches and v hold finite values: attention reads them."""

    def __init__(self, G: int, lens: Tuple[int, ...]):
        B, Hk, D, bs = len(lens), DECODE_HK, DECODE_D, DECODE_BS
        self.kind, self.T, self.Hq, self.Hk, self.D, self.G = "rope_kv", B, G * Hk, Hk, D, G
        self.name = f"decode_rope_b{B}_g{G}_n{'_'.join(map(str, lens))}"
        g = _rng(self.name)
        self.cos, self.sin = tables(D)
        self.lens = np.array(lens, dtype=np.int32)
        self.pos = self.lens - 1
        self.q = bf16_round(g.standard_normal((B, self.Hq, D)).astype(np.float32))
        self.k = bf16_round(g.standard_normal((B, Hk, D)).astype(np.float32))
        v = bf16_round(g.standard_normal((B, Hk, D)).astype(np.float32))
        v.reshape(-1)[::7] = -0.0
        self.v = to_bits(v)
        self.max_blocks = 2
        nb = self.max_blocks * B + 3
        self.bt = g.permutation(nb)[:self.max_blocks * B].reshape(B, self.max_blocks).astype(np.int32)
        self.S = nb * bs
        self.slots = (self.bt[np.arange(B), self.pos // bs] * bs + self.pos % bs).astype(np.int32)
        self.kc0 = to_bits(bf16_round(g.standard_normal((self.S, Hk, D)).astype(np.float32)))
        self.vc0 = to_bits(bf16_round(g.standard_normal((self.S, Hk, D)).astype(np.float32)))
        self.dup = []
        self.rk, tk = rope_core(self.k, self.cos, self.sin, self.pos, np.float64)
        self.rq, tq = rope_core(self.q, self.cos, self.sin, self.pos, np.float64)
        self.Ek, self.Eq = E_ROPE * tk, E_ROPE * tq
        assert_normal_or_zero(self.rk, self.name)

    def verdict(self, got: Dict[str, np.ndarray], ref=None) -> Verdict:
        kc, vc = np.asarray(got["kc"]), np.asarray(got["vc"])
        other = np.setdiff1d(np.arange(self.S), self.slots)
        v = Verdict()
        v.add("cache_k", self.rk.size, *judge(kc[self.slots], self.rk, self.Ek))
        v.add("cache_v", self.v.size, bit_mismatches(vc[self.slots], self.v))
        v.add("cache_rest", 2 * other.size * self.Hk * self.D,
              bit_mismatches(kc[other], self.kc0[other]) + bit_mismatches(vc[other], self.vc0[other]))
        return v

    def mutants(self) -> List[Tuple[str, dict]]:
        m = list(_ROPE_MUTANTS) + [("sin_negated_from_pair_48", {"sin_neg_from": 48}),
                                   ("cache_k_not_roped", {"cache_k_not_roped": True}),
                                   ("v_from_head_h+1", {"v_head_roll": -1})]
        if self.T > 1:
            m += [("slot_of_b+1", {"slot_roll": -1}), ("slot_of_b-1", {"slot_roll": 1})]
        if not self.pos.any():                       # row 0 sits at the same place at any pitch
            m = [x for x in m if x[0] != "table_pitch_D"]
        return m


@functools.lru_cache(maxsize=None)
def decode_rope_case(G: int, lens: Tuple[int, ...]) -> DecodeRopeCase:
    return DecodeRopeCase(G, lens)


def decode_rope_keys() -> List[tuple]:
    return ([(G, (n,)) for G in DECODE_GS for n in DECODE_LENS]
            + [(G, DECODE_LENS + (33,)) for G in DECODE_GS])


# (name, G, Hk, block size, nsplit, lens): attention itself on the synthetic
# tables, the only direct check of the decode kernel's q rope in the upper pairs.
# A head whose weight sits on its planted probes (all equal to its roped q) is
# blind to a wrong q rope; each case keeps heads without probes, which are not.
ATTENTION_CASES = (("synth_b1_g8_s4", 8, 2, 32, 4, (90,)),
                   ("synth_b2_g4_s1", 4, 2, 32, 1, (33, 64)),
                   ("synth_b5_g1_s4", 1, 2, 16, 4, (1, 2, 33, 64, 97)))


@functools.lru_cache(maxsize=None)
def attention_case(name: str):
    """A rope DecodeCase of tests/attention_oracle.py built on the synthetic
    tables. Its oracle sees q roped in fp64 and NOT rounded (the kernel keeps
    the roped q in fp32) and the new key as stored, rounded to bf16. Returns
    (case, q with sin negated from pair 48, also fp64) -- N, T = 4 N and the
    fp64 oracle are the existing ones."""
    import torch

    import attention_oracle as ao

    spec = next(c for c in ATTENTION_CASES if c[0] == name)
    _, G, Hk, bs, nsplit, lens = spec
    cos, sin = tables(ao.D_HEAD)
    saved = ao.decode_lens, ao.rope_tables
    ao.decode_lens = lambda B, bs_, ns, maxlen, rot: list(lens)
    ao.rope_tables = lambda: (torch.from_numpy(cos), torch.from_numpy(sin))
    try:
        c = ao.DecodeCase(name, len(lens), G, Hk, bs, nsplit, max(lens), None, rope=True,
                          index=100 + [x[0] for x in ATTENTION_CASES].index(name))
    finally:
        ao.decode_lens, ao.rope_tables = saved
    pos = np.array(lens) - 1
    q, k = c.q.float().numpy(), c.k_new.float().numpy()
    q64 = rope_core(q, cos, sin, pos, np.float64)[0]
    k_stored = bf16_round(rope_core(k, cos, sin, pos, np.float32)[0])
    c.set_roped(torch.from_numpy(q64), torch.from_numpy(k_stored))
    c.q_eff = torch.from_numpy(q64)                        # set_roped narrows to fp32
    for a in ("ref", "noise"):
        c.__dict__.pop(a, None)
    q_mut = torch.from_numpy(rope_core(q, cos, sin, pos, np.float64, sin_neg_from=48)[0])
    return c, q_mut


# --------------------------------------------------------------------------
# silu_mul
# --------------------------------------------------------------------------
SILU_GRID_STRIDE_N = 2048 * 256 * 8 + 24


@functools.lru_cache(maxsize=None)
def all_gates() -> np.ndarray:
    """Every bf16 normal with 2^-20 <= |g| <= 60, and +-0, shuffled (a gate's
    neighbours then differ from it by far more than an ulp)."""
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    v = from_bits(bits)
    a = np.abs(_f64(v))
    keep = ((a >= 2.0 ** -20) & (a <= 60.0)) | (a == 0)
    g = v[keep]
    assert g.size == 2 * (26 * 128 - 15) + 2
    return _rng("gates").permutation(g)


class SiluCase:
    def __init__(self, n: int):
        assert n % 8 == 0
        self.n, self.name = n, f"silu_mul_n{n}"
        r = _rng(self.name)
        gates = all_gates()
        self.g = np.resize(gates, n) if n >= gates.size else gates[r.permutation(gates.size)[:n]]
        cls = np.repeat(r.integers(-3, 4, n // 8), 8)                    # a magnitude class per unit
        mant = 1.0 + r.integers(0, 128, n) / 128.0
        self.u = (mant * np.exp2(cls) * (r.integers(0, 2, n) * 2 - 1)).astype(np.float32)
        to_bits(self.u)
        self.r = self._core(np.float64)
        assert_normal_or_zero(self.r, self.name)
        self.E = E_SILU * np.abs(self.r)

    def _core(self, ft, **mut) -> np.ndarray:
        g, u = self.g.astype(ft), self.u.astype(ft)
        if mut.get("gate_lo_hi_exchanged"):
            g = g[np.arange(self.n) ^ 1]
        if mut.get("u_next_word"):
            u = np.roll(u, -2)
        if mut.get("silu_of_u"):
            g, u = u, g
        with np.errstate(over="ignore"):
            e = np.exp(g if mut.get("exp_plus") else -g).astype(ft)
            sig = ft(1.0) / (ft(1.0) + e)
            out = sig * u if mut.get("sigmoid_only") else g / (ft(1.0) + e) * u
        return out

    def emulation(self, **mut) -> Dict[str, np.ndarray]:
        out = to_bits(bf16_round(self._core(np.float32, **mut)))
        if mut.get("last_unit_dropped"):
            out[-8:] = PATTERN
        return {"out": out}

    def verdict(self, got: Dict[str, np.ndarray]) -> Verdict:
        v = Verdict()
        v.add("out", self.n, *judge(got["out"], self.r, self.E))
        return v

    def mutants(self) -> List[Tuple[str, dict]]:
        return [("silu_of_u_times_g", {"silu_of_u": True}), ("sigmoid_without_g", {"sigmoid_only": True}),
                ("exp_of_plus_g", {"exp_plus": True}), ("gate_lo_hi_exchanged", {"gate_lo_hi_exchanged": True}),
                ("u_from_next_word", {"u_next_word": True}), ("last_unit_dropped", {"last_unit_dropped": True})]


@functools.lru_cache(maxsize=None)
def silu_case(n: int) -> SiluCase:
    return SiluCase(n)


def silu_keys() -> List[int]:
    return [8, 2056, -(-all_gates().size // 8) * 8, SILU_GRID_STRIDE_N]


# --------------------------------------------------------------------------
# kv_write
# --------------------------------------------------------------------------
KV_KEYS = ((5, 1, 8), (37, 4, 128), (4100, 8, 128))      # the last: T * Hk * D / 8 items > 2048 * 256


class KvWriteCase:
    def __init__(self, T: int, Hk: int, D: int):
        self.T, self.Hk, self.D, self.name = T, Hk, D, f"kv_write_t{T}_hk{Hk}_d{D}"
        g = _rng(self.name)
        self.S = T + 19
        self.slots = g.permutation(self.S)[:T].astype(np.int32)
        self.k = g.integers(0, 1 << 16, (T, Hk, D)).astype(np.uint16)
        self.v = g.integers(0, 1 << 16, (T, Hk, D)).astype(np.uint16)
        if T >= 3:                                     # duplicate slots carrying identical rows
            self.k[T - 1], self.v[T - 1], self.slots[T - 1] = self.k[T - 2], self.v[T - 2], self.slots[T - 2]
        self.kc0 = g.integers(0, 1 << 16, (self.S, Hk, D)).astype(np.uint16)
        self.vc0 = g.integers(0, 1 << 16, (self.S, Hk, D)).astype(np.uint16)

    def emulation(self, **mut) -> Dict[str, np.ndarray]:
        kc, vc = self.kc0.copy(), self.vc0.copy()
        slots = np.roll(self.slots, mut.get("slot_roll", 0))
        k, v = (self.v, self.k) if mut.get("k_v_exchanged") else (self.k, self.v)
        kc[slots], vc[slots] = k, v
        if mut.get("last_unit_dropped"):
            kc[slots, -1, -8:] = self.kc0[slots, -1, -8:]
            vc[slots, -1, -8:] = self.vc0[slots, -1, -8:]
        return {"kc": kc, "vc": vc}

    def verdict(self, got: Dict[str, np.ndarray]) -> Verdict:
        kc, vc = np.asarray(got["kc"]), np.asarray(got["vc"])
        other = np.setdiff1d(np.arange(self.S), self.slots)
        v = Verdict()
        v.add("cache_k", self.k.size, bit_mismatches(kc[self.slots], self.k))
        v.add("cache_v", self.v.size, bit_mismatches(vc[self.slots], self.v))
        v.add("cache_rest", 2 * other.size * self.Hk * self.D,
              bit_mismatches(kc[other], self.kc0[other]) + bit_mismatches(vc[other], self.vc0[other]))
        return v

    def mutants(self) -> List[Tuple[str, dict]]:
        return [("slot_of_t+1", {"slot_roll": -1}), ("slot_of_t-1", {"slot_roll": 1}),
                ("k_v_exchanged", {"k_v_exchanged": True}), ("last_unit_dropped", {"last_unit_dropped": True})]


@functools.lru_cache(maxsize=None)
def kv_write_case(T: int, Hk: int, D: int) -> KvWriteCase:
    return KvWriteCase(T, Hk, D)
