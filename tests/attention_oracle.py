"""fp64 attention oracles, wrong-kernel mutants, and probe-planting input
builders for the attention parity tests. CPU only, no pytest dependency.

Why this exists: attention outputs on soft random inputs are means of hundreds
of v rows, so an element-wise tolerance of a few 1e-2 hides a dropped tile, an
off-by-one mask or a permuted block table. The tests built on this module

  * draw PEAKED scores (q, k ~ 1.5 * randn, v ~ randn) so single keys matter,
  * PLANT probes on the keys only one row / one range boundary ever sees,
  * measure `row_rel_err`: per output vector max|got-ref| / max|ref|,
  * and prove on the CPU (tests/test_attention_oracle.py) that every mutant
    below lands far above the tolerance the GPU tests use.

Layouts follow `ops.attention_prefill` (q [B,Sq,Hq,D], k/v [B,Skv,Hk,D]) and
`ops.attention_decode_paged` (q [B,Hq,D], caches [nb,bs,Hk,D], block table
[B,max_blocks] int32, lens [B] int32).
"""

from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

D_HEAD = 128
PEAK = 1.5            # q/k magnitude: scores ~ N(0, 2.25^2) at scale D^-0.5
PROBE_IN = 1.0        # planted key that must count:      k = q
PROBE_OUT = 1.5       # planted key that must NOT count:  k = 1.5 q
POISON_K = 2.0        # decode: keys past seq_len:        k = 2 q
POISON_V = 4.0
INV_LOG2E = 1.0 / 1.4426950408889634
TOL_FACTOR = 4.0      # T = 4 N
MUTANT_FACTOR = 4.0   # every mutant >= 4 T


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# --------------------------------------------------------------------------
# metric
# --------------------------------------------------------------------------
def row_rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max over output vectors of max_d|got-ref| / max_d|ref|; inf when `got`
    holds a non-finite value."""
    g = got.detach().to("cpu", torch.float64)
    r = ref.detach().to("cpu", torch.float64)
    assert g.shape == r.shape, (g.shape, r.shape)
    if not torch.isfinite(g).all():
        return float("inf")
    num = (g - r).abs().amax(dim=-1)
    den = r.abs().amax(dim=-1).clamp_min(1e-30)
    return float((num / den).max())


# --------------------------------------------------------------------------
# prefill oracle (+ mutants, + kernel-precision emulation)
# --------------------------------------------------------------------------
def _prefill_core(q, k, v, scale, dtype, round_p, *, causal_shift=0,
                  row_shift: Optional[Dict[int, int]] = None,
                  drop: Optional[Tuple[int, int, int]] = None,
                  swap_q_heads: Optional[Tuple[int, int]] = None,
                  roll_kv_heads: int = 0, scale_mul: float = 1.0,
                  zero_v: Optional[Tuple[int, int]] = None):
    B, Sq, Hq, D = q.shape
    Skv, Hk = k.shape[1], k.shape[2]
    G = Hq // Hk
    off = Skv - Sq
    sc = (D ** -0.5 if scale is None else scale) * scale_mul
    qd, kd, vd = q.to(dtype), k.to(dtype), v.to(dtype)
    if zero_v is not None:
        vd = vd.clone()
        vd[:, zero_v[0]:zero_v[1]] = 0
    # row i may use keys 0 .. limit[i]
    limit = torch.arange(Sq) + off + causal_shift
    for r, d in (row_shift or {}).items():
        limit[r] += d
    visible = torch.arange(Skv)[None, :] <= limit[:, None]
    if drop is not None:
        a, b_, r0 = drop
        visible[r0:, a:b_] = False
    src = list(range(Hq))
    if swap_q_heads is not None:
        h0, h1 = swap_q_heads
        src[h0], src[h1] = h1, h0
    out = torch.zeros(B, Sq, Hq, D, dtype=dtype)
    neg = torch.tensor(float("-inf"), dtype=dtype)
    for b in range(B):
        for h in range(Hq):
            hk = (h // G + roll_kv_heads) % Hk
            s = (qd[b, :, src[h]] @ kd[b, :, hk].T) * sc
            s = torch.where(visible, s, neg)
            mx = s.amax(dim=1, keepdim=True)
            mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
            p = torch.exp(s - mx)
            l = p.sum(dim=1, keepdim=True)
            if round_p:
                p = p.to(torch.bfloat16).to(dtype)
            o = p @ vd[b, :, hk]
            out[b, :, h] = torch.where(l > 0, o / l.clamp_min(1e-300), torch.zeros_like(o))
    return out


def prefill_oracle(q, k, v, scale=None, **mutant) -> torch.Tensor:
    """Causal attention in fp64 (row i sees keys 0 .. Skv-Sq+i). Keyword
    knobs give the answer of one specific wrong kernel:
      causal_shift=+1/-1          mask off by one for every row
      row_shift={row: +1/-1}      mask off by one for single rows
      drop=(a, b, r0)             keys [a, b) ignored by rows >= r0
      swap_q_heads=(h0, h1)       two q-heads of a GQA group exchanged
      roll_kv_heads=1             q-head group reads the next kv head
      scale_mul=INV_LOG2E         exp2-domain scale folded wrongly
      zero_v=(a, b)               V rows [a, b) read as zero
    """
    return _prefill_core(q, k, v, scale, torch.float64, False, **mutant)


def prefill_emulation(q, k, v, scale=None) -> torch.Tensor:
    """A correct kernel's rounding: fp32 throughout, P rounded to bf16 before
    P.V while the row sum keeps the unrounded P (attention_prefill.hip: v2
    stores f32_to_bf16(p) to the P tile and adds p to psum; v3/v4 pack with
    v_cvt_pk_bf16_f32 after psum +=), output rounded to bf16."""
    return _prefill_core(q, k, v, scale, torch.float32, True).to(torch.bfloat16)


# --------------------------------------------------------------------------
# decode oracle
# --------------------------------------------------------------------------
def split_ranges(n: int, nsplit: int) -> List[Tuple[int, int, int]]:
    """Non-empty (split, kstart, kend) with chunk = ceil(n / nsplit)."""
    chunk = _ceil_div(n, nsplit)
    out = []
    for s in range(nsplit):
        ks = s * chunk
        ke = min(n, ks + chunk)
        if ke > ks:
            out.append((s, ks, ke))
    return out


def wave_ranges(n: int, nsplit: int, rope: bool = False) -> List[Tuple[int, int, int, int]]:
    """Non-empty (split, wave, start, end): each split's key span is cut into
    four sub-ranges of ceil(span / 4). With rope the newest key n-1 comes from
    registers, so the spans cover the cached keys [0, n-1) only."""
    n_c = n - 1 if rope else n
    out = []
    for s, ks, ke in split_ranges(n, nsplit):
        ke_c = min(ke, n_c)
        span = ke_c - ks
        wch = _ceil_div(max(span, 0), 4)
        for w in range(4):
            ws = ks + w * wch
            we = min(ke_c, ws + wch)
            if we > ws:
                out.append((s, w, ws, we))
    return out


def _decode_core(q, kc, vc, bt, lens, scale, dtype, *, nsplit=1, rope=False,
                 len_delta=0, bt_roll=False, last_block_wrong=False,
                 split_first=None, split_last=None, wave_first=None,
                 wave_last=None, dup_boundary=None, avg_combine=False,
                 gqa_swap=False):
    B, Hq, D = q.shape
    nb, bs, Hk, _ = kc.shape
    G = Hq // Hk
    sc = D ** -0.5 if scale is None else scale
    kflat = kc.reshape(nb * bs, Hk, D).to(dtype)
    vflat = vc.reshape(nb * bs, Hk, D).to(dtype)
    qd = q.to(dtype)
    out = torch.zeros(B, Hq, D, dtype=dtype)
    for b in range(B):
        n_true = int(lens[b])
        n = n_true + len_delta
        if n <= 0:
            continue
        pos = torch.arange(n)
        blk = pos // bs
        row = bt[b].long()
        if bt_roll:
            row = row.roll(1)
        entry = row[blk]
        if last_block_wrong:
            nblk = _ceil_div(n, bs)
            wrong = nblk - 2 if nblk >= 2 else 1
            entry = torch.where(blk == nblk - 1, row[wrong], entry)
        slot = entry * bs + pos % bs
        K = kflat[slot]            # [n, Hk, D]
        V = vflat[slot]
        w = torch.ones(n, dtype=dtype)
        sr = {s: (ks, ke) for s, ks, ke in split_ranges(n, nsplit)}
        wr = {(s, wv): (ws, we) for s, wv, ws, we in wave_ranges(n, nsplit, rope)}
        if split_first is not None and split_first in sr:
            w[sr[split_first][0]] = 0
        if split_last is not None and split_last in sr:
            w[sr[split_last][1] - 1] = 0
        if wave_first is not None and wave_first in wr:
            w[wr[wave_first][0]] = 0
        if wave_last is not None and wave_last in wr:
            w[wr[wave_last][1] - 1] = 0
        if dup_boundary is not None and dup_boundary in sr:
            w[sr[dup_boundary][0]] = 2
        for hk in range(Hk):
            qg = qd[b, hk * G:(hk + 1) * G]            # [G, D]
            s = (qg @ K[:, hk].T) * sc                 # [G, n]
            vv = V[:, hk]                              # [n, D]

            def soft(lo, hi):
                ww = w[lo:hi]
                live = ww > 0
                if not bool(live.any()):
                    return None
                ss = s[:, lo:hi]
                mx = ss[:, live].amax(dim=1, keepdim=True)
                p = torch.exp(ss - mx) * ww
                return (p @ vv[lo:hi]) / p.sum(dim=1, keepdim=True)

            if avg_combine:
                parts = [soft(ks, ke) for ks, ke in sr.values()]
                parts = [p for p in parts if p is not None]
                o = torch.stack(parts).mean(dim=0)
            else:
                o = soft(0, n)
                if o is None:
                    o = torch.zeros(G, D, dtype=dtype)
            if gqa_swap and G >= 2:
                o = o.clone()
                o[[0, 1]] = o[[1, 0]]
            out[b, hk * G:(hk + 1) * G] = o
    return out


def decode_oracle(q, kc, vc, bt, lens, scale=None, **mutant) -> torch.Tensor:
    """Paged single-token attention in fp64. Keyword knobs (nsplit / rope give
    the kernel's key partition for the range mutants):
      len_delta=-1/+1             newest key ignored / slot past the end read
      bt_roll=True                block table row rotated by one entry
      last_block_wrong=True       last block fetched from another table entry
      split_first=s, split_last=s first / last key of split s dropped
      wave_first=(s, w), wave_last=(s, w)   same for a wave sub-range
      dup_boundary=s              first key of split s counted twice
      avg_combine=True            splits merged by plain average
      gqa_swap=True               first two heads of every GQA group exchanged
    """
    return _decode_core(q, kc, vc, bt, lens, scale, torch.float64, **mutant)


def decode_emulation(q, kc, vc, bt, lens, scale=None) -> torch.Tensor:
    """A correct kernel's rounding: fp32 throughout, output rounded to bf16."""
    return _decode_core(q, kc, vc, bt, lens, scale, torch.float32).to(torch.bfloat16)


# --------------------------------------------------------------------------
# prefill cases
# --------------------------------------------------------------------------
# (name, B, Hq, Hk, Sq, Skv, scale, strided)
PREFILL_CASES = [
    ("mha_129", 1, 4, 4, 129, 129, None, False),
    ("gqa4_257", 1, 8, 2, 257, 257, None, False),
    ("gqa2_300", 1, 8, 4, 300, 300, None, False),
    ("gqa8_130_450", 1, 8, 1, 130, 450, None, False),
    ("gqa4_b2_64_320", 2, 4, 1, 64, 320, None, False),
    ("gqa4_row1_200", 1, 8, 2, 1, 200, None, False),
    ("gqa2_33", 1, 4, 2, 33, 33, None, False),
    ("gqa4_257_scale02", 1, 8, 2, 257, 257, 0.2, False),
    ("gqa4_257_qkvslices", 1, 8, 2, 257, 257, None, True),
]
PROBE_ROWS = (0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256)


class PrefillCase:
    def __init__(self, name, B, Hq, Hk, Sq, Skv, scale, strided):
        self.name, self.B, self.Hq, self.Hk = name, B, Hq, Hk
        self.Sq, self.Skv, self.scale, self.strided = Sq, Skv, scale, strided
        G = Hq // Hk
        off = Skv - Sq
        gen = torch.Generator().manual_seed(1000 + Sq * 7 + Skv + Hq)
        q = (torch.randn(B, Sq, Hq, D_HEAD, generator=gen) * PEAK).to(torch.bfloat16)
        k = (torch.randn(B, Skv, Hk, D_HEAD, generator=gen) * PEAK).to(torch.bfloat16)
        v = torch.randn(B, Skv, Hk, D_HEAD, generator=gen).to(torch.bfloat16)
        rows = sorted({r for r in PROBE_ROWS if r < Sq} | {Sq - 1})
        # planted keys: (key, kv head) -> sum of weight * q[:, row, head]
        plant: Dict[Tuple[int, int], torch.Tensor] = {}

        def add(key, row, head, wgt):
            kk = (key, head // G)
            plant[kk] = plant.get(kk, 0) + wgt * q[:, row, head].float()

        self.diag_rows, self.leak_rows = [], []
        for i, r in enumerate(rows):
            h = i % Hq
            add(off + r, r, h, PROBE_IN)          # the diagonal must count
            self.diag_rows.append(r)
            if off + r + 1 < Skv:                 # diagonal+1 must not
                add(off + r + 1, r, h, PROBE_OUT)
                self.leak_rows.append(r)
        # keys either side of the 128-key tile edge, seen by the last row
        self.tile_keys = []
        h_last = (len(rows) - 1) % Hq
        for j, key in enumerate((127, 128)):
            if key < Skv - 1:
                add(key, Sq - 1, (h_last + 1 + j) % Hq, PROBE_IN)
                self.tile_keys.append(key)
        for (key, hk), vec in plant.items():
            k[:, key, hk] = vec.to(torch.bfloat16)
        self.q, self.k, self.v = q, k, v
        # a 16-key group that holds a planted key
        self.group = (112, 128) if Skv > 128 else (0, 16)

    def mutants(self) -> List[Tuple[str, dict]]:
        m: List[Tuple[str, dict]] = [
            ("causal-1", dict(causal_shift=-1)),
            ("scale/log2e", dict(scale_mul=INV_LOG2E)),
            ("drop_last_key", dict(drop=(self.Skv - 1, self.Skv, 0))),
            ("drop_tile0_late_rows", dict(drop=(0, 128, self.Sq // 2))),
            ("drop_16_keys", dict(drop=(*self.group, 0))),
            ("zero_v_16_keys", dict(zero_v=self.group)),
        ]
        m += [(f"row{r}_diag_dropped", dict(row_shift={r: -1})) for r in self.diag_rows]
        m += [(f"row{r}_sees_diag+1", dict(row_shift={r: 1})) for r in self.leak_rows]
        m += [(f"drop_key{key}", dict(drop=(key, key + 1, 0))) for key in self.tile_keys]
        # shape-only applicability
        if self.Sq >= 2:                  # the last row has no key past its diagonal
            m.append(("causal+1", dict(causal_shift=1)))
        if self.Hq // self.Hk >= 2:
            m.append(("swap_q_heads", dict(swap_q_heads=(0, 1))))
        if self.Hk >= 2:
            m.append(("roll_kv_heads", dict(roll_kv_heads=1)))
        return m

    @functools.cached_property
    def ref(self) -> torch.Tensor:
        return prefill_oracle(self.q, self.k, self.v, self.scale)

    @functools.cached_property
    def noise(self) -> float:
        return row_rel_err(prefill_emulation(self.q, self.k, self.v, self.scale), self.ref)

    @property
    def tol(self) -> float:
        return TOL_FACTOR * self.noise

    def mutant_err(self, knobs: dict) -> float:
        return row_rel_err(prefill_oracle(self.q, self.k, self.v, self.scale, **knobs), self.ref)


@functools.lru_cache(maxsize=None)
def prefill_case(name: str) -> PrefillCase:
    for c in PREFILL_CASES:
        if c[0] == name:
            return PrefillCase(*c)
    raise KeyError(name)


# --------------------------------------------------------------------------
# decode cases
# --------------------------------------------------------------------------
# (name, B, G, Hk, block_size, nsplit, maxlen, scale)
DECODE_CASES = [
    # B <= 4: 4-deep pipeline (G <= 4)
    ("b2_g1_bs16_s1", 2, 1, 4, 16, 1, 200, None),
    ("b2_g2_bs32_s3", 2, 2, 2, 32, 3, 333, None),
    ("b2_g4_bs128_s4", 2, 4, 2, 128, 4, 640, None),
    ("b2_g8_bs16_s8", 2, 8, 1, 16, 8, 500, None),
    ("b2_g1_bs128_s8", 2, 1, 2, 128, 8, 300, None),
    ("b2_g2_bs16_s4", 2, 2, 4, 16, 4, 257, None),
    ("b2_g4_bs32_s1", 2, 4, 1, 32, 1, 100, None),
    ("b2_g8_bs32_s3", 2, 8, 2, 32, 3, 640, None),
    ("b2_g4_bs16_s3", 2, 4, 2, 16, 3, 77, None),
    ("b2_g2_bs128_s1", 2, 2, 1, 128, 1, 129, None),
    # B >= 5: 2-deep pipeline
    ("b5_g1_bs32_s4", 5, 1, 4, 32, 4, 333, None),
    ("b5_g2_bs128_s8", 5, 2, 2, 128, 8, 640, None),
    ("b5_g4_bs16_s1", 5, 4, 2, 16, 1, 90, None),
    ("b5_g8_bs32_s3", 5, 8, 1, 32, 3, 500, None),
    ("b5_g1_bs16_s3", 5, 1, 2, 16, 3, 257, None),
    ("b5_g2_bs32_s1", 5, 2, 4, 32, 1, 200, None),
    ("b5_g4_bs128_s4", 5, 4, 1, 128, 4, 400, None),
    ("b5_g8_bs16_s8", 5, 8, 2, 16, 8, 300, None),
    ("b5_g4_bs32_s8", 5, 4, 2, 32, 8, 640, None),
    ("b5_g8_bs128_s1", 5, 8, 1, 128, 1, 260, None),
    ("b9_g1_bs128_s3", 9, 1, 2, 128, 3, 400, None),
    ("b9_g2_bs16_s8", 9, 2, 2, 16, 8, 333, None),
    ("b9_g4_bs32_s4", 9, 4, 2, 32, 4, 640, None),
    ("b9_g8_bs128_s8", 9, 8, 1, 128, 8, 520, None),
    ("b9_g1_bs32_s1", 9, 1, 4, 32, 1, 150, None),
    ("b9_g2_bs32_s3", 9, 2, 1, 32, 3, 257, None),
    ("b9_g4_bs16_s4", 9, 4, 1, 16, 4, 200, None),
    ("b9_g8_bs16_s1", 9, 8, 2, 16, 1, 130, None),
    ("b5_g4_bs32_s4_scale02", 5, 4, 2, 32, 4, 300, 0.2),
]
ROPE_CASES = [
    ("rope_b2_g1_bs32_s4", 2, 1, 4, 32, 4, 200, None),
    ("rope_b2_g2_bs16_s3", 2, 2, 2, 16, 3, 150, None),
    ("rope_b2_g4_bs32_s8", 2, 4, 2, 32, 8, 640, None),
    ("rope_b2_g8_bs128_s1", 2, 8, 1, 128, 1, 300, None),
    ("rope_b5_g1_bs16_s8", 5, 1, 2, 16, 8, 333, None),
    ("rope_b5_g2_bs128_s4", 5, 2, 2, 128, 4, 500, None),
    ("rope_b5_g4_bs32_s3", 5, 4, 2, 32, 3, 257, None),
    ("rope_b5_g8_bs32_s4", 5, 8, 1, 32, 4, 640, None),
    ("rope_b9_g4_bs32_s1", 9, 4, 2, 32, 1, 100, None),
    ("rope_b9_g8_bs16_s3", 9, 8, 2, 16, 3, 200, None),
    ("rope_b9_g2_bs32_s8", 9, 2, 1, 32, 8, 400, None),
    ("rope_b9_g1_bs128_s4", 9, 1, 2, 128, 4, 260, None),
]
ROPE_MAX_POS = 1024
ROPE_THETA = 500000.0


def decode_lens(B: int, bs: int, nsplit: int, maxlen: int, rot: int) -> List[int]:
    """The maximum plus edge lengths: 1, 2, bs-1, bs, bs+1, a length that
    leaves a split empty (nsplit+1 gives chunk 2), and one with n % 4 != 0 and
    n % 16 != 0. A batch of 9 holds all of them; smaller batches take a
    window of the list that `rot` rotates from case to case."""
    odd = min(maxlen - 1, 3 * bs + 7)
    while odd % 4 == 0 or odd % 16 == 0:
        odd -= 1
    pool = [1, bs + 1, nsplit + 1, bs - 1, odd, 2, bs]
    pool = [min(max(x, 1), maxlen) for x in pool]
    pool = pool[rot % 7:] + pool[:rot % 7]
    lens = [maxlen] + pool[: B - 1]
    while len(lens) < B:
        lens.append(max(1, maxlen // 2 + 3))
    return lens


def probe_keys(n: int, nsplit: int, bs: int, rope: bool) -> List[int]:
    keys = {0, n - 1}
    for _, ks, ke in split_ranges(n, nsplit):
        keys |= {ks, ke - 1}
    for _, _, ws, we in wave_ranges(n, nsplit, rope):
        keys |= {ws, we - 1}
    for kk in (bs - 1, bs):
        if kk < n:
            keys.add(kk)
    return sorted(keys)


def _rope_f32(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor):
    """Rotate-half RoPE in fp32 on [B, H, D]; only used to PLANT keys that
    line up with the roped q. The tests' reference ropes with torch_ref."""
    c = cos[pos].unsqueeze(1)
    s = sin[pos].unsqueeze(1)
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h].float(), x[..., h:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def rope_tables():
    inv = 1.0 / (ROPE_THETA ** (torch.arange(0, D_HEAD, 2, dtype=torch.float32) / D_HEAD))
    f = torch.outer(torch.arange(ROPE_MAX_POS, dtype=torch.float32), inv)
    return f.cos(), f.sin()


class DecodeCase:
    """Inputs for one paged-decode case.

    Every sequence owns ceil(n/bs) data blocks at shuffled ids plus one POISON
    block that all its unused block-table entries point at (valid ids, never
    -1): keys 2*q with large v, so a read past seq_len changes the answer
    instead of faulting. Slot n of a partial last block is poisoned likewise.
    Probe keys (see probe_keys) are dealt round-robin to q-heads, three or
    more to a head; each is set to that head's q, so the head's weight sits
    equally on its probes and losing or doubling any one of them shows.

    rope=True: `q`, `k_new`, `v_new` are the RAW kernel inputs; `kc`/`vc` is
    the cache BEFORE the call with poison in the new token's slot; `q_eff`,
    `kc_eff`, `vc_eff` (fp32) are what a correct kernel attends over, filled
    in by `set_roped` from the reference RoPE.
    """

    def __init__(self, name, B, G, Hk, bs, nsplit, maxlen, scale, rope, index):
        self.name, self.B, self.G, self.Hk, self.bs = name, B, G, Hk, bs
        self.nsplit, self.maxlen, self.scale, self.rope = nsplit, maxlen, scale, rope
        Hq = self.Hq = G * Hk
        D = D_HEAD
        lens = self.lens_list = decode_lens(B, bs, nsplit, maxlen, index)
        gen = torch.Generator().manual_seed(7000 + 31 * index + (500 if rope else 0))
        nblk = [_ceil_div(n, bs) for n in lens]
        self.max_blocks = max(nblk) + 1
        nb = sum(nblk) + B + 1
        ids = torch.randperm(nb, generator=gen).tolist()
        kc = (torch.randn(nb, bs, Hk, D, generator=gen) * PEAK).to(torch.bfloat16)
        vc = torch.randn(nb, bs, Hk, D, generator=gen).to(torch.bfloat16)
        q = (torch.randn(B, Hq, D, generator=gen) * PEAK).to(torch.bfloat16)
        bt = torch.zeros(B, self.max_blocks, dtype=torch.int32)
        self.lens = torch.tensor(lens, dtype=torch.int32)
        pos = self.lens.long() - 1
        if rope:
            self.cos, self.sin = rope_tables()
            qa = _rope_f32(q, self.cos, self.sin, pos).to(torch.bfloat16)  # aligned keys
            self.k_new = (torch.randn(B, Hk, D, generator=gen) * PEAK).to(torch.bfloat16)
            self.v_new = torch.randn(B, Hk, D, generator=gen).to(torch.bfloat16)
        else:
            qa = q
        kf, vf = kc.view(nb * bs, Hk, D), vc.view(nb * bs, Hk, D)
        slots = []
        for b in range(B):
            n = lens[b]
            mine = [ids.pop() for _ in range(nblk[b])]
            poison = ids.pop()
            bt[b, : nblk[b]] = torch.tensor(mine, dtype=torch.int32)
            bt[b, nblk[b]:] = poison

            def slot(kk, mine=mine):
                return mine[kk // bs] * bs + kk % bs

            pk = (POISON_K * qa[b, ::G].float()).to(torch.bfloat16)     # [Hk, D]
            kc[poison] = pk
            vc[poison] = (torch.randn(bs, Hk, D, generator=gen) * POISON_V).to(torch.bfloat16)
            if n % bs != 0:
                kf[slot(n - 1) + 1] = pk
                vf[slot(n - 1) + 1] = (torch.randn(Hk, D, generator=gen) * POISON_V).to(torch.bfloat16)
            pkeys = probe_keys(n, nsplit, bs, rope)
            # >= 3 probes per probed head: a lone probe holds all the weight,
            # and counting it twice would change nothing
            nh = max(1, min(Hq, len(pkeys) // 3))
            for j, kk in enumerate(pkeys):
                h = (j % nh) * Hq // nh
                if rope and kk == n - 1:
                    # roped k_new == roped q[h]: same position, same rotation
                    self.k_new[b, h // G] = q[b, h]
                else:
                    kf[slot(kk), h // G] = (PROBE_IN * qa[b, h].float()).to(torch.bfloat16)
            if rope:   # a stale read of the new token's slot must show
                kf[slot(n - 1)] = pk
                vf[slot(n - 1)] = (torch.randn(Hk, D, generator=gen) * POISON_V).to(torch.bfloat16)
            slots.append(slot(n - 1))
        self.q, self.kc, self.vc, self.bt = q, kc, vc, bt
        self.slots = torch.tensor(slots, dtype=torch.int32)
        if rope:
            self.q_eff = self.kc_eff = self.vc_eff = None
        else:
            self.q_eff, self.kc_eff, self.vc_eff = q, kc, vc

    def set_roped(self, q_roped: torch.Tensor, k_roped: torch.Tensor) -> None:
        """fp32 reference RoPE of (q, k_new) -> the tensors the oracle sees."""
        nb, bs, Hk, D = self.kc.shape
        self.q_eff = q_roped.float()
        kc = self.kc.float().clone()
        vc = self.vc.float().clone()
        kc.view(nb * bs, Hk, D)[self.slots.long()] = k_roped.float()
        vc.view(nb * bs, Hk, D)[self.slots.long()] = self.v_new.float()
        self.kc_eff, self.vc_eff = kc, vc
        for a in ("ref", "noise"):
            self.__dict__.pop(a, None)

    def mutants(self) -> List[Tuple[str, dict]]:
        """Applicability is decided by shape alone: a range mutant is listed
        when that range holds a key in at least one sequence of the batch."""
        ns, rp = self.nsplit, self.rope
        base = dict(nsplit=ns, rope=rp)
        m: List[Tuple[str, dict]] = [
            ("len-1", dict(len_delta=-1)),
            ("len+1", dict(len_delta=1)),
            ("block_table_rolled", dict(bt_roll=True)),
            ("last_block_wrong_entry", dict(last_block_wrong=True)),
        ]
        splits = sorted({s for n in self.lens_list for s, _, _ in split_ranges(n, ns)})
        waves = sorted({(s, w) for n in self.lens_list for s, w, _, _ in wave_ranges(n, ns, rp)})
        for s in splits:
            m.append((f"split{s}_first_dropped", dict(base, split_first=s)))
            m.append((f"split{s}_last_dropped", dict(base, split_last=s)))
            if s >= 1:
                m.append((f"split{s}_first_twice", dict(base, dup_boundary=s)))
        for s, w in waves:
            m.append((f"split{s}_wave{w}_first_dropped", dict(base, wave_first=(s, w))))
            m.append((f"split{s}_wave{w}_last_dropped", dict(base, wave_last=(s, w))))
        if len(splits) >= 2:
            m.append(("plain_average_combine", dict(base, avg_combine=True)))
        if self.G >= 2:
            m.append(("gqa_head_swap", dict(gqa_swap=True)))
        return m

    @functools.cached_property
    def ref(self) -> torch.Tensor:
        return decode_oracle(self.q_eff, self.kc_eff, self.vc_eff, self.bt, self.lens, self.scale)

    @functools.cached_property
    def noise(self) -> float:
        return row_rel_err(
            decode_emulation(self.q_eff, self.kc_eff, self.vc_eff, self.bt, self.lens, self.scale),
            self.ref)

    @property
    def tol(self) -> float:
        return TOL_FACTOR * self.noise

    def mutant_err(self, knobs: dict) -> float:
        return row_rel_err(
            decode_oracle(self.q_eff, self.kc_eff, self.vc_eff, self.bt, self.lens, self.scale,
                          **knobs), self.ref)


@functools.lru_cache(maxsize=None)
def decode_case(name: str) -> DecodeCase:
    for table, rope in ((DECODE_CASES, False), (ROPE_CASES, True)):
        for i, c in enumerate(table):
            if c[0] == name:
                return DecodeCase(*c, rope=rope, index=i)
    raise KeyError(name)


def rope_case_with_reference(name: str, rope_apply) -> DecodeCase:
    """A rope case whose oracle inputs come from `rope_apply` (the project's
    fp32 reference RoPE) applied to the raw q and new k."""
    c = decode_case(name)
    if c.q_eff is None:
        pos = c.lens.long() - 1
        qr, kr = rope_apply(c.q.float(), c.k_new.float(), c.cos, c.sin, pos)
        c.set_roped(qr, kr)
    return c
