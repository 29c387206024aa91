"""fp64 oracle, wrong-kernel mutants and probe-planting inputs for the paged
APPEND attention tests (B sequences, L_b new query tokens each, attending the
paged cache in place). CPU only, no pytest dependency; the method is that of
tests/attention_oracle.py, whose metric, constants and decode cases it reuses.

The oracle is per (sequence, token) decode attention at length p + 1, with
p = n - L + j the position of new token j. Inputs are PEAKED, unused block
table entries and slot n of a partial block hold POISON, and probes are
planted where only one row or one range boundary looks:

  * past keys (index < n - L): the first and last key of every split and of
    every wave sub-range of the kernel's OWN partition (ops.append_partition),
    plus keys 0, n-L-1, bs-1, bs — each set to PROBE_IN * q of a row that
    also owns a diagonal probe, so that row's weight is shared;
  * new token j: its diagonal key p_j is PROBE_IN * q[j, h] on kv-head 0, and
    for j < L-1 key p_j + 1 is PROBE_OUT * q[j, h'] on kv-head 1 (must not
    count). With Hk = 1 they alternate: IN on even j, OUT on odd j.
"""

from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import torch

from attention_oracle import (
    D_HEAD, MUTANT_FACTOR, PEAK, POISON_K, POISON_V, PROBE_IN, PROBE_OUT,
    TOL_FACTOR, _ceil_div, row_rel_err,
)
from opsagent_amd import ops


# (name, B, G, Hk, block_size, nsplit, lens, q_lens, scale)
APPEND_CASES = [
    # R = L*G of 20 (waves split keys) and 36 (waves split row tiles)
    ("g4_hk2_bs32_s3", 2, 4, 2, 32, 3, [77, 333], [5, 9], None),
    # L at the cap at G = 8: 128 rows, 8 row tiles
    ("g8_hk1_bs16_s4", 2, 8, 1, 16, 4, [130, 40], [16, 3], None),
    # G = 1 (one row tile per block), n == L: token 0 sees only itself
    ("g1_hk4_bs128_s4", 3, 1, 4, 128, 4, [260, 129, 9], [2, 8, 9], None),
    # an L = 1 row beside an L > 1 row
    ("g2_hk2_bs32_s2", 2, 2, 2, 32, 2, [33, 64], [1, 4], None),
    # a mixed decode step: one catch-up row, the rest L = 1; n = 1; an
    # nsplit that leaves splits empty
    ("mixed_g4_hk2_bs16_s4", 5, 4, 2, 16, 4, [500, 17, 200, 1, 48], [9, 1, 1, 1, 1], None),
    # cap per G; new tokens straddle a block boundary (84..99 over 96)
    ("cap_g1_hk2_bs16_s2", 1, 1, 2, 16, 2, [100], [16], None),
    # R = 32 exactly; n - L = 192 on a multiple of 16; n == L at the cap
    ("cap_g2_hk2_bs32_s3", 2, 2, 2, 32, 3, [208, 16], [16, 16], None),
    ("cap_g4_hk1_bs32_s4_scale02", 2, 4, 1, 32, 4, [300, 70], [16, 5], 0.2),
    # R = 3 and R = 10: off a multiple of 16
    ("g1_l3_hk2_bs16_s2", 2, 1, 2, 16, 2, [50, 35], [3, 1], None),
    ("g2_l5_hk2_bs32_s3", 1, 2, 2, 32, 3, [131], [5], None),
    # new tokens 28..39 straddle the split boundary at 30: rows 0, 1 are
    # masked inside split 2 and find split 3 empty
    ("straddle_split_g2_hk2_bs32_s4", 2, 2, 2, 32, 4, [40, 90], [12, 2], None),
    # new tokens 188..199 straddle the wave sub-range boundary at 196
    ("straddle_wave_g2_hk2_bs16_s2", 1, 2, 2, 16, 2, [200], [12], None),
    # row-tile mode (R = 64), new tokens 114..129 straddle the split at 119
    ("straddle_rows_g4_hk2_bs16_s8", 1, 4, 2, 16, 8, [130], [16], None),
    # blocks under 16 keys: the kernel's per-lane block-table path
    ("g4_hk2_bs8_s3", 2, 4, 2, 8, 3, [77, 45], [5, 1], None),
    ("g2_hk2_bs4_s2", 2, 2, 2, 4, 2, [70, 9], [3, 9], None),
]


def partition(n: int, L: int, G: int, nsplit: int, max_q: int):
    """(splits, subs): non-empty (s, kstart, kend) and (s, w, start, end)
    from the kernel's own partition."""
    parts = ops.append_partition(n, L, G, nsplit, max_q)
    chunk = _ceil_div(max(n, 0), nsplit)
    splits, subs = [], []
    for s, sub in enumerate(parts):
        ks, ke = s * chunk, min(n, s * chunk + chunk)
        if ke > ks:
            splits.append((s, ks, ke))
        for w, (ws, we) in enumerate(sub):
            subs.append((s, w, ws, we))
    return splits, subs


def _append_core(q, kc, vc, bt, lens, cu, scale, dtype, round_p, *, nsplit=1,
                 max_q=None, causal_shift=0, no_causal=False, drop_new=False,
                 roll_out=False, cu_off=False, gqa_swap=False, bt_roll=False,
                 last_block_wrong=False, range_key=None, avg_combine=False,
                 beyond_counted=False):
    T, Hq, D = q.shape
    nb, bs, Hk, _ = kc.shape
    G = Hq // Hk
    B = len(lens)
    sc = D ** -0.5 if scale is None else scale
    kflat = kc.reshape(nb * bs, Hk, D).to(dtype)
    vflat = vc.reshape(nb * bs, Hk, D).to(dtype)
    qd = q.to(dtype)
    cu = [int(x) for x in cu]
    qlens = [cu[b + 1] - cu[b] for b in range(B)]
    max_q = max(qlens) if max_q is None else max_q
    out = torch.zeros(T, Hq, D, dtype=dtype)
    neg = torch.tensor(float("-inf"), dtype=dtype)
    for b in range(B):
        n, L = int(lens[b]), qlens[b]
        t0 = cu[b]
        tq = cu[b - 1] if (cu_off and b >= 1) else t0   # cu_q read one entry off
        na = n + 1                       # one slot past the end: poison
        pos = torch.arange(na)
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
        K, V = kflat[slot], vflat[slot]              # [na, Hk, D]
        limit = torch.arange(L) + (n - L) + causal_shift
        if no_causal:
            limit = torch.full((L,), n - 1)
        if drop_new:
            limit = torch.full((L,), n - L - 1)
        splits, subs = partition(n, L, G, nsplit, max_q)
        visible = pos[None, :] <= limit[:, None]     # [L, na]
        if beyond_counted:   # a split wholly past the row's limit is unmasked
            for _, ks, ke in splits:
                rows = limit < ks
                visible[rows, ks:ke] = True
        w = torch.ones(na, dtype=dtype)
        if range_key is not None:
            kind, idx, which, weight = range_key
            table = ({s: (ks, ke) for s, ks, ke in splits} if kind == "split"
                     else {(s, wv): (ws, we) for s, wv, ws, we in subs})
            if idx in table:
                lo, hi = table[idx]
                w[lo if which == "first" else hi - 1] = weight
        qb = qd[tq:tq + L]                           # [L, Hq, D]
        ob = torch.zeros(L, Hq, D, dtype=dtype)
        for hk in range(Hk):
            qg = qb[:, hk * G:(hk + 1) * G]          # [L, G, D]
            s = torch.einsum("lgd,nd->lgn", qg, K[:, hk]) * sc
            vv = V[:, hk]

            def soft(lo, hi):
                """(o, any) of keys [lo, hi): o [L, G, D] normalised."""
                live = (visible[:, lo:hi] & (w[lo:hi] > 0)[None, :])   # [L, k]
                ss = torch.where(live[:, None, :], s[:, :, lo:hi], neg)
                mx = ss.amax(dim=2, keepdim=True)
                mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
                p = torch.exp(ss - mx) * w[lo:hi]
                l = p.sum(dim=2, keepdim=True)
                if round_p:
                    p = p.to(torch.bfloat16).to(dtype)
                o = torch.einsum("lgn,nd->lgd", p, vv[lo:hi])
                o = torch.where(l > 0, o / l.clamp_min(1e-300), torch.zeros_like(o))
                return o, live.any(dim=1)

            if avg_combine:
                acc = torch.zeros(L, G, D, dtype=dtype)
                cnt = torch.zeros(L, dtype=dtype)
                for _, ks, ke in splits:
                    o, has = soft(ks, ke)
                    acc += o * has[:, None, None].to(dtype)
                    cnt += has.to(dtype)
                o = acc / cnt.clamp_min(1)[:, None, None]
            else:
                o, _ = soft(0, na)
            if gqa_swap and G >= 2:
                o = o.clone()
                o[:, [0, 1]] = o[:, [1, 0]]
            ob[:, hk * G:(hk + 1) * G] = o
        if roll_out and L >= 2:
            ob = ob.roll(1, dims=0)
        out[t0:t0 + L] = ob
    return out


def append_oracle(q, kc, vc, bt, lens, cu, scale=None, **mutant) -> torch.Tensor:
    """Paged append attention in fp64. Keyword knobs give one wrong kernel
    (nsplit / max_q give the kernel's key partition for the range mutants):
      causal_shift=-1/+1          every token's limit off by one
      no_causal=True              every new token sees all n keys
      drop_new=True               every new token sees only the n - L past keys
      roll_out=True               outputs rolled by one token within a sequence
      cu_off=True                 cu_q read one entry off (q of the previous row)
      gqa_swap=True               first two heads of every GQA group exchanged
      bt_roll / last_block_wrong  as for decode
      range_key=(kind, idx, which, weight)   first/last key of a split
                                  ("split", s) or wave sub-range ("wave", (s, w))
                                  dropped (weight 0) or doubled (weight 2)
      avg_combine=True            splits merged by plain average
      beyond_counted=True         a split wholly past a row's limit is counted
    """
    return _append_core(q, kc, vc, bt, lens, cu, scale, torch.float64, False, **mutant)


def append_emulation(q, kc, vc, bt, lens, cu, scale=None) -> torch.Tensor:
    """A correct kernel's rounding: fp32 throughout, P rounded to bf16 before
    P.V while the row sum keeps the unrounded P, output rounded to bf16."""
    return _append_core(q, kc, vc, bt, lens, cu, scale, torch.float32, True).to(torch.bfloat16)


class AppendCase:
    """Inputs for one append case. Every sequence owns ceil(n/bs) data blocks
    at shuffled ids plus one POISON block behind all its unused block-table
    entries; slot n of a partial last block is poisoned likewise. `qkv` is a
    [T, (Hq+2Hk)*128] buffer and `q` its strided head-slice view."""

    def __init__(self, name, B, G, Hk, bs, nsplit, lens, qlens, scale, index):
        self.name, self.B, self.G, self.Hk, self.bs = name, B, G, Hk, bs
        self.nsplit, self.scale = nsplit, scale
        self.lens_list, self.qlens = list(lens), list(qlens)
        assert len(lens) == B and len(qlens) == B
        assert all(1 <= L <= n for n, L in zip(lens, qlens))
        Hq = self.Hq = G * Hk
        D = D_HEAD
        self.max_q = max(qlens)
        T = self.T = sum(qlens)
        gen = torch.Generator().manual_seed(9000 + 37 * index)
        nblk = [_ceil_div(n, bs) for n in lens]
        self.max_blocks = max(nblk) + 1
        nb = sum(nblk) + B + 1
        ids = torch.randperm(nb, generator=gen).tolist()
        kc = (torch.randn(nb, bs, Hk, D, generator=gen) * PEAK).to(torch.bfloat16)
        vc = torch.randn(nb, bs, Hk, D, generator=gen).to(torch.bfloat16)
        qkv = (torch.randn(T, (Hq + 2 * Hk) * D, generator=gen) * PEAK).to(torch.bfloat16)
        q = qkv[:, : Hq * D].view(T, Hq, D)
        bt = torch.zeros(B, self.max_blocks, dtype=torch.int32)
        cu = [0]
        for L in qlens:
            cu.append(cu[-1] + L)
        kf, vf = kc.view(nb * bs, Hk, D), vc.view(nb * bs, Hk, D)
        for b in range(B):
            n, L, t0 = lens[b], qlens[b], cu[b]
            mine = [ids.pop() for _ in range(nblk[b])]
            poison = ids.pop()
            bt[b, : nblk[b]] = torch.tensor(mine, dtype=torch.int32)
            bt[b, nblk[b]:] = poison

            def slot(kk, mine=mine):
                return mine[kk // bs] * bs + kk % bs

            q_last = q[t0 + L - 1]                                      # [Hq, D]
            pk = (POISON_K * q_last[::G].float()).to(torch.bfloat16)    # [Hk, D]
            kc[poison] = pk
            vc[poison] = (torch.randn(bs, Hk, D, generator=gen) * POISON_V).to(torch.bfloat16)
            if n % bs != 0:
                kf[slot(n - 1) + 1] = pk
                vf[slot(n - 1) + 1] = (torch.randn(Hk, D, generator=gen) * POISON_V).to(torch.bfloat16)
            # decode-style probes on the past keys, aligned with the last token
            past = n - L
            splits, subs = partition(n, L, G, nsplit, self.max_q)
            keys = {0, past - 1, bs - 1, bs}
            for _, ks, ke in splits:
                keys |= {ks, ke - 1}
            for _, _, ws, we in subs:
                keys |= {ws, we - 1}
            pkeys = sorted(k for k in keys if 0 <= k < past)
            # Each past probe is aligned with ONE row that also owns a
            # diagonal probe — (token j, head j % G) on kv-head 0 — so that
            # row's weight sits equally on its probes and losing or doubling
            # any of them shows (a lone probe holds all the weight; counting
            # it twice would change nothing). Rows whose diagonal key is a
            # range boundary come first, then the last token; two or more
            # past probes to a row.
            diag = [j for j in range(L) if Hk >= 2 or j % 2 == 0]
            edge = [j for j in diag if past + j in keys]
            order = edge + [j for j in reversed(diag) if j not in edge]
            order = order[: max(1, len(pkeys) // 2)]
            for i, kk in enumerate(pkeys):
                j = order[i % len(order)]
                kf[slot(kk), 0] = (PROBE_IN * q[t0 + j, j % G].float()).to(torch.bfloat16)
            # probes on the new keys
            for j in range(L):
                p = past + j
                if Hk >= 2:
                    kf[slot(p), 0] = (PROBE_IN * q[t0 + j, j % G].float()).to(torch.bfloat16)
                    if j < L - 1:
                        kf[slot(p + 1), 1] = (
                            PROBE_OUT * q[t0 + j, G + j % G].float()).to(torch.bfloat16)
                elif j % 2 == 0:
                    kf[slot(p), 0] = (PROBE_IN * q[t0 + j, j % G].float()).to(torch.bfloat16)
                    if j < L - 1:
                        kf[slot(p + 1), 0] = (
                            PROBE_OUT * q[t0 + j, (j + 1) % G].float()).to(torch.bfloat16)
        self.qkv, self.q, self.kc, self.vc, self.bt = qkv, q, kc, vc, bt
        self.lens = torch.tensor(lens, dtype=torch.int32)
        self.cu = torch.tensor(cu, dtype=torch.int32)

    def mutants(self) -> List[Tuple[str, dict]]:
        """Applicability is decided by shape alone."""
        base = dict(nsplit=self.nsplit, max_q=self.max_q)
        m: List[Tuple[str, dict]] = [
            ("causal-1", dict(causal_shift=-1)),
            ("causal+1", dict(causal_shift=1)),
            ("new_keys_dropped", dict(drop_new=True)),
            ("block_table_rolled", dict(bt_roll=True)),
            ("last_block_wrong_entry", dict(last_block_wrong=True)),
        ]
        if max(self.qlens) >= 2:
            m.append(("no_causal_among_new", dict(no_causal=True)))
            m.append(("outputs_rolled", dict(roll_out=True)))
        if self.B >= 2:
            m.append(("cu_q_one_entry_off", dict(cu_off=True)))
        if self.G >= 2:
            m.append(("gqa_head_swap", dict(gqa_swap=True)))
        splits, waves, beyond = set(), set(), False
        nonempty = 0
        for n, L in zip(self.lens_list, self.qlens):
            sp, sb = partition(n, L, self.G, self.nsplit, self.max_q)
            splits |= {s for s, _, _ in sp}
            waves |= {(s, w) for s, w, _, _ in sb}
            nonempty = max(nonempty, len(sp))
            beyond |= any(ks > n - L for _, ks, _ in sp)
        for s in sorted(splits):
            m.append((f"split{s}_first_dropped", dict(base, range_key=("split", s, "first", 0))))
            m.append((f"split{s}_last_dropped", dict(base, range_key=("split", s, "last", 0))))
            if s >= 1:
                m.append((f"split{s}_first_twice", dict(base, range_key=("split", s, "first", 2))))
        for s, w in sorted(waves):
            m.append((f"split{s}_wave{w}_first_dropped",
                      dict(base, range_key=("wave", (s, w), "first", 0))))
            m.append((f"split{s}_wave{w}_last_dropped",
                      dict(base, range_key=("wave", (s, w), "last", 0))))
            if (s, w) != (0, 0):
                m.append((f"split{s}_wave{w}_first_twice",
                          dict(base, range_key=("wave", (s, w), "first", 2))))
        if nonempty >= 2:
            m.append(("plain_average_combine", dict(base, avg_combine=True)))
        if beyond:
            m.append(("split_beyond_limit_counted", dict(base, beyond_counted=True)))
        return m

    def _run(self, fn, **knobs):
        return fn(self.q, self.kc, self.vc, self.bt, self.lens_list, self.cu.tolist(),
                  self.scale, **knobs)

    @functools.cached_property
    def ref(self) -> torch.Tensor:
        return self._run(append_oracle)

    @functools.cached_property
    def noise(self) -> float:
        return row_rel_err(self._run(append_emulation), self.ref)

    @property
    def tol(self) -> float:
        return TOL_FACTOR * self.noise

    def mutant_err(self, knobs: dict) -> float:
        return row_rel_err(self._run(append_oracle, **knobs), self.ref)


@functools.lru_cache(maxsize=None)
def append_case(name: str) -> AppendCase:
    for i, c in enumerate(APPEND_CASES):
        if c[0] == name:
            return AppendCase(*c, index=i)
    raise KeyError(name)


APPEND_CASE_NAMES = [c[0] for c in APPEND_CASES]
__all__ = [
    "APPEND_CASES", "APPEND_CASE_NAMES", "AppendCase", "append_case", "append_oracle",
    "append_emulation", "partition", "MUTANT_FACTOR", "TOL_FACTOR", "row_rel_err",
]
