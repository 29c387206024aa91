"""The whole-model oracle for an fp8 KV cache: teacher forcing on the
device's own codes and scales, the write criterion that forcing makes
necessary, a recorder that keeps one write event per row and checks the
cache's integrity, a simulated device for the CPU proof and the mutants on
it. No pytest dependency; see docs/KERNELS.md, "whole model, fp8 KV cache".

An ENTRY here is a write event: one row of one forward, the token and
position it was computed for and the two code rows and two scales per layer
that its forward left in its cache slot. The same prefix computed twice
(resume after preemption) is two entries with their own codes. Every entry
attends entries only, its own included, through `code * scale` exactly as
read back, so a code flip between two correct quantisers changes the input
of the oracle as well and no longer compounds through the layers.
"""

from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence

import torch

import model_cases as mc
from model_cases import MUTANT_FACTOR, TOL_FACTOR, row_rel_err  # noqa: F401 (re-exported)
from opsagent_amd.ops import torch_ref

E4M3_MAX = 448.0
SCALE_SLACK = 2.0 ** -8     # bf16 rounding of the row's absmax element
GATHER_KINDS = ("prefill", "catchup", "verify")   # rows that read bf16(code * scale)


# --------------------------------------------------------------------------
# cache contents
# --------------------------------------------------------------------------
@dataclasses.dataclass
class Cache:
    """What the entries' forwards wrote. codes uint8 [L, 2, E, Hk, D] (K, V),
    scales float32 [L, 2, E, Hk]."""
    codes: torch.Tensor
    scales: torch.Tensor

    def values(self) -> torch.Tensor:
        """code * scale, exact in fp64: [L, 2, E, Hk, D]."""
        return (self.codes.view(torch.float8_e4m3fn).double()
                * self.scales.double().unsqueeze(-1))

    def kv(self) -> list:
        d = self.values()
        return [(d[l, 0], d[l, 1]) for l in range(d.shape[0])]


def kv_of(values: torch.Tensor) -> list:
    return [(values[l, 0], values[l, 1]) for l in range(values.shape[0])]


def quant_device(x: torch.Tensor, fmax: float = E4M3_MAX):
    """The write kernel's form, x * (fmax / absmax) with scale absmax / fmax;
    torch_ref.quant_fp8 divides by the scale, so the two differ by code
    flips, which both criteria have to stand."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True).clamp_min(1e-8)
    codes = (xf * (fmax / amax)).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, (amax / fmax).squeeze(-1)


class SimDevice:
    """The `device` hook of mc.forward: quantises every layer's bf16 k and v
    as the write kernel does and hands back what a read of the cache gives.
    Keeps the rows it quantised for the write-side mutants."""

    def __init__(self):
        self.codes, self.scales, self.rows = [], [], []

    def __call__(self, layer, k, v, k_raw):
        kc, ks = quant_device(k)
        vc, vs = quant_device(v)
        self.codes.append(torch.stack([kc, vc]))
        self.scales.append(torch.stack([ks, vs]))
        self.rows.append((k.float(), v.float(), k_raw.float()))
        c = Cache(self.codes[-1][None], self.scales[-1][None]).values()[0]
        return c[0].to(k.dtype), c[1].to(k.dtype)

    def cache(self) -> Cache:
        return Cache(torch.stack(self.codes), torch.stack(self.scales))


# --------------------------------------------------------------------------
# the two criteria
# --------------------------------------------------------------------------
def judge(W, tok, pos, count, cache: Cache, roots: Sequence[int], gathered=None,
          bf16: bool = True, zeros=None, want_logits: bool = False) -> dict:
    """The forced oracle and the forced emulation of the entries, and from
    them every noise figure: N (hidden), NL (logits), N_w and N_k [L, 2, root]
    (written value, pre-quantisation row), all per root sequence. Also the
    write criterion of `cache` itself: val_ratio and scale_ratio [L, 2, E,
    Hk], each error divided by its bound."""
    KV = cache.kv()
    hid, logits, own = mc.forward(W, tok, pos, count, zeros, forced=KV, want_kv=True,
                                  want_logits=want_logits)
    ehid, elog, eown = mc.forward(W, tok, pos, count, zeros, dtype=torch.float32, rnd=bf16,
                                  forced=KV, gathered=gathered, want_kv=True,
                                  want_logits=want_logits)
    roots_t = torch.as_tensor(list(roots))
    nroot = int(roots_t.max()) + 1
    r = torch.stack([torch.stack(p) for p in own])                  # [L, 2, E, Hk, D]
    e = torch.stack([torch.stack(p) for p in eown]).float()
    qc, qs = torch_ref.quant_fp8(e)
    deq = Cache(qc, qs.view(e.shape[:-1])).values()
    rmax = r.abs().amax(dim=-1)
    w_stat = (deq - r).abs().amax(dim=-1) / rmax.clamp_min(1e-30)   # [L, 2, E, Hk]
    k_stat = (e.double() - r).abs().amax(dim=-1) / rmax.clamp_min(1e-30)
    N, NL = [], []
    L = r.shape[0]
    N_w = torch.zeros(L, 2, nroot, dtype=torch.float64)
    N_k = torch.zeros(L, 2, nroot, dtype=torch.float64)
    for g in range(nroot):
        sel = roots_t == g
        N.append(row_rel_err(ehid[sel], hid[sel]))
        NL.append(row_rel_err(elog[sel], logits[sel]) if want_logits else None)
        N_w[:, :, g] = w_stat[:, :, sel].amax(dim=(-1, -2))
        N_k[:, :, g] = k_stat[:, :, sel].amax(dim=(-1, -2))
    out = dict(N=N, NL=NL, N_w=N_w, N_k=N_k, hidden=hid, logits=logits, own=r, rmax=rmax,
               roots=roots_t)
    out["val_ratio"], out["scale_ratio"] = write_ratios(out, cache)
    return out


def write_ratios(J: dict, cache: Cache):
    """The write criterion of `cache` against the oracle rows of J: per
    entry, layer, K/V and kv-head, max|d - r| / max|r| over 4 N_w and
    |448 scale / absmax(r) - 1| over 4 N_k + 2^-8."""
    r, rmax, g = J["own"], J["rmax"], J["roots"]
    val = (cache.values() - r).abs().amax(dim=-1) / rmax.clamp_min(1e-30)
    sc = (E4M3_MAX * cache.scales.double() / rmax.clamp_min(1e-8) - 1.0).abs()
    bw = TOL_FACTOR * J["N_w"][:, :, g].unsqueeze(-1)
    bk = TOL_FACTOR * J["N_k"][:, :, g].unsqueeze(-1) + SCALE_SLACK
    return val / bw, sc / bk


def row_ratios(J: dict, rows: torch.Tensor) -> List[float]:
    """err / T of each entry's device row against the forced oracle."""
    g = J["roots"].tolist()
    return [row_rel_err(rows[i].float()[None], J["hidden"][i][None]) / (TOL_FACTOR * J["N"][g[i]])
            for i in range(rows.shape[0])]


# --------------------------------------------------------------------------
# recorder: write events and cache integrity
# --------------------------------------------------------------------------
class Fp8Recorder(mc.Recorder):
    """mc.Recorder on an engine with an fp8 cache. Record i is also write
    event i: once its forward has returned (never inside capture) the bits
    its slot holds at every layer are read back and kept, `last_write[slot]`
    points at it, and `keys[i]` lists the events in the owner's slots at
    positions 0..p. A shadow of the cache holds every slot's bits as of its
    last recorded write; after every step the live chains must equal it."""

    def __init__(self, engine):
        kv = engine.kv
        assert kv.fp8 and kv.scales is not None
        self.keys: List[List[int]] = []
        self.last_write: Dict[int, int] = {}
        self._codes: List[torch.Tensor] = []      # per forward [L, 2, n, Hk, D] on the CPU
        self._scales: List[torch.Tensor] = []
        self._shadow = self._read_all(kv)
        self.integrity_checks = 0
        self.integrity_slots = 0
        super().__init__(engine)

    @staticmethod
    def _flat(kv):
        ns = kv.num_blocks * kv.block_size
        codes = [t.view(ns, *t.shape[2:]) for pair in kv.layers for t in pair]
        scales = [t.view(ns, t.shape[2]) for pair in kv.scales for t in pair]
        return codes, scales

    def _read_all(self, kv):
        codes, scales = self._flat(kv)
        return [torch.stack(codes), torch.stack(scales)]       # [L * 2, slots, ...]

    def _read(self, idx: torch.Tensor):
        codes, scales = self._flat(self.e.kv)
        return torch.stack([c[idx] for c in codes]), torch.stack([s[idx] for s in scales])

    def _chain_slots(self, seq, n: int) -> List[int]:
        bs = self.e.kv.block_size
        return [seq.blocks[j // bs] * bs + j % bs for j in range(n)]

    def _after_rows(self, recs):
        base = len(self.records) - len(recs)
        L = len(self.e.kv.layers)
        idx = torch.tensor([r.slot for r in recs], device=self._shadow[0].device)
        assert len(set(idx.tolist())) == len(recs), "two rows of one forward share a slot"
        codes, scales = self._read(idx)
        self._shadow[0][:, idx] = codes
        self._shadow[1][:, idx] = scales
        self._codes.append(codes.cpu().view(L, 2, *codes.shape[1:]))
        self._scales.append(scales.cpu().view(L, 2, *scales.shape[1:]))
        for i, r in enumerate(recs):
            self.last_write[r.slot] = base + i
        for r in recs:
            seq = self.e.requests[r.rid].seq
            ks = []
            for j, s in enumerate(self._chain_slots(seq, r.pos + 1)):
                ev = self.last_write.get(s)
                assert ev is not None, (
                    f"{r.kind} row of request {r.rid} at position {r.pos} attends slot {s} "
                    f"(position {j}), which no recorded forward wrote")
                w = self.records[ev]
                assert w.pos == j and w.prefix[-1] == r.prefix[j], (
                    f"slot {s} was last written for token {w.prefix[-1]} at position {w.pos}; "
                    f"request {r.rid} keeps token {r.prefix[j]} at position {j} there")
                ks.append(ev)
            assert ks[-1] == self.last_write[r.slot]
            self.keys.append(ks)

    def check_integrity(self):
        """Every slot of every live chain holds the bits of its last recorded
        write, and that write was for the chain's token at that position."""
        slots: List[int] = []
        for req in self.e.running:
            seq = req.seq
            if seq is None or req.req_id not in self.prompt_len:
                continue
            chain = self._chain_slots(seq, seq.num_cached)
            for j, s in enumerate(chain):
                ev = self.last_write.get(s)
                assert ev is not None, f"request {req.req_id}: no write known for slot {s}"
                w = self.records[ev]
                assert w.pos == j and w.prefix[-1] == seq.token_ids[j], (
                    f"request {req.req_id}, position {j}: slot {s} was written for token "
                    f"{w.prefix[-1]} at position {w.pos}")
            slots.extend(chain)
        if not slots:
            return
        idx = torch.tensor(sorted(set(slots)), device=self._shadow[0].device)
        codes, scales = self._read(idx)
        for name, got, want in (("codes", codes, self._shadow[0][:, idx]),
                                ("scales", scales, self._shadow[1][:, idx])):
            if not torch.equal(got.view(torch.uint8), want.view(torch.uint8)):
                bad = (got != want).flatten(2).any(dim=2).nonzero()[0].tolist()
                raise AssertionError(
                    f"cache {name} of slot {int(idx[bad[1]])}, layer {bad[0] // 2} "
                    f"{'KV'[bad[0] % 2]} changed after its last recorded write")
        self.integrity_checks += 1
        self.integrity_slots += len(idx)

    def step(self):
        super().step()
        self.check_integrity()

    def cache(self) -> Cache:
        return Cache(torch.cat(self._codes, dim=2), torch.cat(self._scales, dim=2))


def entries_of(rec: Fp8Recorder):
    """tokens, positions, count matrix and root sequence number per entry."""
    n = len(rec.records)
    assert len(rec.keys) == n
    tok = [r.prefix[-1] for r in rec.records]
    pos = torch.tensor([r.pos for r in rec.records], dtype=torch.long)
    count = torch.zeros(n, n, dtype=torch.float64)
    roots: Dict[int, int] = {}
    root_of = []
    for i, ks in enumerate(rec.keys):
        count[i, ks] = 1
        root_of.append(roots.setdefault(ks[0], len(roots)))
    return tok, pos, count, root_of


def check_recorded(W, rec: Fp8Recorder, bf16: bool, values: Optional[torch.Tensor] = None):
    """Both criteria on everything the recorder holds. `values` replaces
    what the entries attend (the read-side mutants of the GPU self-check);
    the write criterion always judges the recorded cache."""
    tok, pos, count, root_of = entries_of(rec)
    cache = rec.cache()
    gathered = torch.tensor([r.kind in GATHER_KINDS for r in rec.records])
    if values is None:
        J = judge(W, tok, pos, count, cache, root_of, gathered, bf16, want_logits=True)
    else:
        J = judge(W, tok, pos, count, _Values(cache, values), root_of, gathered, bf16,
                  want_logits=True)
    J["ratio"] = row_ratios(J, torch.stack([r.row for r in rec.records]).cpu())
    J["where"] = list(range(len(tok)))
    J["root_of"] = root_of
    return J


class _Values(Cache):
    """A cache whose read side gives other values than its bits."""

    def __init__(self, cache: Cache, values: torch.Tensor):
        super().__init__(cache.codes, cache.scales)
        self._read_values = values

    def kv(self):
        return kv_of(self._read_values)


# --------------------------------------------------------------------------
# simulated device on the scripted scenarios
# --------------------------------------------------------------------------
def gathered_rows(S: mc.Scripted) -> torch.Tensor:
    """Entries computed by a prefill-form forward (everything but decode)."""
    return ~S.decode_rows()


def roots_of(S: mc.Scripted) -> List[int]:
    roots: Dict[int, int] = {}
    return [roots.setdefault(ks[0], len(roots)) for ks in S.script.keys]


def simulate(W, S: mc.Scripted):
    """The emulation unforced, attending its own quantised cache. Returns
    (hidden rows, SimDevice)."""
    dev = SimDevice()
    sc = S.script
    hid, _ = mc.forward(W, sc.tok, sc.positions(), sc.count(), dtype=torch.float32, rnd=True,
                        device=dev, gathered=gathered_rows(S), want_logits=False)
    return hid, dev


def cold_rows(S: mc.Scripted) -> torch.Tensor:
    """Entries of a prefill with no past: each sequence's prompt up to its
    first multi-token group, entries shared with an earlier sequence left
    out."""
    cold = torch.zeros(len(S.script), dtype=torch.bool)
    seen = set()
    for s, (c, n) in enumerate(zip(S.chains, S.prompt)):
        end = min([a for q, a, _ in S.groups if q == s] + [n])
        new = [i for i in c[:end] if i not in seen]
        if len(new) == end:
            cold[new] = True
        seen.update(c)
    return cold


READ_MUTANTS = [
    "v_scale_ignored", "kv_scales_exchanged", "scale_slot+1", "scale_next_head", "scale_head0",
    "scales_prev_layer", "cache_prev_layer", "own_key_unquantised", "cold_prefill_unquantised",
    # the bf16 suite's, on the forced oracle
    "chunk_ignores_past", "past_blocks_rolled", "pos+1", "pos-1", "next_row_block_table",
    "cu_q_off", "no_causal_appended", "newest_key_dropped",
]
WRITE_MUTANTS = [
    "k_unroped", "k_other_head", "k_ungained", "kv_slices_exchanged", "scale_fnuz_240",
    "scale_previous_occupant", "codes_token+1", "codes_token-1",
]


def mutate_values(cache: Cache, name: str) -> torch.Tensor:
    """[L, 2, E, Hk, D] values a wrong read side makes of a correct cache."""
    f = cache.codes.view(torch.float8_e4m3fn).double()
    s = cache.scales.double()
    if name == "v_scale_ignored":
        s = s.clone()
        s[:, 1] = 1.0
    elif name == "kv_scales_exchanged":
        s = s.flip(1)
    elif name == "scale_slot+1":
        s = s.roll(-1, 2)
    elif name == "scale_next_head":
        s = s.roll(-1, 3)
    elif name == "scale_head0":
        s = s[..., :1].expand_as(s)
    elif name == "scales_prev_layer":
        s = torch.cat([s[:1], s[:-1]])
    elif name == "cache_prev_layer":
        f, s = torch.cat([f[:1], f[:-1]]), torch.cat([s[:1], s[:-1]])
    else:
        raise KeyError(name)
    return f * s.unsqueeze(-1)


def read_mutant_margin(S: mc.Scripted, name: str, W: dict, cache: Cache, ref: torch.Tensor,
                       N: float) -> Optional[float]:
    """err(mutant, forced oracle) / T, None where the scenario has no such
    step."""
    sc = S.script
    kw = dict(pos=sc.positions(), count=sc.count(), forced=cache.kv())
    if name == "own_key_unquantised":
        kw["alt"] = (torch.eye(len(sc), dtype=torch.bool), None)
    elif name == "cold_prefill_unquantised":
        cold = cold_rows(S)
        if not bool(cold.any()):
            return None
        kw["alt"] = (cold[:, None] & (sc.count() > 0), None)
    elif name in mc.ROW_MUTANTS:
        m = mc.mutant_kwargs(S, name, W)
        if m is None:
            return None
        kw.update(pos=m["pos"], count=m["count"], zeros=m["zeros"])
    else:
        kw["forced"] = kv_of(mutate_values(cache, name))
    got, _ = mc.forward(W, sc.tok, want_logits=False, **kw)
    return row_rel_err(got, ref) / (TOL_FACTOR * N)


def mutate_writes(dev: SimDevice, name: str) -> Cache:
    """The cache a wrong write side leaves."""
    codes, scales = [], []
    for k, v, k_raw in dev.rows:
        fmax = E4M3_MAX
        if name == "k_unroped":
            k = k_raw
        elif name == "k_other_head":
            k = k.roll(1, 1)
        elif name == "k_ungained":
            k = k / mc.GAIN
        elif name == "kv_slices_exchanged":
            k, v = v, k_raw
        elif name == "scale_fnuz_240":
            fmax = 240.0
        kc, ks = quant_device(k, fmax)
        vc, vs = quant_device(v, fmax)
        c, s = torch.stack([kc, vc]), torch.stack([ks, vs])
        if name == "scale_previous_occupant":
            s = s.roll(1, 1)
        elif name == "codes_token+1":
            c, s = c.roll(-1, 1), s.roll(-1, 1)
        elif name == "codes_token-1":
            c, s = c.roll(1, 1), s.roll(1, 1)
        codes.append(c)
        scales.append(s)
    return Cache(torch.stack(codes), torch.stack(scales))


def write_mutant_margin(J: dict, dev: SimDevice, name: str) -> float:
    """The larger of the two write figures over its bound, largest entry."""
    val, sc = write_ratios(J, mutate_writes(dev, name))
    return float(torch.maximum(val, sc).max())
