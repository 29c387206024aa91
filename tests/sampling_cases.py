"""Cases, fp64 oracle and mutants for the seeded sampler (ops.sample_masked).

Not a test. Shared by test_sampling_oracle.py (CPU) and test_sampling_gpu.py.

The oracle implements the contract of docs/DESIGN.md "Sampling" in float64 on
exactly known operands: logits are bf16 values, an adjustment is one fp32 add,
s = fl32(z * inv_temp) is one fp32 multiply, so z and s are known exactly.

Two windows decide which comparisons are exact; both are properties of the
inputs, asserted when the cases are built:

* Filter window, 2^-14 of Z. No value level of a case has
  |M_>(v) - top_p Z| <= 2^-14 Z. The kernel's s - s_max carries at most
  88 * 2^-24 relative error into exp, exp adds <= 2 ulp, the integer sums add
  nothing of that order: below 2^-17 in all. The top level is exempt: its
  M_> is an empty sum, zero in every arithmetic, and 0 <= top_p Z holds for
  any top_p >= 0. top_p is placed at the midpoint between the two level masses
  around its nominal value. Inside the window the kept count and the smallest
  kept z must match exactly.
* Draw window, 2^-12 on the key gap. The fp32 key has an ulp of 2^-18 below
  64 and carries two one-ulp logf. A draw whose two best oracle keys differ
  by <= 2^-12 is ambiguous: any token whose oracle key is within 2^-12 of the
  best passes. Every other draw must match exactly. At most 1 % of a case's
  draws may be ambiguous. Greedy rows compare exactly known values and are
  never ambiguous.

Layout: per vocabulary size there are m specs (m divides 16). Draw d of a size
uses spec d % m at step index d // m; a launch is 16 consecutive draws, so
row b's cyclic neighbours in a launch are always specs (b +- 1) % m, which
differ from it in temperature, k, p, seed, step, mask and adjustments.
"""

from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

FILTER_WINDOW = 2.0**-14
DRAW_WINDOW = 2.0**-12
ROWS_PER_LAUNCH = 16
CHUNK_TOKENS = 8192  # a chunk size for the mutant that counts tokens from its chunk's start
INF_BITS = 0x7F800000

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10. Counter words are broadcastable integer arrays, the key
    two ints. Returns four uint64 arrays holding 32-bit words."""
    c = [np.asarray(x).astype(np.uint64) & _M32 for x in (c0, c1, c2, c3)]
    k0 = np.uint64(int(k0) & 0xFFFFFFFF)
    k1 = np.uint64(int(k1) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    sh = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c[0]
        p1 = m1 * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & _M32, (p0 >> sh) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def to_bf16_values(x: np.ndarray) -> np.ndarray:
    """Round fp32 to the nearest-even bf16 value, returned as fp32."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return (u << np.uint64(16)).astype(np.uint32).view(np.float32)


def f32_bits(v) -> int:
    return int(np.asarray([v], dtype=np.float32).view(np.int32)[0])


@dataclasses.dataclass(eq=False)
class Spec:
    name: str
    logits: np.ndarray                 # fp32 [V], bf16 values
    mask: Optional[np.ndarray] = None  # bool [V]
    temperature: float = 0.0           # 0 = greedy
    top_k: int = 0
    top_p: float = 1.0                 # nominal; the constructor moves it to a midpoint
    seed: int = 0
    step0: int = 0
    adj_tok: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.int32))
    adj_val: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.float32))
    n_steps: int = 0
    tie_at_k: bool = False             # planted: a tie group must straddle the k cut
    tie_at_p: bool = False             # planted: a tie group must straddle the nucleus boundary
    # filled by the constructor
    inv_temp: np.float32 = np.float32(0)
    margin: float = float("inf")       # nearest level distance to top_p, in units of Z
    expect: Optional["Result"] = None

    @property
    def V(self) -> int:
        return self.logits.shape[0]

    @property
    def steps(self) -> np.ndarray:
        return np.uint64(self.step0) + np.arange(self.n_steps, dtype=np.uint64)


@dataclasses.dataclass
class Result:
    tokens: np.ndarray            # int64 [N]
    gaps: np.ndarray              # float64 [N], best key minus second best
    near: Dict[int, np.ndarray]   # step index -> tokens within the draw window of the best
    kept: int
    zmin_bits: int
    exact: bool                   # greedy or empty: never ambiguous

    def ambiguous(self) -> np.ndarray:
        if self.exact:
            return np.zeros(self.tokens.shape[0], dtype=bool)
        return self.gaps <= DRAW_WINDOW


# --------------------------------------------------------------------------
# oracle
# --------------------------------------------------------------------------
FILTER_MUTANTS = ["k-1", "k+1", "k_tie_split", "p_fewer", "p_more", "p_ge", "p_all",
                  "p_tie_split"]
MASK_MUTANTS = ["filters_before_mask", "mask_ignored", "mask_word_off1", "tail_ones", "mask_row+1"]
ADJ_MUTANTS = ["adj_row+1", "adj_row-1", "adj_drop_last"]
ROW_MUTANTS = ["inv_temp_row+1", "inv_temp_row-1", "temp_after_draw"]
GEN_MUTANTS = ["step_ignored", "step_hi_ignored", "seed_hi_ignored", "word_plus1",
               "chunk_local_counter", "u_shift8"]
TIE_MUTANTS = ["tie_highest"]
MUTANTS = FILTER_MUTANTS + MASK_MUTANTS + ADJ_MUTANTS + ROW_MUTANTS + GEN_MUTANTS + TIE_MUTANTS
_NEIGHBOUR_MUTANTS = {"mask_row+1", "adj_row+1", "adj_row-1", "inv_temp_row+1", "inv_temp_row-1"}


def _mask_of(spec: Spec, mut: Optional[str], nxt: Spec) -> Optional[np.ndarray]:
    m = spec.mask
    V = spec.V
    if mut == "mask_ignored":
        return None
    if mut == "mask_row+1":
        return nxt.mask
    if m is None:
        return None
    if mut == "mask_word_off1":
        out = np.zeros(V, dtype=bool)
        out[: max(0, V - 32)] = m[32:]
        return out
    if mut == "tail_ones":
        out = m.copy()
        out[((V - 1) // 32) * 32:] = True
        return out
    return m


def _top_k_keep(z, cand, k, split):
    idx = np.nonzero(cand)[0]
    if not 0 < k < idx.shape[0]:
        return cand.copy()
    order = idx[np.lexsort((idx, -z[idx]))]  # value descending, index ascending
    keep = np.zeros_like(cand)
    if split:
        keep[order[:k]] = True
    else:
        keep[idx[z[idx] >= z[order[k - 1]]]] = True
    return keep


def _top_p_keep(z, s, base, keep_k, top_p, mut):
    """Levels and masses over `base`; returns (keep, margin, tie) where tie is
    (multiplicity of the lowest kept level, whether a cut by sort position
    would split that level)."""
    idx = np.nonzero(base)[0]
    lev, inv = np.unique(z[idx], return_inverse=True)
    lev, inv = lev[::-1], lev.shape[0] - 1 - inv  # descending
    w = np.exp(s[idx] - s[idx].max())
    mass = np.bincount(inv, weights=w, minlength=lev.shape[0])
    Z = mass.sum()
    above = np.concatenate(([0.0], np.cumsum(mass)[:-1]))
    P = float(np.float32(top_p)) * Z
    test = above + mass if mut == "p_ge" else above
    n = int(np.count_nonzero(test <= P))  # a prefix: `test` is nondecreasing
    if mut == "p_fewer":
        n -= 1
    if mut == "p_more":
        n += 1
    margin = float(np.min(np.abs(above[1:] - P)) / Z) if lev.shape[0] > 1 else float("inf")
    if n <= 0:
        return np.zeros_like(base), margin, (0, False)
    n = min(n, lev.shape[0])
    # the lowest kept level: a rule that walks a sorted list keeps member i of
    # it (ties in index order) iff the mass before it, above + i w, is <= P
    members = idx[inv == n - 1]
    w_l = mass[n - 1] / members.shape[0]
    by_pos = above[n - 1] + np.arange(members.shape[0]) * w_l <= P
    tie = (int(members.shape[0]), bool(not by_pos.all()))
    if mut == "p_tie_split":
        keep = keep_k & (z > lev[n - 1])
        keep[members[by_pos]] = True
        return keep & keep_k, margin, tie
    return keep_k & (z >= lev[n - 1]), margin, tie


@functools.lru_cache(maxsize=None)
def _filter_cached(spec_id, mut, prev_id, next_id):
    spec, prev, nxt = _BY_ID[spec_id], _BY_ID[prev_id], _BY_ID[next_id]
    V = spec.V
    atok, aval = spec.adj_tok, spec.adj_val
    if mut == "adj_row+1":
        atok, aval = nxt.adj_tok, nxt.adj_val
    elif mut == "adj_row-1":
        atok, aval = prev.adj_tok, prev.adj_val
    elif mut == "adj_drop_last":
        atok, aval = atok[:-1], aval[:-1]
    z32 = spec.logits.copy()
    z32[atok] = z32[atok] + aval  # one fp32 add
    z = z32.astype(np.float64)
    it32 = spec.inv_temp
    if mut == "inv_temp_row+1":
        it32 = nxt.inv_temp
    elif mut == "inv_temp_row-1":
        it32 = prev.inv_temp
    with np.errstate(invalid="ignore", over="ignore"):
        s = (z32 * np.float32(it32)).astype(np.float32).astype(np.float64)
        finite = z32 > -np.inf  # false for NaN
    mask = _mask_of(spec, mut, nxt)
    allowed = np.ones(V, dtype=bool) if mask is None else mask
    legacy = mut == "filters_before_mask"
    cand = finite if legacy else finite & allowed
    out = dict(z=z, s=s, it=float(it32), margin=float("inf"))
    if not cand.any():
        out.update(keep=np.zeros(0, np.int64), greedy=False)
        return out
    if not it32 > 0:
        c = np.nonzero(cand & allowed)[0]
        out.update(keep=c, greedy=True)
        return out
    k = spec.top_k + (1 if mut == "k+1" else -1 if mut == "k-1" else 0)
    keep = _top_k_keep(z, cand, k, mut == "k_tie_split")
    if spec.top_p < 1.0:
        base = cand if mut == "p_all" else keep
        keep, out["margin"], out["p_tie"] = _top_p_keep(z, s, base, keep, spec.top_p, mut)
    if legacy:
        keep = keep & allowed
    out.update(keep=np.nonzero(keep)[0], greedy=False)
    return out


_BY_ID: Dict[int, Spec] = {}


def run_oracle(spec: Spec, prev: Spec, nxt: Spec, steps: np.ndarray,
               mut: Optional[str] = None) -> Result:
    """Oracle for `spec` at each of `steps`, as row between `prev` and `nxt`."""
    for sp in (spec, prev, nxt):
        _BY_ID[id(sp)] = sp
    nb = mut in _NEIGHBOUR_MUTANTS
    f = _filter_cached(id(spec), mut, id(prev) if nb else id(spec), id(nxt) if nb else id(spec))
    idx, z, s = f["keep"], f["z"], f["s"]
    N = steps.shape[0]
    highest = mut == "tie_highest"
    if idx.shape[0] == 0:
        return Result(np.full(N, -1, np.int64), np.full(N, np.inf), {}, 0, INF_BITS, True)
    if f["greedy"]:
        zc = z[idx]
        top = idx[zc == zc.max()]
        win = int(top[-1] if highest else top[0])
        return Result(np.full(N, win, np.int64), np.zeros(N), {}, int(idx.shape[0]),
                      f32_bits(zc.max()), True)
    t = idx % CHUNK_TOKENS if mut == "chunk_local_counter" else idx
    sel = ((t + 1) & 3) if mut == "word_plus1" else (t & 3)
    seed = spec.seed & (0xFFFFFFFF if mut == "seed_hi_ignored" else (1 << 64) - 1)
    base = z[idx] if mut == "temp_after_draw" else s[idx]
    tokens = np.empty(N, np.int64)
    gaps = np.empty(N, np.float64)
    near: Dict[int, np.ndarray] = {}
    K = idx.shape[0]
    rows = max(1, (1 << 21) // K)
    for a in range(0, N, rows):
        st = steps[a:a + rows].astype(np.uint64)
        if mut == "step_ignored":
            st = np.zeros_like(st)
        elif mut == "step_hi_ignored":
            st = st & _M32
        words = philox4x32_10((t >> 2)[None, :], (st & _M32)[:, None],
                              (st >> np.uint64(32))[:, None], 0, seed, seed >> 32)
        r = np.choose(np.broadcast_to(sel[None, :], words[0].shape), words)
        if mut == "u_shift8":  # bits 8..30 of the word instead of 9..31
            u = (2.0 * ((r >> np.uint64(8)) & np.uint64(0x7FFFFF)).astype(np.float64) + 1.0) * 2.0**-24
        else:
            u = (2.0 * (r >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0**-24
        key = base[None, :] - np.log(-np.log(u))
        best = key.max(axis=1)
        if highest:
            win = K - 1 - np.argmax(key[:, ::-1], axis=1)
        else:
            win = np.argmax(key, axis=1)
        tokens[a:a + rows] = idx[win]
        if K > 1:
            second = np.partition(key, K - 2, axis=1)[:, K - 2]
            gaps[a:a + rows] = best - second
        else:
            gaps[a:a + rows] = np.inf
        for i in np.nonzero(gaps[a:a + rows] <= DRAW_WINDOW)[0]:
            near[a + int(i)] = idx[key[i] >= best[i] - DRAW_WINDOW]
    zk = z[idx]
    return Result(tokens, gaps, near, int(K), f32_bits(zk.min()), False)


def compare(res: Result, tokens: np.ndarray, lo: int = 0) -> Tuple[int, int]:
    """(wrong, ambiguous) for `tokens` against res.tokens[lo : lo + len]."""
    n = tokens.shape[0]
    exp = res.tokens[lo:lo + n]
    amb = res.ambiguous()[lo:lo + n]
    wrong = 0
    for i in np.nonzero(tokens != exp)[0]:
        if amb[i] and int(tokens[i]) in set(res.near[lo + int(i)].tolist()):
            continue
        wrong += 1
    return wrong, int(amb.sum())


def count_departures(res: Result, other: Result) -> int:
    """Non-ambiguous draws of `res` on which `other` names another token."""
    n = min(res.tokens.shape[0], other.tokens.shape[0])
    return int(np.count_nonzero((res.tokens[:n] != other.tokens[:n]) & ~res.ambiguous()[:n]))


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
def _randn_logits(V: int, scale: float, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return to_bf16_values((scale * rng.standard_normal(V)).astype(np.float32))


def _adj(pairs) -> Tuple[np.ndarray, np.ndarray]:
    pairs = sorted(pairs)
    return (np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.float32))


def _allow(V: int, toks) -> np.ndarray:
    m = np.zeros(V, dtype=bool)
    m[list(toks)] = True
    return m


def _finalize(specs: List[Spec], n_steps: int) -> List[Spec]:
    """Fix inv_temp, move top_p to the midpoint of its two neighbouring level
    masses, run the oracle and assert both windows."""
    m = len(specs)
    assert ROWS_PER_LAUNCH % m == 0
    for sp in specs:
        sp.n_steps = n_steps
        sp.inv_temp = np.float32(1.0 / sp.temperature) if sp.temperature > 0 else np.float32(0)
    for i, sp in enumerate(specs):
        if sp.temperature > 0 and sp.top_p < 1.0:
            sp.top_p = _midpoint_top_p(sp)
        prev, nxt = specs[(i - 1) % m], specs[(i + 1) % m]
        sp.expect = run_oracle(sp, prev, nxt, sp.steps)
        sp.margin = _filter_cached(id(sp), None, id(sp), id(sp))["margin"]
        if sp.temperature > 0 and sp.top_p < 1.0:
            assert sp.margin > FILTER_WINDOW, (sp.name, sp.margin)
        if sp.tie_at_k:
            st = structure(sp)
            assert st["use_k"] and st["zs"][sp.top_k] == st["zs"][sp.top_k - 1], sp.name
        if sp.tie_at_p:
            n_tie, split = _filter_cached(id(sp), None, id(sp), id(sp))["p_tie"]
            assert n_tie > 1 and split, (sp.name, n_tie, split)
        amb = int(sp.expect.ambiguous().sum())
        assert amb <= 0.01 * n_steps, (sp.name, amb)
    return specs


def _midpoint_top_p(sp: Spec) -> float:
    """top_p halfway between the largest M_>/Z <= nominal and the smallest
    above it (or 1 when every level is kept), as an fp32 value."""
    _BY_ID[id(sp)] = sp
    f = _filter_cached(id(sp), None, id(sp), id(sp))
    _filter_cached.cache_clear()
    z, s = f["z"], f["s"]
    with np.errstate(invalid="ignore"):
        cand = sp.logits.copy()
        cand[sp.adj_tok] = cand[sp.adj_tok] + sp.adj_val
        cand = cand > -np.inf
    if sp.mask is not None:
        cand &= sp.mask
    keep = _top_k_keep(z, cand, sp.top_k, False)
    idx = np.nonzero(keep)[0]
    lev, inv = np.unique(z[idx], return_inverse=True)
    inv = lev.shape[0] - 1 - inv
    w = np.exp(s[idx] - s[idx].max())
    mass = np.bincount(inv, weights=w, minlength=lev.shape[0])
    frac = np.concatenate(([0.0], np.cumsum(mass)[:-1])) / mass.sum()
    if sp.top_p < 1e-6:
        return sp.top_p  # only the exempt top level can be kept
    lo = frac[frac <= sp.top_p].max()
    hi = frac[frac > sp.top_p].min() if (frac > sp.top_p).any() else 1.0
    return float(np.float32((lo + hi) / 2))


HI = 1 << 32


@functools.lru_cache(maxsize=None)
def specs_for(V: int) -> List[Spec]:
    if V == 8:
        tie = to_bf16_values(np.array([0.5, 2.0, -1.0, 2.0, 0.25, -3.0, 1.0, 2.0], np.float32))
        lg = _randn_logits(8, 2.0, 80)
        tie_k = to_bf16_values(np.array([0.5, 1.5, -1.0, 0.25, 1.0, -2.0, 1.0, 0.75], np.float32))
        return _finalize([
            Spec("v8_temp", lg, temperature=1.0, seed=11),
            Spec("v8_greedy_tie", tie, seed=12),
            # tokens 4 and 6 tie at the k = 2 cut
            Spec("v8_mask3_k2", tie_k, tie_at_k=True, mask=_allow(8, [1, 4, 6]), temperature=0.8, top_k=2, seed=13,
                 step0=HI + 7),
            Spec("v8_none_allowed", lg, mask=_allow(8, []), temperature=1.0, seed=14),
        ], 2000)
    if V == 40:
        lg = _randn_logits(40, 2.0, 400)
        lg2 = _randn_logits(40, 3.0, 401)
        am = int(np.argmax(lg))
        inf_row = lg2.copy()
        inf_row[33] = -np.inf
        not_am = np.ones(40, bool)
        not_am[am] = False
        masked_hi = _allow(40, [2, 9, 17, 33, 38])
        return _finalize([
            Spec("v40_temp", lg, temperature=0.7, seed=0x1234),
            Spec("v40_not_argmax_p", lg, mask=not_am, temperature=1.0, top_p=0.6, seed=21),
            Spec("v40_single", lg2, mask=_allow(40, [37]), temperature=1.3, seed=22),
            Spec("v40_inf_k2", inf_row, mask=_allow(40, [3, 33, 34, 39]), temperature=0.9,
                 top_k=2, seed=23, step0=HI * 3),
            # +100 on a masked token must never win; first and last granule
            Spec("v40_adj_masked", lg, mask=masked_hi, temperature=1.0, seed=24,
                 adj_tok=_adj([(0, 100.0), (2, 1.5), (39, 100.0), (38, -0.75)])[0],
                 adj_val=_adj([(0, 100.0), (2, 1.5), (39, 100.0), (38, -0.75)])[1]),
            Spec("v40_greedy_adj", lg2, seed=25,
                 adj_tok=_adj([(int(np.argmax(lg2)), -20.0), (31, 0.125)])[0],
                 adj_val=_adj([(int(np.argmax(lg2)), -20.0), (31, 0.125)])[1]),
            Spec("v40_kbig_ptiny", lg2, temperature=1.0, top_k=50, top_p=1e-9, seed=26),
            # spec 0 again with a seed that differs in the high word only
            Spec("v40_seed_hi", lg, temperature=0.7, seed=0x1234 + (5 << 32), top_k=7, top_p=0.8),
        ], 2000)
    if V == 4104:
        lg = _randn_logits(V, 3.0, 4100)
        flat = _randn_logits(V, 1.0, 4101)
        order = np.argsort(-lg, kind="stable")
        tie_k = lg.copy()
        tie_k[order[47:53]] = lg[order[49]]      # tie group over ranks 48..53, cut at 50
        tie_p = lg.copy()
        tie_p[order[3:9]] = lg[order[5]]         # tie group where the nucleus ends
        w_tie = np.exp(tie_p.astype(np.float64) - float(tie_p.max()))
        # nominal top_p in the middle of the group's mass: by value the whole
        # group is kept, a cut by sort position would keep four of the six
        p_in_tie = float((w_tie[tie_p > tie_p[order[5]]].sum()
                          + 0.5 * w_tie[tie_p == tie_p[order[5]]].sum()) / w_tie.sum())
        pen = _adj([(int(order[0]), -30.0), (int(order[1]), -0.5), (4103, 2.0), (0, -1.0)])
        three = _allow(V, [5, 1024 * 8 // 2 + 3, 4103])
        not_am = np.ones(V, bool)
        not_am[order[0]] = False
        return _finalize([
            Spec("v4104_temp", lg, temperature=1.0, seed=31),
            Spec("v4104_k50_tie", tie_k, temperature=1.0, top_k=50, seed=32, tie_at_k=True,
                 adj_tok=_adj([(7, 0.5)])[0], adj_val=_adj([(7, 0.5)])[1]),
            Spec("v4104_p_tie", tie_p, temperature=1.0, top_p=p_in_tie, seed=33, tie_at_p=True),
            Spec("v4104_both_pen", lg, temperature=0.8, top_k=50, top_p=0.7, seed=34,
                 adj_tok=pen[0], adj_val=pen[1]),
            Spec("v4104_greedy_mask3", lg, mask=three, seed=35),
            Spec("v4104_k1", lg, temperature=1.2, top_k=1, seed=36,
                 adj_tok=_adj([(int(order[0]), -9.0)])[0], adj_val=_adj([(int(order[0]), -9.0)])[1]),
            Spec("v4104_k2_not_argmax", lg, mask=not_am, temperature=1.0, top_k=2, seed=37),
            Spec("v4104_flat_p", flat, temperature=1.5, top_p=0.5, seed=38, step0=HI + 123,
                 adj_tok=_adj([(1, 0.25), (4100, -0.25)])[0],
                 adj_val=_adj([(1, 0.25), (4100, -0.25)])[1]),
        ], 2000)
    if V == 32776:
        lg = _randn_logits(V, 3.0, 32700)
        far = _allow(V, [5, 9000, 32775])
        ends = _adj([(3, 1.0), (32770, 6.0), (16000, -2.0)])
        return _finalize([
            Spec("v32776_temp", lg, temperature=1.0, seed=41),
            Spec("v32776_both_adj", lg, temperature=0.9, top_k=50, top_p=0.8, seed=42,
                 adj_tok=ends[0], adj_val=ends[1]),
            Spec("v32776_mask3", lg, mask=far, temperature=2.0, seed=43, step0=HI * 2 + 1),
            Spec("v32776_p", lg, temperature=1.0, top_p=0.5, seed=44 + (1 << 40)),
        ], 64)
    if V == 128256:
        lg = _randn_logits(V, 3.0, 128000)
        rng = np.random.default_rng(128001)
        some = rng.random(V) < 0.3
        toks = np.sort(rng.choice(V, 256, replace=False))
        toks[0], toks[-1] = 2, V - 3
        toks = np.unique(toks)
        vals = rng.uniform(-2.0, 2.0, toks.shape[0]).astype(np.float32)
        return _finalize([
            Spec("v128k_temp", lg, temperature=1.0, seed=51),
            Spec("v128k_k50", lg, temperature=0.7, top_k=50, seed=52),
            Spec("v128k_p_mask", lg, mask=some, temperature=1.0, top_p=0.9, seed=53),
            Spec("v128k_both_adj256", lg, temperature=0.8, top_k=50, top_p=0.9, seed=54,
                 step0=HI * 7, adj_tok=toks.astype(np.int32), adj_val=vals),
        ], 64)
    raise KeyError(V)


VOCABS = [8, 40, 4104, 32776, 128256]


def launches(V: int) -> List[List[Tuple[int, int]]]:
    """Every draw of the size as launches of 16 rows of (spec index, step index)."""
    specs = specs_for(V)
    m, n = len(specs), specs[0].n_steps
    draws = [(d % m, d // m) for d in range(m * n)]
    return [draws[a:a + ROWS_PER_LAUNCH] for a in range(0, len(draws), ROWS_PER_LAUNCH)]


def mutant_steps(V: int) -> int:
    return 64 if V <= 4104 else 8


@functools.lru_cache(maxsize=None)
def mutant_results(V: int, mut: Optional[str]) -> List[Result]:
    """Oracle under `mut` for the first mutant_steps(V) steps of each spec."""
    specs = specs_for(V)
    m = len(specs)
    n = mutant_steps(V)
    return [run_oracle(sp, specs[(i - 1) % m], specs[(i + 1) % m], sp.steps[:n], mut)
            for i, sp in enumerate(specs)]


def pack_mask(mask: np.ndarray) -> np.ndarray:
    """bool [V] -> int32 words [ceil(V/32)], bit t of the row = token t."""
    V = mask.shape[0]
    pad = np.zeros(((V + 31) // 32) * 32, dtype=np.uint8)
    pad[:V] = mask
    return np.packbits(pad, bitorder="little").view(np.int32)


def structure(spec: Spec) -> dict:
    """What decides which filter mutants apply to a spec: the candidate
    values in descending order, the top-k survivors and the kept levels."""
    _BY_ID[id(spec)] = spec
    f = _filter_cached(id(spec), None, id(spec), id(spec))
    z = f["z"]
    with np.errstate(invalid="ignore"):
        cand = z > -np.inf
    if spec.mask is not None:
        cand = cand & spec.mask
    zs = np.sort(z[cand])[::-1]
    sampled = spec.temperature > 0
    use_k = sampled and 0 < spec.top_k < zs.shape[0]
    n_k = int(_top_k_keep(z, cand, spec.top_k, False).sum()) if sampled else zs.shape[0]
    return dict(
        zs=zs, sampled=sampled, use_k=use_k, use_p=sampled and spec.top_p < 1.0,
        n_after_k=n_k, kept=f["keep"].shape[0],
        kept_levels=int(np.unique(z[f["keep"]]).shape[0]),
    )


def applies(mut: str, spec: Spec) -> bool:
    """Filter mutants only: does `mut` alter the kept set of `spec` by its
    construction? The k mutants are judged on specs without top-p, so that the
    second filter cannot hide the first."""
    st = structure(spec)
    zs, k = st["zs"], spec.top_k
    if st["kept"] == 0:
        return False
    if mut == "k-1":
        return st["use_k"] and not st["use_p"] and k >= 2 and zs[k - 2] != zs[k - 1]
    if mut == "k+1":
        return st["use_k"] and not st["use_p"] and zs[k] != zs[k - 1]
    if mut == "k_tie_split":
        return st["use_k"] and not st["use_p"] and zs[k] == zs[k - 1]
    if mut == "p_fewer":
        return st["use_p"] and st["kept_levels"] >= 2
    if mut == "p_more":
        return st["use_p"] and st["kept"] < st["n_after_k"]
    if mut == "p_ge":
        return st["use_p"]
    if mut == "p_all":
        return st["use_p"] and st["use_k"]
    if mut == "p_tie_split":
        if not st["use_p"]:
            return False
        n_tie, split = _filter_cached(id(spec), None, id(spec), id(spec))["p_tie"]
        return n_tie > 1 and split
    raise KeyError(mut)
