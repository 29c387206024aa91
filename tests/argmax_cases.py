"""Cases, oracle, partition emulation and wrong-kernel mutants for the masked
greedy pick (sampling.hip: masked_argmax_scan / masked_argmax_finish). CPU
only, no pytest dependency; shared by tests/test_argmax_oracle.py (CPU proof
that every mutant is visible) and the GPU file tests/test_argmax_gpu.py.

Results are token indices and are compared exactly.

  * oracle: among allowed tokens whose logit is > -inf the largest by IEEE
    comparison (-0 equals +0), the lowest index among equals, -1 if none.
  * the scan runs 16 chunks of ceil(V / 128) * 8 tokens; inside a chunk a
    block pass is 2048 tokens, a wave 512, a thread 8. `tie_pairs` puts two
    equal maxima either side of each of those edges, in both halves of one
    word, at the first and last token and inside the short last chunk.
  * every pair gives rows: the lower index must win; with the lower token
    masked the higher must; -0 below +0 and +0 below -0 with every other
    allowed logit negative (the lower index must win both).
  * mask rows: the unmasked maximum disallowed, one token at V - 1, nothing
    allowed, every allowed logit -inf, an allowed -inf beside finite ones.
    Masked rows carry a random mask of their own and a disallowed decoy above
    the maximum, so neighbouring rows differ in mask and in where the maximum
    is (asserted); odd rows set the bits >= V of the last mask word.
  * `emulate` walks the kernel's own partition: float comparison with the
    lowest index inside a wave, the packed {ordered value, 0x7fffffff - idx}
    key across waves and chunks. Its knobs are the mutants. `canon=False` is
    the kernel as it stood before -0 was canonicalised where the key is packed.

A case is (V, B, masked): the rows of a vocabulary size in launches of B rows
(the list cycles to fill the last launch). A mutant must change >= 1 row of
every case it applies to.
"""

from __future__ import annotations

import collections
import functools
import zlib
from typing import Dict, List, Optional, Tuple

import numpy as np

CHUNKS, PASS, WAVE_TOKENS, UNIT = 16, 2048, 512, 8
VOCABS = (8, 40, 4104, 32776, 128256)
# B 65 crosses the finish kernel's blocks of 64; the finish kernel never sees
# V, and 65 rows of 128256 would be 16 MB
BATCHES = {8: (1, 3, 65), 40: (1, 3, 65), 4104: (1, 3, 65), 32776: (1, 3, 65), 128256: (1, 3)}
NEG_ZERO = np.float32(-0.0)


def chunk_tokens(V: int) -> int:
    return -(-V // 128) * 8


def to_bf16_values(x: np.ndarray) -> np.ndarray:
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return (u << np.uint64(16)).astype(np.uint32).view(np.float32)


def pack_mask(mask: np.ndarray, high_bits: bool = False) -> np.ndarray:
    """bool [V] -> uint32 words [ceil(V/32)]; `high_bits` sets the bits >= V."""
    V = mask.shape[0]
    pad = np.full(-(-V // 32) * 32, 1 if high_bits else 0, dtype=np.uint8)
    pad[:V] = mask
    return np.packbits(pad, bitorder="little").view(np.uint32)


def tie_pairs(V: int) -> List[Tuple[str, int, int]]:
    """(edge name, lower token, higher token), every token < V."""
    c = chunk_tokens(V)
    last0 = ((V - 1) // c) * c                       # first token of the last chunk
    cand = [("word_halves", 2, 3), ("thread_7_8", 7, 8), ("wave_511_512", 511, 512),
            ("pass_2047_2048", 2047, 2048), ("chunk_edge", c - 1, c),
            ("chunk3_thread", 3 * c + 7, 3 * c + 8), ("chunk5_wave", 5 * c + 511, 5 * c + 512),
            ("chunk9_edge", 10 * c - 1, 10 * c), ("first_last", 0, V - 1),
            ("last_chunk", last0 + 1, V - 2), ("last_chunk_edge", last0 - 1, last0)]
    inside0 = ("thread_7_8", "wave_511_512", "pass_2047_2048")   # edges inside chunk 0
    out, seen = [], set()
    for name, a, b in cand:
        if not 0 <= a < b < V or (a, b) in seen:
            continue
        if (name in inside0 and b >= c) or (name in ("chunk3_thread", "chunk5_wave") and a // c != b // c):
            continue
        seen.add((a, b))
        out.append((name, a, b))
    return out


Row = collections.namedtuple("Row", "name logits mask high_bits expect")


def oracle_row(x: np.ndarray, allowed: Optional[np.ndarray]) -> int:
    with np.errstate(invalid="ignore"):
        cand = x > -np.inf
    if allowed is not None:
        cand = cand & allowed
    if not cand.any():
        return -1
    m = x[cand].max()
    return int(np.nonzero(cand & (x == m))[0][0])


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=None)
def rows(V: int, masked: bool) -> Tuple[Row, ...]:
    out: List[Row] = []

    def add(name, x, mask, protect=()):
        r = _rng(f"{name}-{V}-{masked}")
        x = to_bf16_values(x)
        hb = False
        if masked:
            mask = mask.copy()
            free = np.setdiff1d(np.nonzero(~mask)[0], np.asarray(protect, dtype=np.int64))
            if free.size:                            # a disallowed decoy above every maximum
                x[free[r.integers(free.size)]] = 64.0
            hb = len(out) % 2 == 1
        out.append(Row(name, x, mask if masked else None, hb,
                       oracle_row(x, mask if masked else None)))

    def background(name, negative=False):
        r = _rng(f"bg-{name}-{V}-{masked}")
        x = r.standard_normal(V).astype(np.float32)
        if negative:
            x = -np.abs(x) - np.float32(0.01)
        m = r.random(V) < 0.5 if masked else np.ones(V, dtype=bool)
        return x, m

    # by variant, then by edge: consecutive rows have their maximum elsewhere
    pairs = tie_pairs(V)
    for edge, a, b in pairs:
        x, m = background(f"tie-{edge}")
        x[[a, b]] = 8.0
        m[[a, b]] = True
        add(f"tie_{edge}", x, m)
    for edge, a, b in pairs if masked else ():
        x, m = background(f"tie-{edge}")
        x[[a, b]] = 8.0
        m[b], m[a] = True, False
        add(f"tie_{edge}_lower_masked", x, m, protect=[a])
    for tag, va, vb in (("neg_then_pos", NEG_ZERO, 0.0), ("pos_then_neg", 0.0, NEG_ZERO)):
        for edge, a, b in pairs:
            x, m = background(f"zero-{edge}-{tag}", negative=True)
            x[a], x[b] = va, vb
            m[[a, b]] = True
            add(f"zero_{edge}_{tag}", x, m)
    if masked:
        x, m = background("max_disallowed")
        top = V // 3
        x[top], m[top] = 16.0, False
        add("max_disallowed", x, m, protect=[top])
        x, m = background("single_last")
        m[:] = False
        m[V - 1] = True
        add("single_token_last", x, m)
        x, m = background("nothing")
        m[:] = False
        add("nothing_allowed", x, m)
        x, m = background("all_neg_inf")
        x[m] = -np.inf
        add("allowed_all_neg_inf", x, m)
        x, m = background("neg_inf_beside")
        lowest = np.nonzero(m)[0][: max(1, min(5, int(m.sum()) - 1))]
        x[lowest] = -np.inf
        add("neg_inf_beside_finite", x, m)
    # conditions the method rests on
    for i, row in enumerate(out):
        nxt = out[(i + 1) % len(out)]
        if masked:
            assert not np.array_equal(row.mask, nxt.mask), (V, row.name)
        if row.expect >= 0 and nxt.expect >= 0:
            assert row.expect != nxt.expect, (V, row.name, nxt.name)
    return tuple(out)


def launches(V: int, B: int, masked: bool) -> List[List[int]]:
    """Row indices of every launch of the case: consecutive rows, the list
    cycled to fill the last launch."""
    n = len(rows(V, masked))
    total = -(-n // B) * B
    idx = [i % n for i in range(total)]
    return [idx[i:i + B] for i in range(0, total, B)]


def case_keys() -> List[Tuple[int, int, bool]]:
    return [(V, B, masked) for V in VOCABS for B in BATCHES[V] for masked in (False, True)]


def key_id(key) -> str:
    V, B, masked = key
    return f"v{V}-b{B}-{'mask' if masked else 'nomask'}"


# --------------------------------------------------------------------------
# the kernel's partition, with mutant knobs
# --------------------------------------------------------------------------
def _ordered(x: np.ndarray) -> np.ndarray:
    u = x.astype(np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)


def emulate(x: np.ndarray, words: Optional[np.ndarray], *, canon: bool = True,
            highest_on_tie: bool = False, mask_ignored: bool = False, mask_word_plus_1: bool = False,
            bits_reversed: bool = False, last_chunk_dropped: bool = False,
            last_unit_dropped: bool = False, boundary_token_dropped: bool = False,
            lo_hi_exchanged: bool = False, neg_inf_selectable: bool = False) -> int:
    V = x.shape[0]
    c = chunk_tokens(V)
    t = np.arange(V)
    src = t ^ 1 if lo_hi_exchanged else t
    val = x[src].astype(np.float32)
    if words is None or mask_ignored:
        allowed = np.ones(V, dtype=bool)
    else:
        w = t >> 5
        if mask_word_plus_1:
            w = w + 1
        ws = np.concatenate([words.astype(np.uint32), np.zeros(2, np.uint32)])
        bit = (t & 31) if not bits_reversed else ((t & 24) | (7 - (t & 7)))
        allowed = ((ws[w] >> bit.astype(np.uint32)) & 1).astype(bool)
    chunk, rel = t // c, t % c
    live = np.ones(V, dtype=bool)
    nchunks = -(-V // c)
    if last_chunk_dropped:
        live &= chunk < nchunks - 1
    if last_unit_dropped:
        end = np.minimum((chunk + 1) * c, V)
        live &= t < end - UNIT
    if boundary_token_dropped:
        live &= ~((rel == 0) & (chunk > 0))
    with np.errstate(invalid="ignore"):
        cand = allowed & live & ((val > -np.inf) if not neg_inf_selectable else ~np.isnan(val))
    if not cand.any():
        return -1
    # inside a wave: IEEE comparison, lowest index (a thread's passes ascend);
    # the same order as the key of the canonicalised value
    order, starts = _wave_order(V)
    tie = np.uint64(0x7FFFFFFF) - t.astype(np.uint64) if not highest_on_tie else t.astype(np.uint64)
    inner = np.where(cand, (_ordered(val + np.float32(0.0)) << np.uint64(32)) | tie, np.uint64(0))
    top = np.maximum.reduceat(inner[order], starts)
    top = top[top > 0]
    win = (top & np.uint64(0xFFFFFFFF)).astype(np.int64)
    if not highest_on_tie:
        win = 0x7FFFFFFF - win
    # across waves, blocks and chunks: the packed key
    v = val[win] + np.float32(0.0) if canon else val[win]
    outer = (_ordered(v) << np.uint64(32)) | tie[win]
    return int(win[int(np.argmax(outer))])


@functools.lru_cache(maxsize=None)
def _wave_order(V: int):
    """Tokens sorted by (chunk, wave of the block), and where each wave starts."""
    c = chunk_tokens(V)
    t = np.arange(V)
    wave = (t // c) * 4 + ((t % c) % PASS) // WAVE_TOKENS
    order = np.argsort(wave, kind="stable")
    starts = np.nonzero(np.diff(wave[order], prepend=-1))[0]
    return order, starts


MUTANTS: Dict[str, dict] = {
    "highest_index_on_ties": {"highest_on_tie": True},
    "neg_zero_below_pos_zero": {"canon": False},
    "mask_ignored": {"mask_ignored": True},
    "mask_of_row_b+1": {"mask_roll": -1},
    "mask_of_row_b-1": {"mask_roll": 1},
    "mask_word_plus_1": {"mask_word_plus_1": True},
    "bit_order_reversed": {"bits_reversed": True},
    "last_chunk_dropped": {"last_chunk_dropped": True},
    "last_unit_of_chunk_dropped": {"last_unit_dropped": True},
    "boundary_token_dropped": {"boundary_token_dropped": True},
    "lo_hi_exchanged": {"lo_hi_exchanged": True},
    "neg_inf_selectable": {"neg_inf_selectable": True},
}


def applies(name: str, key) -> bool:
    V, B, masked = key
    if name.startswith("mask_of_row"):
        return masked and B >= 2
    if name in ("mask_ignored", "bit_order_reversed"):
        return masked
    if name == "mask_word_plus_1":
        return masked and V > 32
    if name == "neg_inf_selectable":
        return masked                     # the all -inf row is a masked one
    if name == "boundary_token_dropped":
        return masked and V > chunk_tokens(V)   # a second chunk, and rows whose lower token is masked
    if name == "neg_zero_below_pos_zero":
        return V > chunk_tokens(V)        # a pair in two waves, blocks or chunks
    return True


@functools.lru_cache(maxsize=None)
def _words(V: int, masked: bool, i: int) -> Optional[np.ndarray]:
    r = rows(V, masked)[i]
    return None if r.mask is None else pack_mask(r.mask, r.high_bits)


def launch_words(V: int, masked: bool, launch: List[int]) -> Optional[np.ndarray]:
    """uint32 [B, ceil(V/32)] of one launch, None for an unmasked case."""
    if not masked:
        return None
    return np.stack([_words(V, masked, i) for i in launch])


def run_emulation(key, knobs: dict) -> List[np.ndarray]:
    """The (mutated) kernel's answer for every launch of the case."""
    V, B, masked = key
    knobs = dict(knobs)
    roll = knobs.pop("mask_roll", 0)
    rs = rows(V, masked)
    out = []
    for launch in launches(V, B, masked):
        words = launch_words(V, masked, launch)
        if roll and words is not None:
            words = np.roll(words, roll, axis=0)
        if roll:
            got = [emulate(rs[i].logits, words[j], **knobs) for j, i in enumerate(launch)]
        else:
            got = [_emulate_row(V, masked, i, tuple(sorted(knobs.items()))) for i in launch]
        out.append(np.array(got, dtype=np.int64))
    return out


@functools.lru_cache(maxsize=None)
def _emulate_row(V: int, masked: bool, i: int, knobs: tuple) -> int:
    return emulate(rows(V, masked)[i].logits, _words(V, masked, i), **dict(knobs))


def expected(key) -> List[np.ndarray]:
    V, B, masked = key
    rs = rows(V, masked)
    return [np.array([rs[i].expect for i in launch], dtype=np.int64) for launch in launches(V, B, masked)]


def rows_changed(key, knobs: dict) -> int:
    return int(sum((g != e).sum() for g, e in zip(run_emulation(key, knobs), expected(key))))
