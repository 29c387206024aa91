"""masked_argmax (sampling.hip) on a real MI355X (`pytest -m gpu`) against the
oracle of tests/argmax_cases.py: token indices, compared exactly.

Rows, launches and the wrong kernels that the rows are proven to catch come
from tests/argmax_cases.py and tests/test_argmax_oracle.py. The raw C entry is
called with `ws` filled with ones (the launcher's memset must be real) and
`out` inside a patterned buffer whose other bits must not change; every launch
runs twice and must give identical bits. Each case prints
`ARGMAX <case> rows mismatches` (visible with -s).
"""

import functools

import numpy as np
import pytest
import torch

import argmax_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 16
PATTERN = -0x5A5A5A5B
KEYS = ac.case_keys()


def _lib():
    from opsagent_amd.ops import hip_lib

    return hip_lib, hip_lib.get_lib()


@functools.lru_cache(maxsize=None)
def _bf16_rows(V, masked):
    """Every row of a size as bf16 on the CPU; a launch uploads its own rows."""
    rs = ac.rows(V, masked)
    return torch.from_numpy(np.stack([r.logits for r in rs])).to(torch.bfloat16)


def run_launch(logits, words, V):
    """One launch through oa_masked_argmax; returns (rc, tokens int64 numpy)."""
    hip_lib, lib = _lib()
    B = logits.shape[0]
    ws = torch.full((B,), 0x0101010101010101, dtype=torch.int64, device=DEV)
    buf = torch.full((B + 2 * PAD,), PATTERN, dtype=torch.int32, device=DEV)
    out = buf[PAD:PAD + B]
    mask = None if words is None else torch.from_numpy(words.view(np.int32).copy()).to(DEV)
    rc = lib.oa_masked_argmax(hip_lib.current_stream_ptr(), logits.data_ptr(),
                              None if mask is None else mask.data_ptr(), ws.data_ptr(),
                              out.data_ptr(), B, V)
    torch.cuda.synchronize()
    got = buf.cpu()
    assert (got[:PAD] == PATTERN).all() and (got[PAD + B:] == PATTERN).all(), "wrote outside out"
    return rc, got[PAD:PAD + B].numpy().astype(np.int64)


def run_case(key, roll=0):
    V, B, masked = key
    all_rows = _bf16_rows(V, masked)
    got = []
    for launch in ac.launches(V, B, masked):
        logits = all_rows[torch.tensor(launch)].to(DEV).contiguous()
        words = ac.launch_words(V, masked, launch)
        if roll:
            words = np.roll(words, roll, axis=0)
        rc, a = run_launch(logits, words, V)
        assert rc == 0, f"{ac.key_id(key)}: rc={rc}"
        rc, b = run_launch(logits, words, V)
        assert rc == 0 and np.array_equal(a, b), f"{ac.key_id(key)}: two launches differ"
        got.append(a)
    return got


@pytest.mark.parametrize("key", KEYS, ids=[ac.key_id(k) for k in KEYS])
def test_masked_argmax(key):
    V, B, masked = key
    got, want = run_case(key), ac.expected(key)
    rs = ac.rows(V, masked)
    bad = [(rs[i].name, int(g), int(w))
           for launch, gl, wl in zip(ac.launches(V, B, masked), got, want)
           for i, g, w in zip(launch, gl, wl) if g != w]
    n = sum(len(w) for w in want)
    print(f"\nARGMAX {ac.key_id(key)} rows={n} mismatches={len(bad)}")
    assert not bad, f"{ac.key_id(key)}: (row, got, oracle) {bad[:8]}"


def test_public_wrapper_follows_the_oracle():
    from opsagent_amd import ops

    V = 4104
    for masked in (False, True):
        rs = ac.rows(V, masked)
        idx = list(range(len(rs)))
        words = ac.launch_words(V, masked, idx)
        mask = None if words is None else torch.from_numpy(words.view(np.int32).copy()).to(DEV)
        got = ops.greedy_sample_masked(_bf16_rows(V, masked).to(DEV), mask)
        assert got.dtype == torch.int32 and got.cpu().tolist() == [r.expect for r in rs]


def test_launcher_rejects_v_not_multiple_of_8():
    logits = torch.zeros(2, 12, dtype=torch.bfloat16, device=DEV)
    rc, got = run_launch(logits, None, 12)
    assert rc == -100
    assert (got == PATTERN).all(), "a rejected launch wrote out"


@pytest.mark.parametrize("key", [(4104, 3, True), (32776, 65, True)], ids=ac.key_id)
def test_comparison_sees_a_wrong_mask(key):
    """The harness itself: the real kernel fed the mask of row b + 1 is a
    mutant of the CPU proof. It must agree with that mutant's own emulation on
    every row, and miss the true oracle on at least as many rows as the CPU
    mutant predicts."""
    knobs = ac.MUTANTS["mask_of_row_b+1"]
    got = run_case(key, roll=knobs["mask_roll"])
    own, want = ac.run_emulation(key, knobs), ac.expected(key)
    assert all(np.array_equal(g, o) for g, o in zip(got, own)), "the mutant's own answer"
    wrong = int(sum((g != w).sum() for g, w in zip(got, want)))
    predicted = ac.rows_changed(key, knobs)
    print(f"\nARGMAX self-check {ac.key_id(key)}: {wrong} rows off the oracle, CPU mutant predicts {predicted}")
    assert predicted >= 1 and wrong >= predicted
