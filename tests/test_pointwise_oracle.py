"""CPU proof that the pointwise GPU tests can fail
(tests/test_pointwise_gpu.py; cases, oracles, emulations and mutants in
tests/pointwise_cases.py).

For every case the GPU file runs, the fp32 emulation of the kernel (same
operations, bf16 output) must pass the rounding test with ZERO failing
elements, and every wrong kernel of `case.mutants()` must fail it on >=
MIN_FAIL elements. The conditions the method rests on are asserted as the
cases are built (every oracle value a bf16 normal or 0, neighbouring rows >= 4x
apart in rms, eps deciding the small rows, every probe >= 1/16 of its row) and
spot-checked here. Run with -s for the counts; the last test prints the
weakest mutant per family.
"""

import collections

import numpy as np
import pytest

import pointwise_cases as pc

_weakest = collections.defaultdict(lambda: (float("inf"), 0, 0, "", ""))
_emulated = collections.defaultdict(lambda: [0, 0, float("-inf")])


def _prove(family, case):
    v = case.verdict(case.emulation())
    e = _emulated[family]
    e[0], e[1], e[2] = e[0] + v.n, e[1] + v.fails, max(e[2], v.worst)
    assert v.fails == 0, f"{case.name}: the emulation fails {v}"
    assert v.worst <= 1.0
    res = [(name, case.verdict(case.emulation(**knobs)).fails) for name, knobs in case.mutants()]
    w_name, w = min(res, key=lambda r: r[1])
    print(f"\n{case.name}: {v.n} elements, emulation 0 failures (worst {v.worst:.3f}), "
          f"mutants={len(res)} weakest={w_name} ({w} elements)")
    if w / v.n < _weakest[family][0]:
        _weakest[family] = (w / v.n, w, v.n, w_name, case.name)
    weak = [r for r in res if r[1] < pc.MIN_FAIL]
    assert not weak, f"{case.name}: mutants under {pc.MIN_FAIL} failing elements: {weak}"


def _norm_id(k):
    return f"{'fused-' if k[3] else ''}d{k[0]}-r{k[1]}-eps{k[2]:g}"


@pytest.mark.parametrize("key", pc.norm_keys(), ids=_norm_id)
def test_rmsnorm_mutants_visible(key):
    _prove("fused_add_rmsnorm" if key[3] else "rmsnorm", pc.norm_case(*key))


@pytest.mark.parametrize("key", pc.rope_keys("rope") + pc.rope_keys("rope_kv"),
                         ids=lambda k: f"{k[0]}-t{k[1]}-hq{k[2]}-hk{k[3]}-d{k[4]}")
def test_rope_mutants_visible(key):
    _prove(key[0], pc.rope_case(*key))


@pytest.mark.parametrize("key", pc.decode_rope_keys(), ids=lambda k: f"g{k[0]}-n{'_'.join(map(str, k[1]))}")
def test_decode_rope_mutants_visible(key):
    _prove("decode_rope", pc.decode_rope_case(*key))


@pytest.mark.parametrize("name", [c[0] for c in pc.ATTENTION_CASES])
def test_attention_sees_q_rope_of_upper_pairs(name):
    """Attention on the synthetic tables: a q whose sin is negated from pair 48
    must land >= 4 T from the fp64 oracle (T = 4 N of the existing emulation)."""
    import attention_oracle as ao

    c, q_mut = pc.attention_case(name)
    n, t = c.noise, c.tol
    assert 0.0 < n < 2.0 ** -6 and t == ao.TOL_FACTOR * n
    err = ao.row_rel_err(ao.decode_oracle(q_mut, c.kc_eff, c.vc_eff, c.bt, c.lens, c.scale), c.ref)
    print(f"\n{name}: N={n:.5f} T={t:.5f} q_sin_negated_from_pair_48 at {err / t:.1f} T")
    assert err >= ao.MUTANT_FACTOR * t
    assert int(c.lens.max()) <= pc.TABLE_P


@pytest.mark.parametrize("n", pc.silu_keys())
def test_silu_mul_mutants_visible(n):
    _prove("silu_mul", pc.silu_case(n))


@pytest.mark.parametrize("key", pc.KV_KEYS, ids=lambda k: f"t{k[0]}-hk{k[1]}-d{k[2]}")
def test_kv_write_mutants_visible(key):
    _prove("kv_write", pc.kv_write_case(*key))


def test_weakest_mutant_per_family():
    """Report only (needs the tests above in the same run)."""
    for fam in sorted(_weakest):
        _, w, n, m, name = _weakest[fam]
        en, ef, ew = _emulated[fam]
        print(f"\n{fam}: emulation {ef} failures of {en} (worst {ew:.3f}); "
              f"weakest mutant {m}: {w} of {n} on {name}")
        assert w >= pc.MIN_FAIL and ef == 0


# --------------------------------------------------------------------------
# the criterion and the inputs
# --------------------------------------------------------------------------
def test_the_criterion():
    r = np.array([1.0, 1.0, 1.0, -3.0, 0.0, 0.0, 2.0 ** -126])
    E = np.zeros_like(r)
    assert pc.ulp_bf16(r).tolist() == [2.0 ** -7] * 3 + [2.0 ** -6, 0.0, 0.0, 2.0 ** -133]
    got = pc.to_bits(np.array([1.0, 1.0 + 2.0 ** -7, 1.0 - 2.0 ** -8, -3.0, -0.0, 2.0 ** -126, 2.0 ** -126],
                              dtype=np.float32))
    fails, _ = pc.judge(got, r, E)
    assert fails == 2                                   # a whole ulp off, and a non-zero for an exact 0
    # half an ulp is in, a hair more is out; E lets exactly that hair in
    r = np.array([1.0 + 2.0 ** -8 + 2.0 ** -20])
    up, down = pc.to_bits(np.float32([1.0 + 2.0 ** -7])), pc.to_bits(np.float32([1.0]))
    assert pc.judge(up, r, np.zeros(1))[0] == 0 and pc.judge(down, r, np.zeros(1))[0] == 1
    assert pc.judge(down, r, np.array([2.0 ** -20]))[0] == 0
    assert pc.judge(np.array([pc.PATTERN], np.uint16), np.ones(1), np.ones(1))[0] == 1, "NaN fails"
    x = np.float32([1.00390625, 1.01171875, -1.00390625])           # ties: to even
    assert pc.bf16_round(x).tolist() == [1.0, 1.015625, -1.0]


def test_norm_inputs():
    assert pc.norm_probes(8) == [0, 7]
    assert pc.norm_probes(2056) == [0, 7, 8, 511, 512, 2047, 2048, 2055]
    assert pc.norm_probes(1032) == [0, 7, 8, 511, 512, 1024, 1031]
    assert {6143, 6144, 8176, 8183} <= set(pc.norm_probes(8184))
    c = pc.norm_case(8192, 6, 1e-5, True)
    assert c.rms_sep >= 4.0
    s = c.x.astype(np.float64) + c.res.astype(np.float64)
    assert ((s * s).mean(-1)[list(pc.SMALL_ROWS)] < 1e-5).all()
    assert len(set(np.abs(c.w).tolist())) > 100 and (c.w != np.roll(c.w, 1)).all()


def test_rope_inputs():
    for D in pc.ROPE_DS:
        cos, sin = pc.tables(D)
        assert cos.shape == (pc.TABLE_P, D // 2) and cos.dtype == np.float32
        assert (np.abs(cos) <= 1).all() and (cos * 4096 == np.round(cos * 4096)).all()
        code = np.round(cos * 4096.0).astype(np.int64) * 10000 + np.round(sin * 4096.0).astype(np.int64)
        assert np.unique(code).size == cos.size, "every (position, pair) cell differs"
        # the upper pairs rotate by O(1): not one bf16 ulp, as with theta = 500000 at low positions
        assert np.abs(sin[:, D // 4:]).mean() > 0.4
    c = pc.rope_case("rope_kv", 37, 5, 3, 128)
    assert 0 in c.pos and pc.TABLE_P - 1 in c.pos
    assert len(set(c.slots.tolist())) == c.T - 3, "three rows repeat a slot"
    v = c.v.reshape(-1)
    assert (v == 0x8000).any() and (v == 0x7FC0).any() and (v == 0xFFFF).any()
    T, Hq, Hk, D = pc.GRID_STRIDE_ROPE
    assert T * Hq * D // 8 > 2048 * 256
    T, Hq, Hk, D = pc.GRID_STRIDE_ROPE_KV
    assert T * (Hq + 2 * Hk) * D // 8 > 2048 * 256 > T * (Hq + Hk) * D // 8, "the v copies stride too"


def test_silu_and_kv_inputs():
    g = pc.all_gates()
    a = np.abs(g.astype(np.float64))
    assert a.max() == 60.0 and a[a > 0].min() == 2.0 ** -20 and (a == 0).sum() == 2
    assert np.unique(pc.to_bits(g)).size == g.size == 6628
    c = pc.silu_case(pc.silu_keys()[2])
    assert np.unique(pc.to_bits(c.g)).size == 6628, "the exhaustive case holds every gate"
    assert pc.SILU_GRID_STRIDE_N // 8 > 2048 * 256
    T, Hk, D = pc.KV_KEYS[-1]
    assert T * Hk * D // 8 > 2048 * 256
