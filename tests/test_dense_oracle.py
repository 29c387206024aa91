"""CPU proof that the bf16 dense GEMV GPU tests can fail
(tests/test_dense_bf16_gpu.py; cases, oracle, emulation and mutants in
tests/dense_cases.py).

For every case the GPU file runs:

  N = row_rel_err(fp32 emulation with bf16 output, fp64 oracle)
  T = 4 N

and every wrong kernel of `case.mutants()` must land at >= 4 T. The conditions
the method rests on are asserted here too: neighbouring batch rows differ in
rms by >= 2x, every MFMA run meets the conditions of gemv_bf16_use_mfma and no
VALU run does, the probes sit on the edges of the piece walk, and the depth
table mirrors gemv.hip. Run with -s to see N, T and the weakest mutant per
case; the last test prints the weakest mutant per family.
"""

import collections
import os
import re

import pytest
import torch

import dense_cases as dc
from opsagent_amd import ops

KEYS = dc.dense_keys()
_weakest = collections.defaultdict(lambda: (float("inf"), "", ""))
_tol_range = collections.defaultdict(lambda: (float("inf"), 0.0))
_FAMILIES = collections.defaultdict(set)
for _r in dc.DENSE_RUNS:
    _FAMILIES[_r.key].add(dc.family(_r))


@pytest.mark.parametrize("key", KEYS, ids=[dc.key_id(k) for k in KEYS])
def test_dense_mutants_visible(key):
    case = dc.dense_case(*key)
    n, t = case.noise, case.tol
    assert t == dc.TOL_FACTOR * n
    # bf16 rounds by at most 2^-8 of a value (8 significant bits). Output
    # rounding alone is < 2^-7 with room for fp32; behind the MFMA kernel's
    # staged norm each of gate and up carries 2^-8 more, silu's slope 1.3 at
    # most on top of gate's: (1 + 1.3 + 1) 2^-8 < 2^-6
    staged = case.kind == "mfma" and case.mode & 1
    assert 0.0 < n < (2.0 ** -6 if staged else 2.0 ** -7), f"{case.name}: implausible noise floor {n}"
    if case.M >= 2:
        assert case.rms_sep >= 2.0, f"{case.name}: rms of neighbouring rows within {case.rms_sep:.2f}x"
    errs = [(m, case.mutant_err(knobs)) for m, knobs in case.mutants()]
    w_name, w = min(errs, key=lambda e: e[1])
    print(f"\n{case.name}: N={n:.5f} T={t:.5f} mutants={len(errs)} weakest={w_name} ({w / t:.1f} T)")
    for fam in _FAMILIES[key]:
        if w / t < _weakest[fam][0]:
            _weakest[fam] = (w / t, w_name, case.name)
        lo, hi = _tol_range[fam]
        _tol_range[fam] = (min(lo, t), max(hi, t))
    weak = [(m, round(e / t, 2)) for m, e in errs if not e >= dc.MUTANT_FACTOR * t]
    assert not weak, f"{case.name}: T={t:.5f}, mutants under 4T: {weak}"


def test_weakest_mutant_per_family():
    """Report only (needs the test above in the same run)."""
    for fam in sorted(_weakest):
        r, m, name = _weakest[fam]
        lo, hi = _tol_range[fam]
        print(f"\nweakest {fam}: {r:.1f} T  {m} on {name}; T {lo:.5f} .. {hi:.5f}")
        assert r >= dc.MUTANT_FACTOR


# --------------------------------------------------------------------------
# the case list against the code it is meant to reach
# --------------------------------------------------------------------------
def _eligible(monkeypatch, run):
    dc.set_env(monkeypatch, run.env)
    _, M, _, K, _, gu = run.key
    return ops._bf16_mfma_ok(M, K, gateup=gu)


@pytest.mark.parametrize("run", dc.MFMA_RUNS + dc.MFMA_GU_RUNS,
                         ids=[dc.run_id(r) for r in dc.MFMA_RUNS + dc.MFMA_GU_RUNS])
def test_mfma_runs_are_eligible(run, monkeypatch):
    """A shape that fell back to hipBLASLt would not count as coverage."""
    assert _eligible(monkeypatch, run), run
    _, M, _, K, _, gu = run.key
    q = K // 4
    assert q % 32 == 0 and (q // 32) % (4 if gu else 8) == 0, "whole ring fills per quarter"
    assert M * (2 * K + 16) <= 147456


def test_valu_runs_are_not_eligible(monkeypatch):
    for run in dc.VALU_WIDE_RUNS + dc.OPS_RUNS:
        assert not _eligible(monkeypatch, run), run
    for run in dc.VALU_RUNS + dc.RW4_RUNS + dc.VALU_GU_RUNS:
        assert run.key[1] <= 2 and run.entry in ("ku", "rw4", "gu_ku")


def test_runs_reach_the_paths_they_are_meant_for():
    shapes = {(r.key[1], r.key[2], r.key[3]) for r in dc.MFMA_RUNS}
    assert any(K // 4 == 32 * 8 for _, _, K in shapes), "one ring fill, no refill"
    assert {M * (2 * K + 16) for M, _, K in shapes} >= {98432, 131328}
    assert any(N == 1 for _, N, _ in shapes) and any(N % 16 == 1 for _, N, _ in shapes)
    assert {r.key[1] for r in dc.MFMA_RUNS if not r.env} == {3, 5, 8}
    assert {r.key[1] for r in dc.MFMA_RUNS if r.env} == {2, 9, 15, 16}
    assert any(r.key[3] // 4 == 32 * 4 for r in dc.MFMA_GU_RUNS)
    # VALU: every instantiated M, all modes, both depths of a class, the
    # grid-stride pass of each rows-per-wave form, an odd N at two rows per wave
    assert {r.key[1] for r in dc.VALU_WIDE_RUNS} == {3, 4, 5, 6, 7, 8, 12, 16}
    assert {(r.rw, r.ku) for r in dc.VALU_RUNS} == {(1, 1), (1, 2), (1, 8), (2, 1)}
    assert {r.key[4] for r in dc.VALU_RUNS} == {0, 1, 2, 3}
    for rw, (N, _) in dc.GRID_STRIDE.items():
        assert N > 2048 * 4 * rw and N < 2 * 2048 * 4 * rw
    assert dc.GRID_STRIDE[2][0] % 2 == 1
    # M >= 3 through oa_gemv_ex: N <= 6144 is the one-row class, above it two rows
    assert any(r.key[2] > 6144 and r.key[2] % 2 for r in dc.VALU_WIDE_RUNS)
    assert all(r.key[3] % 512 for r in dc.VALU_WIDE_RUNS)


def test_depth_table_mirrors_the_source():
    src = os.path.join(os.path.dirname(ops.__file__), "csrc", "gemv.hip")
    with open(src) as f:
        defines = re.findall(r"#define GEMV_KU_(\w+)_M([12])\s+(\d+)", f.read())
    found = {f"{c}_M{m}": int(v) for c, m, v in defines}
    assert len(found) == 2 * len(dc.SHIPPED_KU)
    for cls, ku in dc.SHIPPED_KU.items():
        assert found[f"{cls}_M1"] == ku and found[f"{cls}_M2"] == ku, cls


def test_probes_sit_on_the_partition_edges():
    assert dc.piece_walk(4616, 8) == [(0, 8), (8, 1)]
    assert dc.piece_walk(7688, 8) == [(0, 8), (8, 4), (12, 2), (14, 1)]
    assert dc.piece_walk(7688, 4) == [(0, 4), (4, 4), (8, 4), (12, 2), (14, 1)]
    assert dc.piece_walk(7688, 1) == [(r, 1) for r in range(15)]
    assert dc.piece_walk(520, 8) == [(0, 1)] and dc.piece_walk(16, 2) == []
    assert dc.valu_probes(8) == [0, 7]
    assert dc.valu_probes(16) == [0, 7, 8, 15]
    assert dc.valu_probes(520) == [0, 7, 8, 15, 16, 511, 512, 519]
    assert dc.valu_probes(1040) == [0, 7, 8, 15, 16, 511, 512, 1023, 1024, 1032, 1039]
    p = dc.valu_probes(7688)
    for r in range(1, 16):
        assert r * 512 - 1 in p and r * 512 in p
    assert 7680 in p and 7687 in p
    p = dc.mfma_probes(6144, False)              # quarter 1536, refill after 256
    for k in (0, 7, 8, 31, 32, 255, 256, 1504, 1535, 1536, 1791, 1792, 3071, 3072, 4607, 4608,
              4863, 4864, 6112, 6143):
        assert k in p
    p = dc.mfma_probes(1024, False)              # nk = PF: no refill
    assert p == [0, 7, 8, 31, 32, 224, 255, 256, 480, 511, 512, 736, 767, 768, 992, 1023]
    assert 127 in dc.mfma_probes(1536, True) and 128 in dc.mfma_probes(1536, True)   # PF = 4


def test_inputs_make_a_neighbour_visible():
    c = dc.dense_case("valu", 16, 9, 1040, 3, False)
    assert c.rms_sep >= 2.0
    w = c.w.float()
    assert (w[:, c.probes].abs() >= 3 * 0.125).all()
    assert (w[-2:, c.probes].abs() >= 24).all(), "the last two rows sit in the largest class"
    assert (c.wn.float()[c.probes] == 2.0).all()
    xp = c.x.float()[:, c.probes].abs()
    assert (xp[0::2] >= 28 * 2.0 ** -5).all(), "even batch rows: every probe large"
    assert (xp[1::2, 0::2] >= 28 * 2.0 ** -5).all() and (xp[1::2, 1::2] >= 28 * 2.0 ** -8).all()
    assert (torch.sign(c.x.float()[:, c.probes]) == torch.sign(c.x.float()[0, c.probes])).all()
    g = dc.dense_case("mfma", 5, 16, 1536, 1, True)
    assert (g.w.float()[[14, 15, 30, 31]][:, g.probes].abs() >= 24).all(), "of each half"
    assert dc.rms_separation(torch.ones(3, 8)) == 1.0
