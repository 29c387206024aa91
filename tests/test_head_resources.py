"""Register budget of the fused decode head (head_argmax.hip), checked at
compile time in the manner of tests/test_gemv_resources.py: every instantiation
the launcher can reach must have 0 B of scratch and a VGPR count that keeps the
waves its grid supplies.

Grid (oa_head_argmax_grid): at most 256 * HEAD_WAVES(M) blocks of 4 waves on
256 CUs x 4 SIMDs, i.e. HEAD_WAVES(M) waves per SIMD. 512 VGPRs per SIMD lane,
allocated in blocks of 8:
  * M = 1, 8 waves per SIMD -> at most 64 VGPRs
  * M = 2, 7 waves per SIMD -> at most 72 VGPRs
The finish kernel is one block and must merely not spill.
"""

import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
    "opsagent_amd", "ops", "csrc",
)
SRC = os.path.join(CSRC, "head_argmax.hip")

VGPR_FILE = 512


def vgpr_cap(waves):
    return (VGPR_FILE // waves) // 8 * 8


def source_constants():
    src = open(SRC).read()
    ku = {}
    for m in (1, 2):
        mm = re.search(rf"#define HEAD_ARGMAX_KU_M{m} (\d+)", src)
        assert mm, f"HEAD_ARGMAX_KU_M{m} not found in head_argmax.hip"
        ku[m] = int(mm.group(1))
    mm = re.search(r"#define HEAD_WAVES\(M\) \(\(M\) == 1 \? (\d+) : (\d+)\)", src)
    assert mm, "HEAD_WAVES not found in head_argmax.hip"
    waves = {1: int(mm.group(1)), 2: int(mm.group(2))}
    # every (M, KU) the launcher instantiates
    inst = {(int(a), int(b)) for a, b in re.findall(r"head_argmax_launch<(\d), (\d)>", src)}
    return ku, waves, inst


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """mangled kernel name -> [VGPRs, scratch bytes per lane]"""
    tmp = tmp_path_factory.mktemp("head_res")
    out = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
         "-Rpass-analysis=kernel-resource-usage",
         "-c", SRC, "-o", str(tmp / "k.o")],
        capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    current_fn = ""
    for ln in out.stderr.splitlines():
        if "Function Name:" in ln:
            current_fn = ln.rsplit(None, 2)[-2]
            res[current_fn] = [None, None]
        elif " VGPRs:" in ln and current_fn:
            res[current_fn][0] = int(ln.split(" VGPRs:")[1].split()[0])
        elif "ScratchSize [bytes/lane]:" in ln and current_fn:
            res[current_fn][1] = int(ln.split("ScratchSize [bytes/lane]:")[1].split()[0])
    return res


def lookup(usage, prefix):
    hits = [v for k, v in usage.items() if k.startswith(prefix)]
    assert len(hits) == 1, f"{prefix}: {len(hits)} kernels"
    return hits[0]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_head_kernels_fit_their_grids(usage):
    ku, waves, inst = source_constants()
    for m in (1, 2):
        assert (m, ku[m]) in inst, f"shipped depth {ku[m]} at M={m} is not instantiated"
    kernels = [k for k in usage if "head_argmax_kernel" in k]
    assert len(kernels) == len(inst), f"{sorted(kernels)} vs {sorted(inst)}"
    over = []
    for m, k in sorted(inst):
        cap = vgpr_cap(waves[m])
        vgprs, scratch = lookup(usage, f"_Z18head_argmax_kernelILi{m}ELi{k}EE")
        print(f"head_argmax_kernel<{m}, {k}>: {vgprs} VGPRs (cap {cap}), scratch {scratch}")
        if vgprs > cap or scratch != 0:
            over.append(f"<{m}, {k}>: {vgprs} VGPRs > {cap} or scratch {scratch} != 0")
    vgprs, scratch = lookup(usage, "_Z18head_argmax_finish")
    print(f"head_argmax_finish: {vgprs} VGPRs, scratch {scratch}")
    if scratch != 0:
        over.append(f"finish: scratch {scratch} != 0")
    assert not over, "\n".join(over)


def test_grid_cap_matches_resident_waves():
    """the grid function and the kernel attribute share HEAD_WAVES"""
    src = open(SRC).read()
    assert "amdgpu_waves_per_eu(HEAD_WAVES(M))" in src
    assert "256 * (M == 1 ? HEAD_WAVES(1) : HEAD_WAVES(2))" in src
