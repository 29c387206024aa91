"""Register budget of the pipelined decode GEMVs (gemv.hip), checked at compile
time with the parsing of tests/test_kernel_resources.py: the M = 1 and M = 2
instantiations the dispatcher launches by default must keep as many waves
resident per SIMD as their grids supply, and none may spill.

Grids (gemv.hip dispatch, 256 CUs x 4 SIMDs, 512 VGPRs per SIMD lane):
  * two rows per wave (lm_head, 70B shapes) and gate-up cap the grid at 2048
    blocks of 4 waves = 32 waves per CU = 8 per SIMD  -> at most 64 VGPRs
  * one row per wave with the fused norm is qkv, N = 6144: 24 waves per CU =
    6 per SIMD                                         -> at most 80 VGPRs
  * one row per wave without norm is o_proj / down, N = 4096: 16 waves per
    CU = 4 per SIMD                                    -> at most 128 VGPRs
The two-row forms at M = 2 carry two activation rows and four accumulators per
slot; their depth-1 forms needed 74-78 VGPRs (6 waves per SIMD) before the
pipeline existed, so 8 waves is not theirs to keep. Their ceiling is the 6
waves they had: at most 80 VGPRs.
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


TWO_ROW_CAP = {1: 64, 2: 80}


def shipped_depths():
    src = open(os.path.join(CSRC, "gemv.hip")).read()
    out = {}
    for name in ("RW1", "RW1_NORM", "RW2", "RW2_NORM", "GATEUP"):
        for m in (1, 2):
            mm = re.search(rf"#define GEMV_KU_{name}_M{m} (\d+)", src)
            assert mm, f"GEMV_KU_{name}_M{m} not found in gemv.hip"
            out[(name, m)] = int(mm.group(1))
    return out


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """mangled kernel name -> (VGPRs, scratch bytes per lane)"""
    tmp = tmp_path_factory.mktemp("gemv_res")
    out = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
         "-Rpass-analysis=kernel-resource-usage",
         "-c", os.path.join(CSRC, "gemv.hip"), "-o", str(tmp / "k.o")],
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


def b(v):
    return "Lb1E" if v else "Lb0E"


def gemv_name(M, norm, addres, rw, ku):
    return f"_Z11gemv_kernelILi{M}E{b(norm)}{b(addres)}Li{rw}ELi{ku}EE"


def gateup_name(M, norm, ku):
    return f"_Z18gemv_gateup_kernelILi{M}E{b(norm)}Li{ku}EE"


def lookup(usage, prefix):
    hits = [v for k, v in usage.items() if k.startswith(prefix)]
    assert len(hits) == 1, f"{prefix}: {len(hits)} kernels"
    return hits[0]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
@pytest.mark.parametrize("M", [1, 2])
def test_shipped_depths_fit_their_grids(usage, M):
    ku = shipped_depths()
    two_row_cap = TWO_ROW_CAP[M]
    cases = []
    for addres in (False, True):
        cases.append((gemv_name(M, False, addres, 1, ku[("RW1", M)]), 128))
        cases.append((gemv_name(M, True, addres, 1, ku[("RW1_NORM", M)]), 80))
        cases.append((gemv_name(M, False, addres, 2, ku[("RW2", M)]), two_row_cap))
        cases.append((gemv_name(M, True, addres, 2, ku[("RW2_NORM", M)]), two_row_cap))
    for norm in (False, True):
        cases.append((gateup_name(M, norm, ku[("GATEUP", M)]), two_row_cap))
    over = []
    for name, cap in cases:
        vgprs, scratch = lookup(usage, name)
        print(f"{name}: {vgprs} VGPRs (cap {cap}), scratch {scratch}")
        if vgprs > cap or scratch != 0:
            over.append(f"{name}: {vgprs} VGPRs > {cap} or scratch {scratch} != 0")
    assert not over, "\n".join(over)
