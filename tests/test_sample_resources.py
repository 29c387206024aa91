"""Register budget of the seeded sampler (sample.hip), checked at compile time
in the manner of tests/test_head_resources.py: every kernel in the file has
0 B of scratch and a VGPR count that lets its block exist.

The finish kernel is one block of SAMPLE_THREADS = 1024 lanes per row: 16
waves, four per SIMD. 512 VGPRs per SIMD lane, allocated in blocks of 8, so at
most 128 VGPRs; above that the block cannot launch at all. The two chunk
kernels run SAMPLE_CHUNK_THREADS = 256 lanes, one wave per SIMD, and are held
to the same 128 so that four of their blocks fit a CU."""

import os
import re
import shutil
import subprocess

import pytest

SRC = os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
    "opsagent_amd", "ops", "csrc", "sample.hip",
)
VGPR_FILE = 512
SIMDS = 4
WAVE = 64


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """mangled kernel name -> [VGPRs, scratch bytes per lane]"""
    tmp = tmp_path_factory.mktemp("sample_res")
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


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_sample_kernels_fit(usage):
    src = open(SRC).read()
    threads = int(re.search(r"#define SAMPLE_THREADS (\d+)", src).group(1))
    assert "__launch_bounds__(SAMPLE_THREADS)" in src
    assert "__launch_bounds__(SAMPLE_CHUNK_THREADS)" in src
    waves_per_simd = threads // WAVE // SIMDS
    cap = (VGPR_FILE // waves_per_simd) // 8 * 8
    names = ("sample_chunk_first", "sample_chunk_hist", "sample_row_finish")
    assert len(usage) == len(names), sorted(usage)
    for want in names:
        hits = [k for k in usage if want in k]
        assert len(hits) == 1, (want, sorted(usage))
        vgprs, scratch = usage[hits[0]]
        print(f"{want}: {vgprs} VGPRs (cap {cap}), scratch {scratch}")
        assert scratch == 0, f"{want}: scratch {scratch} B"
        assert vgprs <= cap, f"{want}: {vgprs} VGPRs > {cap}"


def test_lds_budget_matches_the_launcher():
    """hist (SAMPLE_BINS u64) + one bitmap byte per granule stay inside the
    64 KB a block may ask for without an attribute."""
    src = open(SRC).read()
    bins = int(re.search(r"#define SAMPLE_BINS (\d+)", src).group(1))
    granules = int(re.search(r"#define SAMPLE_MAX_GRANULES (\d+)", src).group(1))
    assert bins * 8 + granules + 1024 <= 64 * 1024
    assert "V / 8 > SAMPLE_MAX_GRANULES" in src
