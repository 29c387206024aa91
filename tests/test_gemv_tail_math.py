"""The K-piece / tail index arithmetic the pipelined GEMVs use
(opsagent_amd/ops/csrc/gemv_tile.h) is plain host+device C++. Build the
stand-alone sweep program under ASan + UBSan and run it: for K/2 from 4 to 8192
in steps of 4 and every depth, each 16-byte unit of a row is loaded exactly once
and none lies past the row end. CPU only — nothing is loaded into Python."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opsagent_amd", "ops", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "gemv_tile_sweep.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
def test_pieces_cover_each_unit_once_and_stay_in_row(tmp_path):
    exe = str(tmp_path / "gemv_tile_sweep")
    cc = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
         "-I", CSRC, SRC, "-o", exe],
        capture_output=True, text=True, timeout=300,
    )
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "gemv_tile_sweep OK" in run.stdout
