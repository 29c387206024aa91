"""Register budget of the decode attention kernels (attention_decode.hip),
checked at compile time with the parsing of tests/test_gemv_resources.py.

Every decode_attn_kernel<G, FUSED, ROPE, DEEP> and decode_combine_kernel<G>
instantiation must compile for gfx950 with zero scratch.

The 4-deep rope forms <4, *, true, true> are what the engine runs at B <= 4.
Their grid is B * Hk x nsplit blocks of 4 waves; on the engine's frozen split
count (8 kv heads x 32 splits) that is 256 blocks at B = 1 and 512 at B = 2 on
256 CUs x 4 SIMDs: 1 and 2 waves per SIMD. A SIMD lane has 512 VGPRs, so two
resident waves need at most 256 each.

The 2-deep rope forms <4, *, true, false> run at B > 4, where the batch fills
the chip and resident waves hide the latency: they keep the three waves per
SIMD they have always had, at most 512 / 3 = 170 VGPRs rounded down to the
allocation granule of 8, i.e. 168.
"""

import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
    "opsagent_amd", "ops", "csrc",
)

GROUPS = (1, 2, 4, 8)
ROPE_DEEP_G4_CAP = 256
ROPE_SHALLOW_G4_CAP = 168


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """mangled kernel name -> (VGPRs, AGPRs, scratch bytes per lane)"""
    tmp = tmp_path_factory.mktemp("decode_attn_res")
    out = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
         "-Rpass-analysis=kernel-resource-usage",
         "-c", os.path.join(CSRC, "attention_decode.hip"), "-o", str(tmp / "k.o")],
        capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    current_fn = ""
    for ln in out.stderr.splitlines():
        if "Function Name:" in ln:
            current_fn = ln.rsplit(None, 2)[-2]
            res[current_fn] = [None, None, None]
        elif " VGPRs:" in ln and current_fn:
            res[current_fn][0] = int(ln.split(" VGPRs:")[1].split()[0])
        elif " AGPRs:" in ln and current_fn:
            res[current_fn][1] = int(ln.split(" AGPRs:")[1].split()[0])
        elif "ScratchSize [bytes/lane]:" in ln and current_fn:
            res[current_fn][2] = int(ln.split("ScratchSize [bytes/lane]:")[1].split()[0])
    return res


def b(v):
    return "Lb1E" if v else "Lb0E"


def attn_name(G, fused, rope, deep):
    return f"_Z18decode_attn_kernelILi{G}E{b(fused)}{b(rope)}{b(deep)}E"


def combine_name(G):
    return f"_Z21decode_combine_kernelILi{G}EE"


def lookup(usage, prefix):
    hits = [v for k, v in usage.items() if k.startswith(prefix)]
    assert len(hits) == 1, f"{prefix}: {len(hits)} kernels"
    return hits[0]


ALL_KERNELS = [
    attn_name(G, fused, rope, deep)
    for G in GROUPS
    for fused in (False, True)
    for rope in (False, True)
    for deep in (False, True)
] + [combine_name(G) for G in GROUPS]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_every_instantiation_has_zero_scratch(usage):
    ours = [k for k in usage if "decode_attn_kernel" in k or "decode_combine_kernel" in k]
    assert len(ours) == len(ALL_KERNELS), sorted(ours)
    bad = []
    for name in ALL_KERNELS:
        vgprs, agprs, scratch = lookup(usage, name)
        print(f"{name}: {vgprs} VGPRs, {agprs} AGPRs, scratch {scratch}")
        if scratch != 0:
            bad.append(f"{name}: scratch {scratch} B/lane")
    assert not bad, "\n".join(bad)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
@pytest.mark.parametrize("fused", [False, True], ids=["two_kernel", "fused"])
def test_rope_deep_g4_keeps_two_waves_per_simd(usage, fused):
    name = attn_name(4, fused, True, True)
    vgprs, agprs, scratch = lookup(usage, name)
    print(f"{name}: {vgprs} VGPRs + {agprs} AGPRs (cap {ROPE_DEEP_G4_CAP}), scratch {scratch}")
    # VGPRs and AGPRs share the SIMD's unified register file
    assert vgprs + agprs <= ROPE_DEEP_G4_CAP
    assert scratch == 0


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
@pytest.mark.parametrize("fused", [False, True], ids=["two_kernel", "fused"])
def test_rope_shallow_g4_keeps_three_waves_per_simd(usage, fused):
    name = attn_name(4, fused, True, False)
    vgprs, agprs, scratch = lookup(usage, name)
    print(f"{name}: {vgprs} VGPRs + {agprs} AGPRs (cap {ROPE_SHALLOW_G4_CAP}), scratch {scratch}")
    assert vgprs + agprs <= ROPE_SHALLOW_G4_CAP
    assert scratch == 0
