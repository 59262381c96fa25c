"""Build-time guard for csrc/augment.hip: every kernel of the device-side augmentation and of the fused aug-alignment loss compiles for
gfx950 with no VGPR / SGPR spills and no scratch, and keeps the occupancy it has today.

Today (waves/SIMD as the compiler reports them): aug_mean 8 (41 VGPRs), aug_apply 5 (41 VGPRs; 31,684 bytes of LDS per workgroup of four
waves: five workgroups per compute unit), align_pixels 8 (40), align_finish 8 (36)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
OCCUPANCY_FLOOR = {"aug_mean": 8, "aug_apply": 5, "align_pixels": 8, "align_finish": 8}
LDS_CEILING = {"aug_mean": 2048, "aug_apply": 32 * 1024, "align_pixels": 0, "align_finish": 2048}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_augment_kernels_have_no_spills(tmp_path):
    src = os.path.join(ROOT, "stego_amd", "csrc", "augment.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
           str(tmp_path / "augment.o"), "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    kernels, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    ours = {k: v for k, v in kernels.items() if any(key in k for key in OCCUPANCY_FLOOR)}
    assert len(ours) == len(OCCUPANCY_FLOOR), sorted(kernels)
    for k, v in ours.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        key = [key for key in OCCUPANCY_FLOOR if key in k]
        assert len(key) == 1, k
        assert v["Occupancy [waves/SIMD]"] >= OCCUPANCY_FLOOR[key[0]] and v["LDS Size [bytes/block]"] <= LDS_CEILING[key[0]], (k, v)
