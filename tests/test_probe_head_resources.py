"""Build-time guard for csrc/probe_head.hip: every instantiation of the fused probe-head kernel (8, 16, 32 and 64 label slots)
compiles for gfx950 with no VGPR / SGPR spills and no scratch, and keeps the occupancy it has today."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_probe_head_kernel_has_no_spills(tmp_path):
    src = os.path.join(ROOT, "stego_amd", "csrc", "probe_head.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
           str(tmp_path / "probe_head.o"), "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    kernels, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    probe = {k: v for k, v in kernels.items() if "probe_head_kernel" in k}
    assert len(probe) == 4, sorted(kernels)
    for k, v in probe.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        floor = 2 if "ILi64E" in k else 4        # today: 86 / 100 / 100 VGPRs at 8 / 16 / 32 slots (5 / 4 / 4 waves), 177 at 64 (2 waves)
        assert v["Occupancy [waves/SIMD]"] >= floor, (k, v)
