"""Build-time guard for csrc/confusion.hip: every kernel (the probe-confusion kernel at 8, 16, 32 and 64 label slots, the counting
kernel for scores and for label maps) compiles for gfx950 with no VGPR / SGPR spills and no scratch, and keeps the occupancy it has
today."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_confusion_kernels_have_no_spills(tmp_path):
    src = os.path.join(ROOT, "stego_amd", "csrc", "confusion.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
           str(tmp_path / "confusion.o"), "-Rpass-analysis=kernel-resource-usage"]
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
    probe = {k: v for k, v in kernels.items() if "probe_confusion_kernel" in k}
    count = {k: v for k, v in kernels.items() if "confusion_count_kernel" in k}
    assert len(probe) == 4 and len(count) == 2, sorted(kernels)
    assert not any("probe_head_kernel" in k for k in kernels), sorted(kernels)      # those stay in probe_head.hip
    for k, v in {**probe, **count}.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
    for k, v in probe.items():
        floor = 3 if "ILi64E" in k else 4        # today: 98 / 114 / 126 VGPRs at 8 / 16 / 32 slots (4 waves), 136 at 64 (3 waves)
        assert v["Occupancy [waves/SIMD]"] >= floor, (k, v)
    for k, v in count.items():                   # today: 34 VGPRs (scores) and 10 (label maps), 8 waves
        assert v["Occupancy [waves/SIMD]"] >= 8, (k, v)
