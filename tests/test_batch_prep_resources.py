"""Build-time guard for csrc/batch_prep.hip: both instantiations of the batch-preparation kernel (16 pixels per lane with 16-byte
stores, and the one-pixel form for R % 4 != 0) compile without spills and keep the occupancy they have today."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_batch_prep_kernel_has_no_spills(tmp_path):
    src = os.path.join(ROOT, "stego_amd", "csrc", "batch_prep.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "stego_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           "-c", src, "-o", str(tmp_path / "batch_prep.o"), "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    kernels, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    prep = {k: v for k, v in kernels.items() if "batch_prep_kernel" in k}
    assert len(prep) == 2, sorted(kernels)
    for k, v in prep.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["Occupancy [waves/SIMD]"] >= 4, (k, v)          # 102 registers at 16 pixels per lane today
