"""Build-time guard for csrc/optim_step.hip: the one kernel of the fused Adam step compiles for gfx950 with no VGPR / SGPR spills, no
scratch and no LDS (the ticket lives in global memory), at 8 waves per SIMD or more."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_adam_step_kernel_has_no_spills(tmp_path):
    src = os.path.join(ROOT, "stego_amd", "csrc", "optim_step.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
           str(tmp_path / "optim_step.o"), "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    kernels, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    assert len(kernels) == 1 and "adam_step_kernel" in next(iter(kernels)), sorted(kernels)     # one launch: one kernel
    for k, v in kernels.items():                   # today: 54 VGPRs, 8 waves
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] == 0, (k, v)
        assert v["Occupancy [waves/SIMD]"] >= 8, (k, v)
