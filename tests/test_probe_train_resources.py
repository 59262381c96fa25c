"""Build-time guard for csrc/probe_train.hip: every kernel of the fused probe training call compiles for gfx950 with no VGPR / SGPR
spills and no scratch, and keeps the occupancy it has today.

Today (waves/SIMD from the compiler's register count): probe_train_kernel<8> 5 (94 VGPRs), <16> 4 (116), <32> 3 (166; 27 labels,
the training shape: three workgroups of four waves per compute unit), <64> 1 (256); probe_train_reduce 8 (22)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
OCCUPANCY_FLOOR = {"probe_train_kernelILi8E": 5, "probe_train_kernelILi16E": 4, "probe_train_kernelILi32E": 3,
                   "probe_train_kernelILi64E": 1, "probe_train_reduce": 8}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_probe_train_kernels_have_no_spills(tmp_path):
    src = os.path.join(ROOT, "stego_amd", "csrc", "probe_train.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
           str(tmp_path / "probe_train.o"), "-Rpass-analysis=kernel-resource-usage"]
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
    probe = {k: v for k, v in kernels.items() if "probe_train" in k}
    assert len(probe) == 5, sorted(kernels)
    for k, v in probe.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        floor = [f for key, f in OCCUPANCY_FLOOR.items() if key in k]
        assert len(floor) == 1 and v["Occupancy [waves/SIMD]"] >= floor[0], (k, v)
