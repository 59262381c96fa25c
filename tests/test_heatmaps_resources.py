"""Build-time guard for csrc/corr_heat.hip: the low-resolution kernel and both instantiations of the write kernel (16-byte and
4-byte stores) compile for gfx950 with no VGPR / SGPR spills and no scratch, and keep the occupancy they have today."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_heatmap_kernels_have_no_spills(tmp_path):
    src = os.path.join(ROOT, "stego_amd", "csrc", "corr_heat.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", src, "-o", str(tmp_path / "corr_heat.o"),
           "-Rpass-analysis=kernel-resource-usage"]
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
    low = {k: v for k, v in kernels.items() if "heat_low_kernel" in k}
    write = {k: v for k, v in kernels.items() if "heat_write_kernel" in k}
    assert len(low) == 1 and len(write) == 2, sorted(kernels)      # flags and shapes are run-time parameters; the store width is not
    for k, v in {**low, **write}.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
    for k, v in low.items():
        # today: 116 VGPRs + 64 AGPRs (the 128 x 128 fp32 accumulator tile) = 2 waves per SIMD by registers, which is also what its
        # 76800 bytes of LDS allow (two workgroups of four waves per CU)
        assert v["Occupancy [waves/SIMD]"] >= 2, (k, v)
    for k, v in write.items():
        # today: 50 VGPRs with 16-byte stores, 32 with 4-byte stores: the full 8 waves per SIMD, what a store-bound kernel wants
        assert v["Occupancy [waves/SIMD]"] >= 8, (k, v)
