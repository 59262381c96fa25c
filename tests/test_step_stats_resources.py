"""Build-time guard for csrc/step_stats.hip: the one kernel of the step statistics compiles for gfx950 with no VGPR / SGPR spills and no
scratch, and its LDS is what its design declares: the 1549 threshold keys, one set of 1548 uint32 counters per wave and the few words
of the workgroup fold - 31 KB, so five workgroups share a compute unit."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_step_stats_kernel_has_no_spills(tmp_path):
    src = os.path.join(ROOT, "stego_amd", "csrc", "step_stats.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
           str(tmp_path / "step_stats.o"), "-Rpass-analysis=kernel-resource-usage"]
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
    assert len(kernels) == 1 and "step_stats_kernel" in next(iter(kernels)), sorted(kernels)     # one launch: one kernel
    waves, limits, buckets = 4, 1549, 1548
    declared = 4 * limits + 4 * waves * buckets                    # keys, per-wave counters
    for k, v in kernels.items():                   # today: 95 VGPRs, 31120 bytes of LDS, 5 waves per SIMD
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert declared <= v["LDS Size [bytes/block]"] <= declared + 256, (k, v, declared)     # + the fold's stage (28 bytes per wave) and a flag
        assert v["VGPRs"] <= 128 and v["Occupancy [waves/SIMD]"] >= 4, (k, v)
