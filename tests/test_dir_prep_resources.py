"""Build-time guard for csrc/batch_prep_dir.hip and csrc/salience_draw.hip: both instantiations of the directory batch-preparation
kernel (16 pixels per lane with 16-byte stores, and the one-pixel form for R % 4 != 0) and both of the salience draw (float32 and
one-byte masks) compile for gfx950 without spills or scratch and keep the occupancy they have today."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _resources(tmp_path, name):
    src = os.path.join(ROOT, "stego_amd", "csrc", name + ".hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "stego_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           "-c", src, "-o", str(tmp_path / (name + ".o")), "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    kernels, fn = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            fn = m.group(1)
            kernels[fn] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and fn:
            kernels[fn][m.group(1)] = int(m.group(2))
    return kernels


def _no_spills(k, v):
    assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_dir_prep_kernel_has_no_spills(tmp_path):
    kernels = _resources(tmp_path, "batch_prep_dir")
    prep = {k: v for k, v in kernels.items() if "dir_prep_kernel" in k}
    assert len(prep) == 2 and not any("batch_prep_kernel" in k for k in kernels), sorted(kernels)
    for k, v in prep.items():
        _no_spills(k, v)
        vec = "ILi16E" in k
        assert v["Occupancy [waves/SIMD]"] >= (4 if vec else 8), (k, v)      # 106 registers at 16 pixels per lane today, 13 at one
        assert v["LDS Size [bytes/block]"] == 3 * 256 * 4, (k, v)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_salience_draw_kernel_has_no_spills(tmp_path):
    kernels = _resources(tmp_path, "salience_draw")
    draw = {k: v for k, v in kernels.items() if "salience_draw_kernel" in k}
    assert len(draw) == 2, sorted(kernels)
    for k, v in draw.items():
        _no_spills(k, v)
        assert v["Occupancy [waves/SIMD]"] >= 8, (k, v)                      # 19 registers today; 1024 threads are 4 waves per SIMD
        assert v["LDS Size [bytes/block]"] <= 40 * 1024, (k, v)              # 35856 today: four workgroups of a compute unit's 160 KB
