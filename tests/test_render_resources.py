"""Build-time guard for csrc/render.hip: the three label-type instantiations of the render kernel and both range kernels compile for
gfx950 with no VGPR / SGPR spills and no scratch, and their static LDS (label tile, row stages, colour table) stays below the 64 KB
every kernel may use: 53 504 bytes with int64 labels (three workgroups per compute unit), 33 920 with int32 or uint8 labels.

Today: 94 / 152 / 48 VGPRs with int64 / int32 / uint8 labels (a thread's label and image loads are all in flight together)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INSTANCES = {"labels_i64": "render_kernelIlE", "labels_i32": "render_kernelIiE", "labels_u8": "render_kernelIhE",
             "range_partial": "range_partial_kernel", "range_final": "range_final_kernel"}
TILE, STAGE, TABLE = 17 * 288, 16 * 768, 512 * 4


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """name -> resource figures of every kernel of render.hip, from one compilation."""
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    tmp = tmp_path_factory.mktemp("render")
    src = os.path.join(ROOT, "stego_amd", "csrc", "render.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
           str(tmp / "render.o"), "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp))
    assert res.returncode == 0, res.stderr[-2000:]
    out, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


@pytest.mark.parametrize("inst", sorted(INSTANCES))
def test_render_kernels_have_no_spills(kernels, inst):
    hits = [v for k, v in kernels.items() if INSTANCES[inst] in k]
    assert len(hits) == 1, (inst, sorted(kernels))
    v = hits[0]
    print(inst, v)
    assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (inst, v)
    if inst.startswith("labels"):
        assert v["LDS Size [bytes/block]"] == TILE * (8 if inst == "labels_i64" else 4) + STAGE + TABLE, (inst, v)
        assert v["Occupancy [waves/SIMD]"] >= 3, (inst, v)         # three workgroups per compute unit, by LDS and by registers
    else:
        assert v["LDS Size [bytes/block]"] <= 64, (inst, v)
