"""Build-time guard for csrc/probe_train.hip: every kernel of the fused probe training call compiles for gfx950 with no VGPR / SGPR
spills and no scratch, and keeps the occupancy it has today.

Today (waves/SIMD from the compiler's register count): probe_train_kernel<8> 5 (94 VGPRs), <16> 4 (116), <32> 3 (166; 27 labels,
the training shape: three workgroups of four waves per compute unit), <64> 1 (256); probe_train_reduce 8 (22)."""
import pytest

from stego_amd import _build

OCCUPANCY_FLOOR = {"probe_train_kernelILi8E": 5, "probe_train_kernelILi16E": 4, "probe_train_kernelILi32E": 3,
                   "probe_train_kernelILi64E": 1, "probe_train_reduce": 8}


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_probe_train_kernels_have_no_spills():
    kernels = _build.kernel_resources("probe_train.hip")
    probe = {k: v for k, v in kernels.items() if "probe_train" in k}
    assert len(probe) == 5, sorted(kernels)
    for k, v in probe.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        floor = [f for key, f in OCCUPANCY_FLOOR.items() if key in k]
        assert len(floor) == 1 and v["Occupancy [waves/SIMD]"] >= floor[0], (k, v)
