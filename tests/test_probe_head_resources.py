"""Build-time guard for csrc/probe_head.hip: every instantiation of the fused probe-head kernel (8, 16, 32 and 64 label slots)
compiles for gfx950 with no VGPR / SGPR spills and no scratch, and keeps the occupancy it has today."""
import pytest

from stego_amd import _build


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_probe_head_kernel_has_no_spills():
    kernels = _build.kernel_resources("probe_head.hip")
    probe = {k: v for k, v in kernels.items() if "probe_head_kernel" in k}
    assert len(probe) == 4, sorted(kernels)
    for k, v in probe.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        floor = 2 if "ILi64E" in k else 4        # today: 86 / 100 / 100 VGPRs at 8 / 16 / 32 slots (5 / 4 / 4 waves), 177 at 64 (2 waves)
        assert v["Occupancy [waves/SIMD]"] >= floor, (k, v)
