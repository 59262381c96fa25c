"""Build-time guard for csrc/confusion.hip: every kernel (the probe-confusion kernel at 8, 16, 32 and 64 label slots, the counting
kernel for scores and for label maps) compiles for gfx950 with no VGPR / SGPR spills and no scratch, and keeps the occupancy it has
today."""
import pytest

from stego_amd import _build


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_confusion_kernels_have_no_spills():
    kernels = _build.kernel_resources("confusion.hip")
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
