"""Build-time guard for csrc/augment.hip: every kernel of the device-side augmentation and of the fused aug-alignment loss compiles for
gfx950 with no VGPR / SGPR spills and no scratch, and keeps the occupancy it has today.

Today (waves/SIMD as the compiler reports them): aug_mean 8 (41 VGPRs), aug_apply 5 (41 VGPRs; 31,684 bytes of LDS per workgroup of four
waves: five workgroups per compute unit), align_pixels 8 (40), align_finish 8 (36)."""
import pytest

from stego_amd import _build

OCCUPANCY_FLOOR = {"aug_mean": 8, "aug_apply": 5, "align_pixels": 8, "align_finish": 8}
LDS_CEILING = {"aug_mean": 2048, "aug_apply": 32 * 1024, "align_pixels": 0, "align_finish": 2048}


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_augment_kernels_have_no_spills():
    kernels = _build.kernel_resources("augment.hip")
    ours = {k: v for k, v in kernels.items() if any(key in k for key in OCCUPANCY_FLOOR)}
    assert len(ours) == len(OCCUPANCY_FLOOR), sorted(kernels)
    for k, v in ours.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        key = [key for key in OCCUPANCY_FLOOR if key in k]
        assert len(key) == 1, k
        assert v["Occupancy [waves/SIMD]"] >= OCCUPANCY_FLOOR[key[0]] and v["LDS Size [bytes/block]"] <= LDS_CEILING[key[0]], (k, v)
