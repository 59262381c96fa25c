"""Build-time guard for csrc/corr_heat.hip: the low-resolution kernel and both instantiations of the write kernel (16-byte and
4-byte stores) compile for gfx950 with no VGPR / SGPR spills and no scratch, and keep the occupancy they have today."""
import pytest

from stego_amd import _build


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_heatmap_kernels_have_no_spills():
    kernels = _build.kernel_resources("corr_heat.hip")
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
