"""Build-time guard for csrc/optim_step.hip: the one kernel of the fused Adam step compiles for gfx950 with no VGPR / SGPR spills, no
scratch and no LDS (the ticket lives in global memory), at 8 waves per SIMD or more."""
import pytest

from stego_amd import _build


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_adam_step_kernel_has_no_spills():
    kernels = _build.kernel_resources("optim_step.hip")
    assert len(kernels) == 1 and "adam_step_kernel" in next(iter(kernels)), sorted(kernels)     # one launch: one kernel
    for k, v in kernels.items():                   # today: 54 VGPRs, 8 waves
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] == 0, (k, v)
        assert v["Occupancy [waves/SIMD]"] >= 8, (k, v)
