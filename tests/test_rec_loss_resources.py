"""Build-time guard for csrc/rec_loss.hip: both kernels of the fused reconstruction loss compile for gfx950 with no VGPR / SGPR spills
and no scratch, and keep the occupancy they have today.

Today (waves/SIMD as the compiler reports them): rec_tiles<1> 2 (228 VGPRs), rec_tiles<2 .. 4> 1 (242, 256, 256 VGPRs; the workgroup is four
waves, one per SIMD, and its LDS, up to 151 KiB of dynamic memory sized by C at the launch, allows one workgroup per compute unit at
C = 1024 and two at C = 384); rec_finish<1 .. 4> 3, 2, 2, 1 (128, 140, 160, 179 VGPRs; 18,952 to 68,104 bytes of static LDS: the waves'
code tiles, then their sums)."""
import pytest

from stego_amd import _build

OCCUPANCY_FLOOR = {"rec_tiles": 1, "rec_finish": 1}
LDS_CEILING = {"rec_tiles": 0, "rec_finish": 68104}           # static bytes: rec_tiles' LDS is dynamic (stego_rec_loss_plan reports it)
INSTANCES = {"rec_tiles": 4, "rec_finish": 4}


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_rec_loss_kernels_have_no_spills():
    kernels = _build.kernel_resources("rec_loss.hip")
    ours = {k: v for k, v in kernels.items() if any(key in k for key in OCCUPANCY_FLOOR)}
    assert len(ours) == sum(INSTANCES.values()), sorted(kernels)
    for k, v in sorted(ours.items()):
        print(k, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        key = [key for key in OCCUPANCY_FLOOR if key in k]
        assert len(key) == 1, k
        assert v["Occupancy [waves/SIMD]"] >= OCCUPANCY_FLOOR[key[0]] and v["LDS Size [bytes/block]"] <= LDS_CEILING[key[0]], (k, v)
